"""The numpy f64 / Python-int restatement of es_map_splat / es_map_resolve / es_map_project / es_map_occupancy (csrc/predict.hip, DESIGN
3i): the kernels' operation order, the pixel loops vectorised.  TEST INFRASTRUCTURE: the product never imports it (tools/bench_scene_map.py
times it as the alternative a user had).  Footprints and the trail are drawn by render_spec.draw_boxes: no raster rule is restated here.

splat() and project() assert their own precondition unless told that the case is exact by construction: no (p - x0) / cell, (p_y - y0) /
cell or (p_z - z_min) * 1024 of a pixel that passed the earlier tests, and no 4u + 0.5 of a usable corner, within 1e-9 of an integer; no
depth within 1e-9 of max_depth, no p_z within 1e-9 of the z cut, no |u| within 1e-9 of the guard band.  Every value is a handful of f64
products and sums of the same operands in the same order on both sides, so the kernels reproduce them bit for bit -- the margin only
absorbs the last-bit freedom of the six cos / sin of a box.  A population that violates it gets another seed, never a tolerance."""
import numpy as np

import render_spec as R

REC, GUARD = R.REC, R.GUARD
EDGES, FACES = R.EDGES, R.FACES
Z_STEPS = 1024.0
EPS = 1e-9


class Grid:
    def __init__(self, x0, y0, cell, width, height, z_min=-1.0, z_max=2.0, max_depth=8.0):
        self.x0, self.y0, self.cell, self.z_min, self.z_max, self.max_depth = (np.float64(v) for v in (x0, y0, cell, z_min, z_max, max_depth))
        self.width, self.height = int(width), int(height)
        self.nz = int(np.ceil((self.z_max - self.z_min) * Z_STEPS))


def _off_integer(a):
    return np.abs(a - np.rint(a))


def pixel_keys(depth, frames, chw, rays, G, exact=False):
    """-> (key (V,H,W) int64, 0 where the pixel is dropped; cell (V,H,W) int64 = row * Wm + column, -1 where dropped)"""
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    img = R.to_hwc(frames, chw)
    h, w = img.shape[1:3]
    rays = np.asarray(rays, np.float64).reshape(V, 12)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    fx, fy = x.astype(np.float64), y.astype(np.float64)
    cx, cy = ((2 * x + 1) * w) // (2 * W), ((2 * y + 1) * h) // (2 * H)
    key = np.zeros((V, H, W), np.int64)
    cell = np.full((V, H, W), -1, np.int64)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for v in range(V):
            d = depth[v].astype(np.float64)
            ok = (d > 0.0) & (d <= G.max_depth)
            M, c = rays[v, :9].reshape(3, 3), rays[v, 9:]
            p = [c[k] + d * ((M[k, 0] * fx + M[k, 1] * fy) + M[k, 2]) for k in range(3)]
            if not exact:
                assert not (np.isfinite(d) & (np.abs(d - G.max_depth) <= EPS)).any(), f'view {v}: a depth on max_depth'
                assert not (ok & ((np.abs(p[2] - G.z_min) <= EPS) | (np.abs(p[2] - G.z_max) <= EPS))).any(), f'view {v}: a point on the z cut'
            ok &= (p[2] >= G.z_min) & (p[2] < G.z_max)
            zs = (p[2] - G.z_min) * Z_STEPS
            gx, gy = (p[0] - G.x0) / G.cell, (p[1] - G.y0) / G.cell
            if not exact:
                near = ok & (np.abs(gx) < 1e7) & (np.abs(gy) < 1e7)
                bad = near & ((_off_integer(zs) <= EPS) | (_off_integer(gx) <= EPS) | (_off_integer(gy) <= EPS))
                assert not bad.any(), f'view {v}: {int(bad.sum())} pixels within 1e-9 of a cell or height boundary: change the seed'
            zq = np.floor(zs)
            ix, iy = np.floor(gx), np.floor(gy)
            ok &= (ix >= 0.0) & (ix < np.float64(G.width)) & (iy >= 0.0) & (iy < np.float64(G.height))
            zq, ix, iy = (np.where(ok, a, 0).astype(np.int64) for a in (zq, ix, iy))
            col = img[v][cy, cx].astype(np.int64)
            k = ((zq + 1) << 24) | (col[..., 0] << 16) | (col[..., 1] << 8) | col[..., 2]
            key[v] = np.where(ok, k, 0)
            cell[v] = np.where(ok, (G.height - 1 - iy) * G.width + ix, -1)
    return key, cell


def splat(depth, frames, chw, rays, G, keys=None, exact=False):
    """-> keys (Hm, Wm) int64: `keys` (or an empty map) raised by every pixel of the V views"""
    out = np.zeros((G.height, G.width), np.int64) if keys is None else np.array(keys, np.int64).reshape(G.height, G.width)
    key, cell = pixel_keys(depth, frames, chw, rays, G, exact)
    ok = cell >= 0
    np.maximum.at(out.reshape(-1), cell[ok], key[ok])
    return out


def census(depth, frames, chw, rays, G, exact=False):
    """what a test asserts on the spec's own output so that it cannot pass on an empty map -> dict(accepted = the fraction of pixels that
    reach a cell, shared = the fraction of non-empty cells that received two or more points, ties = the number of cells whose winner was
    decided by the colour: another point of the cell shares the winner's height step and has a smaller packed colour)"""
    key, cell = pixel_keys(depth, frames, chw, rays, G, exact)
    ok = cell >= 0
    c, k = cell[ok], key[ok]
    cnt = np.bincount(c, minlength=1)
    top = np.zeros(len(cnt), np.int64)
    np.maximum.at(top, c, k)
    rival = (k >> 24 == top[c] >> 24) & (k != top[c])          # a point at the winner's height step with another (smaller) colour
    ties = len(np.unique(c[rival]))
    return dict(accepted=float(ok.mean()) if ok.size else 0.0, shared=float((cnt >= 2).sum()) / max(int((cnt >= 1).sum()), 1), ties=ties)


def resolve(keys, G, background=(0, 0, 0), shade=1):
    """-> (image (Hm, Wm, 3) u8, height (Hm, Wm) f32 with NaN where empty)"""
    keys = np.asarray(keys, np.int64).reshape(G.height, G.width)
    full = keys != 0
    zq = (keys >> 24) - 1
    col = np.stack([(keys >> 16) & 255, (keys >> 8) & 255, keys & 255], -1)
    if shade:
        span = max(1, G.nz - 1)
        s = 160 + (96 * np.minimum(zq, span)) // span
        col = (col * s[..., None] + 128) >> 8
    img = np.where(full[..., None], col, np.asarray(background, np.int64).reshape(1, 1, 3)).astype(np.uint8)
    hz = np.where(full, G.z_min + (zq.astype(np.float64) + 0.5) / Z_STEPS, np.nan).astype(np.float32)
    return img, hz


def project(boxes, G, exact=False):
    """boxes (n, 9) f32 -> rec (1, n, REC) int32: the record of render_spec.project for the orthographic view from above"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 9)
    n = len(boxes)
    rec = np.zeros((1, n, REC), np.int32)
    for i in range(n):
        b = boxes[i].astype(np.float64)
        c, h = b[:3], b[3:6] * 0.5
        Rm = R.rotation(boxes[i, 6:9])
        mask = 0
        x0 = y0 = 2 ** 31 - 1
        x1 = y1 = -2 ** 31
        for k in range(8):
            l = [h[a] if k & (1 << a) else -h[a] for a in range(3)]
            X = c[0] + ((Rm[0, 0] * l[0] + Rm[0, 1] * l[1]) + Rm[0, 2] * l[2])
            Y = c[1] + ((Rm[1, 0] * l[0] + Rm[1, 1] * l[1]) + Rm[1, 2] * l[2])
            u, w = (X - G.x0) / G.cell, np.float64(G.height) - (Y - G.y0) / G.cell
            if not exact:
                assert abs(abs(u) - GUARD) > EPS and abs(abs(w) - GUARD) > EPS, f'box {i} corner {k}: on the guard band'
            if not (u <= GUARD and u >= -GUARD and w <= GUARD and w >= -GUARD):
                continue
            fu, fw = 4.0 * u + 0.5, 4.0 * w + 0.5
            if not exact:
                assert abs(fu - np.rint(fu)) > EPS and abs(fw - np.rint(fw)) > EPS, \
                    f'box {i} corner {k}: ({u}, {w}) within 1e-9 of a quarter-pixel rounding boundary: change the seed'
            qx, qy = int(np.floor(fu)), int(np.floor(fw))
            rec[0, i, 2 * k], rec[0, i, 2 * k + 1] = qx, qy
            mask |= 1 << k
            x0, x1, y0, y1 = min(x0, qx), max(x1, qx), min(y0, qy), max(y1, qy)
        rec[0, i, 16] = mask
        rec[0, i, 17:21] = (x0, y0, x1, y1)
    return rec


def draw_boxes(image, boxes, colors, G, radius_q=4, alpha=192, exact=False):
    """footprints over image (Hm, Wm, 3) u8 -> a new image"""
    return R.draw_boxes(np.asarray(image, np.uint8)[None], 0, project(boxes, G, exact), colors, radius_q, alpha)[0]


def draw_trail(image, centres, color, G, radius_q=6, exact=False):
    c = np.asarray(centres, np.float32).reshape(len(centres), -1)
    boxes = np.zeros((len(c), 9), np.float32)
    boxes[:, :c.shape[1]] = c
    return draw_boxes(image, boxes, np.asarray(color, np.uint8).reshape(1, 3).repeat(len(c), 0), G, radius_q, 256, exact)


def draw_occupancy(image, occ, rmin, size, palette, G, alpha=128):
    """the top surface of occ (X, Y, Z) u8 over image (Hm, Wm, 3) u8 -> a new image"""
    img = np.asarray(image, np.uint8).astype(np.int64)
    occ = np.asarray(occ, np.uint8)
    X, Y, Z = occ.shape
    palette = np.asarray(palette, np.uint8).reshape(-1, 3).astype(np.int64)
    C = len(palette)
    rmin, size = np.asarray(rmin, np.float64), np.asarray(size, np.float64)
    py, px = np.meshgrid(np.arange(G.height), np.arange(G.width), indexing='ij')
    Xc = G.x0 + (px.astype(np.float64) + 0.5) * G.cell
    Yc = G.y0 + ((G.height - 1 - py).astype(np.float64) + 0.5) * G.cell
    fi, fj = np.floor((Xc - rmin[0]) / size[0]), np.floor((Yc - rmin[1]) / size[1])
    ok = (fi >= 0.0) & (fi <= np.float64(X - 1)) & (fj >= 0.0) & (fj <= np.float64(Y - 1))
    i, j = np.where(ok, fi, 0).astype(np.int64), np.where(ok, fj, 0).astype(np.int64)
    cols = occ[i, j].astype(np.int64)                                   # (Hm, Wm, Z)
    good = (cols >= 1) & (cols < C)
    top = Z - 1 - np.argmax(good[..., ::-1], -1)
    label = np.where(ok & good.any(-1), np.take_along_axis(cols, top[..., None], -1)[..., 0], 0)
    out = np.where((label > 0)[..., None], R.blend(img, palette[label], int(alpha)), img)
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ populations
def down_camera(eye, focal, H, W):
    """-> (extrinsic, intrinsic) f64 4 x 4 of a camera at `eye` looking straight down: image x along +x of the world, image y along -y, the
    principal point at (W / 2, H / 2).  With dyadic eye / focal every product of the splat is exact."""
    Rm = np.array([[1., 0., 0.], [0., -1., 0.], [0., 0., -1.]])
    E = np.eye(4)
    E[:3, :3] = Rm
    E[:3, 3] = -Rm @ np.asarray(eye, np.float64)
    K = np.eye(4)
    K[0, 0] = K[1, 1] = focal
    K[0, 2], K[1, 2] = W / 2, H / 2
    return E, K


def ring(V, H, W, radius=2.5, height=1.4):
    """V cameras on a ring looking inward and a little down, as a walk round a room -> (extrinsic, intrinsic) f32 (V, 4, 4)"""
    cams = [R.camera((radius * np.cos(a), radius * np.sin(a), height), a + np.pi + 0.15, -0.45, 0.8 * W, H, W)
            for a in 0.4 + 2 * np.pi * np.arange(V) / max(V, 1)]
    return np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])


FLOOR_Z = 0.1


def depth_population(rays, H, W, seed, max_depth=6.0):
    """depth maps of a small room seen through `rays` (V, 12): the lower half of every image sees the flat floor z = FLOOR_Z (so many
    points of one cell share their height step and the colour decides) with a hole every 11 pixels, the upper half a bumpy surface 1 .. 3.7 m away with pixel noise;
    one of every kind of pixel the kernel drops is sprinkled in (as many as fit, never the last pixel): 0, a negative, NaN, +inf, just
    above max_depth, 1e9, -inf"""
    rng = np.random.default_rng(seed)
    rays = np.asarray(rays, np.float64).reshape(-1, 12)
    V = len(rays)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    d = np.zeros((V, H, W))
    for v in range(V):
        M, c = rays[v, :9].reshape(3, 3), rays[v, 9:]
        rz = (M[2, 0] * x + M[2, 1] * y) + M[2, 2]
        with np.errstate(divide='ignore', invalid='ignore'):
            floor = (FLOOR_Z - c[2]) / rz
        bumps = 2.2 + 1.2 * np.sin(3 * x / max(W, 1) + v) * np.cos(2 * y / max(H, 1) - v) + rng.uniform(-0.3, 0.3, (H, W))
        d[v] = np.where((y >= H / 2) & np.isfinite(floor) & (floor > 0.3) & (floor < max_depth - 0.1), floor, bumps)
        d[v] = np.where((y >= H / 2) & ((x + 3 * y) % 11 == 5), 1.5 * d[v], d[v])       # a hole in the floor: points below the z cut
    d = d.astype(np.float32)
    flat = d.reshape(-1)
    odd = np.array([0.0, -1.5, np.nan, np.inf, np.float32(max_depth) * np.float32(1.001), 1e9, -np.inf], np.float32)
    where = rng.permutation(flat.size - 1)[:min(len(odd), flat.size - 1)]
    flat[where] = odd[:len(where)]
    return d


def scene(V, H, W, Hm, Wm, seed, extent=5.0, z=(-0.25, 1.0)):
    """-> (rays (V, 12) f64, depth (V, H, W) f32, Grid): ring() seen through rays whose y row is scaled by Hm / Wm -- an affine camera is
    as good an input as a rigid one -- so that the cloud's footprint has the map's aspect whatever (Hm, Wm); the grid covers `extent`
    metres in x round the ring's centre, less than the cloud, and cuts the height to z"""
    E, K = ring(V, H, W)
    rays = R.rays_of(E, K)
    sy = Hm / Wm
    rays[:, 3:6] *= sy
    rays[:, 10] *= sy
    G = Grid(-extent / 2 + 0.0137, -extent * sy / 2 + 0.0071, extent / Wm, Wm, Hm, z_min=z[0], z_max=z[1], max_depth=6.0)
    return rays, depth_population(rays, H, W, seed, G.max_depth), G


def banded_frames(V, h, w, chw, seed):
    """frames whose colours come from a small pool, so that points of equal height in one cell differ in colour often enough for ties"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (5, 3), dtype=np.uint8)
    img = pool[rng.integers(0, len(pool), (V, h, w))]
    return np.ascontiguousarray(img.transpose(0, 3, 1, 2)) if chw else img


def map_boxes(n, seed, G):
    """n boxes over the grid: first a box beyond the guard band, a zero-size box and three overlapping ones (as many as fit), then seeded"""
    rng = np.random.default_rng(seed)
    cx, cy = float(G.x0 + G.cell * G.width / 2), float(G.y0 + G.cell * G.height / 2)
    ext = float(G.cell * max(G.width, G.height))
    sp = np.array([[cx + 5000.0 * float(G.cell), cy, 0.5, 0.5, 0.5, 0.5, 0.2, 0.0, 0.0],
                   [cx + 0.13 * ext, cy - 0.21 * ext, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                   [cx, cy, 0.5, 0.45 * ext, 0.3 * ext, 0.6, 0.5, 0.2, -0.3],
                   [cx + 0.1 * ext, cy + 0.05 * ext, 0.6, 0.3 * ext, 0.5 * ext, 0.7, -0.4, 0.1, 0.2],
                   [cx - 0.08 * ext, cy - 0.06 * ext, 0.4, 0.35 * ext, 0.25 * ext, 1.1, 1.0, -0.2, 0.1]], np.float32)
    out = np.zeros((n, 9), np.float32)
    out[:min(n, len(sp))] = sp[:n]
    for i in range(len(sp), n):
        out[i, :3] = (cx + rng.uniform(-0.6, 0.6) * ext, cy + rng.uniform(-0.6, 0.6) * ext, rng.uniform(0, 1.5))
        out[i, 3:6] = rng.uniform(0.02, 0.3, 3) * ext
        out[i, 6:] = rng.uniform(-np.pi, np.pi, 3) * (1.0, 0.3, 0.3)
    return out
