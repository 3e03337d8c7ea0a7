"""The numpy restatement of es_render_project / es_render_boxes / es_render_occupancy (csrc/predict.hip): f64 and int64, the
kernels' operation order, the pixel loops vectorised.  TEST INFRASTRUCTURE: the product never imports it (tools/bench_render.py times it
as the only alternative a user had).

project() asserts its own preconditions: no projected coordinate within 1e-6 of a quarter-pixel rounding boundary, no corner within 1e-9
of the usable / unusable decision (z = 1e-4, |u| or |v| = 4096) and no camera centre within 1e-9 of a box face -- the six f64 cos / sin of
a box are the only library calls of the kernels and may differ in the last bit between libraries; everything after the rounding is exact.
A population that violates one gets another seed, never a tolerance."""
import numpy as np

REC = 24
SKIP = 256
GUARD = 4096.0
EPS_Z = 1e-4
SHADE = (256, 208, 160)
CHUNK = 64                     # RND_CHUNK of predict.hip: records per LDS round
EDGES = [(lo, lo | (1 << a)) for a in range(3) for lo in range(8) if not lo & (1 << a)]


def faces():
    out = []
    for a in range(3):
        b, c = (1 if a == 0 else 0), (1 if a == 2 else 2)
        for s in range(2):
            p0 = s << a
            p1 = p0 | (1 << b)
            out.append((p0, p1, p1 | (1 << c), p0 | (1 << c)))
    return out


FACES = faces()


def rotation(angles):
    a, b, g = (np.float64(x) for x in angles)
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    return np.array([[ca * cc - sa * sb * sc, -(sa * cb), ca * sc + sa * sb * cc],
                     [sa * cc + ca * sb * sc, ca * cb, sa * sc - ca * sb * cc],
                     [-(cb * sc), sb, cb * cc]], np.float64)


def project(boxes, extrinsic, intrinsic, check=True):
    """boxes (n,9) f32, extrinsic / intrinsic (V,4,4) f32 -> rec (V,n,REC) int32"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 9)
    extrinsic = np.asarray(extrinsic, np.float32).reshape(-1, 4, 4)
    intrinsic = np.asarray(intrinsic, np.float32).reshape(-1, 4, 4)
    V, n = len(extrinsic), len(boxes)
    rec = np.zeros((V, n, REC), np.int32)
    for v in range(V):
        e, K = extrinsic[v].astype(np.float64), intrinsic[v].astype(np.float64)
        for i in range(n):
            b = boxes[i].astype(np.float64)
            c, h = b[:3], b[3:6] * 0.5
            R = rotation(boxes[i, 6:9])
            d = np.array([-((e[0, j] * e[0, 3] + e[1, j] * e[1, 3]) + e[2, j] * e[2, 3]) - c[j] for j in range(3)])
            loc = np.array([(R[0, j] * d[0] + R[1, j] * d[1]) + R[2, j] * d[2] for j in range(3)])
            inside = bool(np.all(loc <= h) and np.all(loc >= -h))
            if check:
                assert np.all(np.abs(np.abs(loc) - h) > 1e-9), f'view {v} box {i}: the camera centre lies on a face of the box'
            mask = SKIP if inside else 0
            x0 = y0 = 2 ** 31 - 1
            x1 = y1 = -2 ** 31
            for k in range(8):
                l = [h[a] if k & (1 << a) else -h[a] for a in range(3)]
                X = [c[r] + ((R[r, 0] * l[0] + R[r, 1] * l[1]) + R[r, 2] * l[2]) for r in range(3)]
                cam = [((e[r, 0] * X[0] + e[r, 1] * X[1]) + e[r, 2] * X[2]) + e[r, 3] for r in range(3)]
                z = cam[2]
                if check:
                    assert abs(z - EPS_Z) > 1e-9, f'view {v} box {i} corner {k}: z on the usable threshold'
                if not z >= EPS_Z:
                    continue
                u = (((K[0, 0] * cam[0] + K[0, 1] * cam[1]) + K[0, 2] * cam[2]) + K[0, 3]) / z
                w = (((K[1, 0] * cam[0] + K[1, 1] * cam[1]) + K[1, 2] * cam[2]) + K[1, 3]) / z
                if check:
                    assert abs(abs(u) - GUARD) > 1e-9 and abs(abs(w) - GUARD) > 1e-9, f'view {v} box {i} corner {k}: on the guard band'
                if not (u <= GUARD and u >= -GUARD and w <= GUARD and w >= -GUARD):
                    continue
                fu, fw = 4.0 * u + 0.5, 4.0 * w + 0.5
                if check:
                    assert abs(fu - np.rint(fu)) > 1e-6 and abs(fw - np.rint(fw)) > 1e-6, \
                        f'view {v} box {i} corner {k}: ({u}, {w}) within 1e-6 of a quarter-pixel rounding boundary: change the seed'
                qx, qy = int(np.floor(fu)), int(np.floor(fw))
                rec[v, i, 2 * k], rec[v, i, 2 * k + 1] = qx, qy
                mask |= 1 << k
                x0, x1, y0, y1 = min(x0, qx), max(x1, qx), min(y0, qy), max(y1, qy)
            rec[v, i, 16] = mask
            rec[v, i, 17:21] = (x0, y0, x1, y1)
    return rec


def to_hwc(src, chw):
    src = np.asarray(src, np.uint8)
    return np.ascontiguousarray(src.transpose(0, 2, 3, 1)) if chw else src.copy()


def blend(c, col, alpha):
    return (c * alpha + col * (256 - alpha) + 128) >> 8


def _cross(q, a, b, px, py):
    dx, dy = int(q[2 * b]) - int(q[2 * a]), int(q[2 * b + 1]) - int(q[2 * a + 1])
    return dx * (py - int(q[2 * a + 1])) - dy * (px - int(q[2 * a]))


def draw_boxes(src, chw, rec, colors, radius_q=4, alpha=192, cull=True):
    """-> dst (V,H,W,3) u8.  cull: evaluate a box only inside its grown rectangle (what makes the spec usable as a host renderer; the
    result does not depend on it -- test_render_spec.py checks that on a population)"""
    img = to_hwc(src, chw).astype(np.int64)
    V, H, W, _ = img.shape
    rec = np.asarray(rec, np.int32).reshape(V, -1, REC)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3).astype(np.int64)
    r2 = int(radius_q) * int(radius_q)
    for v in range(V):
        for i in range(rec.shape[1]):
            q = rec[v, i].astype(np.int64)
            m = int(q[16])
            if m & SKIP or not m & 255:
                continue
            xa, xb, ya, yb = 0, W - 1, 0, H - 1
            if cull:                                   # pixels with q17 - r <= 4x + 2 <= q19 + r (and the same in y)
                xa, xb = max(0, -((-(int(q[17]) - radius_q - 2)) // 4)), min(W - 1, (int(q[19]) + radius_q - 2) // 4)
                ya, yb = max(0, -((-(int(q[18]) - radius_q - 2)) // 4)), min(H - 1, (int(q[20]) + radius_q - 2) // 4)
                if xa > xb or ya > yb:
                    continue
            py, px = np.meshgrid(4 * np.arange(ya, yb + 1, dtype=np.int64) + 2, 4 * np.arange(xa, xb + 1, dtype=np.int64) + 2, indexing='ij')
            near = np.zeros(px.shape, bool)
            covered = np.zeros(px.shape, bool)
            for a, b in EDGES:
                if not (m >> a) & (m >> b) & 1:
                    continue
                ax, ay = int(q[2 * a]), int(q[2 * a + 1])
                dx, dy = int(q[2 * b]) - ax, int(q[2 * b + 1]) - ay
                ex, ey = px - ax, py - ay
                cr = dx * ey - dy * ex
                dot, len2 = dx * ex + dy * ey, dx * dx + dy * dy
                fx, fy = ex - dx, ey - dy
                near |= np.where(dot <= 0, ex * ex + ey * ey <= r2, np.where(dot >= len2, fx * fx + fy * fy <= r2, cr * cr <= r2 * len2))
            for f in FACES:
                if not all((m >> p) & 1 for p in f):
                    continue
                fs = [_cross(q, f[j], f[(j + 1) % 4], px, py) for j in range(4)]
                pos = (fs[0] >= 0) & (fs[1] >= 0) & (fs[2] >= 0) & (fs[3] >= 0)
                neg = (fs[0] <= 0) & (fs[1] <= 0) & (fs[2] <= 0) & (fs[3] <= 0)
                covered |= (pos | neg) & ((fs[0] != 0) | (fs[1] != 0) | (fs[2] != 0) | (fs[3] != 0))
            win = img[v, ya:yb + 1, xa:xb + 1]
            col = colors[i][None, None, :]
            win[...] = np.where(near[..., None], col, np.where(covered[..., None], blend(win, col, int(alpha)), win))
    return img.astype(np.uint8)


def render_boxes(src, chw, boxes, extrinsic, intrinsic, colors, radius_q=4, alpha=192, check=True):
    return draw_boxes(src, chw, project(boxes, extrinsic, intrinsic, check), colors, radius_q, alpha)


def rays_of(extrinsic, intrinsic):
    """(V,4,4) matrices -> (V,12) f64: the 3 x 3 R^T K^-1 row-major, then the camera centre -R^T t.  What embodiedscan_amd.render forms on
    the host (numpy f64); restated here so that a test can build rays without the product."""
    E = np.asarray(extrinsic, np.float64).reshape(-1, 4, 4)
    K = np.asarray(intrinsic, np.float64).reshape(-1, 4, 4)
    out = np.zeros((len(E), 12), np.float64)
    for v in range(len(E)):
        Rt = E[v, :3, :3].T
        out[v, :9] = (Rt @ np.linalg.inv(K[v, :3, :3])).reshape(-1)
        out[v, 9:] = -(Rt @ E[v, :3, 3])
    return out


def draw_occupancy(src, chw, rays, occ, rmin, size, palette, alpha=128):
    """-> dst (V,H,W,3) u8; occ (X,Y,Z) u8, palette (C,3) u8"""
    img = to_hwc(src, chw).astype(np.int64)
    V, H, W, _ = img.shape
    occ = np.asarray(occ, np.uint8)
    n = occ.shape
    palette = np.asarray(palette, np.uint8).reshape(-1, 3).astype(np.int64)
    C = len(palette)
    rays = np.asarray(rays, np.float64).reshape(V, 12)
    rmin, size = np.asarray(rmin, np.float64), np.asarray(size, np.float64)
    fy, fx = np.meshgrid(np.arange(H, dtype=np.float64) + 0.5, np.arange(W, dtype=np.float64) + 0.5, indexing='ij')
    inf = np.float64(np.inf)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for v in range(V):
            M, o = rays[v, :9].reshape(3, 3), rays[v, 9:]
            d = [(M[i, 0] * fx + M[i, 1] * fy) + M[i, 2] for i in range(3)]
            tmin, tmax = np.zeros((H, W)), np.full((H, W), inf)
            axis = np.zeros((H, W), np.int64)
            miss = np.zeros((H, W), bool)
            for i in range(3):
                lo, hi = rmin[i], rmin[i] + np.float64(n[i]) * size[i]
                zero = d[i] == 0.0
                if not (o[i] >= lo and o[i] < hi):
                    miss |= zero
                t0, t1 = (lo - o[i]) / d[i], (hi - o[i]) / d[i]
                sw = t0 > t1
                t0, t1 = np.where(sw, t1, t0), np.where(sw, t0, t1)
                up = ~zero & (t0 > tmin)
                tmin, axis = np.where(up, t0, tmin), np.where(up, i, axis)
                tmax = np.where(~zero & (t1 < tmax), t1, tmax)
            miss |= ~(tmin <= tmax)
            idx, step, tnext, dt = [], [], [], []
            for i in range(3):
                k = np.floor(((o[i] + tmin * d[i]) - rmin[i]) / size[i])
                k = np.clip(np.where(np.isfinite(k), k, 0), 0, n[i] - 1).astype(np.int64)
                idx.append(k)
                step.append(np.where(d[i] > 0.0, 1, np.where(d[i] < 0.0, -1, 0)))
                zero = d[i] == 0.0
                tnext.append(np.where(zero, inf, ((rmin[i] + (k + (d[i] > 0.0)).astype(np.float64) * size[i]) - o[i]) / d[i]))
                dt.append(np.where(zero, inf, size[i] / np.where(d[i] > 0.0, d[i], -d[i])))
            label = np.zeros((H, W), np.int64)
            active = ~miss
            for _ in range(n[0] + n[1] + n[2]):
                if not active.any():
                    break
                l = occ[idx[0], idx[1], idx[2]].astype(np.int64)
                hit = active & (l >= 1) & (l < C)
                label = np.where(hit, l, label)
                active &= ~hit
                a = np.where((tnext[0] <= tnext[1]) & (tnext[0] <= tnext[2]), 0, np.where(tnext[1] <= tnext[2], 1, 2))
                for i in range(3):
                    mv = active & (a == i)
                    k = idx[i] + step[i]
                    out = mv & ((k < 0) | (k > n[i] - 1))
                    active &= ~out
                    mv &= ~out
                    idx[i] = np.where(mv, k, idx[i])
                    tnext[i] = np.where(mv, tnext[i] + dt[i], tnext[i])
                    axis = np.where(mv, i, axis)
            got = label > 0
            shade = np.asarray(SHADE, np.int64)[axis]
            col = (palette[label] * shade[..., None]) >> 8
            img[v] = np.where(got[..., None], blend(img[v], col, int(alpha)), img[v])
    return img.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ populations
def camera(eye, yaw=0.0, pitch=0.0, focal=60.0, H=48, W=64):
    """-> (extrinsic, intrinsic) f32 4 x 4: a camera at `eye` in a z-up world looking along +x turned by yaw (about z) and pitch; camera
    axes x right, y down, z forward"""
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    fwd = np.array([cy * cp, sy * cp, sp])
    right = np.array([sy, -cy, 0.0])
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])                     # world -> camera
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ np.asarray(eye, np.float64)
    K = np.eye(4)
    K[0, 0] = K[1, 1] = focal
    K[0, 2], K[1, 2] = W / 2 + 0.37, H / 2 - 0.21
    return E.astype(np.float32), K.astype(np.float32)


def special_boxes():
    """for the camera(eye=(0, 0, 1)) looking along +x: one box of every kind the issue lists, then three mutually overlapping ones"""
    return np.array([
        [-3.0, 0.2, 1.0, 0.8, 0.6, 0.5, 0.3, 0.1, -0.2],        # behind the camera
        [0.3, 0.9, 1.1, 1.4, 0.5, 0.6, 0.2, 0.0, 0.1],          # straddles the camera plane: some corners unusable
        [0.1, -0.05, 1.05, 1.0, 1.2, 0.9, 0.4, 0.1, 0.0],       # contains the camera
        [2.0, 30.0, 1.0, 0.5, 0.5, 0.5, 0.0, 0.0, 0.0],         # wholly off-screen
        [0.0305, 1.2, 1.9, 0.06, 0.5, 0.5, 0.0, 0.0, 0.0],      # z from 0.0005 with a large offset: corners beyond the guard band
        [2.5, 0.4, 0.8, 0.0, 0.0, 0.0, 0.3, 0.2, 0.1],          # zero size
        [3.0, 0.0, 1.0, 1.2, 1.0, 0.8, 0.5, 0.2, -0.3],         # three mutually overlapping boxes
        [3.2, 0.3, 1.1, 1.0, 1.3, 0.7, -0.4, 0.1, 0.2],
        [2.8, -0.2, 0.9, 0.9, 0.8, 1.1, 1.0, -0.2, 0.1]], np.float32)


def population(n, seed):
    """n boxes: the special ones first (as many as fit), then seeded boxes in front of the cameras of views()"""
    rng = np.random.default_rng(seed)
    sp = special_boxes()
    out = np.zeros((n, 9), np.float32)
    out[:min(n, len(sp))] = sp[:n]
    for i in range(len(sp), n):
        out[i, :3] = rng.uniform((1.5, -2.5, 0.0), (6.0, 2.5, 2.0))
        out[i, 3:6] = rng.uniform(0.1, 1.0, 3)
        out[i, 6:] = rng.uniform(-np.pi, np.pi, 3) * (1.0, 0.3, 0.3)
    return out


def views(V, H, W, focal=None):
    cams = [camera((0, 0, 1), 0.0, 0.0, focal or 0.9 * W, H, W), camera((0.5, -1.0, 1.2), 0.35, -0.1, focal or 0.7 * W, H, W),
            camera((5.5, 0.5, 1.5), 2.9, -0.2, focal or 0.8 * W, H, W)]
    return np.stack([c[0] for c in cams[:V]]), np.stack([c[1] for c in cams[:V]])


def frames(V, H, W, chw, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (V, 3, H, W) if chw else (V, H, W, 3), dtype=np.uint8)


def colours(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (max(n, 1), 3), dtype=np.uint8)[:n]
