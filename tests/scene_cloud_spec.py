"""The numpy f64 / Python-int restatement of es_cloud_splat / es_cloud_mask / es_cloud_points / es_cloud_label / es_occ_face_mask /
es_occ_face_quads (csrc/predict.hip): the kernels' operation order, the pixel loops vectorised.  TEST INFRASTRUCTURE: the product
never imports it (tools/bench_scene_cloud.py times it as one alternative a user had).

pixel_records() and label() assert their own precondition unless told that the case is exact by construction: no accepted p_k / cell and no
d * 256 within 1e-9 of an integer (a d * 256 that IS an integer is exact by construction: a product with a power of two rounds nowhere), no
depth within 1e-9 of max_depth, no p_z within 1e-9 of a finite z cut, no |l_k| within 1e-9 of half_k + grow.  Every value is a handful of
f64 products and sums of the same operands in the same order on both sides, so the kernels reproduce them bit for bit -- the margin only
absorbs the last-bit freedom of the six cos / sin of a box.  A population that violates it
gets another seed, never a tolerance."""
import numpy as np

import render_spec as R
from scene_map_spec import banded_frames, depth_population, ring  # noqa: F401  (the populations of the map are the cloud's)

EPS = 1e-9
OFF = 1 << 17
FIELD = 18
FMASK = (1 << FIELD) - 1
PROBES = 64                          # ES_CLOUD_PROBES
CHUNK = R.CHUNK                      # boxes per LDS round of k_cloud_label
# face f = -x, +x, -y, +y, -z, +z: its corners as bits (x | y << 1 | z << 2) of the unit cube, counter-clockwise seen from outside
FACE_CORNERS = ((0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6))


class Grid:
    def __init__(self, cell, z_min=-np.inf, z_max=np.inf, max_depth=6.0):
        self.cell, self.z_min, self.z_max, self.max_depth = (np.float64(v) for v in (cell, z_min, z_max, max_depth))

    def host(self):
        return [float(self.cell), float(self.z_min), float(self.z_max), float(self.max_depth)]


def _off_integer(a):
    return np.abs(a - np.rint(a))


def es_hash(keys, mask):
    """splitmix64 finaliser of common.h -> slot"""
    x = np.asarray(keys, np.int64).astype(np.uint64)
    with np.errstate(over='ignore'):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        x = x ^ (x >> np.uint64(31))
    return (x & np.uint64(0xffffffff)).astype(np.int64) & int(mask)


def pack(i):
    """(..., 3) int64 voxel indices -> key of sample 0"""
    i = np.asarray(i, np.int64)
    return ((i[..., 0] + OFF) << (2 * FIELD)) | ((i[..., 1] + OFF) << FIELD) | (i[..., 2] + OFF)


def unpack(keys):
    k = np.asarray(keys, np.int64)
    return np.stack([((k >> (2 * FIELD)) & FMASK) - OFF, ((k >> FIELD) & FMASK) - OFF, (k & FMASK) - OFF], -1)


def pixel_records(depth, frames, chw, rays, G, exact=False):
    """-> (key (V,H,W) int64, -1 where the pixel is dropped; val (V,H,W) int64, 0 where dropped)"""
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    img = R.to_hwc(frames, chw)
    h, w = img.shape[1:3]
    rays = np.asarray(rays, np.float64).reshape(V, 12)
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    fx, fy = x.astype(np.float64), y.astype(np.float64)
    cx, cy = ((2 * x + 1) * w) // (2 * W), ((2 * y + 1) * h) // (2 * H)
    key = np.full((V, H, W), -1, np.int64)
    val = np.zeros((V, H, W), np.int64)
    lo, hi = np.float64(-OFF), np.float64(OFF)
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
            g = [p[k] / G.cell for k in range(3)]
            ds = d * 256.0
            if not exact:
                bad = ok & (((_off_integer(ds) <= EPS) & (ds != np.rint(ds))) | (_off_integer(g[0]) <= EPS) | (_off_integer(g[1]) <= EPS) | (_off_integer(g[2]) <= EPS))
                assert not bad.any(), f'view {v}: {int(bad.sum())} pixels within 1e-9 of a voxel or depth-step boundary: change the seed'
            i = [np.floor(a) for a in g]
            for a in i:
                ok &= (a >= lo) & (a < hi)
            i = np.stack([np.where(ok, a, 0).astype(np.int64) for a in i], -1)
            dq = np.where(ok, np.floor(ds), 0).astype(np.int64)
            col = img[v][cy, cx].astype(np.int64)
            vv = (((1 << 21) - dq) << 24) | (col[..., 0] << 16) | (col[..., 1] << 8) | col[..., 2]
            key[v] = np.where(ok, pack(i), -1)
            val[v] = np.where(ok, vv, 0)
    return key, val


def fuse(key, val):
    """the table's content after every accepted pixel found a slot -> (keys ascending, val = the max, hits = the count) of the distinct voxels"""
    ok = key >= 0
    keys, inv, cnt = np.unique(key[ok], return_inverse=True, return_counts=True)
    top = np.zeros(len(keys), np.int64)
    np.maximum.at(top, inv.reshape(-1), val[ok])
    return keys, top, cnt.astype(np.int64)


def splat(depth, frames, chw, rays, G, exact=False):
    return fuse(*pixel_records(depth, frames, chw, rays, G, exact))


def select(keys, vals, hits, min_hits=1):
    """es_cloud_mask + es_compact_mask + es_sort_u64: the rows with hits >= min_hits in ascending key order"""
    m = hits >= max(int(min_hits), 0)
    return keys[m], vals[m], hits[m]


def points(keys, vals, hits, cell):
    """-> (xyz (n,3) f32, rgb (n,3) u8, hits (n,) i32) of sorted rows"""
    i = unpack(keys).astype(np.float64)
    xyz = ((i + 0.5) * np.float64(cell)).astype(np.float32).reshape(-1, 3)
    rgb = np.stack([(vals >> 16) & 255, (vals >> 8) & 255, vals & 255], -1).astype(np.uint8).reshape(-1, 3)
    return xyz, rgb, np.minimum(hits, 2 ** 31 - 1).astype(np.int32)


def cloud(depth, frames, chw, rays, G, min_hits=1, exact=False):
    k, v, h = select(*splat(depth, frames, chw, rays, G, exact), min_hits)
    return (k,) + points(k, v, h, G.cell)


def inside(xyz, boxes, grow=0.0, exact=False):
    """-> (n, m) bool: point i inside box j"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
    boxes = np.asarray(boxes, np.float32).reshape(-1, 9)
    out = np.zeros((len(xyz), len(boxes)), bool)
    grow = np.float64(grow)
    for j in range(len(boxes)):
        b = boxes[j].astype(np.float64)
        c, half = b[:3], b[3:6] * 0.5 + grow
        Rm = R.rotation(boxes[j, 6:9])
        dx = xyz - c
        ok = np.ones(len(xyz), bool)
        for k in range(3):
            l = (Rm[0, k] * dx[:, 0] + Rm[1, k] * dx[:, 1]) + Rm[2, k] * dx[:, 2]
            if not exact:
                assert not (np.abs(np.abs(l) - half[k]) <= EPS).any(), f'box {j} axis {k}: a point within 1e-9 of the face: change the seed'
            ok &= (l <= half[k]) & (l >= -half[k])
        out[:, j] = ok
    return out


def label(xyz, boxes, grow=0.0, exact=False):
    """-> (label (n,) i32 = the smallest box index that holds the point or -1, support (m,) i32)"""
    ins = inside(xyz, boxes, grow, exact)
    m = ins.shape[1]
    lab = np.where(ins.any(1), np.argmax(ins, 1), -1).astype(np.int32) if m else np.full(len(ins), -1, np.int32)
    return lab, np.bincount(lab[lab >= 0], minlength=m).astype(np.int32)[:m]


def face_mask(occ, C):
    """occ (X,Y,Z) u8 -> (6XYZ,) int32: element 6 * ((i*Y + j)*Z + k) + f"""
    occ = np.asarray(occ, np.uint8)
    good = (occ >= 1) & (occ.astype(np.int64) < C)
    pad = np.zeros(tuple(s + 2 for s in occ.shape), bool)
    pad[1:-1, 1:-1, 1:-1] = good
    out = np.zeros(occ.shape + (6,), np.int32)
    X, Y, Z = occ.shape
    for f in range(6):
        a, step = f >> 1, 1 if f & 1 else -1
        sl = [slice(1, X + 1), slice(1, Y + 1), slice(1, Z + 1)]
        sl[a] = slice(1 + step, occ.shape[a] + 1 + step)
        out[..., f] = good & ~pad[tuple(sl)]
    return out.reshape(-1)


def face_quads(occ, rmin, size, elements):
    """elements (F,) ascending -> (verts (4F,3) f32, face_label (F,) u8)"""
    occ = np.asarray(occ, np.uint8)
    X, Y, Z = occ.shape
    e = np.asarray(elements, np.int64)
    f, cell = e % 6, e // 6
    idx = np.stack([cell // (Y * Z), (cell // Z) % Y, cell % Z], -1)
    rmin, size = np.asarray(rmin, np.float64), np.asarray(size, np.float64)
    corners = np.asarray(FACE_CORNERS, np.int64)[f]                               # (F, 4)
    bits = np.stack([(corners >> a) & 1 for a in range(3)], -1)                      # (F, 4, 3)
    verts = (rmin + (idx[:, None, :] + bits).astype(np.float64) * size).astype(np.float32).reshape(-1, 3)
    return verts, occ.reshape(-1)[cell].astype(np.uint8)


def mesh(occ, rmin, size, C):
    el = np.flatnonzero(face_mask(occ, C))
    v, fl = face_quads(occ, rmin, size, el)
    return v, np.arange(4 * len(el), dtype=np.int32).reshape(-1, 4), fl


def census(depth, frames, chw, rays, G, exact=False):
    """what a test asserts on the spec's own output so that it cannot pass on an empty cloud -> dict(accepted = the fraction of pixels
    that reach a voxel, pixels = their number, distinct = the voxels, shared = the fraction of voxels that received two or more pixels,
    ties = the voxels whose winner was decided by the colour: another pixel of the voxel shares the winner's 1/256 m step and has a smaller
    packed colour)"""
    key, val = pixel_records(depth, frames, chw, rays, G, exact)
    ok = key >= 0
    keys, inv, cnt = np.unique(key[ok], return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    top = np.zeros(len(keys), np.int64)
    np.maximum.at(top, inv, val[ok])
    rival = (val[ok] >> 24 == top[inv] >> 24) & (val[ok] != top[inv])
    return dict(accepted=float(ok.mean()) if ok.size else 0.0, pixels=int(ok.sum()), distinct=len(keys),
                shared=float((cnt >= 2).sum()) / max(len(keys), 1), ties=len(np.unique(inv[rival])))


def longest_run(keys, cap):
    """the longest cyclic run of occupied slots after the distinct `keys` were inserted by linear probing from es_hash into `cap` slots.
    The SET of occupied slots does not depend on the insertion order, and an insertion probes no further than to the end of the run it
    starts in: a longest run below ES_CLOUD_PROBES proves that no order drops a pixel."""
    keys = np.unique(np.asarray(keys, np.int64))
    assert len(keys) < cap
    full = np.zeros(cap, bool)
    for s in es_hash(keys, cap - 1).tolist():
        while full[s]:
            s = (s + 1) & (cap - 1)
        full[s] = True
    if not full.any():
        return 0
    start = int(np.flatnonzero(~full)[0])
    rolled = np.roll(full, -start)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], rolled.astype(np.int8), [0]])))
    return int((edges[1::2] - edges[::2]).max())


def capacity(distinct):
    """the tests' sizing: the power of two >= 4 * distinct + 2"""
    cap = 2
    while cap < 4 * distinct + 2:
        cap *= 2
    return cap


# ------------------------------------------------------------------------------------------------------------------ populations
def scene(V, H, W, seed, max_depth=6.0):
    """-> (rays (V, 12) f64, depth (V, H, W) f32, extrinsic, intrinsic): scene_map_spec.ring() and its room"""
    E, K = ring(V, H, W)
    rays = R.rays_of(E, K)
    return rays, depth_population(rays, H, W, seed, max_depth), E, K


def cloud_boxes(m, seed, xyz):
    """m boxes over the cloud xyz: first a zero-size box, three overlapping ones (the lowest index must win), a box that holds no point and one
    that holds all (as many as fit), then seeded boxes round points of the cloud"""
    rng = np.random.default_rng(seed)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    lo, hi = (xyz.min(0), xyz.max(0)) if len(xyz) else (np.zeros(3), np.ones(3))
    mid, ext = (lo + hi) / 2, np.maximum(hi - lo, 0.5)
    sp = np.array([[*(mid + 0.0131), 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                   [*mid, *(0.45 * ext), 0.5, 0.2, -0.3],
                   [*(mid + 0.1 * ext), *(0.5 * ext), -0.4, 0.1, 0.2],
                   [*(mid - 0.08 * ext), *(0.4 * ext), 1.0, -0.2, 0.1],
                   [*(hi + 50.0), 1.0, 1.0, 1.0, 0.3, 0.0, 0.0],
                   [*mid, *(4.0 * ext + 1.0), 0.1, 0.05, -0.05]], np.float32)
    out = np.zeros((m, 9), np.float32)
    out[:min(m, len(sp))] = sp[:m]
    for i in range(len(sp), m):
        out[i, :3] = xyz[rng.integers(len(xyz))] + rng.uniform(-0.1, 0.1, 3) if len(xyz) else rng.uniform(-1, 1, 3)
        out[i, 3:6] = rng.uniform(0.05, 0.4, 3) * ext
        out[i, 6:] = rng.uniform(-np.pi, np.pi, 3) * (1.0, 0.3, 0.3)
    return out


def occ_volume(shape, seed, C):
    """labels 0, 1, 2, C - 1, C and 255 (each forced in where the volume has room); a single voxel is C - 1"""
    rng = np.random.default_rng(seed)
    pool = np.array([0, 0, 0, 1, 2, C - 1, C, 255], np.uint8)
    occ = pool[rng.integers(0, len(pool), shape)]
    if occ.size == 1:
        occ[...] = C - 1
    else:
        occ.reshape(-1)[rng.permutation(occ.size)[:4]] = (0, C - 1, C, 255)
    return occ
