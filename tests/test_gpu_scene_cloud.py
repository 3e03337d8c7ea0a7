"""es_cloud_splat / es_cloud_mask / es_cloud_points / es_cloud_label / es_occ_face_mask / es_occ_face_quads (csrc/predict.hip) and
embodiedscan_amd.scene_cloud / inference(cloud=) held to tests/scene_cloud_spec.py ON EVERY BYTE: the table as a set of (key, val, hits),
the sorted rows, xyz / rgb / hits / label / support, vertices, quads and face labels.

Depth (H, W) in {(1, 1), (5, 67), (48, 64)}, frames at the same size and at sizes that do not divide ((3, 5), (50, 130)), both layouts, V in
{1, 3}, cells 0.0316, 0.2507 and 64 m -- at 64 m eight voxels take every pixel, the worst contention at the smallest shape --, cap = the
power of two >= 4 * distinct + 2, min_hits in {1, 2}; depth seed 7, frame seed 8.  Every buffer carries a sentinel tail that must survive,
the inputs stay as they were, the refusals write nothing, two runs are bit-equal.

Asserted on the SPEC's output, so that no test passes on an empty cloud (census_conditions): accepted share >= 1/4 and longest probe run
< 64 in every case; voxels holding two or more pixels >= 1/2 at cells 0.2507 and 64 m (not for the single-pixel depth maps: one voxel,
nothing to share); at least one voxel decided by the colour tie-break for (48, 64) at V = 1 and 3 and (5, 67) at V = 3 at those cells; distinct
voxels >= 0.3 x accepted pixels at cell 0.0316 for (5, 67) and (48, 64), the insertion-heavy case.

Every body is a function of `dev`: tests/test_emu_scene_cloud.py runs the same bodies on the CPU emulator."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_spec as RS
import scene_cloud_spec as S
import test_gpu_scene_map as TM
from test_gpu_scene_map import SENT_F, SENT_I, SENT_K, SENT_U8, _hip, _padded, _same, _st

pytestmark = pytest.mark.gpu
ROOT = TM.ROOT
DEPTHS = [(1, 1), (5, 67), (48, 64)]
CELLS = [0.0316, 0.2507, 64.0]
COUNTS = [0, 1, 63, 64, 65, 300]
GRIDS = [(1, 1, 1), (3, 2, 5), (8, 8, 4)]
N_CLASSES = 5
DEPTH_SEED, FRAME_SEED = 7, 8


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _grid4(G, **kw):
    v = dict(cell=G.cell, z_min=G.z_min, z_max=G.z_max, max_depth=G.max_depth)
    v.update(kw)
    arr = (ctypes.c_double * 4)(*[float(v[k]) for k in ('cell', 'z_min', 'z_max', 'max_depth')])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def empty_table(cap):
    return np.full(cap, -1, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(2, np.int32)


def run_splat(dev, depth, frames, chw, rays, G, cap, table=None, expect=0, dims=None, grid=None, cap_arg=None):
    """one launch on sentinel-tailed buffers -> (tkeys, tvals, thits, counters) numpy (None after a refusal); asserts tails and inputs.
    dims: (V, H, W, h, w) passed instead of the true ones, cap_arg: the cap passed (refusals)"""
    hip = _hip()
    P = hip.P
    V, H, W = depth.shape
    h, w = (frames.shape[2], frames.shape[3]) if chw else (frames.shape[1], frames.shape[2])
    d, db = _padded(dev, depth, torch.float32, SENT_F)
    f, fb = _padded(dev, frames, torch.uint8, SENT_U8)
    r, rb = _padded(dev, rays, torch.float64, SENT_F)
    t0 = empty_table(cap) if table is None else table
    outs = [_padded(dev, a, dt, sent) for a, dt, sent in zip(t0, (torch.int64, torch.int64, torch.int32, torch.int32), (SENT_K, SENT_K, SENT_I, SENT_I))]
    before = [t.clone() for t in (db, fb, rb)]
    outs0 = [b.clone() for _, b in outs]
    arr, gp = _grid4(G, **(grid or {}))
    a = dims or (V, H, W, h, w)
    rc = hip.raw('es_cloud_splat')(P(d), a[0], a[1], a[2], P(f), int(chw), a[3], a[4], P(r), gp, P(outs[0][0]), P(outs[1][0]), P(outs[2][0]),
                                    cap if cap_arg is None else cap_arg, P(outs[3][0]), _st())
    torch.cuda.synchronize()
    assert rc == expect, f'es_cloud_splat: status {rc}, expected {expect}'
    _same((db, fb, rb), before, ('depth', 'frames', 'rays'))
    for (view, buf), sent, name in zip(outs, (SENT_K, SENT_K, SENT_I, SENT_I), ('tkeys', 'tvals', 'thits', 'counters')):
        assert bool((buf[view.numel():] == sent).all()), f'the launch wrote past the end of {name}'
    if rc != 0:
        assert all(torch.equal(b, b0) for (_, b), b0 in zip(outs, outs0)), 'a refused es_cloud_splat wrote something'
        return None
    return tuple(view.cpu().numpy() for view, _ in outs)


def table_set(table):
    """-> (keys ascending, vals, hits) of the occupied slots; the empty ones must be untouched"""
    tk, tv, th, _ = table
    full = tk != -1
    assert not tv[~full].any() and not th[~full].any(), 'an empty slot holds a value or a hit'
    assert len(np.unique(tk[full])) == int(full.sum()), 'a key sits in two slots'
    order = np.argsort(tk[full])
    return tk[full][order], tv[full][order], (th[full][order].astype(np.int64) & 0xffffffff)


def run_rows(dev, table, cell, min_hits=1, expect=0):
    """es_cloud_mask + es_compact_mask + es_sort_u64 + es_cloud_points on sentinel-tailed buffers -> (keys, xyz, rgb, hits) numpy"""
    hip = _hip()
    P = hip.P
    tk, tv, th, _ = table
    cap = len(tk)
    k, kb = _padded(dev, tk, torch.int64, SENT_K)
    v, vb = _padded(dev, tv, torch.int64, SENT_K)
    h, hb = _padded(dev, th, torch.int32, SENT_I)
    before = [t.clone() for t in (kb, vb, hb)]
    mask, mb = _padded(dev, np.full(cap, SENT_I), torch.int32, SENT_I)
    assert hip.raw('es_cloud_mask')(P(k), P(h), cap, min_hits, P(mask), _st()) == 0
    torch.cuda.synchronize()
    assert bool((mb[cap:] == SENT_I).all()), 'es_cloud_mask wrote past the end of the mask'
    want_mask = (tk != -1) & ((th.astype(np.int64) & 0xffffffff) >= min_hits)
    assert np.array_equal(mask.cpu().numpy(), want_mask.astype(np.int32)), 'the mask differs'
    scratch = torch.empty(cap + cap // 2048 + 8, dtype=torch.int32, device=dev)
    sel, src = torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
    cnt = ctypes.c_int(0)
    hip.call('es_compact_mask', P(k), cap, P(mask), P(scratch), P(sel), P(src), ctypes.addressof(cnt), _st())
    n = cnt.value
    assert n == int(want_mask.sum())
    keys, kob = _padded(dev, np.full(n, SENT_K), torch.int64, SENT_K)
    rows = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    if n:
        nb = int(hip.raw('es_sort_scratch_bytes')(n))
        sc = torch.empty(nb, dtype=torch.uint8, device=dev)
        hip.call('es_sort_u64', P(sel), P(src), n, P(sc), nb, P(keys), P(rows), _st())
    xyz, xb = _padded(dev, np.full(n * 3, SENT_F), torch.float32, SENT_F)
    rgb, rb = _padded(dev, np.full(n * 3, SENT_U8), torch.uint8, SENT_U8)
    hits, ib = _padded(dev, np.full(n, SENT_I), torch.int32, SENT_I)
    rc = hip.raw('es_cloud_points')(P(keys), P(rows), n, P(v), P(h), float(cell), P(xyz), P(rgb), P(hits), _st())
    torch.cuda.synchronize()
    assert rc == expect
    _same((kb, vb, hb), before, ('tkeys', 'tvals', 'thits'))
    assert bool((xb[n * 3:] == SENT_F).all()) and bool((rb[n * 3:] == SENT_U8).all()) and bool((ib[n:] == SENT_I).all()), 'a row output overran'
    return keys.cpu().numpy(), xyz.cpu().numpy().reshape(n, 3), rgb.cpu().numpy().reshape(n, 3), hits.cpu().numpy()


def same_rows(got, want, what):
    for name, g, w in zip(('keys', 'xyz', 'rgb', 'hits'), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f'{what}: {name} {g.dtype} {g.shape} against {w.dtype} {w.shape}'
        assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), f'{what}: {name} differs in {int((g != w).sum())} elements'


def population(H, W, V, fh, fw, chw, cell):
    """-> (rays, depth, frames, Grid): the room of scene_map_spec at depth seed 7, frame seed 8; three views are cut in height"""
    rays, depth, _, _ = S.scene(V, H, W, DEPTH_SEED)
    z = (-np.inf, np.inf) if V == 1 else (-0.6, 2.7)
    return rays, depth, S.banded_frames(V, fh, fw, chw, FRAME_SEED), S.Grid(cell, *z)


def census_conditions(H, W, V, cell, cen, keys, cap):
    """the issue's table, on the spec's output"""
    assert cen['accepted'] >= 0.25, cen
    assert S.longest_run(keys, cap) < S.PROBES
    if cell > 0.1 and H * W > 1:
        assert cen['shared'] >= 0.5, cen
        if (H, W) == (48, 64) or ((H, W) == (5, 67) and V == 3):
            assert cen['ties'] >= 1, cen
    if cell < 0.1 and H * W > 1:
        assert cen['distinct'] >= 0.3 * cen['pixels'], cen


def splat_case(dev, H, W, V, fh, fw, chw, cell):
    rays, depth, frames, G = population(H, W, V, fh, fw, chw, cell)
    cen = S.census(depth, frames, chw, rays, G)
    want = S.splat(depth, frames, chw, rays, G)
    cap = S.capacity(len(want[0]))
    print(f'depth {V}x{H}x{W} frames {fh}x{fw} cell {cell}: {cen} cap {cap}')
    census_conditions(H, W, V, cell, cen, want[0], cap)
    table = run_splat(dev, depth, frames, chw, rays, G, cap)
    got = table_set(table)
    for name, g, w in zip(('keys', 'vals', 'hits'), got, want):
        assert np.array_equal(g, w), f'the table {name} differ in {int((g != w).sum()) if g.shape == w.shape else (g.shape, w.shape)}'
    assert (int(table[3][0]), int(table[3][1])) == (cen['pixels'], 0), f'counters {table[3]} against {cen["pixels"]} accepted, 0 dropped'
    again = run_splat(dev, depth, frames, chw, rays, G, cap)
    assert all(np.array_equal(a, b) for a, b in zip(table_set(again), got)) and np.array_equal(again[3], table[3]), 'two runs differ'
    if V > 1:                                                   # the views one by one, last first, onto the growing table
        acc = None
        for v in reversed(range(V)):
            acc = run_splat(dev, depth[v:v + 1], frames[v:v + 1], chw, rays[v:v + 1], G, cap, table=acc)
        assert all(np.array_equal(a, b) for a, b in zip(table_set(acc), got)) and np.array_equal(acc[3], table[3]), 'the views one by one differ'
    for min_hits in (1, 2):
        k, v, h = S.select(*want, min_hits)
        same_rows(run_rows(dev, table, cell, min_hits), (k,) + S.points(k, v, h, cell), f'min_hits {min_hits}')
        if min_hits == 2 and cell > 0.1 and H * W > 1:
            assert 0 < len(k) <= len(want[0])
    return table, want


@pytest.mark.parametrize('cell', CELLS)
@pytest.mark.parametrize('H,W', DEPTHS)
def test_depth_shapes_and_cells(dev, H, W, cell):
    for V, (fh, fw), chw in ((1, (H, W), 1), (3, (3, 5), 0), (3, (50, 130), 1)):
        splat_case(dev, H, W, V, fh, fw, chw, cell)


def test_both_layouts_give_one_cloud(dev):
    rays, depth, _, G = population(48, 64, 3, 50, 130, 0, 0.2507)
    hwc = S.banded_frames(3, 50, 130, 0, FRAME_SEED)
    chw = np.ascontiguousarray(hwc.transpose(0, 3, 1, 2))
    want = S.splat(depth, hwc, 0, rays, G)
    cap = S.capacity(len(want[0]))
    a, b = table_set(run_splat(dev, depth, hwc, 0, rays, G, cap)), table_set(run_splat(dev, depth, chw, 1, rays, G, cap))
    assert all(np.array_equal(x, y) and np.array_equal(x, w) for x, y, w in zip(a, b, want)) and len(want[0]) > 100


def test_one_cloud_any_order(dev):
    """the views added one by one, reversed, and all at once give bit-equal sorted rows"""
    rays, depth, frames, G = population(48, 64, 3, 50, 130, 1, 0.0316)
    want = S.cloud(depth, frames, 1, rays, G)
    cap = S.capacity(len(want[0]))
    rows = []
    for order in ((0, 1, 2), (2, 1, 0), None):
        if order is None:
            table = run_splat(dev, depth, frames, 1, rays, G, cap)
        else:
            table = None
            for v in order:
                table = run_splat(dev, depth[v:v + 1], frames[v:v + 1], 1, rays[v:v + 1], G, cap, table=table)
        rows.append(run_rows(dev, table, G.cell))
        same_rows(rows[-1], want, f'order {order}')
    assert len(want[0]) > 1000


@pytest.mark.parametrize('cap', [8, 128])
def test_a_table_that_is_too_small_reports_it(dev, cap):
    """a reported overflow, not a fault: whatever the arrival order, what the table holds is true and every pixel is accounted for"""
    rays, depth, frames, G = population(48, 64, 3, 50, 130, 1, 0.0316)
    keys, vals, hits = S.splat(depth, frames, 1, rays, G)
    cen = S.census(depth, frames, 1, rays, G)
    assert len(keys) > 8000
    table = run_splat(dev, depth, frames, 1, rays, G, cap)
    k, v, h = table_set(table)
    accepted, dropped = (int(x) & 0xffffffff for x in table[3])
    assert dropped > 0
    at = np.searchsorted(keys, k)
    assert (at < len(keys)).all() and np.array_equal(keys[np.minimum(at, len(keys) - 1)], k), 'a stored key is no voxel of the spec'
    assert (v <= vals[at]).all() and (h <= hits[at]).all() and (h >= 1).all()
    assert int(h.sum()) == accepted and accepted + dropped == cen['pixels']
    if cap == 8:
        assert len(k) == 8, 'a slot of the full table stayed empty'


def test_scene_cloud_full(dev):
    from embodiedscan_amd import scene_cloud as SC
    V, H, W = 3, 48, 64
    rays, depth, E, K = S.scene(V, H, W, DEPTH_SEED)
    frames = S.banded_frames(V, 50, 130, 1, FRAME_SEED)
    cl = SC.SceneCloud(dev, cell=0.0316, capacity=128, max_depth=6.0)
    cl.add(torch.from_numpy(depth).to(dev), torch.from_numpy(frames).to(dev), E.astype(np.float64), K.astype(np.float64))
    with pytest.raises(SC.CloudFull) as err:
        cl.points()
    e = err.value
    assert e.dropped > 0 and e.capacity == 128 and e.occupied == 128 and e.fit_capacity >= 2 * 8000 and e.fit_cell > 0.0316
    assert str(e.dropped) in str(e) and 'capacity=' in str(e) and 'cell=' in str(e)
    big = SC.SceneCloud(dev, cell=0.0316, capacity=e.fit_capacity, max_depth=6.0)
    big.add(torch.from_numpy(depth).to(dev), torch.from_numpy(frames).to(dev), E.astype(np.float64), K.astype(np.float64))
    assert big.points()[0].shape[0] > 8000, 'the capacity the message names does not fit'


# ------------------------------------------------------------------------------------------------------------------ labels
@functools.lru_cache(maxsize=None)
def label_cloud():
    """the points every label case shares: the (48, 64), V = 3 room at 0.0316 m, every seventh row of it (1 279 points: five workgroups)"""
    rays, depth, frames, G = population(48, 64, 3, 50, 130, 1, 0.0316)
    xyz = S.cloud(depth, frames, 1, rays, G)[1][::7].copy()
    xyz.setflags(write=False)
    return xyz


def run_label(dev, xyz, boxes, grow=0.0, expect=0, n=None, m=None):
    hip = _hip()
    P = hip.P
    nn, mm = len(xyz), len(boxes)
    p, pb = _padded(dev, np.array(xyz, np.float32), torch.float32, SENT_F)
    b, bb = _padded(dev, np.array(boxes, np.float32).reshape(mm, 9), torch.float32, SENT_F)
    lab, lb = _padded(dev, np.full(nn, SENT_I), torch.int32, SENT_I)
    sup, sb = _padded(dev, np.full(mm, SENT_I), torch.int32, SENT_I)
    before = [t.clone() for t in (pb, bb)]
    rc = hip.raw('es_cloud_label')(P(p), nn if n is None else n, P(b), mm if m is None else m, float(grow), P(lab), P(sup), _st())
    torch.cuda.synchronize()
    assert rc == expect, f'es_cloud_label: status {rc}, expected {expect}'
    _same((pb, bb), before, ('xyz', 'boxes'))
    assert bool((lb[nn:] == SENT_I).all()) and bool((sb[mm:] == SENT_I).all()), 'the launch wrote past the end of an output'
    if rc != 0:
        assert bool((lb == SENT_I).all()) and bool((sb == SENT_I).all()), 'a refused es_cloud_label wrote something'
        return None, None
    return lab.cpu().numpy(), sup.cpu().numpy()


@pytest.mark.parametrize('grow', [0.0, 0.05])
@pytest.mark.parametrize('m', COUNTS)
def test_labels_and_support(dev, m, grow):
    xyz = label_cloud()
    boxes = S.cloud_boxes(m, 40 + m, xyz)
    assert len(xyz) > 1024
    last = np.concatenate([boxes[:5], boxes[6:], boxes[5:6]]) if m >= 6 else boxes[::-1].copy()
    for bx in (boxes, last):                                    # `last`: the box that holds all comes last, so every chunk decides
        wl, ws = S.label(xyz, bx, grow)
        gl, gs = run_label(dev, xyz, bx, grow)
        assert np.array_equal(gl, wl), f'{int((gl != wl).sum())} labels differ'
        assert np.array_equal(gs, ws) and int(ws.sum()) == int((wl >= 0).sum())
        a2, s2 = run_label(dev, xyz, bx, grow)
        assert np.array_equal(a2, gl) and np.array_equal(s2, gs), 'two runs differ'
    if m >= 6:
        ins = S.inside(xyz, boxes, grow)
        assert (ins.sum(1) >= 1).mean() >= 0.25 and (ins.sum(1) >= 2).mean() >= 0.1, 'the boxes hold too few points'
        wl, ws = S.label(xyz, boxes, grow)
        assert not ins[:, 0].any() and not ins[:, 4].any() and ins[:, 5].all(), 'the zero-size, the empty or the all-holding box'
        three = ins[:, 1:4].sum(1) >= 2
        assert three.any() and (wl[three] == 1 + np.argmax(ins[three, 1:4], 1)).all(), 'the lowest index must win'
        assert m < 65 or len(np.unique(S.label(xyz, last, grow)[0] // S.CHUNK)) >= 2, 'no label beyond the first chunk of the LDS staging'
    if m == 0:
        assert (wl == -1).all() and ws.shape == (0,)


# ------------------------------------------------------------------------------------------------------------------ faces
def run_faces(dev, occ, rmin, size, C, expect=0, vdims=None):
    """es_occ_face_mask + es_compact_mask + es_occ_face_quads -> (mask, verts, face_label) numpy"""
    hip = _hip()
    P = hip.P
    X, Y, Z = occ.shape
    ne = 6 * X * Y * Z
    o, ob = _padded(dev, occ, torch.uint8, SENT_U8)
    before = ob.clone()
    mask, mb = _padded(dev, np.full(ne, SENT_I), torch.int32, SENT_I)
    a = vdims or (X, Y, Z)
    rc = hip.raw('es_occ_face_mask')(P(o), a[0], a[1], a[2], C, P(mask), _st())
    torch.cuda.synchronize()
    assert rc == expect, f'es_occ_face_mask: status {rc}, expected {expect}'
    assert torch.equal(ob, before) and bool((mb[ne:] == SENT_I).all())
    if rc != 0:
        assert bool((mb == SENT_I).all()), 'a refused es_occ_face_mask wrote something'
        return None
    scratch = torch.empty(ne + ne // 2048 + 8, dtype=torch.int32, device=dev)
    ids = torch.zeros(ne, dtype=torch.int64, device=dev)
    sel, src = torch.empty(ne, dtype=torch.int64, device=dev), torch.empty(ne, dtype=torch.int32, device=dev)
    cnt = ctypes.c_int(0)
    hip.call('es_compact_mask', P(ids), ne, P(mask), P(scratch), P(sel), P(src), ctypes.addressof(cnt), _st())
    F = cnt.value
    verts, vb = _padded(dev, np.full(F * 12, SENT_F), torch.float32, SENT_F)
    fl, fb = _padded(dev, np.full(F, SENT_U8), torch.uint8, SENT_U8)
    vol = (ctypes.c_double * 6)(*[float(x) for x in rmin], *[float(x) for x in size])
    assert hip.raw('es_occ_face_quads')(P(o), X, Y, Z, ctypes.cast(vol, ctypes.c_void_p), P(src), F, P(verts), P(fl), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ob, before) and bool((vb[F * 12:] == SENT_F).all()) and bool((fb[F:] == SENT_U8).all())
    return mask.cpu().numpy(), verts.cpu().numpy().reshape(F * 4, 3), fl.cpu().numpy()


def faces_case(dev, occ, rmin, size, C):
    want_mask = S.face_mask(occ, C)
    wv, wq, wl = S.mesh(occ, rmin, size, C)
    mask, verts, fl = run_faces(dev, occ, rmin, size, C)
    assert np.array_equal(mask, want_mask), f'{int((mask != want_mask).sum())} face elements differ'
    assert np.array_equal(verts.view(np.uint32), wv.view(np.uint32)) and np.array_equal(fl, wl)
    return want_mask, wv, wl


@pytest.mark.parametrize('shape', GRIDS)
def test_exposed_faces(dev, shape):
    rmin, size = np.array([-0.7, -2.6, 0.013]), np.array([3.0, 2.0, 1.0]) / np.array(shape)
    X, Y, Z = shape
    occ = S.occ_volume(shape, 20 + X, N_CLASSES)
    mask, verts, fl = faces_case(dev, occ, rmin, size, N_CLASSES)
    assert mask.any() and ((fl >= 1) & (fl < N_CLASSES)).all()
    again = run_faces(dev, occ, rmin, size, N_CLASSES)
    assert np.array_equal(again[0], mask) and np.array_equal(again[1].view(np.uint32), verts.view(np.uint32)), 'two runs differ'
    # every quad is counter-clockwise seen from outside: its normal points away from the voxel's centre
    quad = verts.reshape(-1, 4, 3).astype(np.float64)
    normal = np.cross(quad[:, 1] - quad[:, 0], quad[:, 2] - quad[:, 0])
    el = np.flatnonzero(mask)
    cell = el // 6
    centre = rmin + (np.stack([cell // (Y * Z), (cell // Z) % Y, cell % Z], -1) + 0.5) * size
    assert (np.einsum('ij,ij->i', normal, quad.mean(1) - centre) > 0).all(), 'a quad faces inward'
    full = np.full(shape, N_CLASSES - 1, np.uint8)                                  # a full volume: only the boundary
    m, _, _ = faces_case(dev, full, rmin, size, N_CLASSES)
    assert int(m.sum()) == 2 * (X * Y + Y * Z + X * Z)
    for dead in (0, N_CLASSES, 255):                                              # no label at all: no face
        m, v, _ = faces_case(dev, np.full(shape, dead, np.uint8), rmin, size, N_CLASSES)
        assert not m.any() and v.shape == (0, 3)
    i, j, k = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing='ij')
    board = np.where((i + j + k) % 2 == 0, 2, 0).astype(np.uint8)                   # a checkerboard: no filled voxel touches another
    m, _, _ = faces_case(dev, board, rmin, size, N_CLASSES)
    assert int(m.sum()) == 6 * int((board != 0).sum())


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(dev):
    rays, depth, frames, G = population(5, 67, 1, 3, 5, 0, 0.2507)
    V, H, W, h, w = 1, 5, 67, 3, 5
    nan, inf = float('nan'), float('inf')
    for kw in (dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=inf), dict(z_min=1.0, z_max=1.0), dict(z_min=2.0, z_max=1.0), dict(z_min=nan),
               dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=4096.5), dict(max_depth=nan), dict(max_depth=inf)):
        run_splat(dev, depth, frames, 0, rays, G, 64, expect=-4, grid=kw)
    for cap_arg in (0, 1, 3, 48, -64, (1 << 30) + 1):
        run_splat(dev, depth, frames, 0, rays, G, 64, expect=-4, cap_arg=cap_arg)
    for dims in ((65536, H, W, h, w), (V, 0, W, h, w), (V, H, 4097, h, w), (V, H, W, 0, w), (V, H, W, h, 4097)):
        run_splat(dev, depth, frames, 0, rays, G, 64, expect=-4, dims=dims)
    run_splat(dev, depth, frames, 0, rays, G, 64, expect=-5, dims=(-1, H, W, h, w))
    none = run_splat(dev, depth, frames, 0, rays, G, 64, dims=(0, H, W, h, w))                # V = 0: not an error, nothing written
    assert (none[0] == -1).all() and not none[1].any() and not none[2].any() and not none[3].any()
    legal = run_splat(dev, depth, frames, 0, rays, G, 512, grid=dict(z_min=-inf, z_max=inf, max_depth=4096.0))   # infinite cuts are legal
    assert int(legal[3][0]) > 0
    hip = _hip()
    k, kb = _padded(dev, np.full(8, -1), torch.int64, SENT_K)
    h32, _ = _padded(dev, np.zeros(8), torch.int32, SENT_I)
    mask, mb = _padded(dev, np.full(8, SENT_I), torch.int32, SENT_I)
    for cap_arg, mh in ((6, 1), (0, 1), (8, -1)):
        assert hip.raw('es_cloud_mask')(hip.P(k), hip.P(h32), cap_arg, mh, hip.P(mask), _st()) == -4
    out = [_padded(dev, np.full(24, SENT_F), torch.float32, SENT_F), _padded(dev, np.full(24, SENT_U8), torch.uint8, SENT_U8),
           _padded(dev, np.full(8, SENT_I), torch.int32, SENT_I)]
    for n, cell, rc in ((8, 0.0, -4), (8, nan, -4), (8, inf, -4), (-1, 0.1, -5), (0, 0.1, 0)):
        assert hip.raw('es_cloud_points')(hip.P(k), hip.P(h32), n, hip.P(k), hip.P(h32), cell, hip.P(out[0][0]), hip.P(out[1][0]), hip.P(out[2][0]), _st()) == rc
    torch.cuda.synchronize()
    assert bool((mb == SENT_I).all()) and all(bool((b == s).all()) for (_, b), s in zip(out, (SENT_F, SENT_U8, SENT_I))), 'a refused call wrote something'
    xyz = label_cloud()[:70]
    boxes = S.cloud_boxes(6, 1, xyz)
    for kw in (dict(grow=-0.01), dict(grow=nan), dict(grow=inf), dict(m=65536)):
        run_label(dev, xyz, boxes, **dict(dict(expect=-4), **kw))
    for kw in (dict(n=-1), dict(m=-1)):
        run_label(dev, xyz, boxes, expect=-5, **kw)
    lab, sup = run_label(dev, xyz[:0], boxes)                                                 # n = 0: support is zeroed, nothing else
    assert lab.shape == (0,) and not sup.any()
    occ = S.occ_volume((3, 2, 5), 1, N_CLASSES)
    for kw in (dict(C=0), dict(C=257), dict(vdims=(0, 2, 5)), dict(vdims=(3, -1, 5)), dict(vdims=(1024, 1024, 1024))):
        run_faces(dev, occ, np.zeros(3), np.ones(3), kw.pop('C', N_CLASSES), expect=-4, **kw)


# ------------------------------------------------------------------------------------------------------------------ the public interface
def test_scene_cloud_module_against_the_spec(dev):
    from embodiedscan_amd import scene_cloud as SC
    from embodiedscan_amd.render import class_palette
    V, H, W = 3, 48, 64
    rays, depth, Ec, Kc = S.scene(V, H, W, DEPTH_SEED)
    E, K = Ec.astype(np.float64), Kc.astype(np.float64)
    frames = S.banded_frames(V, 50, 130, 1, FRAME_SEED)
    G = S.Grid(0.2507, -0.6, 2.7, 6.0)
    cl = SC.SceneCloud(dev, cell=0.2507, capacity=4096, z=(-0.6, 2.7), max_depth=6.0)
    assert cl.state_bytes() == 4096 * 20 + 8
    d, f = torch.from_numpy(depth).to(dev), torch.from_numpy(frames).to(dev)
    assert cl.add(d, f, E, K) is cl
    for min_hits in (1, 2):
        want = S.cloud(depth, frames, 1, rays, G, min_hits)
        xyz, rgb, hits = cl.points(min_hits)
        assert (xyz.dtype, rgb.dtype, hits.dtype) == (torch.float32, torch.uint8, torch.int32) and xyz.device.type == dev.type
        same_rows((cl.keys.cpu().numpy(), xyz.cpu().numpy(), rgb.cpu().numpy(), hits.cpu().numpy()), want, f'min_hits {min_hits}')
    assert cl.pixel_counts() == (S.census(depth, frames, 1, rays, G)['pixels'], 0)
    cl.clear()
    assert cl.points()[0].shape == (0, 3) and cl.pixel_counts() == (0, 0)
    for v in (2, 0, 1):
        cl.add(d[v:v + 1], f[v:v + 1], E[v:v + 1], K[v:v + 1], layout='chw')
    want = S.cloud(depth, frames, 1, rays, G)
    xyz, rgb, hits = cl.points()
    same_rows((cl.keys.cpu().numpy(), xyz.cpu().numpy(), rgb.cpu().numpy(), hits.cpu().numpy()), want, 'the views one by one')
    boxes = S.cloud_boxes(70, 3, want[1])
    lab, sup = cl.label(xyz, torch.from_numpy(boxes).to(dev), grow=0.05)
    wl, ws = S.label(want[1], boxes, 0.05)
    assert lab.dtype == sup.dtype == torch.int32 and np.array_equal(lab.cpu().numpy(), wl) and np.array_equal(sup.cpu().numpy(), ws)
    lab0, sup0 = SC.label(xyz, torch.zeros((0, 9), device=dev))
    assert bool((lab0 == -1).all()) and sup0.shape == (0,)
    occ, pr, pal = S.occ_volume((8, 8, 4), 4, N_CLASSES), (-0.7, -2.6, 0.0, 2.3, -0.6, 1.0), class_palette(N_CLASSES)
    wide = torch.from_numpy(occ.astype(np.int64)).to(dev)
    wide[0, 0, 0], wide[1, 0, 0] = 300, -2
    ref = occ.copy()
    ref[0, 0, 0] = ref[1, 0, 0] = 0
    verts, quads, fl, colors = SC.occupancy_mesh(wide, pr, pal)
    wv, wq, wfl = S.mesh(ref, np.array(pr[:3]), (np.array(pr[3:]) - np.array(pr[:3])) / np.array(occ.shape), N_CLASSES)
    assert np.array_equal(verts.cpu().numpy().view(np.uint32), wv.view(np.uint32)) and np.array_equal(quads.cpu().numpy(), wq)
    assert np.array_equal(fl.cpu().numpy(), wfl) and np.array_equal(colors.cpu().numpy(), np.repeat(pal[wfl], 4, 0)) and len(wfl) > 20
    assert (quads.dtype, fl.dtype, colors.dtype) == (torch.int32, torch.uint8, torch.uint8)
    empty = SC.occupancy_mesh(torch.zeros((3, 2, 5), dtype=torch.uint8, device=dev), pr, pal)
    assert [tuple(t.shape) for t in empty] == [(0, 3), (0, 4), (0,), (0, 3)]
    z9 = torch.zeros((2, 9), device=dev)
    for bad, msg in ((lambda: cl.add(d.double(), f, E, K), 'float32'), (lambda: cl.add(d, f.float(), E, K), 'uint8'),
                     (lambda: cl.add(d, f[:2], E, K), '2 frames'), (lambda: cl.add(d, f, E[:2], K), 'extrinsic'),
                     (lambda: cl.add(d, f, E, K, layout='hwc'), 'layout'), (lambda: cl.points(min_hits=-1), 'min_hits'),
                     (lambda: cl.label(xyz.double(), z9), 'float32'), (lambda: cl.label(xyz, z9[:, :8]), r'\(m, 9\)'),
                     (lambda: cl.label(xyz, z9, grow=-1.0), 'grow'), (lambda: cl.label(xyz, z9, grow=float('nan')), 'grow'),
                     (lambda: cl.label(xyz, torch.zeros((65536, 9), device=dev)), '65535'),
                     (lambda: SC.occupancy_mesh(wide.float(), pr, pal), 'integer'), (lambda: SC.occupancy_mesh(wide, (0, 0, 0, 1, 1, 0), pal), 'point_cloud_range'),
                     (lambda: SC.occupancy_mesh(wide, pr, np.zeros((0, 3), np.uint8)), 'palette'),
                     (lambda: SC.SceneCloud(dev, cell=0.0), 'cell'), (lambda: SC.SceneCloud(dev, capacity=1000), 'capacity'),
                     (lambda: SC.SceneCloud(dev, capacity=1), 'capacity'), (lambda: SC.SceneCloud(dev, capacity=8, z=(1.0, 1.0)), 'z cut'),
                     (lambda: SC.SceneCloud(dev, capacity=8, max_depth=5000.0), 'max_depth')):
        with pytest.raises(ValueError, match=msg):
            bad()
    if dev.type == 'cuda':
        with pytest.raises(ValueError, match='depth on cpu'):
            cl.add(d.cpu(), f, E, K)
        with pytest.raises(ValueError, match='boxes on cpu'):
            cl.label(xyz, z9.cpu())
    again = cl.points()
    assert torch.equal(again[0], xyz) and torch.equal(again[2], hits), 'a refused call changed the cloud'


# ------------------------------------------------------------------------------------------------------------------ end to end
def _spec_cloud(I, det, dscan, doc, n_views):
    """the rows scene.ply must hold over the first n_views frames, from the scan and cloud.json alone"""
    E, K = I.depth_matrices(dscan)
    rays = RS.rays_of(E, K)
    v = slice(0, n_views)
    G = S.Grid(doc['cell'], max_depth=8.0)
    return S.cloud(dscan['depth'].cpu().numpy()[v], dscan['img'].cpu().numpy()[v], 1, rays[v], G, doc['min_hits'])


def _check_files(I, SC, det, dscan, out, res, n_views, sfx='', track=False):
    """scene<sfx>.ply + boxes<sfx>.ply / occupancy<sfx>.ply + cloud.json in `out` against the spec under the prediction `res` -> rows"""
    from embodiedscan_amd.render import class_palette
    doc = json.load(open(os.path.join(out, 'cloud.json')))
    keys, xyz, rgb, hits = _spec_cloud(I, det, dscan, doc, n_views)
    ply = SC.read_ply(os.path.join(out, f'scene{sfx}.ply'))
    vx = ply['vertex']
    assert list(vx) == ['x', 'y', 'z', 'red', 'green', 'blue', 'hits', 'label', 'instance'] and ply['face'] is None and ply['edge'] is None
    got_xyz = np.stack([vx['x'], vx['y'], vx['z']], -1)
    assert np.array_equal(got_xyz.view(np.uint32), xyz.view(np.uint32)), 'scene.ply: the positions differ'
    assert np.array_equal(np.stack([vx['red'], vx['green'], vx['blue']], -1), rgb) and np.array_equal(vx['hits'], hits)
    if not sfx:                                                  # (cloud.json describes the files written last: the un-numbered ones)
        assert doc['rows'] == len(xyz) and doc['counters'][1] == 0 and (doc['min_hits'] > 1 or doc['counters'][0] == int(hits.sum()))
    pal = I.scene_palette(det)
    assert doc['class_colors'] == pal.tolist() and len(doc['class_names']) == len(pal)
    if torch.is_tensor(res):
        assert (vx['label'] == -1).all() and (vx['instance'] == -1).all()
        occ = res.cpu().numpy()
        pr = np.asarray(det.point_cloud_range, np.float64)
        wv, wq, wl = S.mesh(np.where((occ < 0) | (occ > 255), 0, occ).astype(np.uint8), pr[:3], (pr[3:] - pr[:3]) / np.array(occ.shape, np.float64), len(pal))
        mesh = SC.read_ply(os.path.join(out, f'occupancy{sfx}.ply'))
        mv = mesh['vertex']
        assert list(mv) == ['x', 'y', 'z', 'red', 'green', 'blue'] and np.array_equal(mesh['face'], wq) and (sfx or doc['faces'] == len(wq))
        assert np.array_equal(np.stack([mv['x'], mv['y'], mv['z']], -1).view(np.uint32), wv.view(np.uint32))
        assert np.array_equal(np.stack([mv['red'], mv['green'], mv['blue']], -1), np.repeat(pal[wl], 4, 0))
        return len(xyz)
    boxes = res.bboxes_3d.tensor.cpu().numpy()
    labels = res.labels_3d.cpu().numpy()
    wl, ws = S.label(xyz, boxes, 0.0)
    ids = res.track_ids.cpu().numpy() if track else np.arange(len(boxes))
    assert np.array_equal(vx['label'], np.where(wl >= 0, labels[np.maximum(wl, 0)] if len(boxes) else 0, -1).astype(np.int32)), 'the labels differ'
    assert np.array_equal(vx['instance'], np.where(wl >= 0, ids[np.maximum(wl, 0)] if len(boxes) else 0, -1).astype(np.int32)), 'the instances differ'
    assert (sfx or doc['support'] == ws.tolist()) and res.cloud_support.cpu().tolist() == ws.tolist()
    colors = class_palette(257)[1:][ids % 256] if track else pal[np.clip(labels, 0, len(pal) - 1)]
    bv, be, bc = SC.box_edges(boxes, colors)
    wire = SC.read_ply(os.path.join(out, f'boxes{sfx}.ply'))
    assert np.array_equal(np.stack([wire['vertex'][a] for a in 'xyz'], -1), bv.astype(np.float32)) and len(bv) == 8 * len(boxes)
    assert np.array_equal(wire['edge'][0], be) and np.array_equal(wire['edge'][1], bc)
    return len(xyz)


def _room(I, dev, demo, pipe, cell=0.125):
    """the voxel centres of the demo folder's four frames, from the spec"""
    import test_gpu_inference as TI
    det = TM.stand_in(dev, 'det3d', None)
    return _spec_cloud(I, det, TI._scan(det, demo, pipe), dict(cell=cell, min_hits=1), 4)[1].astype(np.float64)


def _room_boxes(dev, room, n=6):
    """the box list of test_gpu_scene_map's stand-in detector behind a box round the middle of the room's cloud and before one that holds all
    of it, so that points lie in one box, in several, and in none but the last"""
    from embodiedscan_amd.structures import EulerDepthInstance3DBoxes, InstanceData
    small = TM._stand_in_boxes(dev)
    lo, hi = np.percentile(room, [20, 80], 0)
    mid, ext = (room.min(0) + room.max(0)) / 2, room.max(0) - room.min(0)
    extra = torch.tensor([[*np.median(room, 0), *(hi - lo + 0.2), 0.3, 0.0, 0.0], [*mid, *(1.6 * ext + 1.0), -0.2, 0.0, 0.0]], dtype=torch.float32, device=dev)
    boxes = torch.cat([extra[:1], small.bboxes_3d.tensor, extra[1:]])[:n]
    return InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(boxes.contiguous()), scores_3d=torch.linspace(0.9, 0.4, 6, device=dev)[:n].contiguous(),
                        labels_3d=torch.tensor([2, 0, 3, 1, 9, 1], device=dev)[:n])


def test_run_scene_exports_a_given_prediction(dev, tmp_path_factory, tmp_path, launch_log=None):
    """run_scene(cloud=) end to end on the demo folder with the prediction given: boxes and a volume"""
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd import scene_cloud as SC
    demo = TM._demo(tmp_path_factory)
    scene, pipe = os.path.join(demo, 'room'), TM._stand_in_pipeline()
    vol = torch.from_numpy(TM.occ_volume((8, 8, 4), 3).astype(np.int64) % 7).to(dev)
    for kind, pred in (('det3d', _room_boxes(dev, _room(I, dev, demo, pipe))), ('occ', vol)):
        det = TM.stand_in(dev, kind, pred)
        if launch_log is not None:
            launch_log()
        plain = I.run_scene(det, scene, pipe, seed=TI.SEED, filter=None)
        if launch_log is not None:
            assert not any(k.startswith(('k_cloud_', 'k_occ_face_')) for k in launch_log()), 'cloud=None launched a cloud kernel'
        out = str(tmp_path / kind)
        got = I.run_scene(det, scene, pipe, seed=TI.SEED, filter=None, cloud=out, cloud_cell=0.125, cloud_min_hits=1 if kind == 'occ' else 2)
        if launch_log is not None:
            want = {'k_cloud_splat', 'k_cloud_mask', 'k_cloud_points'} | ({'k_occ_face_mask', 'k_occ_face_quads'} if kind == 'occ' else {'k_cloud_label'})
            assert want <= launch_log()
        assert got[0] is plain[0] is pred
        assert sorted(os.listdir(out)) == sorted(['cloud.json', 'occupancy.ply' if kind == 'occ' else 'boxes.ply', 'scene.ply'])
        dscan = TI._scan(det, demo, pipe)
        rows = _check_files(I, SC, det, dscan, out, pred, 4)
        assert rows > 200, 'the recording reaches almost no voxel'
        if kind == 'det3d':
            sup = pred.cloud_support.cpu().tolist()
            assert sup[0] > 0 and sup[-1] > 0 and sum(sup) == rows, f'the support {sup} of {rows} points'


def test_walk_clouds_grow_frame_by_frame(dev, tmp_path_factory, tmp_path, launch_log=None):
    """walk_scene(cloud=, cloud_every=1) on a scripted session: cont-det3d without and with track=, an occupancy volume per frame, and
    cloud=None's launch log.  Cloud t equals a fresh cloud of frames 0 .. t under the prediction of prefix t; the un-numbered files are the
    last prefix's."""
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd import scene_cloud as SC
    demo = TM._demo(tmp_path_factory)
    scene = os.path.join(demo, 'room')
    vol = torch.from_numpy(TM.occ_volume((8, 8, 4), 3).astype(np.int64) % 7).to(dev)
    room = _room(I, dev, demo, TM._walk_pipeline('cont-det3d'))
    scripts = {'cont-det3d': lambda t: _room_boxes(dev, room, t + 3), 'cont-occ': lambda t: torch.roll(vol, t, 0)}
    for name, kind, track in (('plain', 'cont-det3d', None), ('tracked', 'cont-det3d', dict()), ('occ', 'cont-occ', None)):
        det, pipe = TM.walking_stand_in(dev, kind, scripts[kind]), TM._walk_pipeline(kind)
        if launch_log is not None:
            launch_log()
        plain = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=None, track=track))
        if launch_log is not None:
            assert not any(k.startswith(('k_cloud_', 'k_occ_face_')) for k in launch_log()), f'{name}: cloud=None launched a cloud kernel'
        out = str(tmp_path / name)
        got = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=None, track=track, cloud=out, cloud_cell=0.125, cloud_every=1))
        assert [t for t, _ in got] == [t for t, _ in plain] == [0, 1, 2, 3]
        second = 'occupancy' if kind == 'cont-occ' else 'boxes'
        assert sorted(os.listdir(out)) == sorted(['cloud.json', 'scene.ply', f'{second}.ply'] + [f'{s}_{t:04d}.ply' for s in ('scene', second) for t in range(4)])
        dscan = TI._scan(det, demo, pipe)
        rows = []
        for (t, g), (_, p) in zip(got, plain):
            if kind == 'cont-occ':
                assert torch.equal(g, p), f'{name} prefix {t}: cloud= changed the volume'
            else:
                assert torch.equal(g.bboxes_3d.tensor, p.bboxes_3d.tensor) and torch.equal(g.labels_3d, p.labels_3d) and 'cloud_support' not in p
            rows.append(_check_files(I, SC, det, dscan, out, g, t + 1, f'_{t:04d}', track is not None))
        assert rows == sorted(rows) and rows[-1] > rows[0] > 0, f'{name}: the cloud does not grow: {rows}'
        _check_files(I, SC, det, dscan, out, got[-1][1], 4, '', track is not None)
        if name != 'plain':
            continue
        final = str(tmp_path / (name + '_final'))                              # cloud_every = 0: only the un-numbered files
        last = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=None, track=track, cloud=final, cloud_cell=0.125))
        assert sorted(os.listdir(final)) == sorted(['cloud.json', f'{second}.ply', 'scene.ply'])
        _check_files(I, SC, det, dscan, final, last[-1][1], 4, '', track is not None)
        if kind == 'cont-det3d':
            assert [('cloud_support' in r) for _, r in last] == [False, False, False, True]
            rec = I._record(last[-1][1], ['a', 'b', 'c', 'd'] + [f'c{i}' for i in range(10)], t=3)
            assert rec['support'] == last[-1][1].cloud_support.cpu().tolist() and 'support' not in I._record(plain[-1][1], ['a'] * 14)


def _model_case(dev, tmp_path_factory, tmp_path, det, pipe, walk, flt=None):
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd import scene_cloud as SC
    demo = TM._demo(tmp_path_factory)
    scene = os.path.join(demo, 'room')
    out = str(tmp_path / 'cloud')
    kw = dict(seed=TI.SEED) if flt is None else dict(seed=TI.SEED, filter=flt)
    if walk:
        plain = [(t, v.clone() if torch.is_tensor(v) else v) for t, v in I.walk_scene(det, scene, pipe, **kw)]
        got = [(t, v.clone() if torch.is_tensor(v) else v) for t, v in I.walk_scene(det, scene, pipe, cloud=out, cloud_cell=0.1, cloud_every=2, **kw)]
        plain, got = [v for _, v in plain], [v for _, v in got]
    else:
        plain = I.run_scene(det, scene, pipe, **kw)
        got = I.run_scene(det, scene, pipe, cloud=out, cloud_cell=0.1, **kw)
    for g, p in zip(got, plain):
        if torch.is_tensor(g):
            assert torch.equal(g, p), 'cloud= changed the volume'
        else:
            TI._same_instances(g, p, 'cloud= changed the instances')
    dscan = TI._scan(det, demo, pipe)
    assert _check_files(I, SC, det, dscan, out, got[-1], 4) > 200
    if walk:
        _check_files(I, SC, det, dscan, out, got[2], 3, '_0002')
        assert not os.path.exists(os.path.join(out, 'scene_0001.ply'))
    return demo, got


def test_run_scene_cloud_mv3ddet(dev, tmp_path_factory, tmp_path):
    import test_gpu_cont_det as CD
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.config import load_config
    cfg = load_config(os.path.join(ROOT, 'configs', 'mv_3ddet.py'))
    det, _ = I.init_model(cfg, device=dev)
    CD._randomise_statistics(det, dev, seed=2)
    det.bbox_head.test_cfg = dict(TI.TEST_CFG)
    pipe = TI._small_pipeline(cfg)
    demo = TM._demo(tmp_path_factory)
    raw = I.run_scene(det, os.path.join(demo, 'room'), pipe, seed=TI.SEED, filter=None)
    flt = dict(iou_thr=0.15, score_thr=TI._split(raw[0].scores_3d), topk_per_class=2)
    _, got = _model_case(dev, tmp_path_factory, tmp_path, det, pipe, False, flt)
    assert len(got[0].keep) > 0


def test_run_scene_cloud_occupancy(dev, tmp_path_factory, tmp_path):
    import test_gpu_inference as TI
    import test_gpu_occ as TO
    from embodiedscan_amd import inference as I
    cfg = TO._small_cfg()
    cfg['test_pipeline'] = cfg['train_pipeline']                 # (mv_occ.py carries one pipeline, without augmentation)
    det, _ = I.init_model(cfg, device=dev)
    _model_case(dev, tmp_path_factory, tmp_path, det, TI._small_pipeline(cfg), False)


def test_walk_scene_cloud_cont_det_and_the_command_line(dev, tmp_path_factory, tmp_path):
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd import scene_cloud as SC
    det, pipe, cfg_path, ckpt = TM._cont_det(dev, tmp_path_factory)
    demo = TM._demo(tmp_path_factory)
    raw = list(I.walk_scene(det, os.path.join(demo, 'room'), pipe, seed=TI.SEED, filter=None))
    thr = TI._split(torch.cat([r.scores_3d for _, r in raw]))
    flt = dict(score_thr=thr, topk_per_class=2)
    demo, got = _model_case(dev, tmp_path_factory, tmp_path, det, pipe, True, flt)
    out_cli = str(tmp_path / 'cli')
    cmd = [sys.executable, '-m', 'embodiedscan_amd.inference', cfg_path, ckpt, '--root-dir', demo, '--scene', 'room', '--walk', '--seed', str(TI.SEED),
           '--score-thr', repr(thr), '--topk-per-class', '2', '--out', str(tmp_path / 'o.json'), '--cloud', out_cli, '--cloud-cell', '0.1', '--cloud-every', '2']
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    ref = str(tmp_path / 'cloud')
    assert sorted(os.listdir(out_cli)) == sorted(os.listdir(ref))
    for name in os.listdir(ref):
        if name.endswith('.ply'):
            assert open(os.path.join(out_cli, name), 'rb').read() == open(os.path.join(ref, name), 'rb').read(), f'the command line wrote another {name}'
    doc, doc_cli = (json.load(open(os.path.join(d, 'cloud.json'))) for d in (ref, out_cli))
    assert doc_cli.pop('class_names')[:2] == ['chair', 'table'] and doc.pop('class_names')[0] == 'class_0' and doc_cli == doc     # (the configuration's names)
    recs = json.load(open(str(tmp_path / 'o.json')))['results']
    assert [('support' in r) for r in recs] == [True, False, True, True]
    assert recs[3]['support'] == got[3].cloud_support.cpu().tolist()


def test_walk_scene_cloud_cont_occ(dev, tmp_path_factory, tmp_path):
    import test_gpu_cont_occ as CO
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    cfg = CO._small_cfg()
    det, _ = I.init_model(cfg, device=dev)
    _model_case(dev, tmp_path_factory, tmp_path, det, TI._small_pipeline(cfg), True)
