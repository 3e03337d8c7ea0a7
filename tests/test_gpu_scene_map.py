"""es_map_splat / es_map_resolve / es_map_project / es_map_occupancy (csrc/predict.hip) and embodiedscan_amd.scene_map / inference(map=)
held to tests/scene_map_spec.py ON EVERY BYTE: keys, image, height map and records.

Depth (H, W) in {(1, 1), (5, 67), (48, 64)}, frames at the same size and at sizes that do not divide ((3, 5), (50, 130)), both layouts, V in
{1, 3}, maps (Hm, Wm) in {(1, 1), (7, 130), (64, 64)} -- the 1 x 1 map takes every pixel of the largest population, the worst contention at
the smallest shape --, shade 0 / 1, box counts {0, 1, 63, 64, 65} (a box beyond the guard band, a zero-size one and three overlapping ones
first), volumes 1 x 1 x 1, 3 x 2 x 5 and 8 x 8 x 4 with labels 0, C - 1, C and 255, partly outside the map.  The population
(scene_map_spec.scene) holds depth 0, a negative depth, NaN, +-inf, a depth just above max_depth, a depth of 1e9 m, points below and above the
z cut and off every side of the grid; test_population_holds_every_kind asserts that.  Every buffer carries a sentinel tail that must
survive, the inputs stay as they were, the refusals write nothing, two runs are bit-equal.

Asserted on the SPEC's output, so that no test passes on an empty map: in every random case at least a quarter of the pixels are
accepted, at least a tenth of the non-empty cells receive two or more points and at least one cell is decided by the colour tie-break
(splat_population says how the 1 x 1 maps and the one-pixel depth maps get there).  The one exemption is arithmetic: a single depth pixel
in a single view has nothing to share a cell or to tie with; it must be accepted.

Every body is a function of `dev`: tests/test_emu_scene_map.py runs the same bodies on the CPU emulator."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_spec as RS
import scene_map_spec as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_U8, SENT_I, SENT_F, SENT_K = 0xA5, -9, -7.25e5, -77
DEPTHS = [(1, 1), (5, 67), (48, 64)]
MAPS = [(1, 1), (7, 130), (64, 64)]
COUNTS = [0, 1, 63, 64, 65]
GRIDS = [(1, 1, 1), (3, 2, 5), (8, 8, 4)]
N_CLASSES = 5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _hip():
    from embodiedscan_amd import hip
    return hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def _padded(dev, a, dtype, sent, pad=16):
    """a contiguous copy of `a` followed by `pad` sentinels -> (view of the copy, whole buffer)"""
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).reshape(-1)
    buf = torch.full((t.numel() + pad,), sent, dtype=dtype)
    buf[:t.numel()] = t
    buf = buf.to(dev)
    return buf[:t.numel()], buf


def _grid6(G, **kw):
    v = dict(x0=G.x0, y0=G.y0, cell=G.cell, z_min=G.z_min, z_max=G.z_max, max_depth=G.max_depth)
    v.update(kw)
    arr = (ctypes.c_double * 6)(*[float(v[k]) for k in ('x0', 'y0', 'cell', 'z_min', 'z_max', 'max_depth')])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


def _same(ts, befores, names):
    for name, t, t0 in zip(names, ts, befores):
        assert torch.equal(t.view(torch.uint8), t0.view(torch.uint8)), f'{name}: an input (or its tail) was written'


def run_splat(dev, depth, frames, chw, rays, G, keys0=None, expect=0, dims=None, grid=None):
    """one launch on sentinel-tailed buffers -> keys (Hm, Wm) int64 numpy (None after a refusal); asserts tails and inputs.
    dims: (V, H, W, h, w, Wm, Hm) passed instead of the true ones (refusals)"""
    hip = _hip()
    P = hip.P
    V, H, W = depth.shape
    h, w = (frames.shape[2], frames.shape[3]) if chw else (frames.shape[1], frames.shape[2])
    d, db = _padded(dev, depth, torch.float32, SENT_F)
    f, fb = _padded(dev, frames, torch.uint8, SENT_U8)
    r, rb = _padded(dev, rays, torch.float64, SENT_F)
    k0 = np.zeros((G.height, G.width), np.int64) if keys0 is None else keys0
    k, kb = _padded(dev, k0, torch.int64, SENT_K)
    before = [t.clone() for t in (db, fb, rb)]
    kb0 = kb.clone()
    arr, gp = _grid6(G, **(grid or {}))
    a = dims or (V, H, W, h, w, G.width, G.height)
    rc = hip.raw('es_map_splat')(P(d), a[0], a[1], a[2], P(f), int(chw), a[3], a[4], P(r), gp, a[5], a[6], P(k), _st())
    torch.cuda.synchronize()
    assert rc == expect, f'es_map_splat: status {rc}, expected {expect}'
    _same((db, fb, rb), before, ('depth', 'frames', 'rays'))
    assert bool((kb[k.numel():] == SENT_K).all()), 'the launch wrote past the end of keys'
    if rc != 0:
        assert torch.equal(kb, kb0), 'a refused es_map_splat wrote something'
        return None
    return k.cpu().numpy().reshape(G.height, G.width)


def run_resolve(dev, keys, G, background=(0, 0, 0), shade=1, with_height=True, expect=0, dims=None, grid=None, bg=None, with_image=True):
    hip = _hip()
    P = hip.P
    k, kb = _padded(dev, keys, torch.int64, SENT_K)
    n = G.height * G.width
    img, ib = _padded(dev, np.full(n * 3, SENT_U8), torch.uint8, SENT_U8)
    hz, hb = _padded(dev, np.full(n, SENT_F), torch.float32, SENT_F)
    before = kb.clone()
    arr, gp = _grid6(G, **(grid or {}))
    a = dims or (G.width, G.height)
    packed = (background[0] << 16) | (background[1] << 8) | background[2] if bg is None else bg
    rc = hip.raw('es_map_resolve')(P(k), a[0], a[1], gp, packed, shade, P(img) if with_image else 0, P(hz) if with_height else 0, _st())
    torch.cuda.synchronize()
    assert rc == expect, f'es_map_resolve: status {rc}, expected {expect}'
    assert torch.equal(kb, before), 'es_map_resolve wrote into the keys'
    assert bool((ib[n * 3:] == SENT_U8).all()) and bool((hb[n:] == SENT_F).all()), 'the launch wrote past the end of an output'
    if rc != 0 or not with_height:
        assert bool((hb == SENT_F).all()), 'the height map was written without being asked for' if rc == 0 else 'a refused call wrote something'
    if rc != 0 or not with_image:
        assert bool((ib == SENT_U8).all()), 'the image was written without being asked for' if rc == 0 else 'a refused es_map_resolve wrote something'
    if rc != 0:
        return None, None
    return img.cpu().numpy().reshape(G.height, G.width, 3), hz.cpu().numpy().reshape(G.height, G.width)


def run_project(dev, boxes, G, expect=0, n=None, dims=None, grid=None):
    hip = _hip()
    P = hip.P
    nb = len(boxes)
    b, bb = _padded(dev, np.asarray(boxes, np.float32).reshape(nb, 9), torch.float32, SENT_F)
    r, rb = _padded(dev, np.full(nb * S.REC, SENT_I), torch.int32, SENT_I)
    before = bb.clone()
    arr, gp = _grid6(G, **(grid or {}))
    a = dims or (G.width, G.height)
    rc = hip.raw('es_map_project')(P(b), nb if n is None else n, gp, a[0], a[1], P(r), _st())
    torch.cuda.synchronize()
    assert rc == expect, f'es_map_project: status {rc}, expected {expect}'
    assert torch.equal(bb.view(torch.uint8), before.view(torch.uint8)), 'boxes: an input (or its tail) was written'
    assert bool((rb[nb * S.REC:] == SENT_I).all()), 'the launch wrote past the end of the records'
    if rc != 0:
        assert bool((rb == SENT_I).all()), 'a refused es_map_project wrote something'
        return None
    return r.cpu().numpy().reshape(1, nb, S.REC)


def run_footprints(dev, image, rec, colors, G, radius_q=4, alpha=192):
    """the existing es_render_boxes on the map image, in place, as SceneMap.draw_boxes calls it"""
    hip = _hip()
    P = hip.P
    n = rec.shape[1]
    img, ib = _padded(dev, image, torch.uint8, SENT_U8)
    r, _ = _padded(dev, rec, torch.int32, SENT_I)
    c, _ = _padded(dev, np.asarray(colors, np.uint8).reshape(n, 3), torch.uint8, SENT_U8)
    rc = hip.raw('es_render_boxes')(P(img), 0, 1, G.height, G.width, P(r), P(c), n, radius_q, alpha, P(img), _st())
    torch.cuda.synchronize()
    assert rc == 0 and bool((ib[img.numel():] == SENT_U8).all())
    return img.cpu().numpy().reshape(G.height, G.width, 3)


def run_occupancy(dev, image, occ, rmin, size, palette, G, alpha=128, expect=0, C=None, vdims=None, dims=None, grid=None):
    hip = _hip()
    P = hip.P
    img, ib = _padded(dev, image, torch.uint8, SENT_U8)
    o, ob = _padded(dev, occ, torch.uint8, SENT_U8)
    p, pb = _padded(dev, palette, torch.uint8, SENT_U8)
    before = [t.clone() for t in (ob, pb)]
    ib0 = ib.clone()
    vol = (ctypes.c_double * 6)(*[float(x) for x in rmin], *[float(x) for x in size])
    arr, gp = _grid6(G, **(grid or {}))
    X, Y, Z = vdims or occ.shape
    a = dims or (G.width, G.height)
    rc = hip.raw('es_map_occupancy')(P(img), a[0], a[1], gp, P(o), X, Y, Z, ctypes.cast(vol, ctypes.c_void_p), P(p),
                                      len(palette) if C is None else C, alpha, _st())
    torch.cuda.synchronize()
    assert rc == expect, f'es_map_occupancy: status {rc}, expected {expect}'
    _same((ob, pb), before, ('occ', 'palette'))
    assert bool((ib[img.numel():] == SENT_U8).all()), 'the launch wrote past the end of the image'
    if rc != 0:
        assert torch.equal(ib, ib0), 'a refused es_map_occupancy wrote something'
        return None
    return img.cpu().numpy().reshape(G.height, G.width, 3)


# ------------------------------------------------------------------------------------------------------------------ splat + resolve
def splat_population(H, W, V, Hm, Wm, fh, fw, chw, seed):
    """-> (rays, depth, frames, Grid) of one random case.  A 1 x 1 map cuts the height just above the floor's 1/1024 m step, so that the
    flat floor is the top surface of its one cell and the colour decides it; one-pixel depth maps of several views come from a camera
    that stands still for its first two frames (the same pose and depth, another frame), so that their pixels meet in one cell at one
    height, and the third view holds NaN."""
    kw = dict(extent=12.0, z=(-3.0, 4.0)) if H * W == 1 else dict(extent=4.0, z=(-0.25, 0.1005)) if Hm * Wm == 1 else dict(extent=4.0)
    rays, depth, G = S.scene(V, H, W, Hm, Wm, seed, **kw)
    if H * W == 1 and V > 1:
        rays[1] = rays[0]
        depth[:2] = depth[np.isfinite(depth) & (depth > 0) & (depth < G.max_depth)][0]
        depth[2:] = np.nan
    return rays, depth, S.banded_frames(V, fh, fw, chw, 300 + seed), G


def splat_case(dev, H, W, V, Hm, Wm, fh, fw, chw, seed, shade=1):
    rays, depth, frames, G = splat_population(H, W, V, Hm, Wm, fh, fw, chw, seed)
    cen = S.census(depth, frames, chw, rays, G)
    print(f'depth {V}x{H}x{W} frames {fh}x{fw} map {Hm}x{Wm}: {cen}')
    if V * H * W > 1:
        assert cen['accepted'] >= 0.25 and cen['shared'] >= 0.1 and cen['ties'] >= 1, cen
    else:                                                       # one pixel in all: it is accepted, and there is nothing to share or to tie with
        assert cen['accepted'] == 1.0, cen
    want = S.splat(depth, frames, chw, rays, G)
    got = run_splat(dev, depth, frames, chw, rays, G)
    assert np.array_equal(got, want), f'{int((got != want).sum())} keys differ, first at {np.argwhere(got != want)[:5].tolist()}'
    assert np.array_equal(got, run_splat(dev, depth, frames, chw, rays, G)), 'two runs differ'
    if V > 1:                                                   # the views one by one, last first, onto the growing map
        acc = None
        for v in reversed(range(V)):
            acc = run_splat(dev, depth[v:v + 1], frames[v:v + 1], chw, rays[v:v + 1], G, keys0=acc)
        assert np.array_equal(acc, want), 'the views one by one give another map'
    for bg, hgt in (((0, 0, 0), True), ((17, 250, 3), False)):
        wi, wh = S.resolve(want, G, bg, shade)
        gi, gh = run_resolve(dev, got, G, bg, shade, hgt)
        assert np.array_equal(gi, wi), f'{int((gi != wi).any(-1).sum())} pixels differ'
        if hgt:
            assert np.array_equal(gh.view(np.uint32), wh.view(np.uint32)), 'the height maps differ'
            _, alone = run_resolve(dev, got, G, bg, shade, True, with_image=False)
            assert np.array_equal(alone.view(np.uint32), wh.view(np.uint32)), 'the height map alone differs'
            assert np.isnan(wh).sum() == (want == 0).sum()
    return G, want


@pytest.mark.parametrize('Hm,Wm', MAPS)
@pytest.mark.parametrize('H,W', DEPTHS)
def test_depth_and_map_shapes(dev, H, W, Hm, Wm):
    for V, (fh, fw), chw in ((1, (H, W), 1), (3, (3, 5), 0), (3, (50, 130), 1)):
        splat_case(dev, H, W, V, Hm, Wm, fh, fw, chw, seed=V + H + Hm + fh, shade=chw)


def test_both_layouts_give_one_map(dev):
    rays, depth, G = S.scene(3, 48, 64, 64, 64, 5)
    hwc = S.banded_frames(3, 50, 130, 0, 6)
    chw = np.ascontiguousarray(hwc.transpose(0, 3, 1, 2))
    a, b = run_splat(dev, depth, hwc, 0, rays, G), run_splat(dev, depth, chw, 1, rays, G)
    assert np.array_equal(a, b) and np.array_equal(a, S.splat(depth, hwc, 0, rays, G)) and (a != 0).any()


def test_population_holds_every_kind(dev):
    """the 3 x 48 x 64 population on the 64 x 64 map shows every kind of pixel the issue lists"""
    rays, depth, G = S.scene(3, 48, 64, 64, 64, 1, extent=3.0)
    flat = depth.reshape(-1)
    assert (flat == 0).any() and (flat < 0).any() and np.isnan(flat).any() and np.isposinf(flat).any() and np.isneginf(flat).any()
    assert ((flat > G.max_depth) & (flat < 1.01 * G.max_depth)).any() and (flat == np.float32(1e9)).any()
    y, x = np.meshgrid(np.arange(48.), np.arange(64.), indexing='ij')
    below = above = 0
    off = np.zeros(4, bool)
    for v in range(3):
        M, c = rays[v, :9].reshape(3, 3), rays[v, 9:]
        d = depth[v].astype(np.float64)
        live = (d > 0) & (d <= G.max_depth)
        p = [c[k] + d * ((M[k, 0] * x + M[k, 1] * y) + M[k, 2]) for k in range(3)]
        below += int((live & (p[2] < G.z_min)).sum())
        above += int((live & (p[2] >= G.z_max)).sum())
        inz = live & (p[2] >= G.z_min) & (p[2] < G.z_max)
        off |= [(inz & (p[0] < G.x0)).any(), (inz & (p[0] >= G.x0 + G.cell * G.width)).any(), (inz & (p[1] < G.y0)).any(),
                (inz & (p[1] >= G.y0 + G.cell * G.height)).any()]
    assert below > 0 and above > 0 and off.all(), (below, above, off.tolist())
    frames = S.banded_frames(3, 48, 64, 1, 2)
    assert np.array_equal(run_splat(dev, depth, frames, 1, rays, G), S.splat(depth, frames, 1, rays, G))


# ------------------------------------------------------------------------------------------------------------------ footprints
@pytest.mark.parametrize('n', COUNTS)
def test_box_counts_and_footprints(dev, n):
    Hm, Wm = (7, 130) if n == 1 else (64, 64)
    G = S.Grid(-2.0137, -1.3071, 4.0 / Wm, Wm, Hm)
    boxes, colors = S.map_boxes(n, 40 + n, G), RS.colours(n, 60 + n)
    want = S.project(boxes, G)
    got = run_project(dev, boxes, G)
    assert np.array_equal(got, want), f'records differ at {np.argwhere(got != want)[:5].tolist()}'
    assert np.array_equal(got, run_project(dev, boxes, G)), 'two runs differ'
    if n >= 5:
        m = want[0, :, 16]
        assert 0 <= bin(int(m[0]) & 255).count('1') < 8, 'the first box has corners beyond the guard band'
        assert m[1] & 255 == 255 and len({(want[0, 1, 2 * k], want[0, 1, 2 * k + 1]) for k in range(8)}) == 1, 'zero size: one point'
        assert not (m & RS.SKIP).any()
    base = RS.frames(1, Hm, Wm, 0, n)[0]
    for radius_q, alpha in ((4, 192), (6, 256)):
        wi = S.draw_boxes(base, boxes, colors, G, radius_q, alpha)
        gi = run_footprints(dev, base, got, colors, G, radius_q, alpha)
        assert np.array_equal(gi, wi), f'{int((gi != wi).any(-1).sum())} pixels differ'
    if n == 0:
        assert np.array_equal(gi, base)
    if n >= 5:
        assert (wi != base).any(), 'nothing was drawn'
        fwd = S.draw_boxes(base, boxes[2:5], colors[2:5], G)
        rev = S.draw_boxes(base, boxes[2:5][::-1], colors[2:5][::-1], G)
        assert (fwd != rev).any(), 'the three overlapping boxes do not show the composition order'


# ------------------------------------------------------------------------------------------------------------------ occupancy
def occ_volume(shape, seed):
    rng = np.random.default_rng(seed)
    pool = np.array([0, 0, 0, 1, 2, N_CLASSES - 1, N_CLASSES, 255], np.uint8)
    occ = pool[rng.integers(0, len(pool), shape)]
    if occ.size == 1:
        occ[...] = N_CLASSES - 1
    else:
        occ.reshape(-1)[rng.permutation(occ.size)[:4]] = (0, N_CLASSES - 1, N_CLASSES, 255)
    return occ


@pytest.mark.parametrize('shape', GRIDS)
def test_occupancy_top_surface(dev, shape):
    rmin, size = np.array([-0.7, -2.6, 0.0]), np.array([3.0, 2.0, 1.0]) / np.array(shape)      # reaches beyond the map's right and lower edge
    occ, palette = occ_volume(shape, 20 + shape[0]), RS.colours(N_CLASSES, 30 + shape[0])
    for (Hm, Wm), alpha in (((64, 64), 128), ((7, 130), 0), ((1, 1), 256)):
        G = S.Grid(-2.0137, -1.3071 if Hm > 1 else -2.0, 4.0 / Wm, Wm, Hm)
        base = RS.frames(1, Hm, Wm, 0, shape[0])[0]
        want = S.draw_occupancy(base, occ, rmin, size, palette, G, alpha)
        got = run_occupancy(dev, base, occ, rmin, size, palette, G, alpha)
        assert np.array_equal(got, want), f'{int((got != want).any(-1).sum())} pixels differ'
        assert np.array_equal(got, run_occupancy(dev, base, occ, rmin, size, palette, G, alpha)), 'two runs differ'
        if Hm == 64:
            hit = (S.draw_occupancy(base, occ, rmin, size, palette, G, 0) != base).any(-1)
            assert hit.any() and not hit.all(), 'the volume covers nothing (or everything)'
            assert not hit[:, :int(1.2 / G.cell)].any(), 'a pixel left of the volume was written'


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(dev):
    rays, depth, G = S.scene(1, 5, 67, 7, 130, 1)
    frames = S.banded_frames(1, 3, 5, 0, 1)
    V, H, W, h, w, Wm, Hm = 1, 5, 67, 3, 5, 130, 7
    nan = float('nan')
    bad_grids = (dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=float('inf')), dict(z_max=float(G.z_min)), dict(z_min=nan), dict(z_min=-5000.0, z_max=0.0),
                 dict(max_depth=0.0), dict(max_depth=nan))
    for kw in bad_grids:
        run_splat(dev, depth, frames, 0, rays, G, expect=-4, grid=kw)
    for dims in ((-1, H, W, h, w, Wm, Hm), (65536, H, W, h, w, Wm, Hm), (V, 0, W, h, w, Wm, Hm), (V, H, 4097, h, w, Wm, Hm), (V, H, W, 0, w, Wm, Hm),
                 (V, H, W, h, 4097, Wm, Hm), (V, H, W, h, w, 0, Hm), (V, H, W, h, w, Wm, 4097)):
        run_splat(dev, depth, frames, 0, rays, G, expect=-4, dims=dims)
    keys = S.splat(depth, frames, 0, rays, G)
    for kw in (dict(grid=dict(cell=nan)), dict(grid=dict(z_max=float(G.z_min))), dict(dims=(0, Hm)), dict(dims=(Wm, 4097)), dict(bg=-1), dict(bg=1 << 24), dict(with_image=False, with_height=False)):
        run_resolve(dev, keys, G, expect=-4, **kw)
    boxes = S.map_boxes(3, 1, G)
    for kw in (dict(n=-1), dict(grid=dict(cell=0.0)), dict(dims=(4097, Hm)), dict(grid=dict(max_depth=-1.0))):
        run_project(dev, boxes, G, expect=-4, **kw)
    occ, pal, base = occ_volume((3, 2, 5), 1), RS.colours(N_CLASSES, 1), RS.frames(1, Hm, Wm, 0, 1)[0]
    for kw in (dict(alpha=-1), dict(alpha=257), dict(C=0), dict(C=257), dict(vdims=(0, 2, 5)), dict(vdims=(3, 2, -1)), dict(dims=(Wm, 0)),
               dict(grid=dict(cell=nan))):
        run_occupancy(dev, base, occ, np.zeros(3), np.ones(3), pal, G, **dict(dict(expect=-4), **kw))
    run_occupancy(dev, base, occ, np.zeros(3), np.array([1.0, 0.0, 1.0]), pal, G, expect=-4)
    # V = 0 and n = 0 are not errors and write nothing
    assert not run_splat(dev, depth, frames, 0, rays, G, dims=(0, H, W, h, w, Wm, Hm)).any()
    assert run_project(dev, boxes[:0], G).shape == (1, 0, S.REC)


# ------------------------------------------------------------------------------------------------------------------ the public interface
def test_scene_map_module_against_the_spec(dev):
    from embodiedscan_amd import scene_map as SM
    from embodiedscan_amd.render import class_palette
    V, H, W, Hm, Wm = 3, 48, 64, 64, 64
    Ec, Kc = S.ring(V, H, W)
    E, K = Ec.astype(np.float64), Kc.astype(np.float64)
    rays = RS.rays_of(E, K)
    depth = S.depth_population(rays, H, W, 3, 6.0)
    frames = S.banded_frames(V, 50, 130, 1, 4)
    grid = SM.MapGrid(-2.0137, -2.0071, 4.0 / Wm, Wm, Hm, z_min=-0.25, z_max=1.0)
    G = S.Grid(grid.x0, grid.y0, grid.cell, Wm, Hm, grid.z_min, grid.z_max, 6.0)
    m = SM.SceneMap(grid, dev, max_depth=6.0)
    assert m.state_bytes() == Hm * Wm * 8
    d, f = torch.from_numpy(depth).to(dev), torch.from_numpy(frames).to(dev)
    m.add(d, f, E, K)
    want = S.splat(depth, frames, 1, rays, G)
    assert np.array_equal(m.keys.cpu().numpy(), want) and (want != 0).mean() > 0.25
    m.clear()
    assert not bool(m.keys.any())
    for v in (2, 0, 1):
        m.add(d[v:v + 1], f[v:v + 1], E[v:v + 1], K[v:v + 1], layout='chw')
    assert np.array_equal(m.keys.cpu().numpy(), want), 'adding the views one by one gives another map'
    wi, wh = S.resolve(want, G, (9, 8, 7), 1)
    img = m.image(background=(9, 8, 7))
    assert img.shape == (Hm, Wm, 3) and img.dtype == torch.uint8 and np.array_equal(img.cpu().numpy(), wi)
    assert np.array_equal(m.image(shade=False).cpu().numpy(), S.resolve(want, G, (0, 0, 0), 0)[0])
    assert np.array_equal(m.height().cpu().numpy().view(np.uint32), wh.view(np.uint32))
    boxes, colors = S.map_boxes(9, 5, G), RS.colours(9, 6)
    same = m.draw_boxes(img, torch.from_numpy(boxes).to(dev), torch.from_numpy(colors))
    assert same.data_ptr() == img.data_ptr()
    wi = S.draw_boxes(wi, boxes, colors, G, 4, 192)
    assert np.array_equal(img.cpu().numpy(), wi)
    cen = rays[:, 9:] * 0.6
    m.draw_trail(img, cen, (255, 255, 255))
    wt = S.draw_trail(wi, cen.astype(np.float32), (255, 255, 255), G)
    assert np.array_equal(img.cpu().numpy(), wt) and (wt != wi).any()
    occ, pr, pal = occ_volume((8, 8, 4), 4), (-0.7, -2.6, 0.0, 2.3, -0.6, 1.0), class_palette(N_CLASSES)
    wide = torch.from_numpy(occ.astype(np.int64)).to(dev)
    wide[0, 0, 0], wide[1, 0, 0] = 300, -2
    ref = occ.copy()
    ref[0, 0, 0] = ref[1, 0, 0] = 0
    m.draw_occupancy(img, wide, pr, pal, alpha=0.5)
    wo = S.draw_occupancy(wt, ref, np.array(pr[:3]), (np.array(pr[3:]) - np.array(pr[:3])) / np.array(occ.shape), pal, G, 128)
    assert np.array_equal(img.cpu().numpy(), wo) and (wo != wt).any()
    px = np.array([[0.5, 0.5], [10.25, 63.0], [64.0, 0.0]])
    assert np.allclose(m.to_pixels(m.to_metres(px)), px, atol=1e-9) and np.allclose(m.to_metres((0.0, Hm)), (grid.x0, grid.y0))
    z9 = torch.zeros((2, 9), device=dev)
    for bad, msg in ((lambda: m.add(d.double(), f, E, K), 'float32'), (lambda: m.add(d, f.float(), E, K), 'uint8'),
                     (lambda: m.add(d, f[:2], E, K), '2 frames'), (lambda: m.add(d, f, E[:2], K), 'extrinsic'),
                     (lambda: m.add(d, f, E, K, layout='hwc'), 'layout'), (lambda: m.image(out=torch.zeros((Hm, Wm, 4), dtype=torch.uint8, device=dev)), 'map image'),
                     (lambda: m.image(background=(0, 0, 256)), 'background'), (lambda: m.draw_boxes(img, z9[:, :8], colors[:2]), r'\(n, 9\)'),
                     (lambda: m.draw_boxes(img, z9, colors[:3]), 'colors'), (lambda: m.draw_boxes(img, z9, colors[:2], thickness=40), 'thickness'),
                     (lambda: m.draw_boxes(img[:, :, :2], z9, colors[:2]), 'map image'), (lambda: m.draw_occupancy(img, wide.float(), pr, pal), 'integer'),
                     (lambda: m.draw_occupancy(img, wide, (0, 0, 0, 1, 1, 0), pal), 'point_cloud_range'),
                     (lambda: SM.MapGrid(0, 0, 0.0, 4, 4), 'cell'), (lambda: SM.MapGrid(0, 0, 0.1, 4097, 4), '4097'),
                     (lambda: SM.MapGrid(0, 0, 0.1, 4, 4, 1.0, 1.0), 'z cut'), (lambda: SM.SceneMap(grid, dev, max_depth=0), 'max_depth')):
        with pytest.raises(ValueError, match=msg):
            bad()
    if dev.type == 'cuda':
        with pytest.raises(ValueError, match='depth on cpu'):
            m.add(d.cpu(), f, E, K)
        with pytest.raises(ValueError, match='boxes on cpu'):
            m.draw_boxes(img, z9.cpu(), colors[:2])
    assert np.array_equal(m.keys.cpu().numpy(), want), 'a refused call changed the map'


# ------------------------------------------------------------------------------------------------------------------ end to end
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def _spec_map(I, det, dscan, doc, res, n_views, colors=None):
    """the picture map= must have written for the prediction `res` over the first n_views frames, from the scan and map.json alone"""
    from embodiedscan_amd.scene_map import TRAIL_COLOR
    g = doc['grid']
    G = S.Grid(g['x0'], g['y0'], g['cell'], g['width'], g['height'], g['z_min'], g['z_max'], doc['max_depth'])
    E, K = I.depth_matrices(dscan)
    rays = RS.rays_of(E, K)
    v = slice(0, n_views)
    keys = S.splat(dscan['depth'].cpu().numpy()[v], dscan['img'].cpu().numpy()[v], 1, rays[v], G)
    img, _ = S.resolve(keys, G, (0, 0, 0), 1)
    pal = I.scene_palette(det)
    if torch.is_tensor(res):
        occ = res.cpu().numpy()
        pr = np.asarray(det.point_cloud_range, np.float64)
        img = S.draw_occupancy(img, occ.astype(np.uint8), pr[:3], (pr[3:] - pr[:3]) / np.array(occ.shape, np.float64), pal, G, 128)
    else:
        col = pal[np.clip(res.labels_3d.cpu().numpy(), 0, len(pal) - 1)] if colors is None else colors
        img = S.draw_boxes(img, res.bboxes_3d.tensor.cpu().numpy(), col, G, 4, 192)
    return S.draw_trail(img, rays[v, 9:].astype(np.float32), TRAIL_COLOR, G), keys


def _check_matrices(I, dscan):
    """depth_matrices hands back the meta's own matrices -- the depth maps are never resized -- and frame_matrices differs from it by
    exactly the resize's scale_factor, which is not 1 on the demo folder (depth 60 x 80 against frames of 128 x 128)"""
    from embodiedscan_amd import pipeline as PL
    meta = dscan['meta']
    pm = meta[PL.projection_key(meta)]
    raw_e = np.stack([np.asarray(e, np.float64) for e in pm['extrinsic']])
    intr = pm['intrinsic']
    raw_k = np.stack([np.asarray(k, np.float64) for k in intr]) if isinstance(intr, (list, tuple)) else np.repeat(np.asarray(intr, np.float64)[None], len(raw_e), 0)
    E, K = I.depth_matrices(dscan)
    assert np.array_equal(E, raw_e) and np.array_equal(K, raw_k), 'depth_matrices changed the matrices of the depth maps'
    sx, sy = (float(v) for v in meta['scale_factor'])
    assert (sx, sy) != (1.0, 1.0), 'the demo frames were not resized: the case cannot tell the two helpers apart'
    Ef, Kf = I.frame_matrices(dscan)
    want = raw_k.copy()
    want[:, 0, :] *= sx
    want[:, 1, :] *= sy
    assert np.array_equal(Ef, raw_e) and np.array_equal(Kf, want) and not np.array_equal(Kf, K)


def _demo(tmp_path_factory):
    from embodiedscan_amd.synth import write_demo_scene
    demo = str(tmp_path_factory.mktemp('demo'))
    write_demo_scene(demo, 'room', n_frames=4, height=60, width=80, seed=3)
    return demo


def stand_in(dev, kind, prediction):
    """a detector without a network: the attributes inference.run_scene / _map_painter read, `predict` answers `prediction`.  What is under
    test on this path is the map, not the model: the bodies below run unchanged on the emulator, where no whole model runs in the suite."""
    import types
    sample = types.SimpleNamespace(pred_occupancy=prediction) if torch.is_tensor(prediction) else types.SimpleNamespace(pred_instances_3d=prediction)
    return types.SimpleNamespace(task='occ' if 'occ' in kind else 'det3d', continuous=kind.startswith('cont-'), device=dev,
                                 bbox_head=types.SimpleNamespace(num_classes=4), point_cloud_range=[-3.2, -3.2, -0.78, 3.2, 3.2, 1.78],
                                 data_preprocessor=lambda batch, training: dict(inputs=None, data_samples=None),
                                 forward=lambda inputs, samples, mode: [sample])


def _stand_in_boxes(dev, n=4):
    from embodiedscan_amd.structures import EulerDepthInstance3DBoxes, InstanceData
    boxes = np.array([[0.4, 0.3, 0.5, 1.2, 0.8, 1.0, 0.4, 0.0, 0.0], [-1.1, 0.9, 0.4, 0.6, 0.6, 0.8, -0.7, 0.1, 0.0],
                      [0.6, 0.5, 0.7, 0.9, 1.1, 0.5, 1.2, 0.0, 0.2], [1.7, -1.3, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], np.float32)
    return InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(torch.from_numpy(boxes[:n]).to(dev)), scores_3d=torch.tensor([0.9, 0.8, 0.7, 0.6][:n], device=dev),
                        labels_3d=torch.tensor([0, 3, 1, 9][:n], device=dev))


def _stand_in_pipeline():
    import test_gpu_inference as TI
    from embodiedscan_amd.config import load_config
    return TI._small_pipeline(load_config(os.path.join(ROOT, 'configs', 'mv_3ddet.py')))


def test_run_scene_maps_a_given_prediction(dev, tmp_path_factory, tmp_path, launch_log=None):
    """run_scene(map=) end to end on the demo folder (depth 60 x 80 against resized frames) with the prediction given: boxes and a volume"""
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    demo = _demo(tmp_path_factory)
    scene, pipe = os.path.join(demo, 'room'), _stand_in_pipeline()
    vol = torch.from_numpy(occ_volume((8, 8, 4), 3).astype(np.int64) % 7).to(dev)
    for kind, pred in (('det3d', _stand_in_boxes(dev)), ('occ', vol)):
        det = stand_in(dev, kind, pred)
        if launch_log is not None:
            launch_log()
        plain = I.run_scene(det, scene, pipe, seed=TI.SEED, filter=None)
        if launch_log is not None:
            assert not any(k.startswith('k_map_') for k in launch_log()), 'map=None launched a map kernel'
        out = str(tmp_path / kind)
        got = I.run_scene(det, scene, pipe, seed=TI.SEED, filter=None, map=out, map_cell=0.125, map_z=(-0.5, 2.5), class_names=None if kind == 'occ' else ['chair'])
        if launch_log is not None:
            assert {'k_map_splat', 'k_map_resolve', 'k_render_boxes', 'k_map_occupancy' if kind == 'occ' else 'k_map_project'} <= launch_log()
        assert got[0] is plain[0] is pred
        assert sorted(os.listdir(out)) == ['legend.json', 'map.json', 'map.png']
        doc = json.load(open(os.path.join(out, 'map.json')))
        dscan = TI._scan(det, demo, pipe)
        assert tuple(dscan['depth'].shape[1:]) == (60, 80) and tuple(dscan['img'].shape[2:]) != (60, 80)
        _check_matrices(I, dscan)
        want, keys = _spec_map(I, det, dscan, doc, pred, 4)
        png = _png(os.path.join(out, 'map.png'))
        assert np.array_equal(png, want), f'{kind}: {int((png != want).any(-1).sum())} pixels differ'
        assert (keys != 0).sum() > 200, 'the recording reaches almost no cell'
        bare, _ = S.resolve(keys, S.Grid(**doc['grid'], max_depth=doc['max_depth']), (0, 0, 0), 1)
        assert (want != bare).any(), 'neither the prediction nor the trail shows'
        legend = json.load(open(os.path.join(out, 'legend.json')))
        assert list(legend)[0] == ('empty' if kind == 'occ' else 'chair') and len(legend) == 4
        g = doc['grid']
        if kind == 'occ':
            assert (g['x0'], g['y0'], g['width'], g['height']) == (-3.25, -3.25, 52, 52)
        else:
            assert g['width'] * g['cell'] >= 16.0 and (g['z_min'], g['z_max']) == (-0.5, 2.5)


def walking_stand_in(dev, kind, script):
    """stand_in with a walk session: open_walk returns a session whose observe answers script(t) for the t-th frame it is handed, and the
    preprocessor passes the batch's frames and its one sample through -- all that inference.walk_scene reads of a continuous model"""
    import types
    det = stand_in(dev, kind, None)
    det.data_preprocessor = lambda batch, training: dict(inputs=dict(imgs=batch['inputs']['img']), data_samples=batch['data_samples'])
    det.observed = []

    def open_walk(meta, max_frames=None):
        seen = []

        def observe(img, rows, matrices):
            assert img.dim() == 3 and set(matrices) == {'extrinsic', 'intrinsic'}
            seen.append(int(rows.shape[0]))
            det.observed.append(len(seen) - 1)
            return script(len(seen) - 1)
        return types.SimpleNamespace(observe=observe)
    det.open_walk = open_walk
    return det


def _walk_pipeline(kind):
    import test_gpu_cont_det as CD
    import test_gpu_cont_occ as CO
    import test_gpu_inference as TI
    from embodiedscan_amd.config import load_config
    return TI._small_pipeline(load_config(CD.CFG) if kind == 'cont-det3d' else CO._small_cfg())


def test_walk_maps_grow_frame_by_frame(dev, tmp_path_factory, tmp_path, launch_log=None):
    """walk_scene(map=) itself on the demo folder, driven by a scripted session (walking_stand_in): cont-det3d without and with track=, and
    an occupancy volume per frame.  The yielded predictions equal map=None's, which launches no k_map_* kernel; map t equals a fresh map of
    frames 0 .. t under the prediction of prefix t; with track= the boxes take their track's colour and the legend is the tracked one."""
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.render import class_palette
    demo = _demo(tmp_path_factory)
    scene = os.path.join(demo, 'room')
    vol = torch.from_numpy(occ_volume((8, 8, 4), 3).astype(np.int64) % 7).to(dev)
    scripts = {'cont-det3d': lambda t: _stand_in_boxes(dev, min(t + 2, 4)), 'cont-occ': lambda t: torch.roll(vol, t, 0)}
    for name, kind, track in (('plain', 'cont-det3d', None), ('tracked', 'cont-det3d', dict()), ('occ', 'cont-occ', None)):
        det, pipe = walking_stand_in(dev, kind, scripts[kind]), _walk_pipeline(kind)
        if launch_log is not None:
            launch_log()
        plain = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=None, track=track))
        if launch_log is not None:
            assert not any(k.startswith('k_map_') for k in launch_log()), f'{name}: map=None launched a map kernel'
        out = str(tmp_path / name)
        got = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=None, track=track, map=out, map_cell=0.125, map_z=(-0.5, 2.5)))
        if launch_log is not None:
            assert {'k_map_splat', 'k_map_resolve', 'k_render_boxes', 'k_map_occupancy' if kind == 'cont-occ' else 'k_map_project'} <= launch_log()
        assert [t for t, _ in got] == [t for t, _ in plain] == [0, 1, 2, 3] and det.observed == [0, 1, 2, 3] * 2
        dscan = TI._scan(det, demo, pipe)
        assert tuple(dscan['depth'].shape[1:]) == (60, 80) and tuple(dscan['img'].shape[2:]) != (60, 80)
        doc = json.load(open(os.path.join(out, 'map.json')))
        pngs = _maps_of(out, 4)
        filled = []
        for (t, g), (_, p) in zip(got, plain):
            colors = None
            if kind == 'cont-occ':
                assert torch.equal(g, p), f'{name} prefix {t}: map= changed the volume'
            else:
                assert torch.equal(g.bboxes_3d.tensor, p.bboxes_3d.tensor) and torch.equal(g.labels_3d, p.labels_3d)
                if track is not None:
                    assert torch.equal(g.track_ids, p.track_ids) and bool((g.track_ids >= 0).all())
                    colors = class_palette(257)[1:][g.track_ids.cpu().numpy() % 256]
            want, keys = _spec_map(I, det, dscan, doc, g, t + 1, colors)             # a fresh map of frames 0 .. t
            assert np.array_equal(pngs[t], want), f'{name} map {t}: {int((pngs[t] != want).any(-1).sum())} pixels differ'
            filled.append(int((keys != 0).sum()))
        assert filled == sorted(filled) and filled[-1] > filled[0] > 0, f'{name}: the map does not grow: {filled}'
        legend = json.load(open(os.path.join(out, 'legend.json')))
        if track is not None:
            assert legend and all(k.startswith('track_') and set(v) == {'color', 'class_name'} for k, v in legend.items())
        else:
            assert len(legend) == 4 and all(len(v) == 3 for v in legend.values())


def test_run_scene_maps_mv3ddet(dev, tmp_path_factory, tmp_path, launch_log=None):
    import test_gpu_cont_det as CD
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.config import load_config
    demo = _demo(tmp_path_factory)
    cfg = load_config(os.path.join(ROOT, 'configs', 'mv_3ddet.py'))
    det, _ = I.init_model(cfg, device=dev)
    CD._randomise_statistics(det, dev, seed=2)
    det.bbox_head.test_cfg = dict(TI.TEST_CFG)
    pipe = TI._small_pipeline(cfg)
    scene = os.path.join(demo, 'room')
    raw = I.run_scene(det, scene, pipe, seed=TI.SEED, filter=None)
    flt = dict(iou_thr=0.15, score_thr=TI._split(raw[0].scores_3d), topk_per_class=2)
    if launch_log is not None:
        launch_log()
    plain = I.run_scene(det, scene, pipe, seed=TI.SEED, filter=flt)
    if launch_log is not None:
        assert not any(k.startswith('k_map_') for k in launch_log()), 'map=None launched a map kernel'
    out, both = str(tmp_path / 'map'), str(tmp_path / 'both')
    got = I.run_scene(det, scene, pipe, seed=TI.SEED, filter=flt, map=out, map_cell=0.25, class_names=['chair', 'table'])
    if launch_log is not None:
        assert {'k_map_splat', 'k_map_resolve', 'k_map_project'} <= launch_log()
    TI._same_instances(got[0], plain[0], 'map= changed the instances')
    assert len(got[0].keep) > 0
    assert sorted(os.listdir(out)) == ['legend.json', 'map.json', 'map.png']
    doc = json.load(open(os.path.join(out, 'map.json')))
    dscan = TI._scan(det, demo, pipe)
    assert tuple(dscan['depth'].shape[1:]) == (60, 80) and tuple(dscan['img'].shape[2:]) != (60, 80)
    want, keys = _spec_map(I, det, dscan, doc, got[0], 4)
    png = _png(os.path.join(out, 'map.png'))
    assert np.array_equal(png, want), f'{int((png != want).any(-1).sum())} pixels differ'
    assert (keys != 0).mean() > 0.02, 'the recording reaches almost no cell'
    legend = json.load(open(os.path.join(out, 'legend.json')))
    pal = I.scene_palette(det)
    assert len(legend) == det.bbox_head.num_classes and legend['chair'] == pal[0].tolist()
    # map= combines with render=
    I.run_scene(det, scene, pipe, seed=TI.SEED, filter=flt, map=both, map_cell=0.25, render=both, class_names=['chair', 'table'])
    assert np.array_equal(_png(os.path.join(both, 'map.png')), png) and os.path.exists(os.path.join(both, 'frame_0003.png'))


def test_run_scene_maps_occupancy(dev, tmp_path_factory, tmp_path):
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    import test_gpu_occ as TO
    demo = _demo(tmp_path_factory)
    cfg = TO._small_cfg()
    cfg['test_pipeline'] = cfg['train_pipeline']                 # (mv_occ.py carries one pipeline, without augmentation)
    det, _ = I.init_model(cfg, device=dev)
    pipe = TI._small_pipeline(cfg)
    scene = os.path.join(demo, 'room')
    plain = I.run_scene(det, scene, pipe, seed=TI.SEED)
    out = str(tmp_path / 'map')
    got = I.run_scene(det, scene, pipe, seed=TI.SEED, map=out, map_cell=0.1, map_z=(-0.5, 2.5))
    assert torch.equal(got[0], plain[0]), 'map= changed the volume'
    doc = json.load(open(os.path.join(out, 'map.json')))
    pr = [float(x) for x in det.point_cloud_range]
    g = doc['grid']
    assert (g['z_min'], g['z_max']) == (-0.5, 2.5) and g['x0'] <= pr[0] and g['x0'] + g['width'] * g['cell'] >= pr[3] - 1e-9
    dscan = TI._scan(det, demo, pipe)
    want, _ = _spec_map(I, det, dscan, doc, got[0], 4)
    png = _png(os.path.join(out, 'map.png'))
    assert np.array_equal(png, want), f'{int((png != want).any(-1).sum())} pixels differ'
    assert list(json.load(open(os.path.join(out, 'legend.json'))))[0] == 'empty'


def _cont_det(dev, tmp_path_factory):
    import test_gpu_cont_det as CD
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.checkpoint import save_checkpoint
    from embodiedscan_amd.config import load_config
    work = tmp_path_factory.mktemp('cfg')
    base = load_config(CD.CFG)
    cfg_path = os.path.join(str(work), 'cont_det3d_small.py')
    with open(cfg_path, 'w') as f:
        f.write(f"_base_ = [{CD.CFG!r}]\nmodel = dict(test_cfg=dict({', '.join(f'{k}={v!r}' for k, v in TI.TEST_CFG.items())}))\n"
                f"test_pipeline = {TI._small_pipeline(base)!r}\nmetainfo = dict(classes=['chair', 'table'])\n")
    seeded = CD._build(dev)
    CD._randomise_statistics(seeded, dev, seed=2)
    ckpt = os.path.join(str(work), 'weights.pth')
    save_checkpoint(seeded, ckpt)
    det, cfg = I.init_model(cfg_path, ckpt, device=dev)
    return det, I.pipeline_of(cfg), cfg_path, ckpt


def _maps_of(dir, n):
    names = sorted(f for f in os.listdir(dir) if f.endswith('.png'))
    assert names == [f'map_{i:04d}.png' for i in range(n)], names
    return [_png(os.path.join(dir, f)) for f in names]


def test_walk_scene_maps_every_prefix_cont_det(dev, tmp_path_factory, tmp_path, cli=True):
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.render import class_palette
    demo = _demo(tmp_path_factory)
    det, pipe, cfg_path, ckpt = _cont_det(dev, tmp_path_factory)
    scene = os.path.join(demo, 'room')
    raw = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=None))
    thr = TI._split(torch.cat([r.scores_3d for _, r in raw]))
    flt = dict(score_thr=thr, topk_per_class=2)
    plain = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=flt))
    out, trk = str(tmp_path / 'walk'), str(tmp_path / 'trk')
    got = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=flt, map=out, map_cell=0.25))
    assert [t for t, _ in got] == [0, 1, 2, 3]
    dscan = TI._scan(det, demo, pipe)
    doc = json.load(open(os.path.join(out, 'map.json')))
    pngs = _maps_of(out, 4)
    filled = []
    for (t, g), (_, p) in zip(got, plain):
        TI._same_instances(g, p, f'prefix {t}: map= changed the instances')
        want, keys = _spec_map(I, det, dscan, doc, g, t + 1)             # a fresh map of frames 0 .. t
        assert np.array_equal(pngs[t], want), f'map {t}: {int((pngs[t] != want).any(-1).sum())} pixels differ'
        filled.append(int((keys != 0).sum()))
    assert filled == sorted(filled) and filled[-1] > filled[0] > 0, f'the map does not grow: {filled}'
    tracked = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=flt, map=trk, map_cell=0.25, track=dict()))
    pal = class_palette(257)[1:]
    tpngs = _maps_of(trk, 4)
    for (t, g), (_, p) in zip(tracked, plain):
        TI._same_instances(g, p, f'prefix {t}: map= with track= changed the instances')
        want, _ = _spec_map(I, det, dscan, doc, g, t + 1, colors=pal[g.track_ids.cpu().numpy() % 256])
        assert np.array_equal(tpngs[t], want), f'tracked map {t} differs'
    legend = json.load(open(os.path.join(trk, 'legend.json')))
    assert legend and all(k.startswith('track_') and set(v) == {'color', 'class_name'} for k, v in legend.items())
    if not cli:
        return
    out_cli = str(tmp_path / 'cli')
    cmd = [sys.executable, '-m', 'embodiedscan_amd.inference', cfg_path, ckpt, '--root-dir', demo, '--scene', 'room', '--walk', '--seed', str(TI.SEED),
           '--score-thr', repr(thr), '--topk-per-class', '2', '--out', str(tmp_path / 'o.json'), '--map', out_cli, '--map-cell', '0.25']
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    for a, b in zip(_maps_of(out_cli, 4), pngs):
        assert np.array_equal(a, b), 'the command line drew another map'
    assert json.load(open(os.path.join(out_cli, 'map.json'))) == doc


def test_walk_scene_maps_every_prefix_cont_occ(dev, tmp_path_factory, tmp_path):
    import test_gpu_cont_occ as CO
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    demo = _demo(tmp_path_factory)
    cfg = CO._small_cfg()
    det, _ = I.init_model(cfg, device=dev)
    pipe = TI._small_pipeline(cfg)
    scene = os.path.join(demo, 'room')
    plain = [(t, v.clone()) for t, v in I.walk_scene(det, scene, pipe, seed=TI.SEED)]
    out = str(tmp_path / 'occ')
    got = [(t, v.clone()) for t, v in I.walk_scene(det, scene, pipe, seed=TI.SEED, map=out, map_cell=0.1)]
    dscan = TI._scan(det, demo, pipe)
    doc = json.load(open(os.path.join(out, 'map.json')))
    pngs = _maps_of(out, 4)
    for (t, g), (_, p) in zip(got, plain):
        assert torch.equal(g, p), f'prefix {t}: map= changed the volume'
        want, _ = _spec_map(I, det, dscan, doc, g, t + 1)
        assert np.array_equal(pngs[t], want), f'map {t}: {int((pngs[t] != want).any(-1).sum())} pixels differ'
