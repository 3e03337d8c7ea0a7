"""es_render_project / es_render_boxes / es_render_occupancy (csrc/predict.hip) and embodiedscan_amd.render / inference(render=) held
to tests/render_spec.py ON EVERY BYTE.

Frames (H, W) in {(1, 1), (5, 67), (48, 64), (50, 130)} in both layouts, V in {1, 3}, n in {0, 1, 2, chunk - 1, chunk, chunk + 1,
2 chunk + 3} (chunk = 64 records per LDS round), radius_q in {1, 4, 10}, alpha in {0, 192, 256}.  The population (render_spec.population)
starts with a box behind the camera, one straddling the camera plane, one containing the camera, one off-screen, one with corners beyond the
guard band, a zero-size box and three mutually overlapping boxes; test_population_holds_every_kind asserts that from the records.
Occupancy: grids 1 x 1 x 1, 3 x 2 x 5 and 8 x 8 x 4 seen by a camera inside the grid, one outside, one looking away and an axis-parallel
bundle of rays (zero direction components), labels 0, C - 1, C and 255 present.  Every buffer carries a sentinel tail that must survive, the
inputs stay as they were, the refusals write nothing, two runs are bit-equal.

Every body is a function of `dev`: tests/test_emu_render.py runs the same bodies on the CPU emulator."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_spec as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_U8, SENT_I, SENT_F = 0xA5, -9, -7.25e5
CHUNK = S.CHUNK
COUNTS = [0, 1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
SHAPES = [(1, 1), (5, 67), (48, 64), (50, 130)]


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


def run_boxes(dev, src, chw, boxes, E, K, colors, radius_q=4, alpha=192, expect=(0, 0), in_place=False, H=None, W=None):
    """the two launches on sentinel-tailed buffers -> (rec (V,n,REC), dst (V,H,W,3)) as numpy; asserts tails and inputs"""
    hip = _hip()
    P = hip.P
    V, n = len(E), len(boxes)
    if H is None:
        H, W = (src.shape[2], src.shape[3]) if chw else (src.shape[1], src.shape[2])
    s, sb = _padded(dev, src, torch.uint8, SENT_U8)
    b, bb = _padded(dev, np.asarray(boxes, np.float32).reshape(n, 9), torch.float32, SENT_F)
    e, eb = _padded(dev, E, torch.float32, SENT_F)
    k, kb = _padded(dev, K, torch.float32, SENT_F)
    c, cb = _padded(dev, np.asarray(colors, np.uint8).reshape(n, 3), torch.uint8, SENT_U8)
    r, rb = _padded(dev, np.full(V * n * S.REC, SENT_I), torch.int32, SENT_I)
    n_out = int(np.prod(src.shape))
    d, db = (s, sb) if in_place else _padded(dev, np.full(n_out, SENT_U8), torch.uint8, SENT_U8)
    before = [t.clone() for t in (bb, eb, kb, cb)] + ([] if in_place else [sb.clone()])
    rc0 = hip.raw('es_render_project')(P(b), n, P(e), P(k), V, H, W, P(r), _st())
    torch.cuda.synchronize()
    assert rc0 == expect[0], f'es_render_project: status {rc0}, expected {expect[0]}'
    if rc0 != 0:
        assert bool((rb == SENT_I).all()), 'a refused es_render_project wrote something'
    rec_before = rb.clone()
    rc1 = hip.raw('es_render_boxes')(P(s), int(chw), V, H, W, P(r), P(c), n, radius_q, alpha, P(d), _st())
    torch.cuda.synchronize()
    assert rc1 == expect[1], f'es_render_boxes: status {rc1}, expected {expect[1]}'
    for name, t, t0 in zip(('boxes', 'extrinsic', 'intrinsic', 'colors', 'src'), (bb, eb, kb, cb, sb), before):
        assert torch.equal(t, t0), f'{name}: an input (or its tail) was written'
    assert torch.equal(rb, rec_before), 'es_render_boxes wrote into the records'
    assert bool((rb[V * n * S.REC:] == SENT_I).all()) and bool((db[n_out:] == SENT_U8).all()), 'a launch wrote past the end of an output'
    if rc1 != 0:
        if not in_place:
            assert bool((db == SENT_U8).all()), 'a refused es_render_boxes wrote something'
        return None, None
    return r.cpu().numpy().reshape(V, n, S.REC), d.cpu().numpy().reshape(V, H, W, 3)


def boxes_case(dev, H, W, chw, V, n, radius_q=4, alpha=192, seed=0, in_place=False):
    src = S.frames(V, H, W, chw, 100 + seed)
    boxes, (E, K), colors = S.population(n, 7 + seed), S.views(V, H, W), S.colours(n, 50 + seed)
    want_rec = S.project(boxes, E, K)
    want = S.draw_boxes(src, chw, want_rec, colors, radius_q, alpha)
    rec, dst = run_boxes(dev, src, chw, boxes, E, K, colors, radius_q, alpha, in_place=in_place)
    assert np.array_equal(rec, want_rec), f'records differ at {np.argwhere(rec != want_rec)[:5].tolist()}'
    assert dst.shape == want.shape and np.array_equal(dst, want), \
        f'{int((dst != want).any(-1).sum())} pixels differ, first at {np.argwhere((dst != want).any(-1))[:5].tolist()}'
    rec2, dst2 = run_boxes(dev, src, chw, boxes, E, K, colors, radius_q, alpha, in_place=in_place)
    assert np.array_equal(rec, rec2) and np.array_equal(dst, dst2), 'two runs differ'
    return src, want_rec, dst


@pytest.mark.parametrize('chw', [1, 0])
@pytest.mark.parametrize('H,W', SHAPES)
def test_frame_shapes_and_layouts(dev, H, W, chw):
    for V in (1, 3):
        src, rec, dst = boxes_case(dev, H, W, chw, V, 12, seed=V)
        if (H, W) != (1, 1):
            assert (dst != S.to_hwc(src, chw)).any(), 'nothing was drawn'


@pytest.mark.parametrize('n', COUNTS)
def test_counts_around_the_chunk(dev, n):
    src, rec, dst = boxes_case(dev, 48, 64, 1, 3 if n in (CHUNK + 1, 2) else 1, n, seed=n)
    if n == 0:
        assert np.array_equal(dst, S.to_hwc(src, 1)), 'n = 0 transposes the frames'
    if n > CHUNK:
        late = S.draw_boxes(src, 1, rec[:, :CHUNK], S.colours(n, 50 + n)[:CHUNK])
        assert (late != dst).any(), 'no record behind the first chunk reaches a pixel'


@pytest.mark.parametrize('radius_q', [1, 4, 10])
@pytest.mark.parametrize('alpha', [0, 192, 256])
def test_line_widths_and_weights(dev, radius_q, alpha):
    boxes_case(dev, 48, 64, 0, 1, 12, radius_q, alpha, seed=3)


def test_in_place_on_hwc_frames(dev):
    boxes_case(dev, 50, 130, 0, 3, 12, seed=5, in_place=True)


def test_population_holds_every_kind(dev):
    """the records of view 0 at 48 x 64 show each kind of box the population promises, and the composition order shows"""
    H, W = 48, 64
    boxes, (E, K) = S.population(12, 7), S.views(1, H, W)
    rec = S.project(boxes, E, K)[0]
    m = rec[:, 16]
    assert m[0] == 0, 'behind the camera: no usable corner, no skip'
    assert 0 < bin(int(m[1]) & 255).count('1') < 8 and not m[1] & S.SKIP, 'straddles the camera plane'
    assert m[2] & S.SKIP, 'contains the camera'
    assert m[3] & 255 == 255 and (rec[3, 17] > 4 * W or rec[3, 19] < 0), 'wholly off-screen'
    cam_z = boxes[4, 0] + np.array([-1, 1]) * boxes[4, 3] / 2
    assert (cam_z >= 1e-4).all() and 0 < bin(int(m[4]) & 255).count('1') < 8, 'corners in front of the camera but beyond the guard band'
    assert m[5] & 255 == 255 and len({(rec[5, 2 * k], rec[5, 2 * k + 1]) for k in range(8)}) == 1, 'zero size: one point'
    src = S.frames(1, H, W, 0, 1)
    col = S.colours(12, 2)
    fwd = S.draw_boxes(src, 0, rec[None, 6:9], col[6:9])
    rev = S.draw_boxes(src, 0, rec[None, 6:9][:, ::-1], col[6:9][::-1])
    assert (fwd != rev).any(), 'the three overlapping boxes do not show the composition order'
    rec_dev, _ = run_boxes(dev, src, 0, boxes, E, K, col)
    assert np.array_equal(rec_dev[0], rec)


# ------------------------------------------------------------------------------------------------------------------ occupancy
GRIDS = [(1, 1, 1), (3, 2, 5), (8, 8, 4)]
N_CLASSES = 5


def occ_views(H, W, shape):
    """rays (4, 12): a camera inside the grid, one outside looking at it, the same looking away, and an axis-parallel bundle whose
    direction (1, (x + 0.5 - W/2) / 64, (y + 0.5 - H/2) / 64) has exact zeros on the middle column / row (even W, H)"""
    cams = [S.camera((1.45, 0.05, 0.45), 0.4, -0.1, 0.6 * W, H, W), S.camera((-2.0, 0.3, 0.8), -0.1, -0.05, 0.9 * W, H, W),
            S.camera((-2.0, 0.3, 0.8), 3.0, 0.1, 0.9 * W, H, W)]
    rays = np.zeros((4, 12))
    rays[:3] = S.rays_of(np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]))
    rays[3, :9] = (0, 0, 1, 2.0 ** -6, 0, -(W / 2) * 2.0 ** -6, 0, 2.0 ** -6, -(H / 2) * 2.0 ** -6)
    rays[3, 9:] = (-1.0, 0.0, 0.5)
    return rays


def occ_volume(shape, seed):
    rng = np.random.default_rng(seed)
    pool = np.array([0, 0, 0, 0, 1, 2, N_CLASSES - 1, N_CLASSES, 255], np.uint8)
    occ = pool[rng.integers(0, len(pool), shape)]
    if occ.size == 1:
        occ[...] = N_CLASSES - 1
    else:                                                      # every kind of label is present whatever the draw
        flat = occ.reshape(-1)
        flat[rng.permutation(occ.size)[:4]] = (0, N_CLASSES - 1, N_CLASSES, 255)
    return occ


def run_occupancy(dev, src, chw, rays, occ, rmin, size, palette, alpha=128, expect=0, C=None, dims=None, H=None, W=None):
    hip = _hip()
    P = hip.P
    V = len(rays)
    if H is None:
        H, W = (src.shape[2], src.shape[3]) if chw else (src.shape[1], src.shape[2])
    s, sb = _padded(dev, src, torch.uint8, SENT_U8)
    r, rb = _padded(dev, rays, torch.float64, SENT_F)
    o, ob = _padded(dev, occ, torch.uint8, SENT_U8)
    p, pb = _padded(dev, palette, torch.uint8, SENT_U8)
    n_out = int(np.prod(src.shape))
    d, db = _padded(dev, np.full(n_out, SENT_U8), torch.uint8, SENT_U8)
    before = [t.clone() for t in (sb, rb, ob, pb)]
    grid = (ctypes.c_double * 6)(*[float(x) for x in rmin], *[float(x) for x in size])
    X, Y, Z = dims or occ.shape
    rc = hip.raw('es_render_occupancy')(P(s), int(chw), V, H, W, P(r), P(o), X, Y, Z, ctypes.cast(grid, ctypes.c_void_p), P(p),
                                         len(palette) if C is None else C, alpha, P(d), _st())
    torch.cuda.synchronize()
    assert rc == expect, f'es_render_occupancy: status {rc}, expected {expect}'
    for name, t, t0 in zip(('src', 'rays', 'occ', 'palette'), (sb, rb, ob, pb), before):
        assert torch.equal(t, t0), f'{name}: an input (or its tail) was written'
    assert bool((db[n_out:] == SENT_U8).all()), 'the launch wrote past the end of dst'
    if rc != 0:
        assert bool((db == SENT_U8).all()), 'a refused call wrote something'
        return None
    return d.cpu().numpy().reshape(V, H, W, 3)


def occupancy_case(dev, shape, chw, H=48, W=64, alpha=128, seed=0):
    rmin = np.array([0.5, -1.0, 0.0])
    size = np.array([2.0, 2.0, 1.0]) / np.array(shape)
    rays, occ = occ_views(H, W, shape), occ_volume(shape, 20 + seed)
    palette = S.colours(N_CLASSES, 30 + seed)
    src = S.frames(4, H, W, chw, 40 + seed)
    want = S.draw_occupancy(src, chw, rays, occ, rmin, size, palette, alpha)
    base = S.to_hwc(src, chw)
    hit = (S.draw_occupancy(src, chw, rays, occ, rmin, size, palette, 0) != base).any(-1)      # (whatever the weight under test)
    assert hit[0].any() and hit[1].any() and not hit[1].all(), 'the cameras inside / outside the grid see nothing (or everything)'
    assert not hit[2].any(), 'the camera looking away hits the grid'
    got = run_occupancy(dev, src, chw, rays, occ, rmin, size, palette, alpha)
    assert np.array_equal(got, want), f'{int((got != want).any(-1).sum())} pixels differ, first at {np.argwhere((got != want).any(-1))[:5].tolist()}'
    assert np.array_equal(got, run_occupancy(dev, src, chw, rays, occ, rmin, size, palette, alpha)), 'two runs differ'
    return hit


@pytest.mark.parametrize('shape', GRIDS)
def test_occupancy_grids_and_cameras(dev, shape):
    hit = occupancy_case(dev, shape, 1, seed=shape[0])
    if shape == (1, 1, 1):
        H, W = 48, 64                                           # the one voxel is solid: the axis-parallel bundle's zero-component rays hit it
        assert hit[3, H // 2, :].any() and hit[3, :, W // 2].any()


def test_occupancy_odd_frames_and_weights(dev):
    occupancy_case(dev, (3, 2, 5), 0, H=5, W=67, alpha=0, seed=1)
    occupancy_case(dev, (8, 8, 4), 1, H=50, W=130, alpha=256, seed=2)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(dev):
    H, W, V, n = 8, 8, 1, 3
    src = S.frames(V, H, W, 0, 1)
    boxes, (E, K), col = S.population(n, 1), S.views(V, H, W), S.colours(n, 1)
    for kw, exp in ((dict(H=0), (-4, -4)), (dict(W=4097), (-4, -4)), (dict(H=4097), (-4, -4)), (dict(radius_q=0), (0, -4)),
                    (dict(radius_q=65), (0, -4)), (dict(alpha=-1), (0, -4)), (dict(alpha=257), (0, -4))):
        args = dict(dict(H=H, W=W, radius_q=4, alpha=192), **kw)
        run_boxes(dev, src, 0, boxes, E, K, col, args['radius_q'], args['alpha'], expect=exp, H=args['H'], W=args['W'])
    hip, P = _hip(), _hip().P
    buf = torch.full((64,), SENT_U8, dtype=torch.uint8, device=dev)
    ibuf = torch.full((64,), SENT_I, dtype=torch.int32, device=dev)
    assert hip.raw('es_render_project')(0, -1, 0, 0, 1, H, W, P(ibuf), _st()) == -5
    assert hip.raw('es_render_project')(0, 1, 0, 0, -1, H, W, P(ibuf), _st()) == -5
    assert hip.raw('es_render_boxes')(P(buf), 0, 1, 2, 2, P(ibuf), P(buf), -1, 4, 192, P(buf), _st()) == -5
    assert hip.raw('es_render_boxes')(P(buf), 0, -1, 2, 2, P(ibuf), P(buf), 0, 4, 192, P(buf), _st()) == -5
    assert hip.raw('es_render_boxes')(P(buf), 1, 1, 2, 2, P(ibuf), P(buf), 0, 4, 192, P(buf), _st()) == -4, 'in place on (V, 3, H, W) frames'
    assert hip.raw('es_render_project')(0, 0, 0, 0, 3, H, W, P(ibuf), _st()) == 0 and hip.raw('es_render_project')(0, 5, 0, 0, 0, H, W, P(ibuf), _st()) == 0
    assert hip.raw('es_render_boxes')(P(buf), 0, 0, 2, 2, P(ibuf), P(buf), 0, 4, 192, P(buf), _st()) == 0, 'V = 0 is not an error'
    torch.cuda.synchronize()
    assert bool((buf == SENT_U8).all()) and bool((ibuf == SENT_I).all())
    shape = (3, 2, 5)
    rays, occ, pal = occ_views(H, W, shape)[:1], occ_volume(shape, 1), S.colours(N_CLASSES, 1)
    rmin, size = np.zeros(3), np.ones(3)
    for kw in (dict(H=0), dict(W=4097), dict(alpha=-1), dict(alpha=257), dict(C=0), dict(C=257), dict(dims=(0, 2, 5)), dict(dims=(3, 2, -1))):
        args = dict(dict(H=H, W=W, alpha=128, C=None, dims=None), **kw)
        run_occupancy(dev, src, 0, rays, occ, rmin, size, pal, args['alpha'], expect=-4, C=args['C'], dims=args['dims'], H=args['H'], W=args['W'])
    g = (ctypes.c_double * 6)(0, 0, 0, 1, 1, 1)
    assert hip.raw('es_render_occupancy')(P(buf), 0, -1, 2, 2, 0, P(buf), 1, 1, 1, ctypes.cast(g, ctypes.c_void_p), P(buf), 3, 128, P(buf), _st()) == -5


# ------------------------------------------------------------------------------------------------------------------ the public interface
def test_render_module_against_the_spec(dev):
    from embodiedscan_amd import render as RD
    H, W, V, n = 48, 64, 3, 12
    src = S.frames(V, H, W, 1, 9)
    boxes, (E, K), col = S.population(n, 9), S.views(V, H, W), S.colours(n, 9)
    t = torch.from_numpy(src).to(dev)
    got = RD.render_boxes(t, E, K, torch.from_numpy(boxes).to(dev), torch.from_numpy(col), thickness=2, alpha=0.75)
    assert got.shape == (V, H, W, 3) and got.dtype == torch.uint8 and got.device == t.device
    assert np.array_equal(got.cpu().numpy(), S.render_boxes(src, 1, boxes, E, K, col, 4, 192))
    hwc = torch.from_numpy(S.to_hwc(src, 1)).to(dev)
    same = RD.render_boxes(hwc, E, K, torch.from_numpy(boxes).to(dev), torch.from_numpy(col).to(dev), out=hwc)
    assert same.data_ptr() == hwc.data_ptr() and torch.equal(same, got)
    shape, pr = (8, 8, 4), (0.5, -1.0, 0.0, 2.5, 1.0, 1.0)
    cams = [S.camera((1.45, 0.05, 0.45), 0.4, -0.1, 0.6 * W, H, W), S.camera((-2.0, 0.3, 0.8), -0.1, -0.05, 0.9 * W, H, W), S.camera((-2.0, 0.3, 0.8), 3.0, 0.1, 0.9 * W, H, W)]
    Eo, Ko = np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])
    occ = occ_volume(shape, 4)
    pal = RD.class_palette(N_CLASSES)
    wide = torch.from_numpy(occ.astype(np.int64)).to(dev)
    wide[0, 0, 0], wide[1, 0, 0] = 300, -2                       # labels outside u8: transparent
    ref = occ.copy()
    ref[0, 0, 0] = ref[1, 0, 0] = 0
    got = RD.render_occupancy(t, Eo, Ko, wide, pr, pal, alpha=0.5)
    want = S.draw_occupancy(src, 1, S.rays_of(Eo, Ko), ref, np.array(pr[:3]), (np.array(pr[3:]) - np.array(pr[:3])) / np.array(shape), pal, 128)
    assert np.array_equal(got.cpu().numpy(), want) and (want != S.to_hwc(src, 1)).any()
    for bad, msg in ((lambda: RD.render_boxes(t.float(), E, K, torch.zeros((0, 9), device=dev), col[:0]), 'uint8'),
                     (lambda: RD.render_boxes(t, E, K, torch.zeros((2, 8), device=dev), col[:2]), r'\(n, 9\)'),
                     (lambda: RD.render_boxes(t, E[:2], K, torch.zeros((2, 9), device=dev), col[:2]), 'extrinsic'),
                     (lambda: RD.render_boxes(t, E, K, torch.zeros((2, 9), device=dev), col[:3]), 'colors'),
                     (lambda: RD.render_boxes(t, E, K, torch.zeros((2, 9), device=dev), col[:2], thickness=40), 'thickness'),
                     (lambda: RD.render_boxes(t, E, K, torch.zeros((2, 9), device=dev), col[:2], alpha=1.5), 'alpha'),
                     (lambda: RD.render_boxes(t, E, K, torch.zeros((2, 9), device=dev), col[:2], out=torch.zeros((V, H, W, 4), dtype=torch.uint8, device=dev)), 'out'),
                     (lambda: RD.render_occupancy(t, Eo, Ko, wide.float(), pr, pal), 'integer'),
                     (lambda: RD.render_occupancy(t, Eo, Ko, wide, pr, np.zeros((257, 3), np.uint8)), '257'),
                     (lambda: RD.render_occupancy(t, Eo, Ko, wide, (0, 0, 0, 1, 1, 0), pal), 'point_cloud_range')):
        with pytest.raises(ValueError, match=msg):
            bad()
    if dev.type == 'cuda':
        with pytest.raises(ValueError, match='boxes on cpu'):
            RD.render_boxes(t, E, K, torch.zeros((2, 9)), col[:2])
        with pytest.raises(ValueError, match='occ on cpu'):
            RD.render_occupancy(t, Eo, Ko, wide.cpu(), pr, pal)


# ------------------------------------------------------------------------------------------------------------------ end to end
def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def _frames_of(dir, n):
    names = sorted(f for f in os.listdir(dir) if f.endswith('.png'))
    assert names == [f'frame_{i:04d}.png' for i in range(n)], names
    return [_png(os.path.join(dir, f)) for f in names]


def _want_boxes(I, det, dscan, inst, views):
    E, K = I.frame_matrices(dscan)
    pal = I.scene_palette(det)
    lab = inst.labels_3d.cpu().numpy()
    src = dscan['img'].cpu().numpy()
    return S.render_boxes(src[views], 1, inst.bboxes_3d.tensor.cpu().numpy(), E[views].astype(np.float32), K[views].astype(np.float32), pal[lab], 4, 192)


def _want_occ(I, det, dscan, vol, views):
    E, K = I.frame_matrices(dscan)
    pal = I.scene_palette(det)
    pr = np.asarray(det.point_cloud_range, np.float64)
    occ = vol.cpu().numpy()
    assert occ.min() >= 0 and occ.max() <= 255
    return S.draw_occupancy(dscan['img'].cpu().numpy()[views], 1, S.rays_of(E[views], K[views]), occ.astype(np.uint8), pr[:3],
                            (pr[3:] - pr[:3]) / np.array(occ.shape, np.float64), pal, 128)


def test_run_scene_renders_the_final_list(dev, tmp_path_factory):
    import test_gpu_cont_det as CD
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.config import load_config
    from embodiedscan_amd.synth import write_demo_scene
    demo = str(tmp_path_factory.mktemp('demo'))
    write_demo_scene(demo, 'room', n_frames=4, height=60, width=80, seed=3)
    cfg = load_config(os.path.join(ROOT, 'configs', 'mv_3ddet.py'))
    det, _ = I.init_model(cfg, device=dev)
    CD._randomise_statistics(det, dev, seed=2)
    det.bbox_head.test_cfg = dict(TI.TEST_CFG)
    pipe = TI._small_pipeline(cfg)
    plain = I.run_scene(det, os.path.join(demo, 'room'), pipe, seed=TI.SEED, filter=None)
    thr = TI._split(plain[0].scores_3d)
    flt = dict(iou_thr=0.15, score_thr=thr, topk_per_class=2)
    plain = I.run_scene(det, os.path.join(demo, 'room'), pipe, seed=TI.SEED, filter=flt)
    out = str(tmp_path_factory.mktemp('png'))
    got = I.run_scene(det, os.path.join(demo, 'room'), pipe, seed=TI.SEED, filter=flt, render=out, class_names=['chair', 'table'])
    assert len(got) == 1
    TI._same_instances(got[0], plain[0], 'render= changed the instances')
    assert len(got[0].keep) > 0
    dscan = TI._scan(det, demo, pipe)
    want = _want_boxes(I, det, dscan, got[0], slice(None))
    pngs = _frames_of(out, 4)
    for v in range(4):
        assert np.array_equal(pngs[v], want[v]), f'view {v}: {int((pngs[v] != want[v]).any(-1).sum())} pixels differ'
    assert (want != S.to_hwc(dscan['img'].cpu().numpy(), 1)).any(), 'no box reaches a frame'
    legend = json.load(open(os.path.join(out, 'legend.json')))
    pal = I.scene_palette(det)
    assert len(legend) == det.bbox_head.num_classes and legend['chair'] == pal[0].tolist() and legend['class_2'] == pal[2].tolist()


def test_walk_scene_renders_every_prefix_cont_det(dev, tmp_path_factory, tmp_path):
    import test_gpu_cont_det as CD
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.checkpoint import save_checkpoint
    from embodiedscan_amd.config import load_config
    from embodiedscan_amd.synth import write_demo_scene
    demo = str(tmp_path_factory.mktemp('demo'))
    write_demo_scene(demo, 'room', n_frames=4, height=60, width=80, seed=3)
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
    pipe = I.pipeline_of(cfg)
    scene = os.path.join(demo, 'room')
    raw = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=None))
    thr = TI._split(torch.cat([r.scores_3d for _, r in raw]))
    flt = dict(score_thr=thr, topk_per_class=2)
    plain = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=flt))
    out = str(tmp_path / 'walk')
    got = list(I.walk_scene(det, scene, pipe, seed=TI.SEED, filter=flt, render=out))
    assert [t for t, _ in got] == [0, 1, 2, 3]
    dscan = TI._scan(det, demo, pipe)
    pngs = _frames_of(out, 4)
    drawn = 0
    for (t, g), (_, p) in zip(got, plain):
        TI._same_instances(g, p, f'prefix {t}: render= changed the instances')
        want = _want_boxes(I, det, dscan, g, slice(t, t + 1))[0]
        assert np.array_equal(pngs[t], want), f'frame {t}: {int((pngs[t] != want).any(-1).sum())} pixels differ'
        drawn += int((want != S.to_hwc(dscan['img'].cpu().numpy()[t:t + 1], 1)[0]).any())
    assert drawn > 0, 'no box reaches a frame'
    # the command line writes the same files
    cli = str(tmp_path / 'cli')
    cmd = [sys.executable, '-m', 'embodiedscan_amd.inference', cfg_path, ckpt, '--root-dir', demo, '--scene', 'room', '--walk', '--seed', str(TI.SEED),
           '--score-thr', repr(thr), '--topk-per-class', '2', '--out', str(tmp_path / 'o.json'), '--render', cli]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    for a, b in zip(_frames_of(cli, 4), pngs):
        assert np.array_equal(a, b), 'the command line drew another picture'
    legend = json.load(open(os.path.join(cli, 'legend.json')))
    assert list(legend)[:3] == ['chair', 'table', 'class_2']
    assert list(legend.values()) == list(json.load(open(os.path.join(out, 'legend.json'))).values())


def test_walk_scene_renders_every_prefix_cont_occ(dev, tmp_path_factory, tmp_path):
    import test_gpu_cont_occ as CO
    import test_gpu_inference as TI
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.synth import write_demo_scene
    demo = str(tmp_path_factory.mktemp('demo'))
    write_demo_scene(demo, 'room', n_frames=4, height=60, width=80, seed=3)
    cfg = CO._small_cfg()
    det, _ = I.init_model(cfg, device=dev)
    pipe = TI._small_pipeline(cfg)
    scene = os.path.join(demo, 'room')
    plain = [(t, v.clone()) for t, v in I.walk_scene(det, scene, pipe, seed=TI.SEED)]
    out = str(tmp_path / 'occ')
    got = [(t, v.clone()) for t, v in I.walk_scene(det, scene, pipe, seed=TI.SEED, render=out)]
    dscan = TI._scan(det, demo, pipe)
    pngs = _frames_of(out, 4)
    drawn = 0
    for (t, g), (_, p) in zip(got, plain):
        assert torch.equal(g, p), f'prefix {t}: render= changed the volume'
        want = _want_occ(I, det, dscan, g, slice(t, t + 1))[0]
        assert np.array_equal(pngs[t], want), f'frame {t}: {int((pngs[t] != want).any(-1).sum())} pixels differ'
        drawn += int((want != S.to_hwc(dscan['img'].cpu().numpy()[t:t + 1], 1)[0]).any())
    print(f'cont-occ: {drawn} of 4 frames show a voxel')
    legend = json.load(open(os.path.join(out, 'legend.json')))
    assert list(legend)[0] == 'empty' and len(legend) == det.bbox_head.num_classes
