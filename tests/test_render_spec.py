"""tests/render_spec.py against answers known by construction, and the host half of embodiedscan_amd.render (no GPU).

A small box straight ahead: the pixel at its projected centre -- taken from the project's own fusion projection in the oracle
(oracle.model.projection_matrices: intrinsic @ extrinsic in f32, then the perspective division), not from the spec -- carries the blend, a
corner's pixel the edge colour, and pixels outside the grown rectangle the source bytes.  A single occupied voxel is hit by the ray through
its projected centre and by no ray outside the bounding rectangle of its silhouette."""
import os

import numpy as np
import pytest
import torch

import render_spec as S


def _oracle_pixels(points, E, K):
    """(n,3) world points -> (n,2) pixel coordinates through the oracle's fusion projection"""
    from oracle.model import projection_matrices
    proj = projection_matrices(dict(depth2img=dict(extrinsic=[E], intrinsic=[K])))[0]
    p4 = torch.cat([torch.as_tensor(points, dtype=torch.float32), torch.ones(len(points), 1)], 1)
    p2 = p4 @ proj.T
    return (p2[:, :2] / p2[:, 2:3]).numpy().astype(np.float64)


def _corners(box):
    R = S.rotation(box[6:9])
    return np.array([box[:3] + R @ (np.array([1 if k & 1 else -1, 1 if k & 2 else -1, 1 if k & 4 else -1]) * box[3:6] / 2) for k in range(8)])


def test_a_box_straight_ahead():
    H, W = 48, 64
    E, K = S.camera((0, 0, 1), 0.0, 0.0, 60.0, H, W)
    box = np.array([3.0, 0.05, 1.02, 0.5, 0.6, 0.4, 0.3, 0.1, -0.2], np.float32)
    colour = np.array([[200, 40, 90]], np.uint8)
    src = S.frames(1, H, W, 0, 1)
    rec = S.project(box[None], E[None], K[None])
    assert rec[0, 0, 16] == 255
    dst = S.draw_boxes(src, 0, rec, colour, radius_q=4, alpha=192)
    cx, cy = np.floor(_oracle_pixels(box[None, :3], E, K)[0]).astype(int)
    want = (src[0, cy, cx].astype(np.int64) * 192 + colour[0].astype(np.int64) * 64 + 128) >> 8
    assert np.array_equal(dst[0, cy, cx], want), 'the centre pixel carries the blend'
    pix = _oracle_pixels(_corners(box.astype(np.float64)), E, K)
    assert np.abs(rec[0, 0, :16].reshape(8, 2) - 4 * pix).max() <= 0.5 + 1e-3, 'the records are the oracle projection in quarter-pixels'
    for px, py in np.floor(pix).astype(int):
        assert np.array_equal(dst[0, py, px], colour[0]), 'a corner pixel carries the edge colour'
    x0, y0, x1, y1 = rec[0, 0, 17:21]
    ys, xs = np.mgrid[0:H, 0:W]
    outside = (4 * xs + 2 < x0 - 4) | (4 * xs + 2 > x1 + 4) | (4 * ys + 2 < y0 - 4) | (4 * ys + 2 > y1 + 4)
    assert outside.any() and np.array_equal(dst[0][outside], src[0][outside]) and (dst[0][~outside] != src[0][~outside]).any()
    assert np.array_equal(S.draw_boxes(src, 0, rec, colour, cull=False), dst), 'the cull changed a byte'
    chw = np.ascontiguousarray(src.transpose(0, 3, 1, 2))
    assert np.array_equal(S.draw_boxes(chw, 1, rec, colour), dst)


def test_the_cull_and_the_order_on_a_population():
    H, W, V, n = 48, 64, 3, 20
    src, boxes, (E, K), col = S.frames(V, H, W, 1, 2), S.population(n, 3), S.views(V, H, W), S.colours(n, 4)
    rec = S.project(boxes, E, K)
    a = S.draw_boxes(src, 1, rec, col, 10, 100)
    assert np.array_equal(a, S.draw_boxes(src, 1, rec, col, 10, 100, cull=False))
    assert (a != S.draw_boxes(src, 1, rec[:, ::-1], col[::-1], 10, 100)).any(), 'the composition order does not show'
    assert np.array_equal(S.draw_boxes(src, 1, rec[:, :0], col[:0]), S.to_hwc(src, 1))


def test_a_single_voxel():
    H, W = 48, 64
    E, K = S.camera((-2.0, 0.1, 0.6), 0.05, -0.02, 70.0, H, W)
    shape, rmin, size = (3, 2, 5), np.array([0.5, -1.0, 0.0]), np.array([0.5, 0.75, 0.25])
    occ = np.zeros(shape, np.uint8)
    occ[1, 1, 2] = 3
    occ[2, 0, 0], occ[0, 0, 4] = 5, 255                         # label C and 255: transparent
    pal = S.colours(5, 1)
    src = S.frames(1, H, W, 1, 5)
    dst = S.draw_occupancy(src, 1, S.rays_of(E[None], K[None]), occ, rmin, size, pal, 128)
    base = S.to_hwc(src, 1)
    lo = rmin + np.array([1, 1, 2]) * size
    corners = np.array([lo + np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1]) * size for k in range(8)])
    pix = _oracle_pixels(corners, E, K)
    cx, cy = np.floor(_oracle_pixels((lo + size / 2)[None], E, K)[0]).astype(int)
    changed = (dst[0] != base[0]).any(-1)
    assert changed[cy, cx], 'the ray through the voxel\'s projected centre misses it'
    shades = {tuple(((pal[3].astype(np.int64) * s >> 8) * 128 + base[0, cy, cx].astype(np.int64) * 128 + 128) >> 8) for s in S.SHADE}
    assert tuple(dst[0, cy, cx].astype(np.int64)) in shades
    ys, xs = np.nonzero(changed)
    assert xs.min() + 1 >= pix[:, 0].min() and xs.max() <= pix[:, 0].max() and ys.min() + 1 >= pix[:, 1].min() and ys.max() <= pix[:, 1].max(), \
        'a ray outside the silhouette\'s bounding rectangle hit the voxel'
    assert len({tuple(c) for c in dst[0][changed] - 0}) > 1


def test_class_palette():
    from embodiedscan_amd.render import class_palette
    p = class_palette(256)
    assert p.shape == (256, 3) and p.dtype == np.uint8 and np.array_equal(p, class_palette(256)) and np.array_equal(p[:17], class_palette(17))
    assert len({tuple(r) for r in p.tolist()}) == 256, 'two classes share a colour'
    assert class_palette(0).shape == (0, 3) and class_palette(1).tolist() == [[128, 128, 128]]
    with pytest.raises(ValueError):
        class_palette(-1)


def test_save_frames_round_trip(tmp_path):
    from PIL import Image
    from embodiedscan_amd.render import save_frames
    a = S.frames(3, 5, 7, 0, 3)
    paths = save_frames(str(tmp_path / 'out'), torch.from_numpy(a), stem='view', start=2)
    assert [os.path.basename(p) for p in paths] == ['view_0002.png', 'view_0003.png', 'view_0004.png']
    for i, p in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(p)), a[i])
    assert [os.path.basename(p) for p in save_frames(str(tmp_path / 'out'), a[:1])] == ['frame_0000.png']
    with pytest.raises(ValueError):
        save_frames(str(tmp_path), a.astype(np.float32))


def test_host_checks_come_before_any_launch():
    from embodiedscan_amd import render as RD
    t = torch.zeros((2, 3, 4, 5), dtype=torch.uint8)
    eye = np.stack([np.eye(4)] * 2)
    for bad, msg in ((lambda: RD.render_boxes(t.float(), eye, eye, torch.zeros((0, 9)), np.zeros((0, 3), np.uint8)), 'uint8'),
                     (lambda: RD.render_boxes(torch.zeros((2, 3, 4, 3), dtype=torch.uint8), eye, eye, torch.zeros((0, 9)), np.zeros((0, 3), np.uint8)), 'layout'),
                     (lambda: RD.render_boxes(t, eye, eye, torch.zeros((1, 9)), np.zeros((1, 3), np.float32)), 'colors'),
                     (lambda: RD.render_occupancy(t, eye, eye, torch.zeros((2, 2), dtype=torch.long), (0, 0, 0, 1, 1, 1), np.zeros((3, 3), np.uint8)), '3-d')):
        with pytest.raises(ValueError, match=msg):
            bad()
