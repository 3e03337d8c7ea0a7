"""tests/scene_map_spec.py against answers known by construction (CPU): a camera looking straight down with dyadic intrinsics, depths and
grid, so every product of the splat is exact and each pixel lands in a cell and at a height step that can be written down."""
import json

import numpy as np
import pytest

import render_spec as RS
import scene_map_spec as S

H, W, F = 4, 8, 8.0                       # focal 8 px: at depth d a pixel step is d / 8 metres
EYE = (1.0, 2.0, 3.0)


def _down(eye=EYE):
    E, K = S.down_camera(eye, F, H, W)
    return RS.rays_of(E[None], K[None])


def _grid(Wm=8, Hm=8, cell=0.25, x0=0.0, y0=1.0, z_min=0.0, z_max=2.0):
    return S.Grid(x0, y0, cell, Wm, Hm, z_min, z_max, 8.0)


def _frames(seed=0):
    return np.random.default_rng(seed).integers(0, 256, (1, H, W, 3), dtype=np.uint8)


def test_every_pixel_lands_in_its_known_cell():
    """depth 2 everywhere: pixel (x, y) -> X = 1 + 2 (x - 4) / 8 = x / 4, Y = 2 - 2 (y - 2) / 8 = 2.5 - y / 4, Z = 1: cell ix = x exactly on
    the lower edge of cell x (an edge point belongs to the upper cell), iy = 6 - y, zq = 1024"""
    rays, G, fr = _down(), _grid(), _frames()
    depth = np.full((1, H, W), 2.0, np.float32)
    key, cell = S.pixel_keys(depth, fr, 0, rays, G, exact=True)
    for y in range(H):
        for x in range(W):
            r, g, b = (int(c) for c in fr[0, y, x])
            assert cell[0, y, x] == (G.height - 1 - (6 - y)) * G.width + x, (x, y)
            assert key[0, y, x] == ((1024 + 1) << 24) | (r << 16) | (g << 8) | b
    keys = S.splat(depth, fr, 0, rays, G, exact=True)
    assert (keys != 0).sum() == H * W and not keys[:1].any() and not keys[5:].any()
    img, hz = S.resolve(keys, G, (1, 2, 3), 0)
    assert np.array_equal(img[1:5], fr[0]) and (img[0] == (1, 2, 3)).all()
    assert np.all(hz[1:5] == np.float32(1.0 + 0.5 / 1024)) and np.isnan(hz[0]).all()
    with pytest.raises(AssertionError, match='boundary'):
        S.splat(depth, fr, 0, rays, G)                          # not marked exact: the spec refuses its own edge cases


def test_z_cut_is_half_open():
    rays, fr = _down(), _frames()
    depth = np.full((1, H, W), 2.0, np.float32)                 # every point at z = 1
    assert (S.splat(depth, fr, 0, rays, _grid(z_min=1.0, z_max=2.0), exact=True) >> 24 == 1).sum() == H * W, 'z == z_min is kept at zq = 0'
    assert not S.splat(depth, fr, 0, rays, _grid(z_min=0.0, z_max=1.0), exact=True).any(), 'z == z_max is dropped'
    depth[0, 0, 0], depth[0, 0, 1], depth[0, 0, 2], depth[0, 0, 3] = 0.0, -2.0, np.nan, np.inf
    depth[0, 0, 4] = 8.5                                        # beyond max_depth
    assert (S.splat(depth, fr, 0, rays, _grid(z_min=-8.0), exact=True) != 0).sum() == H * W - 5


def test_the_higher_point_wins_and_ties_go_to_the_larger_colour():
    """cells of 1 m: pixels x = 4 .. 7 of row 1 (X = 1 .. 1.75, Y = 2.25) share cell (1, 1)"""
    rays, G = _down(), _grid(Wm=2, Hm=2, cell=1.0)
    fr = np.zeros((1, H, W, 3), np.uint8)
    fr[0, 1, 4:8] = ((1, 9, 9), (200, 0, 0), (3, 250, 250), (3, 251, 0))
    depth = np.zeros((1, H, W), np.float32)
    depth[0, 1, 4:8] = 2.0
    depth[0, 1, 4] = 1.5                                        # the grey point is higher: z = 1.5 against 1.0
    keys = S.splat(depth, fr, 0, rays, G, exact=True)
    assert keys[0, 1] == ((1536 + 1) << 24) | (1 << 16) | (9 << 8) | 9 and (keys != 0).sum() == 1
    depth[0, 1, 4] = 2.0                                        # all four at z = 1: the largest packed colour, (200, 0, 0)
    assert S.splat(depth, fr, 0, rays, G, exact=True)[0, 1] == ((1024 + 1) << 24) | (200 << 16)
    depth[0, 1, 5] = 0.0                                        # without it (3, 251, 0) beats (3, 250, 250)
    assert S.splat(depth, fr, 0, rays, G, exact=True)[0, 1] == ((1024 + 1) << 24) | (3 << 16) | (251 << 8)
    assert S.census(depth, fr, 0, rays, G, exact=True) == dict(accepted=3 / 32, shared=1.0, ties=1)


def test_views_in_any_order_and_grouping():
    rays, depth, G = S.scene(3, 48, 64, 64, 64, 2)
    fr = S.banded_frames(3, 50, 130, 1, 3)
    whole = S.splat(depth, fr, 1, rays, G)
    cen = S.census(depth, fr, 1, rays, G)
    assert cen['accepted'] >= 0.25 and cen['shared'] >= 0.1 and cen['ties'] >= 1, cen
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        acc = None
        for v in order:
            acc = S.splat(depth[v:v + 1], fr[v:v + 1], 1, rays[v:v + 1], G, keys=acc)
        assert np.array_equal(acc, whole), order
    perm = [2, 0, 1]
    assert np.array_equal(S.splat(depth[perm], fr[perm], 1, rays[perm], G), whole)
    hwc = np.ascontiguousarray(fr.transpose(0, 2, 3, 1))
    assert np.array_equal(S.splat(depth, hwc, 0, rays, G), whole)


def test_nearest_frame_pixel_and_identity():
    rays, G = _down(), _grid()
    depth = np.full((1, H, W), 2.0, np.float32)
    small = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(1, 2, 3, 3)           # frames of 2 x 3 against depth of 4 x 8
    key, _ = S.pixel_keys(depth, small, 0, rays, G, exact=True)
    for y in range(H):
        for x in range(W):
            assert key[0, y, x] & 0xff == small[0, (2 * y + 1) * 2 // (2 * H), (2 * x + 1) * 3 // (2 * W), 2]
    assert [(2 * x + 1) * W // (2 * W) for x in range(W)] == list(range(W))


def test_shading_grows_with_height_and_stays_a_byte():
    G = _grid(Wm=3, Hm=1, z_max=1.0)
    assert G.nz == 1024
    keys = np.array([[(1 << 24) | 0xffffff, (1024 << 24) | 0xffffff, (1025 << 24) | 0xffffff]], np.int64)     # zq = 0, the top step, one beyond
    img, _ = S.resolve(keys, G, (0, 0, 0), 1)
    assert img[0, 0, 0] == (255 * 160 + 128) >> 8 and img[0, 1, 0] == 255 and img[0, 2, 0] == 255


def test_a_footprint_lies_where_the_perspective_draw_puts_the_top_face():
    """a box straight under the camera: the top face (z = 1, two metres below the lens) projects to (4 + 4 X', 2 - 4 Y') pixels; the map with
    cells of 1 / 4 m whose origin puts the camera at pixel (4, 2) shows the footprint at exactly those quarter-pixels"""
    E, K = S.down_camera(EYE, F, H, W)
    box = np.array([[1.0, 2.0, 0.5, 1.0, 0.5, 1.0, 0.0, 0.0, 0.0]], np.float32)
    rec = RS.project(box, E[None].astype(np.float32), K[None].astype(np.float32), check=False)[0, 0]
    G = S.Grid(0.0, 2.0 - (H - 2) * 0.25, 0.25, W, H)
    top = S.project(box, G, exact=True)[0, 0]
    for k in range(4, 8):                                       # the four corners with +z: the top face
        assert (rec[2 * k], rec[2 * k + 1]) == (top[2 * k], top[2 * k + 1]), k
    assert top[16] == 255 and list(top[17:21]) == [4 * 2, 4 * 1, 4 * 6, 4 * 3]
    img = S.draw_boxes(np.zeros((H, W, 3), np.uint8), box, np.array([[10, 20, 30]], np.uint8), G, exact=True)
    persp = RS.draw_boxes(np.zeros((1, H, W, 3), np.uint8), 0, rec[None, None], np.array([[10, 20, 30]], np.uint8))[0]
    assert (img[1:3, 2:6] != 0).all() and np.array_equal(img != 0, persp != 0)


def test_guard_band_and_trail_disc():
    G = _grid()
    far = np.array([[0.25 * 5000, 1.0, 0, 0, 0, 0, 0, 0, 0], [0.5, 1.5, 0, 0, 0, 0, 0, 0, 0]], np.float32)
    rec = S.project(far, G, exact=True)[0]
    assert rec[0, 16] == 0 and rec[0, 17] > rec[0, 19] and rec[1, 16] == 255
    img = S.draw_trail(np.zeros((8, 8, 3), np.uint8), far[1:, :3], (255, 255, 255), G, radius_q=6, exact=True)
    on = (img != 0).any(-1)                                      # the disc of radius 1.5 px round the pixel corner (2, 6): the four centres 0.71 px away
    assert on[5:7, 1:3].all() and on.sum() == 4


def test_a_one_voxel_volume():
    G = _grid(Wm=4, Hm=4, cell=0.5, x0=0.0, y0=0.0)
    base = np.full((4, 4, 3), 100, np.uint8)
    pal = np.array([[0, 0, 0], [200, 100, 0]], np.uint8)
    occ = np.ones((1, 1, 1), np.uint8)
    img = S.draw_occupancy(base, occ, (0.5, 0.0, 0.0), (1.0, 1.0, 1.0), pal, G, 128)        # the voxel [0.5, 1.5) x [0, 1): pixel centres .75, 1.25
    assert (img[2:4, 1:3] == (150, 100, 50)).all() and (img[:2] == 100).all() and (img[:, 0] == 100).all() and (img[:, 3] == 100).all()
    for label in (0, 2, 255):                                   # empty, and labels the palette does not hold
        assert np.array_equal(S.draw_occupancy(base, np.full((1, 1, 1), label, np.uint8), (0.5, 0, 0), (1, 1, 1), pal, G), base)
    tall = np.array([[[1, 0, 3, 1, 0, 2]]], np.uint8)           # the highest voxel with 1 <= label < C
    pal3 = np.array([[0, 0, 0], [255, 0, 0], [0, 255, 0]], np.uint8)
    assert (S.draw_occupancy(base, tall, (0.5, 0, 0), (1, 1, 1), pal3, G, 0)[3, 1] == (0, 255, 0)).all()
    assert (S.draw_occupancy(base, tall[:, :, :5], (0.5, 0, 0), (1, 1, 1), pal3, G, 0)[3, 1] == (255, 0, 0)).all()


def test_map_json_round_trip():
    from embodiedscan_amd.scene_map import MapGrid
    g = MapGrid.around(np.array([[0.3, -1.2, 1.5], [2.7, 0.4, 1.4]]), reach=1.0, cell=0.25, z_min=-0.5, z_max=2.5)
    assert (g.x0, g.y0, g.width, g.height) == (-0.75, -2.25, 18, 15)
    back = MapGrid.from_json(json.loads(json.dumps(g.to_json())))
    assert back.to_json() == g.to_json()
    xy = np.array([[0.3, -1.2], [3.7, 1.4], [-0.7, -2.2]])
    px = back.to_pixels(xy)
    assert np.allclose(back.to_metres(px), xy, atol=1e-12)
    assert np.allclose(px[0], ((0.3 + 0.75) / 0.25, 15 - (-1.2 + 2.25) / 0.25))
    G = S.Grid(g.x0, g.y0, g.cell, g.width, g.height)
    rec = S.project(np.array([[0.3, -1.2, 0, 0, 0, 0, 0, 0, 0]], np.float32), G)[0, 0]
    assert (rec[0], rec[1]) == tuple(int(np.floor(4 * c + 0.5)) for c in back.to_pixels(np.float32([0.3, -1.2]).astype(np.float64)))
    with pytest.raises(ValueError, match=r'a cell of .* m or more fits'):
        MapGrid.around(np.zeros((1, 2)), reach=50.0, cell=0.02)
    assert MapGrid.around(np.zeros((1, 2)), reach=8.0, cell=0.02).width == 800


@pytest.mark.parametrize('flags', [['--map-cell', '0.1'], ['--map-z', '-1', '2']])
def test_map_flags_are_refused_without_map(flags, capsys):
    """--map-cell / --map-z shape the map --map writes; alone they would be given in vain, so the command line refuses them before the
    model is built"""
    import os
    from embodiedscan_amd import inference as I
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs', 'mv_3ddet.py')
    with pytest.raises(SystemExit) as e:
        I.main([cfg, '--root-dir', 'nowhere'] + flags)
    assert e.value.code == 2 and '--map DIR' in capsys.readouterr().err
