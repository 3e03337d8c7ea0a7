"""Host side of the walk sessions (CPU, no GPU): the meta rows a session builds frame by frame equal build_fusion_meta on the whole
walk -- for occupancy the one-view row of frame v is the header plus column block v of the V-view row, for detection the row of the
prefix so far is its first t + 1 blocks -- and pipeline.walk_frames hands out the row ranges of prefix_lengths."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scan(T=5, augment=True):
    from embodiedscan_amd.synth import make_scan
    return make_scan(31, n_views=T, height=60, width=80, img_size=(64, 64), n_points=500, n_boxes=3, augment=augment)


@pytest.mark.parametrize('augment', [False, True])
def test_session_meta_rows_equal_the_whole_walk(augment):
    from embodiedscan_amd.hip import CONSTS
    from embodiedscan_amd.models.detectors.walk import WalkMeta
    from embodiedscan_amd.models.layers.fusion_layers.point_fusion import build_fusion_meta
    T = 5
    scan = _scan(T, augment)
    meta, hw, PROJ = scan['meta'], (64, 64), CONSTS['ES_FUSE_PROJ']
    whole = build_fusion_meta([meta], 'DEPTH', hw, T)
    assert float(whole[0, PROJ:].abs().sum()) > 0 and (not augment or float(whole[0, CONSTS['ES_FUSE_NOPS']]) > 0)
    d2i = meta['depth2img']
    const = {k: v for k, v in meta.items()}
    const['depth2img'] = dict(origin=d2i['origin'])                       # what open_walk is given: nothing per frame
    wm = WalkMeta(const, 'DEPTH')
    assert wm.origin is d2i['origin'] and len(wm) == 0
    for t in range(T):
        frame = dict(extrinsic=d2i['extrinsic'][t], intrinsic=d2i['intrinsic'][t])
        one = wm.one_view(frame, hw)                                      # occupancy: the step kernel's row
        assert one.shape == (1, PROJ + 16)
        assert torch.equal(one[0, :PROJ], whole[0, :PROJ]), f'frame {t}: header'
        assert torch.equal(one[0, PROJ:], whole[0, PROJ + 16 * t:PROJ + 16 * (t + 1)]), f'frame {t}: its matrix is column block {t}'
        wm.add(frame)
        row = build_fusion_meta([wm.metainfo()], 'DEPTH', hw, t + 1)      # detection: what _fuse_points makes of the prefix so far
        assert torch.equal(row[0], whole[0, :PROJ + 16 * (t + 1)]), f'prefix {t}: the first {t + 1} blocks'
    assert len(wm) == T
    wm.pop()
    assert len(wm) == T - 1 and len(wm.metainfo()['depth2img']['intrinsic']) == T - 1
    wm.clear()
    assert len(wm) == 0 and wm.metainfo()['depth2img']['extrinsic'] == [] and 'origin' in wm.metainfo()['depth2img']


def test_walk_frames_row_ranges_are_the_prefix_lengths():
    from embodiedscan_amd import pipeline
    T = 5
    scan = _scan(T)
    rng = np.random.default_rng(3)
    sl = [0] + np.cumsum(rng.integers(60, 160, T)).tolist()
    for n_rows in (sl[-1], sl[-2] + 7, sl[2]):                           # the cloud ends inside the last slice / at an earlier one
        d = dict(meta=scan['meta'], points_slice_indices=sl)
        frames = list(pipeline.walk_frames(d, n_rows))
        assert [f[0] for f in frames] == list(range(T))
        ends = pipeline.prefix_lengths(sl, n_rows)
        assert [f[1][1] for f in frames] == ends
        assert [f[1][0] for f in frames] == [0] + ends[:-1], 'each frame starts where the one before ended'
        for t, (_, _, e, i) in enumerate(frames):
            assert e is scan['meta']['depth2img']['extrinsic'][t] and i is scan['meta']['depth2img']['intrinsic'][t]
    d = dict(meta=scan['meta'], points_slice_indices=sl, sel_pix=torch.zeros(sl[-1] - 11, dtype=torch.int32))
    assert [f[1][1] for f in pipeline.walk_frames(d)] == pipeline.prefix_lengths(sl, sl[-1] - 11), 'n_rows None: one row per chosen pixel'


def test_open_walk_refuses_more_frames_than_the_window_kernels_take():
    from embodiedscan_amd.config import build_detector
    det = build_detector(os.path.join(ROOT, 'configs', 'cont_det3d.py'), device='cpu')
    with pytest.raises(ValueError, match='max_frames'):
        det.open_walk({}, max_frames=65)
    with pytest.raises(ValueError, match='max_frames'):
        det.open_walk({}, max_frames=0)
    w = det.open_walk({}, max_frames=64)
    assert w.max_frames == 64 and w.t == 0 and w.state_bytes() == 0
