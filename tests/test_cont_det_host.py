"""Host side of the continuous detection path (CPU, no GPU): the cont-det3d configuration, the scan pipeline built from the
reference's train pipeline, pipeline.make_cont_det_batch and Det3DDataPreprocessor(batchwise_inputs=True) on its result.

make_cont_det_batch is compared with a LITERAL numpy restatement, written below, of the instance part of the reference's
ConstructMultiSweeps (multiview.py:192-222); the reference's own transform classes are not run."""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'reference_cont_det_config.json')
REL = 'detection/cont-det3d_8xb1_embodiedscan-3d-284class-9dof.py'


def _norm(d):
    if isinstance(d, dict):
        return {k: _norm(v) for k, v in d.items()}
    if isinstance(d, (list, tuple)):
        return [_norm(v) for v in d]
    return d


def _ref():
    with open(GOLDEN) as f:
        return json.load(f)['configs'][REL]


def test_cont_det_config_is_mirrored_and_builds():
    from embodiedscan_amd.config import build_detector, build_optim_wrapper, load_config
    from embodiedscan_amd.models.detectors.sparse_featfusion_single_stage import SparseFeatureFusionSingleStage3DDetector
    ref = _ref()
    loc = load_config(os.path.join(ROOT, 'configs', 'cont_det3d.py'))
    a = _norm(ref['model'])
    a['backbone'].pop('init_cfg', None)                                   # torchvision://resnet50: no checkpoints offline
    assert a == _norm(loc['model'])
    for k in ('optim_wrapper', 'train_pipeline', 'test_pipeline'):
        assert _norm(ref[k]) == _norm(loc[k]), k
    det = build_detector(ref, device='cpu')                               # the reference's model section, unchanged
    assert type(det).__name__ == 'Embodied3DDetector' and isinstance(det, SparseFeatureFusionSingleStage3DDetector)
    assert det.data_preprocessor.batchwise_inputs is True and det.predict_chunk >= 1
    assert det.bbox_head.pts_prune_threshold == 20000
    assert build_optim_wrapper(ref).lr == 2e-4
    mv = build_detector(os.path.join(ROOT, 'configs', 'mv_3ddet.py'), device='cpu')
    a, b = det.state_dict(), mv.state_dict()
    assert mv.data_preprocessor.batchwise_inputs is False
    assert sorted(a) == sorted(b) and all(a[k].shape == b[k].shape for k in a)


def test_scan_pipeline_from_the_reference_train_pipeline(tmp_path):
    """sweeps mode, 10 images of n_points // 10 points, flip and rot / scale / trans on; on a synthetic dataset the scan carries 11
    slice indices and one instance-visibility mask per frame"""
    from embodiedscan_amd import synth
    from embodiedscan_amd.datasets import EmbodiedScanDataset
    from embodiedscan_amd.datasets.loading import ScanPipeline
    ref = _ref()
    tr, te = ScanPipeline.from_cfg(ref['train_pipeline']), ScanPipeline.from_cfg(ref['test_pipeline'])
    assert (tr.n_images, tr.ordered, tr.sweeps, tr.view_points) == (10, False, True, 10000)
    assert (te.n_images, te.ordered, te.sweeps, te.view_points) == (50, True, True, 10000)
    assert tr.aug['flip'] and tr.aug['rst'] and tr.point_range is None and not tr.with_occupancy
    assert not te.aug['flip'] and not te.aug['rst']
    _, names = synth.write_dataset(str(tmp_path), n_scans=1, n_frames=12, n_voxels=(8, 8, 4), seed=5)
    pipe = [dict(t, transforms=[dict(u, num_points=200) if u['type'] == 'PointSample' else
                                (dict(u, scale=(64, 48)) if u['type'] == 'Resize' else u) for u in t['transforms']])
            if t['type'] == 'MultiViewPipeline' else t for t in ref['train_pipeline']]
    sp = ScanPipeline.from_cfg(pipe)
    assert sp.sweeps and sp.n_images == 10 and sp.view_points == 200
    ds = EmbodiedScanDataset(str(tmp_path), 'embodiedscan_infos_train.pkl', metainfo=dict(classes=names), pipeline=pipe)
    sc = ds.load_scan(0, np.random.RandomState(2))
    assert sc['points_slice_indices'] == [200 * i for i in range(11)]
    vm = sc['visible_instance_masks']
    assert len(vm) == 10 and all(len(m) == len(sc['gt_labels']) for m in vm)
    assert 'pcd_rotation' in sc['meta'] and 'pcd_horizontal_flip' in sc['meta']


def _restated_instances(gt_bboxes_3d, gt_labels_3d, visible_instance_masks, points_slice_indices):
    """the instance part of ConstructMultiSweeps (multiview.py:192-222) on numpy arrays -> per-prefix boxes and labels"""
    visible_instance_ids = []
    for idx in range(len(visible_instance_masks)):
        visible_instance_ids.append(set(np.argwhere(np.array(visible_instance_masks[idx])).flatten()))
    cumulated_ids = set(visible_instance_ids[0])
    indices = np.array(list(cumulated_ids), dtype=np.int32)
    batch_gt_bboxes_3d = [gt_bboxes_3d[indices]]
    batch_gt_labels_3d = [gt_labels_3d[indices]]
    for idx in range(1, len(points_slice_indices) - 1):
        cumulated_ids = cumulated_ids.union(visible_instance_ids[idx])
        indices = np.array(list(cumulated_ids), dtype=np.int32)
        batch_gt_bboxes_3d.append(gt_bboxes_3d[indices])
        batch_gt_labels_3d.append(gt_labels_3d[indices])
    return batch_gt_bboxes_3d, batch_gt_labels_3d


def _cpu_scan(T=5, G=12, n=700, seed=4):
    """a `dscan` on the CPU with the cloud already un-projected (make_batch is patched to hand it over): frame 0 sees nothing, later
    frames add instances out of index order, ids whose set iteration order is not ascending ({8, 1})"""
    rng = np.random.default_rng(seed)
    vis = np.zeros((T, G), dtype=bool)
    vis[1, [8, 1]] = True
    vis[2, [11, 1, 3]] = True
    vis[3, [0, 8]] = True
    vis[4, [10, 2, 9, 5]] = True
    sl = [0] + np.cumsum(rng.integers(60, 160, T)).tolist()
    return dict(points=torch.from_numpy(rng.random((n, 3)).astype(np.float32)), points_slice_indices=sl, visible_instance_masks=list(vis),
                gt_boxes=rng.random((G, 9)).astype(np.float32), gt_labels=rng.integers(0, 284, G), meta=dict(scan_id='s', img_shape=(48, 64)),
                img=torch.zeros((T, 3, 48, 64), dtype=torch.uint8))


def test_make_cont_det_batch_follows_construct_multi_sweeps(monkeypatch):
    from embodiedscan_amd import pipeline
    from embodiedscan_amd.models.data_preprocessors.data_preprocessor import Det3DDataPreprocessor
    monkeypatch.setattr(pipeline, 'depth_to_points', lambda d: d['points'])
    T = 5
    d = _cpu_scan(T)
    n = d['points'].shape[0]
    assert d['points_slice_indices'][-1] < n or d['points_slice_indices'][-2] < n
    data = pipeline.make_cont_det_batch(d)
    want_b, want_l = _restated_instances(d['gt_boxes'], d['gt_labels'], d['visible_instance_masks'], d['points_slice_indices'])
    pts = data['inputs']['points']
    assert len(pts) == T == len(want_b) and len(data['data_samples']) == 1
    assert [len(p) for p in pts] == [min(e, n) for e in d['points_slice_indices'][1:]]
    assert all(p.data_ptr() == pts[0].data_ptr() for p in pts), 'the prefixes are views of one buffer'
    gi = data['data_samples'][0].gt_instances_3d
    assert len(gi.bboxes_3d) == T and len(gi.labels_3d) == T
    for t in range(T):
        np.testing.assert_array_equal(gi.bboxes_3d[t].tensor.numpy(), want_b[t], err_msg=f'boxes of prefix {t} (order included)')
        np.testing.assert_array_equal(gi.labels_3d[t].numpy(), want_l[t], err_msg=f'labels of prefix {t} (order included)')
    assert tuple(gi.bboxes_3d[0].tensor.shape) == (0, 9) and len(gi.labels_3d[0]) == 0, 'frame 0 sees no instance'
    assert [len(l) for l in gi.labels_3d] == [0, 2, 4, 5, 9]
    order = [int(i) for i in np.array(list(set(np.argwhere(d['visible_instance_masks'][1]).flatten())), dtype=np.int32)]
    assert sorted(order) == [1, 8]
    np.testing.assert_array_equal(gi.labels_3d[1].numpy(), d['gt_labels'][order])
    # an explicit visibility argument replaces the scan's
    vis2 = [np.ones(12, dtype=bool)] * T
    g2 = pipeline.make_cont_det_batch(d, vis2)['data_samples'][0].gt_instances_3d
    assert all(len(l) == 12 for l in g2.labels_3d)
    # batchwise_inputs: T samples with the right boxes each
    out = Det3DDataPreprocessor(batchwise_inputs=True, device='cpu')({'inputs': {'points': pts}, 'data_samples': data['data_samples']}, True)
    assert len(out['data_samples']) == T and len(out['inputs']['points']) == T
    for t, ds in enumerate(out['data_samples']):
        assert ds.gt_instances_3d.bboxes_3d is gi.bboxes_3d[t] and ds.gt_instances_3d.labels_3d is gi.labels_3d[t]
        assert ds.metainfo == data['data_samples'][0].metainfo


def test_detector_refuses_batches_that_are_not_one_walk_through():
    """B = 1 and one sample / one cloud per view, checked before any launch"""
    import pytest
    from embodiedscan_amd.config import build_detector
    det = build_detector(_ref(), device='cpu')
    img = torch.zeros(2, 3, 3, 32, 32)
    with pytest.raises(AssertionError, match='image batch'):
        det.extract_feat({'imgs': img, 'points': [torch.zeros(4, 3)] * 3}, [None] * 3)
    with pytest.raises(AssertionError, match='one data sample per prefix'):
        det.extract_feat({'imgs': img[:1], 'points': [torch.zeros(4, 3)] * 3}, [None] * 2)
    with pytest.raises(AssertionError, match='one cumulative cloud'):
        det.predict({'imgs': img[:1], 'points': [torch.zeros(4, 3)] * 2}, [None] * 3)
