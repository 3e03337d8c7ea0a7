"""Host side of the continuous occupancy path (CPU, no GPU): the cont-occ configuration, the sweeps mode of the scan pipeline and
Det3DDataPreprocessor(batchwise_inputs=True).

The sweeps checks compare the scan pipeline with a LITERAL numpy restatement, written below, of the reference's
AggregateMultiViewPoints(save_slices=True) -> PointsRangeFilter -> ConstructMultiSweeps (multiview.py:139-169,179-246,
points.py:246-277) applied to the unfiltered cloud of the same scan and seed; the reference's own transform classes are not run
(no recorded tests/golden/cont_sweeps.npz)."""
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'reference_cont_configs.json')
REL = 'occupancy/cont-occ_8xb1_embodiedscan-occ-80class.py'


def _norm(d):
    if isinstance(d, dict):
        return {k: _norm(v) for k, v in d.items()}
    if isinstance(d, (list, tuple)):
        return [_norm(v) for v in d]
    return d


def _ref():
    with open(GOLDEN) as f:
        return json.load(f)['configs'][REL]


def test_cont_occ_config_is_mirrored_and_builds():
    from embodiedscan_amd.config import build_detector, build_optim_wrapper, load_config
    from embodiedscan_amd.models.detectors.dense_fusion_occ import DenseFusionOccPredictor
    ref = _ref()
    loc = load_config(os.path.join(ROOT, 'configs', 'cont_occ.py'))
    a = _norm(ref['model'])
    a['backbone'].pop('init_cfg', None)                                   # torchvision://resnet50: no checkpoints offline
    assert a == _norm(loc['model'])
    for k in ('optim_wrapper', 'train_pipeline', 'test_pipeline'):
        assert _norm(ref[k]) == _norm(loc[k]), k
    det = build_detector(ref, device='cpu')                               # the reference's model section, unchanged
    assert type(det).__name__ == 'EmbodiedOccPredictor' and isinstance(det, DenseFusionOccPredictor)
    assert det.data_preprocessor.batchwise_inputs is True
    assert build_optim_wrapper(ref).lr == 1e-4
    mv = build_detector(os.path.join(ROOT, 'configs', 'mv_occ.py'), device='cpu')
    assert mv.data_preprocessor.batchwise_inputs is False and sorted(mv.state_dict()) == sorted(det.state_dict())


def test_scan_pipeline_reads_both_cont_occ_pipelines():
    import pytest
    from embodiedscan_amd.datasets.loading import ScanPipeline
    ref = _ref()
    tr, te = ScanPipeline.from_cfg(ref['train_pipeline']), ScanPipeline.from_cfg(ref['test_pipeline'])
    assert (tr.n_images, tr.ordered, tr.sweeps, tr.view_points) == (10, False, True, 10000)
    assert (te.n_images, te.ordered, te.sweeps, te.view_points) == (20, True, True, 10000)
    assert tr.point_range == tuple(ref['model']['point_cloud_range']) and tr.with_occupancy and not tr.view_masks
    mv = ScanPipeline.from_cfg([t for t in ref['train_pipeline'] if t['type'] != 'ConstructMultiSweeps'])
    assert mv.sweeps is False                                             # save_slices alone changes nothing
    bad = list(ref['train_pipeline'])
    bad.insert(4, dict(type='PointSample', num_points=1000))              # slices of a re-drawn cloud are meaningless
    with pytest.raises(AssertionError, match='PointSample'):
        ScanPipeline.from_cfg(bad)
    with pytest.raises(AssertionError, match='save_slices'):
        ScanPipeline.from_cfg([dict(t, save_slices=False) if t['type'] == 'AggregateMultiViewPoints' else t for t in ref['train_pipeline']])


VIEWS = [dict(type='LoadImageFromFile'), dict(type='LoadDepthFromFile'), dict(type='ConvertRGBDToPoints', coord_type='CAMERA'),
         dict(type='PointSample', num_points=300), dict(type='Resize', scale=(64, 48), keep_ratio=False)]


def _pipe(n_images, box, sweeps=True):
    p = [dict(type='LoadAnnotations3D', with_occupancy=True, with_visible_occupancy_masks=True, with_visible_instance_masks=True),
         dict(type='MultiViewPipeline', n_images=n_images, transforms=VIEWS),
         dict(type='AggregateMultiViewPoints', coord_type='DEPTH', save_slices=True)]
    if box is not None:
        p.append(dict(type='PointsRangeFilter', point_cloud_range=box))
    if sweeps:
        p.append(dict(type='ConstructMultiSweeps'))
    return p + [dict(type='Pack3DDetInputs', keys=['img', 'points', 'gt_bboxes_3d', 'gt_labels_3d', 'gt_occupancy'])]


def _restated_sweeps(cloud, frame_of_point, box, visible_masks):
    """the three reference transforms on an aggregated cloud (numpy): -> slice indices, the T cumulative clouds, the T masks"""
    # AggregateMultiViewPoints(save_slices=True), multiview.py:143-156
    points_slice_indices = [0]
    for idx in range(int(frame_of_point.max()) + 1 if len(frame_of_point) else 0):
        points_slice_indices.append(points_slice_indices[-1] + int((frame_of_point == idx).sum()))
    # PointsRangeFilter, points.py:256-263 (BasePoints.in_range_3d: strict on all six faces); the slice indices are NOT touched
    if box is not None:
        lo, hi = np.asarray(box[:3], np.float32), np.asarray(box[3:], np.float32)
        points_mask = np.all((cloud > lo) & (cloud < hi), axis=1)
        clean_points = cloud[points_mask]
        if not len(clean_points) < 100:
            cloud = clean_points
    # ConstructMultiSweeps, multiview.py:183-227
    cumulated_points = cloud[points_slice_indices[0]:points_slice_indices[1]]
    batch_points = [cumulated_points]
    cumulated_masks = visible_masks[0]
    batch_gt_occupancy_masks = [visible_masks[0]]
    for idx in range(1, len(points_slice_indices) - 1):
        start, end = points_slice_indices[idx], points_slice_indices[idx + 1]
        cumulated_points = np.concatenate([cumulated_points, cloud[start:end]])
        batch_points.append(cumulated_points)
        cumulated_masks = np.logical_or(cumulated_masks, visible_masks[idx])
        batch_gt_occupancy_masks.append(cumulated_masks)
    return points_slice_indices, batch_points, batch_gt_occupancy_masks


def test_sweeps_follow_the_reference_transforms_stale_slices_included(tmp_path):
    """slice indices, the prefixes of the FILTERED cloud and the cumulative masks equal the restatement; with a range that removes
    points the stale indices matter (the prefixes differ from `the points of frames 0 .. t`), without one they do not; the sweeps
    pipeline consumes exactly the RNG values of view choice + per-frame draws"""
    from embodiedscan_amd import pipeline, synth
    from embodiedscan_amd.datasets import EmbodiedScanDataset
    from embodiedscan_amd.datasets.loading import sample_pixels, select_views
    from oracle import pipeline as OP
    _, names = synth.write_dataset(str(tmp_path), n_scans=1, n_frames=6, n_voxels=(8, 8, 4), seed=9)
    mk = lambda p: EmbodiedScanDataset(str(tmp_path), 'embodiedscan_infos_train.pkl', metainfo=dict(classes=names, occ_classes=names),  # noqa: E731
                                       pipeline=p)
    T = 4
    # the unfiltered aggregated cloud of the same seed (the range filter draws nothing, so the pixel choices are the same)
    rng_all = np.random.RandomState(1)
    sc_all = mk(_pipe(T, None)).load_scan(0, rng_all)
    cloud, frame = OP.scan_to_points(sc_all).numpy(), sc_all['sel_view']
    assert cloud.shape == (T * 300, 3) and bool((np.diff(frame) >= 0).all()), 'all V * view_points points, in frame order'
    assert sc_all['points_slice_indices'] == [0, 300, 600, 900, 1200]
    differs = {}
    for name, box in (('filter removes points', [-2.0, -1.5, -0.5, 3.2, 1.5, 2.0]), ('filter removes nothing', [-50, -50, -50, 50, 50, 50]),
                      ('no filter', None)):
        sc = mk(_pipe(T, box)).load_scan(0, np.random.RandomState(1))
        sl, clouds, masks = _restated_sweeps(cloud, frame, box, sc['visible_occupancy_masks'])
        assert sc['points_slice_indices'] == sl, name
        pts = OP.scan_to_points(sc).numpy()
        lens = pipeline.prefix_lengths(sc['points_slice_indices'], len(pts))
        assert len(lens) == T == len(sc['gt_occupancy_masks']) == len(masks)
        for t in range(T):
            np.testing.assert_array_equal(pts[:lens[t]], clouds[t], err_msg=f'{name}: prefix {t}')
            np.testing.assert_array_equal(sc['gt_occupancy_masks'][t], masks[t])
            np.testing.assert_array_equal(masks[t], np.logical_or.reduce(sc['visible_occupancy_masks'][:t + 1]))
        # what a slicing by frame membership would give: the filtered points of frames 0 .. t
        fr = sc['sel_view']
        differs[name] = [lens[t] != int((fr <= t).sum()) for t in range(T)]
        if name == 'filter removes points':
            assert len(pts) < len(cloud) and len(pts) >= 100
    assert any(differs['filter removes points']), 'the range must remove points of an early frame, else the stale indices are not exercised'
    assert not any(differs['filter removes nothing']) and not any(differs['no filter'])
    # RNG: view choice, then one draw per frame -- nothing for an aggregated draw
    rng_b = np.random.RandomState(1)
    ids = select_views(6, T, False, rng_b)
    for j in range(len(ids)):
        sample_pixels(np.ascontiguousarray(sc_all['depth'][j]), 300, rng_b, True)
    assert rng_all.randint(0, 2 ** 31 - 1) == rng_b.randint(0, 2 ** 31 - 1), 'the sweeps pipeline drew more (or fewer) random values'


def _sample(T, with_boxes):
    from embodiedscan_amd.structures import Det3DDataSample, EulerDepthInstance3DBoxes, InstanceData
    g = torch.Generator().manual_seed(3)
    if with_boxes:
        gi = InstanceData(bboxes_3d=[EulerDepthInstance3DBoxes(torch.rand(t + 1, 9, generator=g)) for t in range(T)],
                          labels_3d=[torch.arange(t + 1) for t in range(T)])
    else:
        gi = InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(torch.rand(5, 9, generator=g)), labels_3d=torch.arange(5))
    ds = Det3DDataSample(dict(scan_id='s', img_shape=(48, 64)), gi)
    ds.gt_occupancy = torch.randint(0, 8, (30, 4), generator=g)
    ds.gt_occupancy_masks = [torch.rand(8, 8, 4, generator=g) < 0.2 * (t + 1) for t in range(T)]
    return ds


def test_preprocessor_batchwise_inputs_makes_one_sample_per_prefix():
    from embodiedscan_amd.models.data_preprocessors.data_preprocessor import Det3DDataPreprocessor
    T = 4
    pts = [torch.rand(10 * (t + 1), 3) for t in range(T)]
    for with_boxes in (False, True):
        src = _sample(T, with_boxes)
        out = Det3DDataPreprocessor(batchwise_inputs=True, device='cpu')({'inputs': {'points': pts}, 'data_samples': [src]}, True)
        ss = out['data_samples']
        assert len(ss) == T and len(out['inputs']['points']) == T
        for t, ds in enumerate(ss):
            assert ds.metainfo == src.metainfo and ds.gt_occupancy is src.gt_occupancy
            assert ds.gt_occupancy_masks is src.gt_occupancy_masks[t]
            if with_boxes:
                assert ds.gt_instances_3d.bboxes_3d is src.gt_instances_3d.bboxes_3d[t]
                assert ds.gt_instances_3d.labels_3d is src.gt_instances_3d.labels_3d[t] and len(ds.gt_instances_3d.labels_3d) == t + 1
            else:
                assert ds.gt_instances_3d is src.gt_instances_3d
        ss[0].set_metainfo({'pad_shape': (1, 1)})                       # a copy's meta is its own dict
        assert 'pad_shape' not in src.metainfo and 'pad_shape' not in ss[1].metainfo
    # the default leaves the samples alone: the very list comes back
    src = _sample(T, False)
    samples = [src]
    out = Det3DDataPreprocessor(device='cpu')({'inputs': {'points': pts}, 'data_samples': samples}, True)
    assert out['data_samples'] is samples and isinstance(src.gt_occupancy_masks, list)
    assert Det3DDataPreprocessor(device='cpu').batchwise_inputs is False
