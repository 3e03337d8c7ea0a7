"""tests/det_metric_spec.py against the reference's own indoor_eval (tests/golden/det_metric.npz, recorded by
tools/make_golden_det_metric.py): the generic case and one case per quirk of the evaluator.  The spec performs the reference's numpy
operations, so everything is compared EXACTLY: the key set and its order, every value, the cumulative TP counts behind every
recall curve, the precision curves, and the per-split means as the reference prints them (four decimals)."""
import os

import numpy as np
import pytest

import det_metric_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ('generic', 'classes_split', 'pred_only', 'gt_only', 'pred_in_scene_without_gt', 'three_on_one', 'mid_iou', 'thin_clamp',
         'identical_gt')


def load_case(name):
    """-> dict(scenes, thr, classes, split, keys, vals, curves {(t, label): (recall, precision)}, split_tables)"""
    z = np.load(os.path.join(HERE, 'golden', 'det_metric.npz'))
    k = list(z['names']).index(name)
    pred, gt = z['pred'][z['pred'][:, 0] == k], z['gt'][z['gt'][:, 0] == k]
    n_scenes = int(max(pred[:, 1].max(initial=-1), gt[:, 1].max(initial=-1))) + 1
    scenes = []
    for s in range(n_scenes):
        p, g = pred[pred[:, 1] == s], gt[gt[:, 1] == s]
        scenes.append((p[:, 4:].astype(np.float32), p[:, 3].astype(np.float32), p[:, 2].astype(np.int64), g[:, 3:].astype(np.float32),
                       g[:, 2].astype(np.int64)))
    sel = z['vals'][:, 0] == k
    cur = z['curves'][z['curves'][:, 0] == k]
    curves = {}
    for t, lab in {(int(r[1]), int(r[2])) for r in cur}:
        rows = cur[(cur[:, 1] == t) & (cur[:, 2] == lab)]
        curves[t, lab] = (rows[:, 3], rows[:, 4])
    sp = z['splits'][z['splits'][:, 0] == k] if z['splits'].size else np.zeros((0, 3), np.int64)
    split = tuple(sp[sp[:, 1] == j][:, 2].tolist() for j in range(3)) if len(sp) else None
    tabs = [row[1:] for row in z['split_tables'] if int(row[0]) == k]
    return dict(scenes=scenes, thr=z['thr'][z['thr'][:, 0] == k][:, 1].tolist(), classes=[str(c) for c in z['classes']], split=split,
                keys=[str(x) for x in z['keys'][sel]], vals=z['vals'][sel][:, 1], curves=curves, split_tables=tabs)


def test_the_golden_holds_every_case():
    z = np.load(os.path.join(HERE, 'golden', 'det_metric.npz'))
    assert tuple(z['names']) == NAMES


@pytest.mark.parametrize('name', NAMES)
def test_spec_equals_the_reference(name):
    c = load_case(name)
    C = len(c['classes'])
    ev = S.evaluate(c['scenes'], C, c['thr'])
    ret = S.result_dict(c['scenes'], C, c['thr'], c['classes'], ev)
    assert list(ret) == c['keys']
    for key, want in zip(c['keys'], c['vals']):
        assert ret[key] == want, (key, ret[key], want)                      # bit for bit (no NaN survives the reference's filter)
    has_pred = np.diff(ev['cls_off']) > 0
    for (t, lab), (rec, prec) in c['curves'].items():
        if not has_pred[lab]:
            assert rec.tolist() == [0.0] and prec.tolist() == [0.0]           # ground truth only: the reference's np.zeros(1)
            continue
        np.testing.assert_array_equal(ev['recall'][t, lab], rec, err_msg=f'recall {t} {lab}')
        np.testing.assert_array_equal(ev['precision'][t, lab], prec, err_msg=f'precision {t} {lab}')
        r0, r1 = ev['cls_off'][lab], ev['cls_off'][lab + 1]
        np.testing.assert_array_equal(np.cumsum(ev['tp'][t, r0:r1]), np.rint(rec * ev['npos'][lab]).astype(np.int64), err_msg=f'TP flags {t} {lab}')
    kept = {lab for (_, lab) in c['curves']}
    assert kept == {cl for cl in range(C) if ev['npos'][cl] > 0}            # a class without ground truth is dropped
    if c['split'] is not None:
        means = S.split_means(c['scenes'], C, c['thr'], c['split'], ev)
        assert len(c['split_tables']) == 2 * len(means)
        for head, row in zip(c['split_tables'][0::2], c['split_tables'][1::2]):
            got = means[str(head[0]).replace('_classes', '')]
            assert [f'{got[str(h)]:.4f}' for h in head[1:]] == [str(v) for v in row[1:]]


def test_the_quirks_are_what_their_names_say():
    """the cases do exercise what they were built for (read off the spec, which the test above ties to the reference)"""
    ev = {n: S.evaluate(load_case(n)['scenes'], 5, [0.25, 0.5]) for n in NAMES[2:]}
    assert ev['pred_only']['npos'][3] == 0 and np.isnan(ev['pred_only']['ap'][0, 3])
    assert ev['gt_only']['npos'][2] == 1 and ev['gt_only']['cls_off'][3] == ev['gt_only']['cls_off'][2]
    assert np.isneginf(ev['pred_in_scene_without_gt']['iou_max'][1:]).all() and ev['pred_in_scene_without_gt']['gt_best'][1:].tolist() == [-1, -1]
    assert ev['three_on_one']['gt_best'][:3].tolist() == [0, 0, 0] and ev['three_on_one']['tp'][0].tolist() == [1, 0, 1, 0]
    assert 0.25 < ev['mid_iou']['iou_max'][0] < 0.5 and ev['mid_iou']['tp'][:, 0].tolist() == [1, 0]
    c = load_case('thin_clamp')['scenes'][0]
    from oracle import grounding as OG
    assert OG.box3d_iou(c[0][0], c[3][0]) < 0.25 < 0.5 < ev['thin_clamp']['iou_max'][0]      # the clamp moves it across both thresholds
    assert (S.clamp_thin(c[0][1]) == c[0][1]).all() and ev['thin_clamp']['iou_max'][1] < 0.25  # a face of exactly 2e-4 is not below it
    assert ev['identical_gt']['gt_best'].tolist() == [0, 0] and ev['identical_gt']['tp_total'][:, 0].tolist() == [1, 1]
