"""tests/eval_metric_spec.py against the reference's own GroundingMetric.ground_eval and OccupancyMetric.process + compute_metrics
(tests/golden/ground_metric.npz, tests/golden/occ_metric.npz, recorded by tools/make_golden_eval_metrics.py): a generic case and one
case per quirk of either metric.  The spec performs the reference's arithmetic, so the dicts are compared BIT FOR BIT: the key set,
its order and every value.  The denominator of the grounding metric (1e-14 + 1.0 + 1.0 + ...) is checked against the sequential
loop for every n up to 100 000; that needs no reference run."""
import os

import numpy as np
import pytest

import eval_metric_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
GROUND = ('generic', 'slot10_hit', 'rank11_miss', 'few_queries', 'no_gt', 'three_gt_last', 'mid_iou', 'empty_category', 'single_sample')
OCC = ('generic', 'duplicates', 'no_mask', 'all_hidden', 'gt_only_pred_only', 'pred_label_ge_C')


def load_ground(name):
    """-> dict(samples [(boxes, target scores, gt boxes, (view_dep, hard, unique))], thr, keys, vals)"""
    z = np.load(os.path.join(HERE, 'golden', 'ground_metric.npz'))
    k = list(z['names']).index(name)
    rows = z['samples'][z['samples'][:, 0] == k]
    boxes, gt = z['boxes'][z['boxes'][:, 0] == k], z['gt'][z['gt'][:, 0] == k]
    samples = []
    for r in rows:
        b, g = boxes[boxes[:, 1] == r[1]], gt[gt[:, 1] == r[1]]
        samples.append((b[:, 3:].astype(np.float32), b[:, 2].astype(np.float32), g[:, 2:].astype(np.float32).reshape(-1, 9),
                        (bool(r[2]), bool(r[3]), bool(r[4]))))
    sel = z['vals'][:, 0] == k
    return dict(samples=samples, thr=z['thr'][z['thr'][:, 0] == k][:, 1].tolist(), keys=[str(x) for x in z['keys'][sel]],
                vals=z['vals'][sel][:, 1])


def load_occ(name):
    """-> dict(samples [(pred (X,Y,Z) int64, gt list (M,4) int64, mask or None)], classes, keys, vals, raised)"""
    z = np.load(os.path.join(HERE, 'golden', 'occ_metric.npz'))
    k = list(z['names']).index(name)
    samples, o = [], 0
    for r in z['dims']:
        n = int(r[2] * r[3] * r[4])
        if r[0] == k:
            shape = tuple(int(v) for v in r[2:5])
            lst = z['gt_list'][(z['gt_list'][:, 0] == k) & (z['gt_list'][:, 1] == r[1])][:, 2:]
            samples.append((z['pred'][o:o + n].reshape(shape), lst, z['mask'][o:o + n].reshape(shape).astype(bool) if r[5] else None))
        o += n
    sel = z['vals'][:, 0] == k
    return dict(samples=samples, classes=[str(c) for c in z['classes']], keys=[str(x) for x in z['keys'][sel]], vals=z['vals'][sel][:, 1],
                raised=bool(z['raised'][k]))


def test_the_goldens_hold_every_case():
    assert tuple(np.load(os.path.join(HERE, 'golden', 'ground_metric.npz'))['names']) == GROUND
    assert tuple(np.load(os.path.join(HERE, 'golden', 'occ_metric.npz'))['names']) == OCC


@pytest.mark.parametrize('name', GROUND)
def test_grounding_spec_equals_the_reference(name):
    c = load_ground(name)
    for s in c['samples']:
        S.check_ground_conditions(s, c['thr'])             # the recorded cases honour the conditions the kernels are held under
    ret = S.ground_eval(c['samples'], c['thr'])
    assert list(ret) == c['keys']
    for key, want in zip(c['keys'], c['vals']):
        assert float(ret[key]).hex() == float(want).hex(), (key, ret[key], want)


@pytest.mark.parametrize('name', OCC)
def test_occupancy_spec_equals_the_reference(name):
    c = load_occ(name)
    ret = S.occ_eval(c['samples'], c['classes'])
    assert list(ret) == c['keys']
    for key, want in zip(c['keys'], c['vals']):
        assert float(ret[key]).hex() == float(want).hex(), (key, ret[key], want)
    assert c['raised'] == (len(ret) == 0)                   # the reference divides by zero exactly where no class is kept


def test_the_grounding_quirks_are_what_their_names_say():
    c = {n: load_ground(n) for n in GROUND}
    thr = [0.25, 0.5]
    assert sorted({S.flag_bits(s[3]) for s in c['generic']['samples']}) == list(range(8)) and len(c['generic']['samples']) == 12
    idx, top, hit, iou = S.sample_outputs(c['slot10_hit']['samples'][0], thr)
    assert idx[9] == 0 and top[9] > 0.5 and (top[:9] == 0).all() and hit == 3
    s = c['rank11_miss']['samples'][0]
    idx, top, hit, iou = S.sample_outputs(s, thr)
    assert 0 not in idx.tolist() and hit == 0 and S.topk(s[1], 11)[10] == 0
    idx, top, hit, iou = S.sample_outputs(c['few_queries']['samples'][0], thr)
    assert idx.tolist() == [0, 2, 1] + [-1] * 7 and np.isneginf(top[3:]).all() and hit == 3
    idx, top, hit, iou = S.sample_outputs(c['no_gt']['samples'][0], thr)
    assert iou.shape == (10, 0) and np.isneginf(top).all() and hit == 0
    idx, top, hit, iou = S.sample_outputs(c['three_gt_last']['samples'][0], thr)
    assert iou.shape == (10, 3) and (iou[:, :2] == 0).all() and iou[0, 2] > 0.5 and hit == 3
    idx, top, hit, iou = S.sample_outputs(c['mid_iou']['samples'][0], thr)
    assert 0.25 < top[0] < 0.5 and hit == 1
    e = dict(zip(c['empty_category']['keys'], c['empty_category']['vals']))
    assert e['View-Dep@0.25'] == 0.0 and e['Multi@0.5'] == 0.0
    one = dict(zip(c['single_sample']['keys'], c['single_sample']['vals']))
    assert one['Overall@0.25'] == 1 / (1e-14 + 1.0) and one['Overall@0.25'] < 1.0 and list(one) == [t + '@0.25' for t in S.TYPES]


def test_the_occupancy_quirks_are_what_their_names_say():
    c = {n: load_occ(n) for n in OCC}
    assert all(s[0].shape == (8, 8, 4) for n in OCC for s in c[n]['samples']) and len(c['generic']['classes']) == 5
    lst = c['duplicates']['samples'][0][1]
    vox = [tuple(r[:3]) for r in lst.tolist()]
    dup = [v for v in set(vox) if vox.count(v) > 1]
    assert len(dup) == 20 and all(len({r[3] for r in lst.tolist() if tuple(r[:3]) == v}) == 2 for v in dup)
    gt = S.occ_dense_gt((8, 8, 4), lst, None)
    assert all(gt[v] == [r[3] for r in lst.tolist() if tuple(r[:3]) == v][-1] for v in dup)               # the last one wins
    assert c['no_mask']['samples'][0][2] is None
    assert not c['all_hidden']['samples'][0][2].any() and c['all_hidden']['keys'] == [] and c['all_hidden']['raised']
    assert S.occ_sample_counts(c['all_hidden']['samples'][0], 6).sum() == 0
    k = S.occ_sample_counts(c['gt_only_pred_only']['samples'][0], 6)
    assert k[1].tolist() == [0, 2, 0] and k[2].tolist() == [0, 0, 2] and k[3].tolist() == [2, 3, 3] and k[4:].sum() == 0
    assert c['gt_only_pred_only']['keys'] == ['empty', 'floor', 'wall', 'chair']                          # table and lamp: dropped
    p, lst, m = c['pred_label_ge_C']['samples'][0]
    assert (p == 9).any() and (p == 255).any() and (lst[:, 3] == 7).any()
    k = S.occ_sample_counts((p, lst, m), 6)
    gt = S.occ_dense_gt(p.shape, lst, m)
    vis = gt != 255
    assert k[0, 2] == ((p != 0) & vis).sum() > k[1:, 2].sum() and k[0, 1] == ((gt != 0) & vis).sum() > k[1:, 1].sum()


def test_denominator_equals_the_sequential_sum_for_every_n_up_to_100000():
    """1e-14 + 1.0 + 1.0 + ... as the reference forms it; n + 1e-14 in one step is NOT the same number everywhere"""
    acc = np.add.accumulate(np.concatenate([[1e-14], np.ones(100000)]))
    d = 1e-14
    differs = 0
    for n in range(100001):
        assert acc[n] == d, n
        differs += (n + 1e-14) != d
        d += 1.0
    for n in (0, 1, 2, 3, 7, 1000, 4095, 4096, 99999, 100000):
        assert S.denominator(n) == acc[n]
    assert S.denominator(0) == 1e-14 and S.denominator(1) == 1e-14 + 1.0
    print(f'n + 1e-14 differs from the sequential sum for {differs} of 100001 values of n')


def test_conditions_reject_an_iou_on_the_threshold_and_a_tie_at_the_cut():
    s = load_ground('mid_iou')['samples'][0]
    iou = S.sample_ious(s)[1]
    S.check_ground_conditions(s, [0.25, 0.5], iou)
    with pytest.raises(AssertionError):
        S.check_ground_conditions(s, [float(iou[0, 0]) + 5e-6], iou)
    tied = (s[0], np.array([0.9] * 11, np.float32), s[2], s[3])
    with pytest.raises(AssertionError):
        S.check_ground_conditions(tied, [0.25], iou)
    S.check_ground_conditions(tied, [0.25], iou, tie_ok=True)
