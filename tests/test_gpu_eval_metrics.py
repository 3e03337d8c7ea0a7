"""The grounding and the occupancy metric on the device (embodiedscan_amd/eval: es_ground_hits / es_ground_tally of csrc/ground.hip,
es_occ_confusion of csrc/occ.hip, with es_topk_sorted and es_occ_targets) held to tests/eval_metric_spec.py, which
tests/test_eval_metric_spec.py ties to the reference's own GroundingMetric and OccupancyMetric.

Every body is a function of `dev`; tests/test_emu_eval_metrics.py runs the same bodies on the CPU emulator.  Shape grid -- the
smallest that can still go wrong.  Hits: Q in {0, 1, 9, 10, 11, 65, 256} (fewer than, exactly and more than the ten slots), G in {0, 1,
3}, S in {1, 6, 7, 64, 65} (one lane per (sample, slot), 64-lane workgroups: with ten slots a sample straddles a workgroup from S = 7
on), T in {1, 2, 8}, a sample whose slots are all -1 (Q = 0).  Tally: N in {0, 1, 255, 256, 257, 1000} (256-lane workgroups), T in
{1, 8}.  Confusion: 1, 255, 256, 257 voxels, the real 40 x 40 x 16 volume once, 40 000 voxels (more than the 128 x 256 lanes of the
largest grid, so the stride loop wraps), C in {1, 2, 81, 256}, label 255 under C = 256, an empty list, every voxel ignored.

Input conditions, asserted for every generated sample and never used to skip one (eval_metric_spec.check_ground_conditions): every
IoU entering rule 3 is >= 1e-5 away from every threshold -- ten times the 1e-6 to which tests/test_gpu_grounding.py holds the IoU
kernel against the oracle -- and the 10th and 11th target scores differ (except in the tie-rule test).  Under them the top-k indices,
the hit bits, the tally counts, the confusion counts and the final dicts must be EXACT (the host arithmetic is the spec's on equal
integers); iou_top within 1e-6."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import eval_metric_spec as S

pytestmark = pytest.mark.gpu
THR8 = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------------ cases
def make_sample(rng, Q, G, flags=0):
    """G ground-truth boxes on a line 3 m apart (no two overlap); Q predictions: jittered copies of random ones (IoU between 0 and
    0.9 with their source, none with any other), random boxes when G = 0; target scores: a permutation of a grid (distinct);
    scores_3d (for format_only): another one"""
    gt = np.concatenate([np.stack([3.0 * np.arange(G), np.zeros(G), np.zeros(G)], 1), rng.uniform(0.6, 1.4, (G, 3)),
                         rng.uniform(-3.1, 3.1, (G, 3))], 1).astype(np.float32).reshape(-1, 9)
    if G:
        boxes = gt[rng.integers(0, G, Q)].copy()
    else:
        boxes = np.concatenate([rng.uniform(-2, 2, (Q, 3)), rng.uniform(0.5, 1, (Q, 3)), rng.uniform(-1, 1, (Q, 3))], 1).astype(np.float32)
    boxes = boxes.reshape(-1, 9)
    boxes[:, :3] += rng.uniform(-0.5, 0.5, (Q, 3)).astype(np.float32)
    boxes[:, 3:6] *= rng.uniform(0.6, 1.5, (Q, 3)).astype(np.float32)
    boxes[:, 6:] += rng.uniform(-0.3, 0.3, (Q, 3)).astype(np.float32)
    grid = lambda: (rng.permutation(Q).astype(np.float32) + 1) / np.float32(Q + 1)
    return (boxes, grid(), gt, (bool(flags & 1), bool(flags & 2), bool(flags & 4)), grid())


def grid_cases():
    """-> [(name, samples, thresholds)]"""
    rng = np.random.default_rng(11)
    cyc = lambda vals, n: [vals[i % len(vals)] for i in range(n)]
    mk = lambda qs, gs: [make_sample(rng, q, g, i % 8) for i, (q, g) in enumerate(zip(qs, gs))]
    out = [('S=1 Q=1 G=1 T=1', mk([1], [1]), [0.25]),
           ('S=1 Q=0 (every slot -1)', mk([0], [3]), [0.25, 0.5]),
           ('S=6', mk([0, 1, 9, 10, 11, 65], [1, 0, 3, 1, 3, 1]), [0.25, 0.5]),
           ('S=7', mk([256, 10, 11, 9, 65, 1, 0], [3, 1, 0, 1, 3, 1, 0]), [0.25, 0.5]),
           ('S=64 T=8', mk(cyc([12, 9, 10, 11], 64), cyc([1, 3, 0], 64)), THR8),
           ('S=65', mk(cyc([11, 10, 65, 9, 1], 65), cyc([3, 1, 0, 1], 65)), [0.25, 0.5])]
    return out


_SPEC = {}


def spec_of(name, samples, thr):
    """the specification's outputs, computed once per case and shared (never modified); the input conditions asserted per sample"""
    if name not in _SPEC:
        idx, top, hit = [], [], []
        for s in samples:
            i, t, h, iou = S.sample_outputs(s, thr)
            S.check_ground_conditions(s, thr, iou)
            idx.append(i), top.append(t), hit.append(h)
        _SPEC[name] = dict(idx=np.stack(idx), iou_top=np.stack(top), hit=np.array(hit, np.int32))
    return _SPEC[name]


def run_hits(samples, thr, dev):
    from embodiedscan_amd.eval.grounding_metric import ground_hits
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = ground_hits([t(s[0]) for s in samples], [t(s[1]) for s in samples], [t(s[2]) for s in samples], thr,
                      [S.flag_bits(s[3]) for s in samples], device=dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def as_data_samples(samples, dev, boxes_as_objects=True):
    """what a grounder's predict() hands to the metric: dicts with pred_instances_3d and eval_ann_info"""
    from embodiedscan_amd.structures import EulerDepthInstance3DBoxes
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    wrap = EulerDepthInstance3DBoxes if boxes_as_objects else (lambda x: x)
    out = []
    for s in samples:
        pred = dict(bboxes_3d=wrap(t(s[0])), target_scores_3d=t(s[1]), scores_3d=t(s[4] if len(s) > 4 else s[1]))
        ann = dict(gt_bboxes_3d=wrap(torch.from_numpy(np.ascontiguousarray(s[2]))), is_view_dep=s[3][0], is_hard=s[3][1], is_unique=s[3][2])
        out.append(dict(pred_instances_3d=pred, eval_ann_info=ann))
    return out


def occ_volume(rng, shape, C, n_list, mask_share=0.8, dup=0):
    """-> (pred (X,Y,Z) int64, gt list (M,4) int64, mask or None): labels 1 .. C-1 (and a few >= C), the prediction agrees with the
    ground truth on most voxels"""
    X, Y, Z = shape
    n = X * Y * Z
    flat = rng.permutation(n)[:n_list]
    if dup:
        flat = np.concatenate([flat, flat[:dup]])
    lab = rng.integers(1, max(C, 2) + 2, len(flat))
    lst = np.stack([flat // (Y * Z), (flat // Z) % Y, flat % Z, lab], 1).astype(np.int64)
    pred = S.occ_dense_gt(shape, lst, None)
    noise = rng.random(shape) < 0.3
    pred[noise] = rng.integers(0, max(C, 2) + 2, int(noise.sum()))
    mask = None if mask_share is None else rng.random(shape) < mask_share
    return pred, lst, mask


# ------------------------------------------------------------------------------------------------------------------ bodies
def body_hits_grid(dev, pick=None):
    for name, samples, thr in grid_cases():
        if pick is not None and not pick(name):
            continue
        want = spec_of(name, samples, thr)
        got = run_hits(samples, thr, dev)
        S.check_ground_outputs(want, got, name)
        np.testing.assert_array_equal(got['flags'], [S.flag_bits(s[3]) for s in samples])
        fin = np.isfinite(want['iou_top'])
        print(f"{name}: slots {fin.size} with an IoU {int(fin.sum())} hits {[int((want['hit'] >> t & 1).sum()) for t in range(len(thr))]} "
              f"max |d iou| {np.abs(got['iou_top'][fin] - want['iou_top'][fin]).max() if fin.any() else 0:.2e}")
    if pick is None:
        assert (spec_of(*grid_cases()[1])['idx'] == -1).all()                 # the case with every slot empty is one


def body_tally(dev):
    from embodiedscan_amd.eval.grounding_metric import ground_tally
    rng = np.random.default_rng(5)
    for N in (0, 1, 255, 256, 257, 1000):
        for T in (1, 8):
            hit = rng.integers(0, 1 << T, N).astype(np.int32)
            flags = rng.integers(0, 8, N).astype(np.uint8)
            got = ground_tally(torch.from_numpy(hit).to(dev), torch.from_numpy(flags).to(dev), T).cpu().numpy()
            S.check_counts(got, S.tally(hit, flags, T), f'tally N={N} T={T}')
            assert (got[:, 6, 1] == N).all()


def raw_confusion(pred, gt, C, dev):
    from embodiedscan_amd import hip
    p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    out = torch.full((max(C, 1), 3), -7, dtype=torch.int32, device=dev)
    rc = hip.raw('es_occ_confusion')(hip.P(p), hip.P(g), len(pred), C, hip.P(out), hip.stream())
    return rc, out.cpu().numpy()


def body_confusion(dev):
    rng = np.random.default_rng(9)
    sizes = [(n, C) for n in (1, 255, 256, 257) for C in (1, 2, 81, 256)] + [(40 * 40 * 16, 81), (40000, 256), (40000, 2)]
    for n, C in sizes:
        gt = rng.integers(0, C + 2, n).astype(np.int32)
        gt[rng.random(n) < 0.2] = 255
        pred = np.where(rng.random(n) < 0.6, gt, rng.integers(0, C + 2, n)).astype(np.int64)
        pred[rng.random(n) < 0.05] = 255                                      # a predicted 255 is a label like any other
        rc, got = raw_confusion(pred, gt, C, dev)
        assert rc == 0
        S.check_counts(got, S.occ_confusion(pred, gt, C), f'confusion n={n} C={C}')
    # label 255 under C = 256: an ignored voxel counts nowhere, a predicted 255 on a visible voxel counts in row 255
    gt = np.array([255, 255, 3, 0, 255], np.int32)
    pred = np.array([255, 3, 255, 255, 0], np.int64)
    rc, got = raw_confusion(pred, gt, 256, dev)
    assert rc == 0 and got[255].tolist() == [0, 0, 2] and got[0].tolist() == [1, 1, 2] and got[3].tolist() == [0, 1, 0] and got.sum() == 7
    S.check_counts(got, S.occ_confusion(pred, gt, 256), 'label 255, C = 256')
    # refusals: nothing written
    assert raw_confusion(pred[:4], gt[:4], 257, dev)[0] == -4 and (raw_confusion(pred[:4], gt[:4], 257, dev)[1] == -7).all()
    assert raw_confusion(pred[:4], gt[:4], 0, dev)[0] == -4 and (raw_confusion(pred[:4], gt[:4], 0, dev)[1] == -7).all()
    from embodiedscan_amd import hip
    out = torch.full((3, 3), -7, dtype=torch.int32, device=dev)
    assert hip.raw('es_occ_confusion')(0, 0, -1, 3, hip.P(out), hip.stream()) == -5 and (out == -7).all()


def body_occ_samples(dev):
    """lists -> dense ground truth -> counts through the product's occ_confusion: duplicates, no mask, M = 0, everything ignored,
    an odd volume"""
    from embodiedscan_amd.eval.occupancy_metric import occ_confusion
    rng = np.random.default_rng(13)
    cases = [occ_volume(rng, (5, 3, 7), 6, 40, dup=10), occ_volume(rng, (8, 8, 4), 6, 90, mask_share=None),
             occ_volume(rng, (8, 8, 4), 81, 0), occ_volume(rng, (40, 40, 16), 81, 3000, dup=50)]
    p, lst, _ = occ_volume(rng, (8, 8, 4), 6, 90)
    cases.append((p, lst, np.zeros((8, 8, 4), bool)))
    for k, (pred, lst, mask) in enumerate(cases):
        C = 81 if k in (2, 3) else 6
        got = occ_confusion(torch.from_numpy(pred).to(dev), torch.from_numpy(lst), None if mask is None else torch.from_numpy(mask), C, dev)
        want = S.occ_sample_counts((pred, lst, mask), C)
        S.check_counts(got.cpu().numpy().reshape(C, 3), want, f'occupancy sample {k}')
    assert S.occ_sample_counts(cases[2], 81)[:, 1].sum() == 0 and S.occ_sample_counts(cases[4], 6).sum() == 0


def body_ground_refusals(dev):
    """a refusal is -5 and touches no output"""
    from embodiedscan_amd import hip
    P, st = hip.P, hip.stream()
    hit = torch.full((4,), 7, dtype=torch.int32, device=dev)
    top = torch.full((40,), -3.0, dtype=torch.float32, device=dev)
    cnt = torch.full((8 * 7 * 2,), -3, dtype=torch.int32, device=dev)
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    f = torch.zeros(64, dtype=torch.float32, device=dev)
    fl = torch.zeros(8, dtype=torch.uint8, device=dev)
    for T in (0, 9):
        assert hip.raw('es_ground_hits')(P(f), P(z), P(z), 4, 10, P(f), P(z), hip.farr([0.25] * 9), T, P(hit), P(top), st) == -5
        assert hip.raw('es_ground_tally')(P(z), P(fl), 4, T, P(cnt), st) == -5
    assert hip.raw('es_ground_hits')(P(f), P(z), P(z), -1, 10, P(f), P(z), hip.farr([0.25]), 1, P(hit), P(top), st) == -5
    assert hip.raw('es_ground_hits')(P(f), P(z), P(z), 4, -1, P(f), P(z), hip.farr([0.25]), 1, P(hit), P(top), st) == -5
    assert hip.raw('es_ground_tally')(P(z), P(fl), -1, 2, P(cnt), st) == -5
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert (hit == 7).all() and (top == -3).all() and (cnt == -3).all()


def body_tie_rule(dev):
    """the project's tie rule (the reference leaves ties to an unstable argsort): equal scores go to the lower query index, and
    -0.0 ties with +0.0 -- also ACROSS the cut between the 10th and the 11th"""
    rng = np.random.default_rng(3)
    s = make_sample(rng, 14, 1)
    scores = np.array([0.5, 0.0, 0.5, -0.0, 0.7, 0.0, -0.0, 0.5, -1.0, 0.0, -0.0, 0.0, 0.9, -0.0], np.float32)
    tied = (s[0], scores, s[2], s[3])
    want_idx = [12, 4, 0, 2, 7, 1, 3, 5, 6, 9]
    i, top, hit, iou = S.sample_outputs(tied, [0.25, 0.5])
    assert i.tolist() == want_idx
    S.check_ground_conditions(tied, [0.25, 0.5], iou, tie_ok=True)
    got = run_hits([tied], [0.25, 0.5], dev)
    S.check_ground_outputs(dict(idx=i[None], iou_top=top[None], hit=np.array([hit], np.int32)), got, 'ties')


def body_grounding_metric_object(dev):
    """GroundingMetric through the registry: box objects and plain tensors, several process() calls, the prefix, `size` cutting a
    padded tail, the results cleared, an evaluation with nothing processed"""
    from embodiedscan_amd.registry import METRICS
    name, samples, thr = grid_cases()[2]                               # S = 6
    spec_of(name, samples, thr)                                           # (asserts the input conditions)
    m = METRICS.build(dict(type='GroundingMetric', iou_thr=thr, prefix='val', device=dev))
    ds = as_data_samples(samples, dev)
    m.process({}, ds[:2])
    m.process({}, as_data_samples(samples[2:5], dev, boxes_as_objects=False))
    m.process({}, [ds[5], ds[0], ds[1]])                                # the last two are the padding a loader adds: `size` cuts it
    assert len(m.results) == 8 and all(r[0].dtype == torch.int32 and r[0].shape == (1,) and r[1].dtype == torch.uint8 and r[1].shape == (1,)
                                       for r in m.results)
    ret = m.evaluate(6)
    assert m.results == []
    want = S.ground_eval(samples, thr)
    assert all(k.startswith('val/') for k in ret) and len(ret) == len(want)
    S.check_dict({k[len('val/'):]: v for k, v in ret.items()}, want)
    m2 = METRICS.build(dict(type='GroundingMetric', device=dev))
    assert m2.iou_thr == [0.25, 0.5] and not m2.format_only
    S.check_dict(m2.evaluate(0), S.ground_eval([], [0.25, 0.5]))
    m2.process({}, ds)
    S.check_dict(m2.evaluate(3), S.ground_eval(samples[:3], [0.25, 0.5]))


def body_format_only(dev):
    """format_only: the 20 best boxes and scores by scores_3d, written as lists; the JSON round-trips to the spec's"""
    from embodiedscan_amd.registry import METRICS
    rng = np.random.default_rng(17)
    samples = [make_sample(rng, q, 1) for q in (25, 5, 20, 0, 21)]
    with tempfile.TemporaryDirectory() as tmp:
        m = METRICS.build(dict(type='GroundingMetric', format_only=True, result_dir=os.path.join(tmp, 'out'), device=dev))
        m.process({}, as_data_samples(samples[:3], dev))
        m.process({}, as_data_samples(samples[3:], dev))
        assert m.evaluate(5) == {} and m.results == []
        with open(os.path.join(tmp, 'out', 'test_results.json')) as f:
            saved = json.load(f)
    want = S.saved_results(samples)
    assert [len(r['scores_3d']) for r in saved] == [20, 5, 20, 0, 20]
    assert saved == json.loads(json.dumps(want))


def body_occupancy_metric_object(dev):
    """OccupancyMetric through the registry: several process() calls, `size` cutting a padded tail BEFORE the sum, batchwise_anns,
    the prefix, the results cleared, dict and attribute samples, dataset_meta missing"""
    from embodiedscan_amd.registry import METRICS
    from embodiedscan_amd.structures import Det3DDataSample
    rng = np.random.default_rng(23)
    classes = ['a', 'b', 'c', 'd', 'e']
    vols = [occ_volume(rng, (8, 8, 4), 6, 70, dup=5), occ_volume(rng, (8, 8, 4), 6, 50, mask_share=None), occ_volume(rng, (8, 8, 4), 6, 90)]
    t = lambda a: None if a is None else torch.from_numpy(a)

    def sample(v, as_dict=True):
        d = dict(pred_occupancy=t(v[0]).to(dev), gt_occupancy=t(v[1]))
        if v[2] is not None:
            d['gt_occupancy_masks'] = t(v[2])
        if as_dict:
            return d
        ds = Det3DDataSample()
        for k, x in d.items():
            setattr(ds, k, x)
        return ds
    m = METRICS.build(dict(type='OccupancyMetric', prefix='occ', device=dev))
    with pytest.raises(RuntimeError, match='dataset_meta'):
        m.process({}, [sample(vols[0])])
    m.dataset_meta = dict(classes=classes)
    m.process({}, [sample(vols[0])])
    m.process({}, [sample(vols[1], as_dict=False), sample(vols[2]), sample(vols[0])])          # the last is padding: `size` cuts it
    assert len(m.results) == 4 and all(len(r) == 1 and r[0].dtype == torch.int32 and r[0].shape == (1, 18) for r in m.results)
    ret = m.evaluate(3)
    assert m.results == []
    want = S.occ_eval(vols, classes)
    assert all(k.startswith('occ/') for k in ret)
    S.check_dict({k[len('occ/'):]: v for k, v in ret.items()}, want)
    m2 = METRICS.build(dict(type='OccupancyMetric', batchwise_anns=True, device=dev, dataset_meta=dict(classes=classes)))
    m2.process({}, [sample(v) for v in vols] + [sample(vols[0])])
    S.check_dict(m2.evaluate(1), S.occ_eval(vols + [vols[0]], classes))                         # everything processed is kept
    assert m2.evaluate(0) == {}                                                                 # nothing processed: no class kept


def body_golden(dev):
    """the product end to end against the reference's recorded dicts, bit for bit"""
    from embodiedscan_amd.registry import METRICS
    from test_eval_metric_spec import GROUND, OCC, load_ground, load_occ
    for name in GROUND:
        c = load_ground(name)
        m = METRICS.build(dict(type='GroundingMetric', iou_thr=c['thr'], device=dev))
        m.process({}, as_data_samples(c['samples'], dev))
        S.check_dict(m.evaluate(len(c['samples'])), dict(zip(c['keys'], c['vals'].tolist())))
    for name in OCC:
        c = load_occ(name)
        m = METRICS.build(dict(type='OccupancyMetric', device=dev, dataset_meta=dict(classes=c['classes'])))
        batch = []
        for pred, lst, mask in c['samples']:
            d = dict(pred_occupancy=torch.from_numpy(pred).to(dev), gt_occupancy=torch.from_numpy(lst))
            if mask is not None:
                d['gt_occupancy_masks'] = torch.from_numpy(mask)
            batch.append(d)
        m.process({}, batch)
        S.check_dict(m.evaluate(len(batch)), dict(zip(c['keys'], c['vals'].tolist())))


# ------------------------------------------------------------------------------------------------------------------ tests
def test_hits_grid_against_the_specification(dev):
    body_hits_grid(dev)


def test_tally_counts_are_exact(dev):
    body_tally(dev)


def test_confusion_counts_are_exact_and_refusals_write_nothing(dev):
    body_confusion(dev)


def test_occupancy_samples_from_lists_and_masks(dev):
    body_occ_samples(dev)


def test_grounding_refusals_leave_the_outputs_untouched(dev):
    body_ground_refusals(dev)


def test_equal_target_scores_go_to_the_lower_query(dev):
    body_tie_rule(dev)


def test_grounding_metric_through_the_registry(dev):
    body_grounding_metric_object(dev)


def test_format_only_writes_the_top_20(dev):
    body_format_only(dev)


def test_occupancy_metric_through_the_registry(dev):
    body_occupancy_metric_object(dev)


def test_reference_cases_end_to_end(dev):
    body_golden(dev)


def test_two_runs_are_bit_identical(dev):
    name, samples, thr = grid_cases()[5]
    a, b = run_hits(samples, thr, dev), run_hits(samples, thr, dev)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
