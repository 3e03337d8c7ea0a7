"""The detection metric on the device (embodiedscan_amd/eval, es_det_best_gt / es_det_mark / es_det_ap of csrc/ground.hip) held to
tests/det_metric_spec.py, which tests/test_det_metric_spec.py ties to the reference's own indoor_eval.

Every body is a function of `dev`; tests/test_emu_det_metric.py runs the same bodies on the CPU emulator.  Shape grid -- the smallest
that can still go wrong: P in {0, 1, 63, 64, 65, 257} (one lane per prediction, 64-lane workgroups), (scene, class) groups of 0 / 1 /
17 ground-truth boxes, C = 1 and C = 284 with most classes empty, 1 / 2 / 3 thresholds, a class segment of exactly one scan chunk
(256 ranks) and of one more, one box pointed at by more than 64 predictions spread over several waves, every prediction without a
group, a class without ground truth.

Input conditions, asserted for every prediction (det_metric_spec.check_conditions): scores distinct within a class, |iou_max - t| >=
1e-5 at every threshold, best and second-best IoU >= 1e-5 apart -- ten times the 1e-6 to which tests/test_gpu_grounding.py holds the
IoU kernel against the oracle.  Under them gt_best, the rank order, the TP flags and tp_total must be exact, iou_max within 1e-6, and
AP within ONE f32 ulp: both sides are f64 sums of at most npos non-negative terms (relative error <= npos * 2^-53, far below half an
f32 ulp), so only the final rounding can differ."""
import os

import numpy as np
import pytest
import torch

import det_metric_spec as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------------ cases
def make_scene(rng, groups, n_pred, stray=(), crowd=None):
    """groups: [(class, number of boxes)]: the boxes of a group sit on a line 3 m apart (no two overlap), the scene's ground truth
    is the groups' boxes in a shuffled order.  n_pred predictions are jittered copies of random boxes carrying their class (IoU
    between 0.1 and 0.9 with that box, next to none with any other); `stray`: classes of extra predictions whose class has no box in the scene;
    crowd = (k, n): n of the predictions copy box k."""
    gb, gl = [], []
    for gi, (c, n) in enumerate(groups):
        for k in range(n):
            gb.append(np.concatenate([[3.0 * k, 4.0 * gi, 0.0], rng.uniform(0.6, 1.4, 3), rng.uniform(-3.1, 3.1, 3)]))
            gl.append(c)
    perm = rng.permutation(len(gl))
    gb, gl = np.array(gb, np.float32).reshape(-1, 9)[perm], np.array(gl, np.int64)[perm]
    src = rng.integers(0, max(len(gl), 1), n_pred) if len(gl) else np.zeros(0, np.int64)
    if crowd is not None:
        src[rng.permutation(n_pred)[:crowd[1]]] = crowd[0]
    pb = gb[src].copy() if len(gl) else np.zeros((0, 9), np.float32)
    pb[:, :3] += rng.uniform(-0.3, 0.3, (len(pb), 3)).astype(np.float32)
    pb[:, 3:6] *= rng.uniform(0.6, 1.5, (len(pb), 3)).astype(np.float32)
    pb[:, 6:] += rng.uniform(-0.3, 0.3, (len(pb), 3)).astype(np.float32)
    pl = gl[src] if len(gl) else np.zeros(0, np.int64)
    if len(stray):
        sb = np.concatenate([rng.uniform(-2, 2, (len(stray), 3)), rng.uniform(0.5, 1, (len(stray), 3)), rng.uniform(-1, 1, (len(stray), 3))], 1)
        pb, pl = np.concatenate([pb, sb.astype(np.float32)]), np.concatenate([pl, np.asarray(stray, np.int64)])
        mix = rng.permutation(len(pl))
        pb, pl = pb[mix], pl[mix]
    return [pb, None, pl, gb, gl]


def with_scores(rng, scenes):
    """distinct scores over the whole case (a permutation of a grid), so every class's are distinct"""
    n = sum(len(s[2]) for s in scenes)
    vals = (rng.permutation(n).astype(np.float32) + 1) / np.float32(n + 1)
    o = 0
    for s in scenes:
        s[1] = vals[o:o + len(s[2])]
        o += len(s[2])
    return [tuple(s) for s in scenes]


def grid_cases():
    """-> [(name, scenes, C, thresholds)]"""
    out = []
    rng = np.random.default_rng(7)
    out.append(('P=0 with ground truth', with_scores(rng, [make_scene(rng, [(0, 1), (2, 2)], 0)]), 3, [0.25, 0.5]))
    out.append(('nothing at all', with_scores(rng, [make_scene(rng, [], 0)]), 2, [0.25]))
    out.append(('P=1 C=1 T=1', with_scores(rng, [make_scene(rng, [(0, 1)], 1)]), 1, [0.25]))
    for n in (63, 64, 65):
        out.append((f'P={n}', with_scores(rng, [make_scene(rng, [(0, 3), (1, 1), (3, 17)], n - 2, stray=[2, 4])]), 5, [0.25, 0.5]))
    # 257 predictions over 3 scenes and 284 classes (most empty), groups of 1 and 17, strays of a class with ground truth elsewhere
    # (11), of a class without any (200: npos = 0) and three thresholds
    out.append(('P=257 C=284 T=3', with_scores(rng, [make_scene(rng, [(11, 1), (40, 17), (283, 2)], 100, stray=[200, 5]),
                                                     make_scene(rng, [(40, 2), (0, 1)], 90, stray=[11, 200, 283]),
                                                     make_scene(rng, [(5, 17)], 60, stray=[11, 11])]), 284, [0.25, 0.4, 0.5]))
    # one class: a segment of exactly one scan chunk and of one more; box 3 is copied by 100 predictions at random ranks (4 waves)
    for n in (256, 257):
        out.append((f'one class, {n} ranks', with_scores(rng, [make_scene(rng, [(0, 5)], n, crowd=(3, 100))]), 1, [0.25, 0.5]))
    out.append(('every prediction without a group', with_scores(rng, [make_scene(rng, [(0, 2)], 0, stray=[1] * 70), make_scene(rng, [(1, 1)], 0, stray=[0] * 5)]), 2, [0.25, 0.5]))
    return out


_SPEC = {}


def spec_of(name, scenes, C, thr):
    """the specification's outputs, computed once per case and shared (never modified)"""
    if name not in _SPEC:
        iou_max, gt_best, second = S.best_gt(scenes)
        ev = S.evaluate(scenes, C, thr, best=(iou_max, gt_best))
        S.check_conditions(scenes, thr, ev, second)
        _SPEC[name] = ev
    return _SPEC[name]


def annos(scenes):
    t = lambda a, dt=None: torch.from_numpy(np.asarray(a, dt))
    gt = [dict(gt_bboxes_3d=t(s[3]), gt_labels_3d=t(s[4])) for s in scenes]
    dt = [dict(bboxes_3d=t(s[0]), scores_3d=t(s[1], np.float32), labels_3d=t(s[2])) for s in scenes]
    return gt, dt


def run_device(scenes, C, thr, dev, names=None, split=None):
    """the product's whole pipeline -> (result dict, split results, outputs as numpy)"""
    from embodiedscan_amd.eval.indoor_eval import indoor_eval_full
    gt, dt = annos(scenes)
    ret, splits, _, out = indoor_eval_full(gt, dt, thr, names or [f'c{k}' for k in range(C)], split, device=dev)
    return ret, splits, {k: v.cpu().numpy() for k, v in out.items()}


def check_dict(ret, want):
    """keys and their order equal; recalls exact; per-class APs within one f32 ulp; mAR to f64 rounding of a mean of exact
    terms; mAP: every term is within one ulp (<= 2^-23) and either side's f32 pairwise mean adds at most ceil(log2 n) + 1
    roundings of 2^-24"""
    assert list(ret) == list(want)
    n_kept = sum('_rec_' in k for k in want)                 # (>= the number of kept classes: T times it)
    tol_map = 2.0 ** -23 + 2 * (int(np.ceil(np.log2(max(n_kept, 2)))) + 1) * 2.0 ** -24
    for k in want:
        if '_rec_' in k:
            assert ret[k] == want[k], (k, ret[k], want[k])
        elif k.startswith('mAR'):
            assert abs(ret[k] - want[k]) <= 1e-15 or (np.isnan(ret[k]) and np.isnan(want[k])), (k, ret[k], want[k])
        elif k.startswith('mAP'):
            assert abs(ret[k] - want[k]) <= tol_map or (np.isnan(ret[k]) and np.isnan(want[k])), (k, ret[k], want[k])
        else:
            assert abs(ret[k] - want[k]) <= S.ulp32(want[k]), (k, ret[k], want[k])


# ------------------------------------------------------------------------------------------------------------------ bodies
def body_grid(dev, pick=None):
    for name, scenes, C, thr in grid_cases():
        if pick is not None and not pick(name):
            continue
        ev = spec_of(name, scenes, C, thr)
        ret, _, got = run_device(scenes, C, thr, dev)
        S.check_outputs(ev, got, name)
        names = [f'c{k}' for k in range(C)]
        want = S.result_dict(scenes, C, thr, names, ev)
        check_dict(ret, want)
        fin = np.isfinite(ev['iou_max'])
        print(f"{name}: P {len(fin)} with a group {int(fin.sum())} TPs {ev['tp_total'].sum(1).tolist()} "
              f"max |d iou| {np.abs(got['iou_max'][fin] - ev['iou_max'][fin]).max() if fin.any() else 0:.2e}")


def body_golden(dev):
    """the product against the reference's recorded dicts: the quirk cases (thin clamp, identical boxes, ...) and classes_split"""
    from test_det_metric_spec import NAMES, load_case
    for name in NAMES:
        c = load_case(name)
        C = len(c['classes'])
        ret, splits, got = run_device(c['scenes'], C, c['thr'], dev, c['classes'], c['split'])
        check_dict(ret, dict(zip(c['keys'], c['vals'].tolist())))
        iou_max, gt_best, _ = S.best_gt(c['scenes'])
        S.check_outputs(S.evaluate(c['scenes'], C, c['thr'], best=(iou_max, gt_best)), got, name)
        if c['split'] is not None:
            assert list(splits) == [str(h[0]).replace('_classes', '') for h in c['split_tables'][0::2]]
            for head, row in zip(c['split_tables'][0::2], c['split_tables'][1::2]):
                res = splits[str(head[0]).replace('_classes', '')]
                assert [f'{res[str(h)]:.4f}' for h in head[1:]] == [str(v) for v in row[1:]]
        else:
            assert splits == {}


def body_refusals(dev):
    """a refusal is a negative status and touches no output"""
    from embodiedscan_amd import hip
    P = hip.P
    st = hip.stream()
    tp = torch.full((9 * 4,), 7, dtype=torch.uint8, device=dev)
    z = torch.zeros(8, dtype=torch.int32, device=dev)
    f = torch.zeros(8, dtype=torch.float32, device=dev)
    ap = torch.full((9 * 2,), -3.0, dtype=torch.float32, device=dev)
    tot = torch.full((9 * 2,), -3, dtype=torch.int32, device=dev)
    for T in (0, 9):
        assert hip.raw('es_det_mark')(P(f), P(z), P(z), 4, hip.farr([0.25] * 9), T, 2, P(z), P(tp), st) == -5
        assert hip.raw('es_det_ap')(P(tp), 4, P(z), P(z), 2, T, P(ap), P(tot), st) == -5
    assert hip.raw('es_det_best_gt')(P(f), -1, P(z), P(f), P(z), 0, P(f), P(z), st) == -5
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert (tp == 7).all() and (ap == -3).all() and (tot == -3).all()


def body_metric_object(dev):
    """IndoorDetMetric through the registry: dict and Det3DDataSample samples, eval_ann_info and the gt_instances_3d fall-back,
    box objects and plain tensors, two process() calls, the prefix, `size`, batchwise_anns, and the results cleared"""
    from embodiedscan_amd.registry import METRICS
    from embodiedscan_amd.structures import Det3DDataSample, EulerDepthInstance3DBoxes, InstanceData
    name, scenes, C, thr = grid_cases()[3]
    scenes = [scenes[0], grid_cases()[2][1][0]]
    names = [f'c{k}' for k in range(C)]
    m = METRICS.build(dict(type='IndoorDetMetric', iou_thr=thr, prefix='val', device=dev))
    m.dataset_meta = dict(classes=names, box_type_3d='Euler-Depth')
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dev)
    s0, s1 = scenes
    sample0 = dict(pred_instances_3d=dict(bboxes_3d=EulerDepthInstance3DBoxes(t(s0[0])), scores_3d=t(s0[1]), labels_3d=t(s0[2])),
                   eval_ann_info=dict(gt_bboxes_3d=EulerDepthInstance3DBoxes(torch.from_numpy(s0[3])), gt_labels_3d=s0[4]))
    sample1 = Det3DDataSample(gt_instances_3d=InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(t(s1[3])), labels_3d=t(s1[4])))
    sample1.pred_instances_3d = InstanceData(bboxes_3d=t(s1[0]), scores_3d=t(s1[1]), labels_3d=t(s1[2]))
    m.process({}, [sample0])
    m.process({}, [sample1, sample0])                      # the third is the padding a loader adds: `size` cuts it
    ret = m.evaluate(2)
    assert m.results == []
    want = S.result_dict(scenes, C, thr, names)
    check_dict({k[len('val/'):]: v for k, v in ret.items() if k.startswith('val/')}, want)
    assert len(ret) == len(want)
    m2 = METRICS.build(dict(type='IndoorDetMetric', batchwise_anns=True, device=dev))
    assert m2.iou_thr == [0.25, 0.5] and m2.batchwise_anns
    m2.dataset_meta = dict(classes=names)
    m2.process({}, [sample0, sample1])
    check_dict(m2.evaluate(1), want)                   # batchwise_anns: everything processed is kept


def test_grid_against_the_specification(dev):
    body_grid(dev)


def test_reference_cases_and_class_splits(dev):
    body_golden(dev)


def test_refusals_leave_the_outputs_untouched(dev):
    body_refusals(dev)


def test_metric_object_through_the_registry(dev):
    body_metric_object(dev)


def test_two_runs_are_bit_identical(dev):
    name, scenes, C, thr = grid_cases()[6]
    a, b = run_device(scenes, C, thr, dev), run_device(scenes, C, thr, dev)
    assert a[0] == b[0] or all((a[0][k] == b[0][k]) or (np.isnan(a[0][k]) and np.isnan(b[0][k])) for k in a[0])
    for k in a[2]:
        assert a[2][k].tobytes() == b[2][k].tobytes(), k


def test_predict_process_evaluate_end_to_end(dev):
    """mv-3ddet detector on two synthetic scans (as tests/test_gpu_predict.py builds it): predict -> IndoorDetMetric.process ->
    evaluate, against the spec on CPU copies of the same predictions.  A random detector does not honour the margin conditions, so
    nothing is perturbed: the spec is evaluated with the device's iou_max / gt_best, and the IoU is held separately to 1e-6 of the
    oracle's (and gt_best to a box within 1e-6 of the best)."""
    from embodiedscan_amd import pipeline
    from embodiedscan_amd.config import build_detector
    from embodiedscan_amd.eval.indoor_eval import indoor_eval_full
    from embodiedscan_amd.registry import METRICS
    from embodiedscan_amd.synth import make_scan
    det = build_detector(os.path.join(ROOT, 'configs/mv_3ddet.py'), device=dev, seed=0).to(dev)
    det.bbox_head.test_cfg = dict(nms_pre=300, iou_thr=0.5, score_thr=0.09)
    scans = [make_scan(s, n_views=3, height=120, width=160, img_size=(128, 128), n_points=8000, n_boxes=5) for s in (31, 32)]
    batch = pipeline.make_batch([pipeline.upload_scan(s, dev) for s in scans])
    data = det.data_preprocessor(batch, False)
    out = det.forward(data['inputs'], data['data_samples'], mode='predict')
    C = det.bbox_head.num_classes
    names = [f'c{k}' for k in range(C)]
    preds = [o.pred_instances_3d for o in out]
    # half of every scan's boxes take the label its predictions favour, so that some (scene, class) groups are populated
    samples = []
    for o, sc in zip(out, scans):
        lab = sc['gt_labels'].copy()
        top = torch.bincount(o.pred_instances_3d.labels_3d, minlength=C).argmax().item()
        lab[::2] = top
        samples.append(dict(pred_instances_3d=o.pred_instances_3d, eval_ann_info=dict(gt_bboxes_3d=sc['gt_boxes'], gt_labels_3d=lab)))
    metric = METRICS.build(dict(type='IndoorDetMetric', batchwise_anns=True))
    metric.dataset_meta = dict(classes=names)
    metric.process({}, samples)
    kept = list(metric.results)
    ret = metric.evaluate(len(samples))
    scenes = [(p.bboxes_3d.tensor.cpu().numpy(), p.scores_3d.cpu().numpy(), p.labels_3d.cpu().numpy(), s['eval_ann_info']['gt_bboxes_3d'],
               s['eval_ann_info']['gt_labels_3d']) for p, s in zip(preds, samples)]
    n_pred = sum(len(s[2]) for s in scenes)
    assert n_pred > 20
    gt, dt = annos(scenes)
    _, _, _, dev_out = indoor_eval_full(gt, dt, [0.25, 0.5], names, device=dev)
    got = {k: v.cpu().numpy() for k, v in dev_out.items()}
    # the IoU on its own: 1e-6 against the oracle, and the chosen box within 1e-6 of the best one
    o = 0
    g0 = 0
    n_grouped = 0
    for sc in scenes:
        for i, (rows, v) in enumerate(S.iou_rows(sc)):
            if len(rows) == 0:
                assert np.isneginf(got['iou_max'][o + i]) and got['gt_best'][o + i] == -1
                continue
            n_grouped += 1
            assert abs(float(got['iou_max'][o + i]) - float(v.max())) <= 1e-6
            j = int(got['gt_best'][o + i]) - g0
            assert j in rows.tolist() and float(v.max()) - float(v[rows.tolist().index(j)]) <= 1e-6
        o += len(sc[2])
        g0 += len(sc[4])
    assert n_grouped > 0
    ev = S.evaluate(scenes, C, [0.25, 0.5], best=(got['iou_max'], got['gt_best'].astype(np.int64)))
    # equal scores inside a class would leave the order to the tie rule, which the spec shares (stable): compare as is
    np.testing.assert_array_equal(got['order'], ev['order'])
    np.testing.assert_array_equal(got['tp'], ev['tp'])
    np.testing.assert_array_equal(got['tp_total'], ev['tp_total'])
    check_dict(ret, S.result_dict(scenes, C, [0.25, 0.5], names, ev))
    print(f'end to end: {n_pred} predictions, {n_grouped} with a group, mAP_0.25 {ret["mAP_0.25"]:.4f}')
    assert len(kept) == 2
