"""Specification of the grounding and the occupancy metric (embodiedscan/eval/metrics/grounding_metric.py:70-152,
occupancy_metric.py:42-115) for arbitrary shapes: numpy, f64, plain loops, the IoU from oracle.grounding.  TEST INFRASTRUCTURE -- held
to the reference's own output by tests/golden/ground_metric.npz and tests/golden/occ_metric.npz (tools/make_golden_eval_metrics.py) in
tests/test_eval_metric_spec.py; the kernels and the metric objects are held to it in tests/test_emu_eval_metrics.py and
tests/test_gpu_eval_metrics.py.

Grounding.  A sample is (boxes (Q,9) f32, target_scores (Q) f32, gt_boxes (G,9) f32, (view_dep, hard, unique)).  Rules as numbered
in embodiedscan_amd/eval/grounding_metric.py.  Equal target scores rank by the lower query index -- numpy's STABLE argsort of the
negated scores, for which -0.0 equals +0.0; the reference's unstable argsort agrees wherever the ten highest scores are distinct.

Occupancy.  A sample is (pred (X,Y,Z) int64, gt_list (M,4) int64 {x, y, z, label}, mask (X,Y,Z) bool or None).  Rules as numbered in
embodiedscan_amd/eval/occupancy_metric.py."""
import numpy as np

from oracle import grounding as OG

F32 = np.float32
TYPES = ('Easy', 'Hard', 'View-Dep', 'View-Indep', 'Unique', 'Multi', 'Overall')
TOP_K = 10
SAVE_K = 20
MARGIN = 1e-5


# ------------------------------------------------------------------------------------------------------------------ grounding
def topk(scores, k):
    """rule 1: indices of the k highest scores in descending order (all of them when there are fewer), ties to the lower index"""
    s = np.asarray(scores, F32)
    return np.argsort(-s, kind='stable')[:k]


def sample_ious(sample, k=TOP_K):
    """rules 1, 2 -> (top-k indices, (len(idx), G) f32 IoU matrix)"""
    boxes, tscores, gt = sample[0], sample[1], sample[2]
    idx = topk(tscores, k)
    iou = np.zeros((len(idx), len(gt)), F32)
    for a, q in enumerate(idx):
        for j in range(len(gt)):
            iou[a, j] = F32(OG.box3d_iou(np.asarray(boxes[q], F32), np.asarray(gt[j], F32)))
    return idx, iou


def sample_outputs(sample, thr, k=TOP_K):
    """-> idx (k,) int32 padded with -1, iou_top (k,) f32 (-inf: empty slot or no ground truth), hit: bit t set iff any IoU > thr[t]
    (f32 compare, rule 3), iou: the matrix itself"""
    idx, iou = sample_ious(sample, k)
    pad = np.full(k, -1, np.int32)
    pad[:len(idx)] = idx
    top = np.full(k, -np.inf, F32)
    if iou.shape[1]:
        top[:len(idx)] = iou.max(1)
    hit = 0
    for t, v in enumerate(thr):
        if (iou > F32(v)).any():
            hit |= 1 << t
    return pad, top, hit, iou


def flag_bits(flags):
    """(view_dep, hard, unique) -> bit 0 view-dependent, bit 1 hard, bit 2 unique"""
    vd, hard, uniq = flags
    return (1 if vd else 0) | (2 if hard else 0) | (4 if uniq else 0)


def types_of(bits):
    """rule 4: the four types a sample counts in (indices into TYPES)"""
    return (1 if bits & 2 else 0, 2 if bits & 1 else 3, 4 if bits & 4 else 5, 6)


def tally(hits, flags, T):
    """hits (N) bit masks, flags (N) bit triples -> counts (T,7,2) [found, samples]"""
    counts = np.zeros((T, len(TYPES), 2), np.int64)
    for h, f in zip(hits, flags):
        for ty in types_of(int(f)):
            for t in range(T):
                counts[t, ty, 0] += (int(h) >> t) & 1
                counts[t, ty, 1] += 1
    return counts


def denominator(n):
    """rule 5: the f64 that starts at 1e-14 and has 1.0 added n times, one after the other (np.add.accumulate is sequential)"""
    return float(np.add.accumulate(np.concatenate([[1e-14], np.ones(int(n))]))[-1])


def ground_dict(counts, thr):
    """rules 5, 6: counts (T,7,2) -> the dict ground_eval returns"""
    ret = {}
    for t, v in enumerate(thr):
        for k, name in enumerate(TYPES):
            ret[name + '@' + str(v)] = int(counts[t, k, 0]) / max(denominator(counts[t, k, 1]), 1)
    return ret


def ground_eval(samples, thr):
    hits = [sample_outputs(s, thr)[2] for s in samples]
    return ground_dict(tally(hits, [flag_bits(s[3]) for s in samples], len(thr)), thr)


def saved_results(samples):
    """rule 7: per sample the SAVE_K boxes and scores of highest `scores_3d` (a sample's fifth entry), as lists"""
    out = []
    for s in samples:
        idx = topk(s[4], SAVE_K)
        out.append(dict(bboxes_3d=np.asarray(s[0], F32)[idx].tolist(), scores_3d=np.asarray(s[4], F32)[idx].tolist()))
    return out


def check_ground_conditions(sample, thr, iou=None, tie_ok=False):
    """the input conditions under which hit bits and top-k indices must be exact, asserted for EVERY sample: every IoU entering rule 3
    at least 1e-5 away from every threshold; the 10th and 11th target scores differ (unless the test is about the tie rule)"""
    if iou is None:
        iou = sample_ious(sample)[1]
    for v in np.asarray(iou, np.float64).reshape(-1):
        for t in thr:
            assert abs(v - float(F32(t))) >= MARGIN, (v, t)
    s = np.sort(np.asarray(sample[1], F32))[::-1]
    if not tie_ok and len(s) > TOP_K:
        assert s[TOP_K - 1] != s[TOP_K], 'the 10th and 11th target scores are equal'


def check_ground_outputs(want, got, what=''):
    """want / got: dicts idx (S,K), iou_top (S,K), hit (S).  Indices and hit bits exact, iou_top within 1e-6 (-inf pattern exact)."""
    np.testing.assert_array_equal(got['idx'], want['idx'], err_msg=f'{what}: top-k indices')
    np.testing.assert_array_equal(got['hit'], want['hit'], err_msg=f'{what}: hit bits')
    fin = np.isfinite(want['iou_top'])
    np.testing.assert_array_equal(np.isfinite(got['iou_top']), fin, err_msg=f'{what}: iou_top -inf pattern')
    np.testing.assert_array_equal(got['iou_top'][~fin], want['iou_top'][~fin], err_msg=f'{what}: iou_top of empty slots')
    if fin.any():
        err = np.abs(got['iou_top'][fin].astype(np.float64) - want['iou_top'][fin].astype(np.float64)).max()
        assert err <= 1e-6, f'{what}: iou_top off by {err:.3e}'


def check_dict(got, want):
    """keys, their order and every value equal bit for bit (the host arithmetic is the spec's on equal integers)"""
    assert list(got) == list(want), (list(got), list(want))
    for k in want:
        assert float(got[k]).hex() == float(want[k]).hex(), (k, got[k], want[k])


# ------------------------------------------------------------------------------------------------------------------ occupancy
def occ_dense_gt(shape, gt_list, mask):
    """rule 1: the dense ground truth; the LAST occurrence of a voxel wins, voxels outside the mask become 255, rows outside the
    volume are dropped"""
    X, Y, Z = shape
    gt = np.zeros(shape, np.int64)
    for x, y, z, lab in np.asarray(gt_list, np.int64).reshape(-1, 4):
        if 0 <= x < X and 0 <= y < Y and 0 <= z < Z:
            gt[x, y, z] = lab
    if mask is not None:
        gt[~np.asarray(mask, bool)] = 255
    return gt


def occ_confusion(pred, gt, C):
    """rule 2 -> (C,3) int64 [both, gt, pred] per row"""
    pred, gt = np.asarray(pred, np.int64).reshape(-1), np.asarray(gt, np.int64).reshape(-1)
    keep = gt != 255
    p, g = pred[keep], gt[keep]
    out = np.zeros((C, 3), np.int64)
    out[0] = [((g != 0) & (p != 0)).sum(), (g != 0).sum(), (p != 0).sum()]
    for j in range(1, C):
        out[j] = [((g == j) & (p == j)).sum(), (g == j).sum(), (p == j).sum()]
    return out


def occ_sample_counts(sample, C):
    pred, gt_list, mask = sample
    return occ_confusion(pred, occ_dense_gt(np.asarray(pred).shape, gt_list, mask), C)


def occ_dict(counts, classes):
    """rule 3: (C,3) summed counts -> (dict of the classes with a non-empty union, mean over them or None)"""
    score = np.asarray(counts, np.float64)
    ret = {}
    with np.errstate(all='ignore'):
        for i in range(len(classes) + 1):
            tp, p, g = score[i]
            v = tp / (p + g - tp)
            if np.isnan(v):
                continue
            ret['empty' if i == 0 else classes[i - 1]] = float(v)
    vals = list(ret.values())
    return ret, (sum(vals) / len(vals) if vals else None)


def occ_eval(samples, classes):
    C = len(classes) + 1
    total = np.zeros((C, 3), np.int64)
    for s in samples:
        total += occ_sample_counts(s, C)
    return occ_dict(total, classes)[0]


def check_counts(got, want, what=''):
    """integer counts (tally or confusion): shape and every entry equal"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f'{what}: shape {got.shape} vs {want.shape}'
    np.testing.assert_array_equal(got.astype(np.int64), want.astype(np.int64), err_msg=f'{what}: counts')
