"""Specification of the scene inventory filter (es_box3d_iou_filter, embodiedscan_amd.inference.filter_instances): the greedy of the
reference's demo (demo/demo.py:102-130, nms_filter) in plain Python over a GIVEN IoU matrix, the populations the tests run on, and
the conditions under which the greedy over the oracle's f64 matrix is an independent reference for the kernel.  TEST INFRASTRUCTURE.

The rule.  Rows are visited by descending score, ties to the lower row (Python's stable sort(reverse=True), es_topk_sorted).  A row
is skipped when its class already holds `topk` kept rows, when its score is below `score_thr`, or when iou[row][j] > iou_thr for
any kept row j -- the candidate is the FIRST index.  Both comparisons are made against the f32 thresholds of the C ABI; a NaN IoU
compares false and does not suppress.  A row whose label is outside [0, n_classes) is never kept (the project's addition: the
reference would count it in a dict)."""
import functools
import math

import numpy as np

IOU_THR, SCORE_THR = 0.15, 0.075           # the demo's defaults
TOPKS = (10, 3, 1)
SEEDS = (1, 3, 4)                          # the first three seeds for which conditions() holds (0 and 2: the score threshold removes nothing)


def order_of(scores):
    idx = list(range(len(scores)))
    idx.sort(key=lambda i: scores[i], reverse=True)
    return idx


def greedy(iou, scores, labels, n_classes, iou_thr=IOU_THR, score_thr=SCORE_THR, topk=10):
    """-> the kept rows in selection order.  iou: (n, n) array, f32 (what es_box3d_iou stores) or f64 (the oracle's); numpy compares
    either against the f32 threshold exactly (an f32 is an f64)."""
    thr, sthr = np.float32(iou_thr), np.float32(score_thr)
    scores = np.asarray(scores, np.float32)
    per_class, kept = {}, []
    for i in order_of(scores):
        l = int(labels[i])
        if l < 0 or l >= n_classes:
            continue
        if per_class.get(l, 0) >= topk:
            continue
        if scores[i] < sthr:
            continue
        if any(iou[i][j] > thr for j in kept):
            continue
        kept.append(i)
        per_class[l] = per_class.get(l, 0) + 1
    return kept


def check(label, keep_idx, keep_cnt, iou, scores, labels, n_classes, iou_thr=IOU_THR, score_thr=SCORE_THR, topk=10):
    """the output of a filter against the greedy over `iou`: count and every row, in order"""
    want = greedy(iou, scores, labels, n_classes, iou_thr, score_thr, topk)
    got = [int(v) for v in np.asarray(keep_idx).reshape(-1)[:int(keep_cnt)]]
    assert int(keep_cnt) == len(want), f'{label}: {int(keep_cnt)} rows kept, the greedy keeps {len(want)}'
    assert got == want, f'{label}: kept rows {got} != {want}'
    return want


# ------------------------------------------------------------------------------------------------------------------ populations
def clustered(seed, n_clusters=12, copies=8, n_classes=5, n_ties=10):
    """n_clusters objects, each detected `copies` times: centre jitter N(0, 0.25 x size) per axis, size x U(0.8, 1.25), angle jitter 0.15 rad; 80 % of
    a cluster share its label (the cluster labels are skewed towards the low classes so that a quota of 10 binds); scores U(0, 1) f32
    with n_ties rows at exactly 0.5.  -> dict(boxes (n,9) f32, scores (n) f32, labels (n) int32, n_classes)"""
    rng = np.random.default_rng(1000 + seed)
    side = 3.0 * math.sqrt(n_clusters / 12.0)             # the room grows with the number of objects: the density stays
    cen = np.stack([rng.uniform(-side, side, n_clusters), rng.uniform(-side, side, n_clusters), rng.uniform(0.3, 1.5, n_clusters)], 1)
    size = rng.uniform(0.4, 1.5, (n_clusters, 3))
    ang = np.stack([rng.uniform(-math.pi, math.pi, n_clusters), rng.uniform(-.3, .3, n_clusters), rng.uniform(-.3, .3, n_clusters)], 1)
    p = np.array([.4, .25, .15, .1, .1]) if n_classes == 5 else np.full(n_classes, 1.0 / n_classes)
    clab = rng.choice(n_classes, n_clusters, p=p)
    boxes, labels = [], []
    for c in range(n_clusters):
        for _ in range(copies):
            s = size[c] * rng.uniform(0.8, 1.25, 3)
            boxes.append(np.concatenate([cen[c] + rng.normal(0, 1, 3) * 0.25 * size[c], s, ang[c] + rng.uniform(-.15, .15, 3)]))
            labels.append(clab[c] if rng.random() < 0.8 else rng.integers(0, n_classes))
    n = len(boxes)
    perm = rng.permutation(n)                              # the copies of an object are not neighbours in the input
    boxes, labels = np.asarray(boxes, np.float32)[perm], np.asarray(labels, np.int32)[perm]
    scores = rng.random(n).astype(np.float32)
    scores[rng.choice(n, min(n_ties, n), replace=False)] = 0.5
    return dict(boxes=boxes, scores=scores, labels=labels, n_classes=n_classes)


@functools.lru_cache(maxsize=None)
def oracle_iou(seed):
    """the f64 matrix of oracle.grounding.box3d_iou on clustered(seed) (candidate = first argument); ~9000 Python clippings, computed
    once per process and left unchanged"""
    from oracle import grounding as OG
    b = clustered(seed)['boxes'].astype(np.float64)
    n = len(b)
    out = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            out[i, j] = OG.box3d_iou(b[i], b[j])
    out.setflags(write=False)
    return out


def conditions(pop, iou64, iou_thr=IOU_THR, score_thr=SCORE_THR, topks=TOPKS):
    """what makes the greedy over the f64 oracle matrix a valid reference for a kernel that compares f32-rounded IoUs: no oracle IoU
    within 1e-5 of the threshold (ten times the 1e-6 at which tests/test_gpu_ground_kernels.py holds es_box3d_iou to the oracle), no
    score within one f32 ulp of the score threshold -- and, so that the runs test something, each of the three rules changes the
    result at the largest quota of `topks`, and the quota at every one (at a quota of 1 or 3 every class is full long before the walk
    reaches the rows under the score threshold, and the few rows kept need not overlap: those two rules cannot be required to bind
    there).  -> the nearest off-diagonal IoU to the threshold"""
    thr, sthr = float(np.float32(iou_thr)), np.float32(score_thr)
    off = iou64[~np.eye(len(iou64), dtype=bool)]
    gap = float(np.abs(off - thr).min())
    assert gap > 1e-5, f'an oracle IoU lies {gap:.2e} from the threshold'
    s = pop['scores']
    assert not np.any(np.abs(s - sthr) <= np.spacing(sthr)), 'a score lies within one f32 ulp of the score threshold'
    n, C = len(s), pop['n_classes']
    for topk in topks:
        kept = greedy(iou64, s, pop['labels'], C, iou_thr, score_thr, topk)
        assert greedy(iou64, s, pop['labels'], C, iou_thr, score_thr, n) != kept, f'topk {topk}: the quota removes nothing'
        if topk == max(topks):
            assert greedy(iou64, s, pop['labels'], C, math.inf, score_thr, topk) != kept, f'topk {topk}: the suppression removes nothing'
            assert greedy(iou64, s, pop['labels'], C, iou_thr, -math.inf, topk) != kept, f'topk {topk}: the score threshold removes nothing'
    return gap
