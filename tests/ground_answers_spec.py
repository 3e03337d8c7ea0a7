"""Specification of the grounder's answer selection (es_ground_answers, embodiedscan_amd.inference.select_answers): the rule in plain
Python on top of scene_filter_spec.greedy, the populations the tests run on, and the conditions under which the greedy over the
oracle's f64 matrix is an independent reference for the kernel.  TEST INFRASTRUCTURE.

The rule.  For each prompt, independently: scene_filter_spec.greedy(iou, scores, labels = 0, n_classes = 1, iou_thr, score_thr, topk)
-- rows by descending score, ties to the lower row; a row below score_thr (f32) is skipped; a row whose iou[row][j] exceeds iou_thr
(f32) for an already kept row j is skipped, the candidate being the FIRST index, a NaN IoU not suppressing; the walk stops at topk
kept rows.  The project's additions: a NaN score is never an answer (such a row neither suppresses nor counts: the rule is applied
to the other rows); ans_idx[p][k] = -1 for k >= ans_cnt[p]; the kernel writes every entry of its row."""
import math

import numpy as np

import scene_filter_spec as F

IOU_THR, SCORE_THR = 0.25, 0.4             # the lower IoU of GroundingMetric; a score threshold away from the ties at 0.5
Q = 96                                     # rows of scene_filter_spec.clustered(seed)
TOPKS = (Q, 8, 1)
SEEDS = F.SEEDS                            # (1, 3, 4)
MAX_Q, MAX_P = 1024, 65535                 # limits of es_ground_answers


def answers(iou, scores, iou_thr=IOU_THR, score_thr=SCORE_THR, topk=1):
    """-> the answer rows of ONE prompt in selection order.  iou: (Q, Q) f32 or f64, scores (Q)"""
    scores = np.asarray(scores, np.float32)
    rows = np.flatnonzero(~np.isnan(scores))                  # a NaN score is never an answer
    sub = np.asarray(iou)[np.ix_(rows, rows)]
    kept = F.greedy(sub, scores[rows], np.zeros(len(rows), np.int32), 1, iou_thr, score_thr, topk)
    return [int(rows[k]) for k in kept]


def expected_row(iou, scores, iou_thr, score_thr, topk):
    """-> (ans_idx row (topk) int32 with its -1 tail, ans_cnt)"""
    kept = answers(iou, scores, iou_thr, score_thr, topk)
    return np.asarray(kept + [-1] * (topk - len(kept)), np.int32), len(kept)


def check(label, ans_idx_row, ans_cnt, iou, scores, iou_thr=IOU_THR, score_thr=SCORE_THR, topk=1):
    """one prompt's output row against the rule over `iou`: the count, every index in order, and the -1 tail"""
    want, n = expected_row(iou, scores, iou_thr, score_thr, topk)
    got = np.asarray(ans_idx_row).reshape(-1)
    assert int(ans_cnt) == n, f'{label}: {int(ans_cnt)} answers, the rule gives {n}'
    assert got.shape == (topk,) and got.tolist() == want.tolist(), f'{label}: answers {got.tolist()} != {want.tolist()}'
    return want[:n].tolist()


# ------------------------------------------------------------------------------------------------------------------ populations
def population(seed):
    """scene_filter_spec.clustered(seed) with the labels ignored -> dict(boxes (96, 9) f32, scores (96) f32, ten of them exactly 0.5)"""
    pop = F.clustered(seed)
    return dict(boxes=pop['boxes'], scores=pop['scores'])


def shuffled(seed, k):
    """prompt k of a many-prompt launch: population(seed) under a seeded row permutation with the scores dealt out anew
    -> dict(boxes, scores, perm) with boxes = population(seed).boxes[perm]"""
    pop = population(seed)
    rng = np.random.default_rng(7000 + 100 * seed + k)
    perm = rng.permutation(len(pop['scores']))
    return dict(boxes=pop['boxes'][perm], scores=pop['scores'][rng.permutation(len(perm))], perm=perm)


def spread(q, seed=0):
    """q boxes on a loose lattice (pitch 1.2, sizes 0.5 .. 1.4, any yaw): a box meets a few neighbours only, so a greedy over them
    clips few pairs; every eighth row repeats the row before it under a small shift, both with a score above 0.5, so that the
    suppression has something to remove.  Scores U(0, 1) otherwise, with ties (every 16th row takes the score of row 0)."""
    rng = np.random.default_rng(9000 + 31 * q + seed)
    side = max(int(math.ceil(q ** (1.0 / 3.0))), 1)
    cell = rng.permutation(side ** 3)[:q]
    cen = np.stack([cell % side, (cell // side) % side, cell // (side * side)], 1) * 1.2 + rng.uniform(-.1, .1, (q, 3))
    boxes = np.concatenate([cen, rng.uniform(.5, 1.4, (q, 3)), rng.uniform(-math.pi, math.pi, (q, 1)), rng.uniform(-.3, .3, (q, 2))], 1)
    for i in range(7, q, 8):
        boxes[i] = boxes[i - 1]
        boxes[i, :3] += rng.uniform(-.05, .05, 3)
    scores = rng.random(q).astype(np.float32)
    for i in range(7, q, 8):                               # both rows of a repeated pair lie above 0.5: one of them is suppressed
        scores[i - 1:i + 1] = np.float32(0.5) + np.float32(0.5) * scores[i - 1:i + 1]
    scores[::16] = scores[0]
    return dict(boxes=boxes.astype(np.float32), scores=scores)


def conditions(pop, iou64, iou_thr=IOU_THR, score_thr=SCORE_THR, topks=TOPKS):
    """what makes the rule over the f64 oracle matrix a valid reference for a kernel that compares f32-rounded IoUs -- no oracle IoU
    within 1e-5 of the threshold, no score within one f32 ulp of the score threshold -- and what makes the runs test something: at
    topk = Q the suppression and the score threshold each change the result; at the smaller quotas the quota does.  (Under a binding
    quota the score threshold cannot be required to bind: the quota fills from the top scores first.)
    -> dict(gap, kept per topk, kept without suppression, kept without the score threshold, tied rows among the kept)"""
    thr, sthr = float(np.float32(iou_thr)), np.float32(score_thr)
    off = iou64[~np.eye(len(iou64), dtype=bool)]
    gap = float(np.abs(off - thr).min())
    assert gap > 1e-5, f'an oracle IoU lies {gap:.2e} from the threshold'
    s = pop['scores']
    assert not np.any(np.abs(s - sthr) <= np.spacing(sthr)), 'a score lies within one f32 ulp of the score threshold'
    n = len(s)
    full = answers(iou64, s, iou_thr, score_thr, n)
    no_sup = answers(iou64, s, math.inf, score_thr, n)
    no_thr = answers(iou64, s, iou_thr, -math.inf, n)
    assert no_sup != full, 'the suppression removes nothing'
    assert no_thr != full, 'the score threshold removes nothing'
    kept = {}
    for topk in topks:
        kept[topk] = answers(iou64, s, iou_thr, score_thr, topk)
        if topk < n:
            assert kept[topk] != full and len(kept[topk]) == topk, f'topk {topk}: the quota removes nothing'
    vals, cnt = np.unique(s, return_counts=True)
    tied = set(vals[cnt > 1].tolist())
    return dict(gap=gap, kept={k: len(v) for k, v in kept.items()}, no_suppression=len(no_sup), no_score_thr=len(no_thr),
                tied_kept=sum(1 for i in full if float(s[i]) in tied))
