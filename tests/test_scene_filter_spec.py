"""tests/scene_filter_spec.py alone (no kernel): the populations meet their conditions, hand cases with known answers, and the checker
rejects mutated outputs -- each a correct output with ONE thing wrong."""
import math

import numpy as np
import pytest

import scene_filter_spec as S

NAN = float('nan')


def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the checker accepted {what}')


@pytest.mark.parametrize('seed', S.SEEDS)
def test_populations_meet_their_conditions(seed):
    pop, iou = S.clustered(seed), S.oracle_iou(seed)
    assert pop['boxes'].shape == (96, 9) and pop['boxes'].dtype == np.float32 and pop['scores'].dtype == np.float32
    assert int((pop['scores'] == 0.5).sum()) >= 10, 'the population holds no tied scores'
    gap = S.conditions(pop, iou)
    below = int((pop['scores'] < np.float32(S.SCORE_THR)).sum())
    above = int((iou > np.float32(S.IOU_THR)).sum()) - len(iou)
    kept = {k: len(S.greedy(iou, pop['scores'], pop['labels'], 5, topk=k)) for k in S.TOPKS}
    free = len(S.greedy(iou, pop['scores'], pop['labels'], 5, iou_thr=math.inf))
    print(f'seed {seed}: {above} pairs above the threshold, {below} rows under the score threshold, kept {kept}, without suppression {free}, '
          f'nearest off-diagonal IoU {gap:.1e} from the threshold')
    assert np.allclose(np.diag(iou), 1.0, atol=1e-9) and 3 <= below and above > 100
    ties = [i for i in S.greedy(iou, pop['scores'], pop['labels'], 5, iou_thr=math.inf, topk=96) if pop['scores'][i] == 0.5]
    assert len(ties) >= 2 and ties == sorted(ties), 'tied rows are visited in row order'


def _axis(c, s=(1, 1, 1)):
    return list(c) + list(s) + [0, 0, 0]


def test_hand_cases():
    from oracle import grounding as OG

    def matrix(boxes):
        return np.array([[OG.box3d_iou(np.array(a, float), np.array(b, float)) for b in boxes] for a in boxes])
    same = [_axis((0, 0, 0))] * 3
    iou = matrix(same)
    assert S.greedy(iou, [0.3, 0.9, 0.5], [0, 1, 2], 3) == [1], 'three identical boxes: the highest score stays'
    assert S.greedy(iou, [0.5, 0.5, 0.5], [0, 1, 2], 3) == [0], 'three identical boxes, tied: the lowest row stays'
    touch = [_axis((0, 0, 0)), _axis((1, 0, 0))]
    iou = matrix(touch)
    assert iou[0, 1] == 0.0 and S.greedy(iou, [0.4, 0.6], [0, 0], 1) == [1, 0], 'two face-touching boxes both stay'
    apart = [_axis((3 * k, 0, 0)) for k in range(4)]
    iou = matrix(apart)
    assert S.greedy(iou, [0.2, 0.8, 0.6, 0.4], [0, 0, 0, 0], 1, topk=1) == [1], 'quota 1, disjoint boxes of one class: one box'
    # rows 0 and 1 of class 0 (quota 1), row 2 of class 1 overlaps row 1 only: row 1 is over quota, so it does not suppress row 2
    boxes = [_axis((0, 0, 0)), _axis((5, 0, 0)), _axis((5.2, 0, 0))]
    iou = matrix(boxes)
    assert iou[2, 1] > 0.5 and S.greedy(iou, [0.9, 0.8, 0.7], [0, 0, 1], 2, topk=1) == [0, 2], 'a row over quota suppressed its neighbour'
    assert S.greedy(iou, [0.9, 0.8, 0.7], [0, 0, 1], 2, topk=2) == [0, 1]
    assert S.greedy(iou, [0.9, 0.8, 0.7], [0, 0, 7], 2, topk=2) == [0, 1] and S.greedy(iou, [0.9, 0.8, 0.7], [0, -1, 1], 2) == [0, 2]
    assert S.greedy(np.zeros((0, 0)), [], [], 1) == []
    sthr = np.float32(S.SCORE_THR)
    assert S.greedy(np.eye(2), [sthr, np.nextafter(sthr, np.float32(0))], [0, 0], 1) == [0], 'a score equal to f32(score_thr) is kept'


def test_checker_rejects_mutated_outputs():
    """a swapped tie, a quota off by one, a kept row under the threshold, iou[j][i] taken for iou[i][j] on a NaN pair"""
    pop, iou = S.clustered(S.SEEDS[0]), S.oracle_iou(S.SEEDS[0])
    s, l = pop['scores'], pop['labels']
    good = S.greedy(iou, s, l, 5)
    S.check('good', np.array(good + [-9] * 5), len(good), iou, s, l, 5)
    free = dict(iou_thr=math.inf, topk=96)                     # (no suppression, no quota: every tied row is kept)
    swapped = S.greedy(iou, s, l, 5, **free)
    S.check('free', np.array(swapped), len(swapped), iou, s, l, 5, **free)
    tied = [k for k, r in enumerate(swapped) if s[r] == 0.5]
    assert len(tied) >= 2 and tied[1] == tied[0] + 1
    swapped[tied[0]], swapped[tied[1]] = swapped[tied[1]], swapped[tied[0]]
    _rejected(lambda: S.check('tie', np.array(swapped), len(swapped), iou, s, l, 5, **free), 'two tied rows swapped')
    _rejected(lambda: S.check('short', np.array(good), len(good) - 1, iou, s, l, 5), 'a count one short')
    for topk in (3, 1):
        off = S.greedy(iou, s, l, 5, topk=topk + 1)
        _rejected(lambda: S.check('quota', np.array(off), len(off), iou, s, l, 5, topk=topk), f'a quota of {topk + 1} for {topk}')
    low = S.greedy(iou, s, l, 5, score_thr=-math.inf)
    assert low != good
    _rejected(lambda: S.check('score', np.array(low), len(low), iou, s, l, 5), 'a kept row under the score threshold')
    _rejected(lambda: S.check('strict', np.array(S.greedy(iou, s, l, 5, iou_thr=0.1501)), 0, iou, s, l, 5), 'another IoU threshold')
    # candidate 1 against kept 0: iou[1][0] is NaN (does not suppress), iou[0][1] is not
    m = np.array([[1.0, 0.9], [NAN, 1.0]])
    assert S.greedy(m, [0.9, 0.8], [0, 0], 1) == [0, 1] and S.greedy(m.T, [0.9, 0.8], [0, 0], 1) == [0]
    S.check('nan', np.array([0, 1]), 2, m, [0.9, 0.8], [0, 0], 1)
    _rejected(lambda: S.check('nan', np.array(S.greedy(m.T, [0.9, 0.8], [0, 0], 1)), 1, m, [0.9, 0.8], [0, 0], 1), 'iou[j][i] for iou[i][j]')
