"""tests/track_spec.py alone (no kernel): hand cases with known answers, the mutual-best form against the sorted greedy on matrices
full of exact ties, the walk populations against their conditions, and the checker against mutated outputs -- each a correct output
with ONE thing wrong."""
import numpy as np
import pytest

import track_spec as S

NAN = float('nan')


def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the checker accepted {what}')


def _dets(n, scores=None, labels=None, x0=0.0):
    boxes = np.zeros((n, 9), np.float32)
    boxes[:, 0] = x0 + np.arange(n)
    boxes[:, 3:6] = 1
    return boxes, np.asarray(scores if scores is not None else np.linspace(0.9, 0.5, n), np.float32), np.asarray(labels if labels is not None else np.zeros(n), np.int32)


def test_hand_cases():
    tab = S.new_table(4)
    b, s, l = _dets(2, [0.6, 0.7], [1, 2])
    ids = S.update_spec(tab, 4, 0, np.zeros((2, 0)), 0, b, s, l)
    assert ids.tolist() == [0, 1] and tab['counts'].tolist() == [2, 0], 'an empty table: every detection is born, in row order'
    assert tab['i'][:2].tolist() == [[1, 0, 0, 1, 1], [2, 0, 0, 1, 1]] and tab['f'][:2].tolist() == [[s[0], s[0]], [s[1], s[1]]]
    # row 0 prefers slot 1 (0.8) and slot 1 prefers row 0; row 1 is left with slot 0 (0.3); row 2 has nothing above the threshold
    iou = np.array([[0.5, 0.8], [0.3, 0.7], [0.25, 0.1]], np.float32)
    b2, s2, l2 = _dets(3, [0.9, 0.7, 0.5], [5, 6, 7], x0=10)
    ids = S.update_spec(tab, 4, 1, iou, 2, b2, s2, l2)
    assert ids.tolist() == [1, 0, 2], 'greedy by descending IoU; 0.25 is not above the threshold 0.25'
    assert tab['i'][:3].tolist() == [[6, 0, 1, 2, 1], [5, 0, 1, 2, 1], [7, 1, 1, 1, 1]] and tab['counts'].tolist() == [3, 0]
    assert tab['f'][0].tolist() == [s2[1], s2[1]] and tab['f'][1].tolist() == [s2[0], s2[0]] and np.array_equal(tab['boxes'][1], b2[0])
    # a lower score keeps the track's label; an equal score takes the detection's (>=)
    b3, s3, l3 = _dets(2, [0.5, s2[1]], [8, 9])
    ids = S.update_spec(tab, 4, 2, np.array([[0, 0.9, 0], [0.9, 0, 0]], np.float32), 3, b3, s3, l3, max_age=0)
    assert ids.tolist() == [1, 0] and tab['i'][:3].tolist() == [[9, 0, 2, 3, 1], [5, 0, 2, 3, 1], [7, 1, 1, 1, 0]], 'label rule / track 2 dies at max_age 0'
    assert tab['f'][1].tolist() == [np.float32(0.5), s2[0]]
    # the dead track is never matched again; the table is full after one more birth, the second one is dropped
    b4, s4, l4 = _dets(3)
    ids = S.update_spec(tab, 4, 5, np.array([[0, 0, 0.99], [0, 0, 0.9], [0.3, 0, 0.9]], np.float32), 3, b4, s4, l4)
    assert ids.tolist() == [3, -1, 0] and tab['counts'].tolist() == [4, 1] and tab['i'][2, S.ALIVE] == 0
    # same_class
    tab = S.new_table(4)
    S.update_spec(tab, 4, 0, None, 0, *_dets(2, labels=[1, 2]))
    iou = np.array([[0.9, 0.5], [0.6, 0.8]], np.float32)
    assert S.update_spec(S.copy_table(tab), 4, 1, iou, 2, *_dets(2, labels=[2, 2])).tolist() == [0, 1]
    assert S.update_spec(S.copy_table(tab), 4, 1, iou, 2, *_dets(2, labels=[2, 2]), same_class=True).tolist() == [2, 1], 'only slot 1 carries label 2'
    # NaN is no candidate; the bound m hides the columns at and above it; columns at and above n_tracks are ignored whatever they hold
    assert S.update_spec(S.copy_table(tab), 4, 1, np.array([[NAN, 0.4]], np.float32), 2, *_dets(1)).tolist() == [1]
    assert S.update_spec(S.copy_table(tab), 4, 1, np.array([[0.3, 0.9]], np.float32), 1, *_dets(1)).tolist() == [0]
    assert S.update_spec(S.copy_table(tab), 4, 1, np.array([[0.1, 0.2, 0.99, 0.99]], np.float32), 4, *_dets(1)).tolist() == [2]
    # ties: the lower row, then the lower slot
    assert S.update_spec(S.copy_table(tab), 4, 1, np.full((2, 2), 0.5, np.float32), 2, *_dets(2)).tolist() == [0, 1]
    assert S.update_spec(S.copy_table(tab), 4, 1, np.full((3, 2), 0.5, np.float32), 2, *_dets(3)).tolist() == [0, 1, 2]


def test_mutual_best_rounds_equal_the_sorted_greedy_on_tied_matrices():
    rng = np.random.default_rng(5)
    most = 0
    for k in range(300):
        n, m = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        iou = (rng.integers(0, 5, (n, m)) / np.float32(4)).astype(np.float32)          # five levels: full of exact ties
        if k % 3 == 0:
            iou[rng.random((n, m)) < 0.1] = NAN
        cand = [(j, i) for j in range(n) for i in range(m) if iou[j, i] > np.float32(0.2)]
        r = []
        assert S.mutual_best_match(iou, cand, r) == S.greedy_match(iou, cand), f'matrix {k}'
        most = max(most, r[0])
    assert most >= 4, 'the matrices never need more than a few rounds'
    # the staircase: exactly one pair per round
    n = 40
    iou = np.zeros((n, n), np.float32)
    for j in range(n):
        iou[j, j] = 0.9 - 0.02 * j
        if j + 1 < n:
            iou[j + 1, j] = 0.89 - 0.02 * j
    cand = [(j, i) for j in range(n) for i in range(n) if iou[j, i] > np.float32(0.05)]
    r = []
    assert S.mutual_best_match(iou, cand, r) == S.greedy_match(iou, cand) == {j: j for j in range(n)} and r == [n]


@pytest.mark.parametrize('seed', S.SEEDS)
def test_walks_meet_their_conditions(seed):
    frames = S.walk(seed)
    assert len(frames) == S.T_FRAMES and all(f['boxes'].dtype == np.float32 and f['boxes'].shape == (len(f['scores']), 9) for f in frames)
    c = S.conditions(seed)
    print(f'seed {seed}: {[len(f["scores"]) for f in frames]} detections per frame, {c["births"]} births, {c["deaths"]} deaths, '
          f'{c["contested"]} contested rows, at most {c["rounds"]} rounds; nearest IoU {c["thr_gap"]:.1e} from the threshold, nearest '
          f'candidates of a row or column {c["pair_gap"]:.1e} apart')
    assert c['rounds'] >= 2 and c['births'] > S.N_OBJECTS
    run = S.oracle_run(seed)
    ids = [r[3] for r in run]
    # object 5 is missed at t = 2, 3 and dies at max_age = 1: its detection at t = 4 is a birth, while the walk without ageing
    # continues some track there
    never = S.oracle_run(seed, max_age=-1)
    assert int(never[-1][2]['counts'][0]) < int(run[-1][2]['counts'][0])
    assert all(len(i) == len(f['scores']) for i, f in zip(ids, frames))


def _case(seed=S.SEEDS[0], t=3):
    iou, before, after, ids = S.oracle_run(seed)[t]
    fr = S.walk(seed)[t]
    return dict(before=before, after=S.copy_table(after), ids=ids.copy(), iou=iou, fr=fr, t=t)


def _check(c, label, after=None, ids=None, **kw):
    fr = c['fr']
    args = dict(dict(max_age=1), **kw)
    return S.check(label, c['before'], c['after'] if after is None else after, c['ids'] if ids is None else ids, 64, c['t'], c['iou'], 64, fr['boxes'], fr['scores'], fr['labels'],
                   **args)


def test_checker_rejects_mutated_outputs():
    c = _case()
    _check(c, 'good')
    fr, iou, before = c['fr'], c['iou'], c['before']
    cand = S.candidates(before, iou, 64, fr['labels'], S.IOU_THR, False)
    # a row-argmax matching on a contested row: the row takes its best track although another row holds it
    contested = [j for j in {p[0] for p in cand} if c['ids'][j] != max((p for p in cand if p[0] == j), key=lambda p: float(iou[p]))[1]]
    assert contested
    j = contested[0]
    best = max((p for p in cand if p[0] == j), key=lambda p: float(iou[p]))[1]
    ids = c['ids'].copy()
    ids[j] = best
    _rejected(lambda: _check(c, 'argmax', ids=ids), 'a row-argmax matching on a contested row')
    # a birth out of row order: the ids of the first two births swapped, with their rows
    born = [j for j in range(len(ids)) if c['ids'][j] >= int(before['counts'][0])]
    assert len(born) >= 2
    a, b = born[:2]
    ids, after = c['ids'].copy(), S.copy_table(c['after'])
    ids[a], ids[b] = ids[b], ids[a]
    for k in ('boxes', 'f', 'i'):
        after[k][[c['ids'][a], c['ids'][b]]] = after[k][[c['ids'][b], c['ids'][a]]]
    _rejected(lambda: _check(c, 'birth order', after=after, ids=ids), 'a birth out of row order')
    # a death one frame early / late
    nt0 = int(before['counts'][0])
    dying = [i for i in range(nt0) if before['i'][i, S.ALIVE] and not c['after']['i'][i, S.ALIVE]]
    staying = [i for i in range(nt0) if c['after']['i'][i, S.ALIVE] and c['after']['i'][i, S.LAST] == c['t'] - 1]
    assert dying and staying
    after = S.copy_table(c['after'])
    after['i'][staying[0], S.ALIVE] = 0
    _rejected(lambda: _check(c, 'early', after=after), 'a death one frame early')
    after = S.copy_table(c['after'])
    after['i'][dying[0], S.ALIVE] = 1
    _rejected(lambda: _check(c, 'late', after=after), 'a death one frame late')
    # a reused slot: a birth written over a track that died, instead of a new slot
    dead = [i for i in range(nt0) if not c['after']['i'][i, S.ALIVE]]
    ids, after = c['ids'].copy(), S.copy_table(c['after'])
    last = int(after['counts'][0]) - 1
    j = int(np.nonzero(c['ids'] == last)[0][0])
    for k in ('boxes', 'f', 'i'):
        after[k][dead[0]] = after[k][last]
        after[k][last] = before[k][last]
    after['counts'][0] = last
    ids[j] = dead[0]
    _rejected(lambda: _check(c, 'reuse', after=after, ids=ids), 'a birth in the slot of a dead track')
    # a slot above n_tracks written, a sentinel tail written, det_track written behind n
    after = S.copy_table(c['after'])
    after['f'][int(after['counts'][0]), 0] = 1
    _rejected(lambda: _check(c, 'beyond', after=after), 'a slot above n_tracks written')
    pad_before = {k: np.concatenate([v, np.full((3,) + v.shape[1:], 7, v.dtype)]) for k, v in before.items()}
    pad_after = {k: np.concatenate([v, np.full((3,) + v.shape[1:], 7, v.dtype)]) for k, v in c['after'].items()}
    cp = dict(c, before=pad_before, after=pad_after)
    _check(cp, 'padded')
    for k in S.FIELDS:
        bad = S.copy_table(pad_after)
        bad[k][-1] = 0
        _rejected(lambda: _check(cp, 'tail', after=bad), f'the tail of {k} written')
    tail = np.concatenate([c['ids'], [-9, -9]]).astype(np.int32)
    S.check('tail', before, c['after'], tail, 64, c['t'], iou, 64, fr['boxes'], fr['scores'], fr['labels'], max_age=1, det_track_before=np.full(len(tail), -9))
    tail[-1] = 0
    _rejected(lambda: S.check('tail', before, c['after'], tail, 64, c['t'], iou, 64, fr['boxes'], fr['scores'], fr['labels'], max_age=1,
                              det_track_before=np.full(len(tail), -9)), 'det_track written behind n')


def test_checker_rejects_a_swapped_tie_and_the_strict_label_rule():
    tab = S.new_table(4)
    S.update_spec(tab, 4, 0, None, 0, *_dets(2, [0.5, 0.5], [1, 2]))
    iou = np.full((2, 2), 0.5, np.float32)
    b, s, l = _dets(2, [0.5, 0.4], [3, 4], x0=5)
    after = S.copy_table(tab)
    ids = S.update_spec(after, 4, 1, iou, 2, b, s, l)
    assert ids.tolist() == [0, 1] and after['i'][:2, S.LABEL].tolist() == [3, 2], 'an equal score takes the label, a lower one does not'
    S.check('good', tab, after, ids, 4, 1, iou, 2, b, s, l)
    swapped = S.copy_table(after)
    for k in ('boxes', 'f', 'i'):
        swapped[k][[0, 1]] = 0
    sw = S.copy_table(tab)
    S.update_spec(sw, 4, 1, iou[::-1], 2, b[::-1], s[::-1], l[::-1])                     # rows 0 and 1 exchanged: row 1 takes slot 0
    _rejected(lambda: S.check('tie', tab, sw, np.array([1, 0], np.int32), 4, 1, iou, 2, b, s, l), 'a swapped tie')
    strict = S.copy_table(after)
    strict['i'][0, S.LABEL] = 1                                                          # `>` for `>=`: the equal score left the label
    _rejected(lambda: S.check('strict', tab, strict, ids, 4, 1, iou, 2, b, s, l), '> for >= in the label rule')
    _rejected(lambda: S.check('thr', tab, after, ids, 4, 1, iou, 2, b, s, l, iou_thr=0.5), 'a candidate at the threshold')
