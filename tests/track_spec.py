"""Specification of the track table (es_track_assign, embodiedscan_amd.tracks.TrackTable; the reference has no tracker: the definition
is include/es_hip.h's) in plain Python over a GIVEN IoU matrix, the checker, the walk populations the tests run on and the conditions
under which the spec over the oracle's f64 matrix is an independent reference for the kernel.  TEST INFRASTRUCTURE.

A table is a dict of numpy arrays: boxes (>= cap, 9) f32, f (>= cap, 2) f32 = score, label_score, i (>= cap, 5) int32 = label, first_seen,
last_seen, hits, alive, counts (>= 2) int32 = n_tracks, dropped.  Rows behind `cap` / entries behind counts[1] are sentinel tails:
update_spec never touches them and check() demands that nobody did.

update(t, detections), iou[j][i] = the [j][i] element es_box3d_iou(det_boxes, n, trk_boxes, m) stores (or the oracle's f64 value):
 1. (j, i) is a candidate iff i < min(m, n_tracks), track i is alive, iou[j][i] > f32(iou_thr) (strict; a NaN never is) and, with
    same_class, det_label[j] == label[i];
 2. the candidates are walked by descending IoU, ties to the lower row, then to the lower slot; a pair is taken when both ends are free;
 3. matched (j, i): box and score become the detection's, label and label_score too if det_score >= label_score (f32), hits += 1,
    last_seen = t, det_track[j] = i;
 4. unmatched detections are born in ascending row order into slots n_tracks, n_tracks + 1, ...: first_seen = last_seen = t, hits = 1,
    alive = 1, label_score = score; a birth that finds the table full gets det_track[j] = -1 and counts in `dropped`;
 5. after the births an alive track with t - last_seen > max_age dies (max_age < 0: never); it keeps its row and is never matched again."""
import functools
import math

import numpy as np

IOU_THR = 0.25                             # TrackTable's default
SEEDS = (0, 1, 2, 3, 4, 5)                 # the seeds for which conditions() holds (tests/test_track_spec.py runs every one)
LABEL, FIRST, LAST, HITS, ALIVE = range(5)
FIELDS = ('boxes', 'f', 'i', 'counts')


def new_table(cap, pad=0, sent_f=0.0, sent_i=0):
    """an empty table of capacity `cap` with `pad` sentinel rows behind every array"""
    tab = dict(boxes=np.full((cap + pad, 9), sent_f, np.float32), f=np.full((cap + pad, 2), sent_f, np.float32),
               i=np.full((cap + pad, 5), sent_i, np.int32), counts=np.full(2 + pad, sent_i, np.int32))
    tab['counts'][:2] = 0
    return tab


def copy_table(tab):
    return {k: tab[k].copy() for k in FIELDS}


def candidates(tab, iou, m, det_labels, iou_thr, same_class):
    """rule 1 -> the candidate pairs (j, i), by row, then by slot"""
    n, mm = len(det_labels), min(int(m), int(tab['counts'][0]))
    if n == 0 or mm == 0:
        return []
    with np.errstate(invalid='ignore'):
        ok = np.asarray(iou)[:n, :mm] > np.float32(iou_thr)                          # (a NaN compares false)
    ok &= (tab['i'][:mm, ALIVE] != 0)[None, :]
    if same_class:
        ok &= np.asarray(det_labels, np.int32)[:, None] == tab['i'][:mm, LABEL][None, :]
    return [(int(j), int(i)) for j, i in zip(*np.nonzero(ok))]


def greedy_match(iou, cand):
    """the definition: the candidates sorted by (IoU descending, row, slot), a pair taken when both ends are free -> {row: slot}"""
    rows, cols, out = set(), set(), {}
    for j, i in sorted(cand, key=lambda p: (-float(iou[p[0]][p[1]]), p[0], p[1])):
        if j in rows or i in cols:
            continue
        rows.add(j)
        cols.add(i)
        out[j] = i
    return out


def mutual_best_match(iou, cand, rounds=None):
    """the kernel's form: rounds of pairs that are the best free candidate of their row AND of their column, until a round takes
    nothing -> {row: slot}; rounds: a list that receives the number of rounds that took something"""
    def key(p):
        return (float(iou[p[0]][p[1]]), -p[0], -p[1])
    out, used_cols, n_rounds = {}, set(), 0
    while True:
        free = [p for p in cand if p[0] not in out and p[1] not in used_cols]
        rowbest, colbest = {}, {}
        for p in free:
            if p[0] not in rowbest or key(p) > key(rowbest[p[0]]):
                rowbest[p[0]] = p
            if p[1] not in colbest or key(p) > key(colbest[p[1]]):
                colbest[p[1]] = p
        took = [p for p in rowbest.values() if colbest[p[1]] == p]
        if not took:
            break
        n_rounds += 1
        for j, i in took:
            out[j] = i
            used_cols.add(i)
    if rounds is not None:
        rounds.append(n_rounds)
    return out


def update_spec(tab, cap, t, iou, m, det_boxes, det_scores, det_labels, iou_thr=IOU_THR, same_class=False, max_age=-1, match=greedy_match):
    """one update of `tab` in place -> det_track (n) int32.  iou: anything indexable as iou[j][i] for j < n, i < min(m, n_tracks) (f32 or
    f64: numpy compares either against the f32 threshold exactly); m: the caller's upper bound on n_tracks"""
    det_boxes = np.asarray(det_boxes, np.float32).reshape(-1, 9)
    det_scores, det_labels = np.asarray(det_scores, np.float32), np.asarray(det_labels, np.int32)
    n, nt0 = len(det_scores), int(tab['counts'][0])
    pairs = match(iou, candidates(tab, iou, m, det_labels, iou_thr, same_class))
    det_track = np.full(n, -1, np.int32)
    for j, i in pairs.items():
        tab['boxes'][i] = det_boxes[j]
        tab['f'][i, 0] = det_scores[j]
        if det_scores[j] >= tab['f'][i, 1]:
            tab['f'][i, 1] = det_scores[j]
            tab['i'][i, LABEL] = det_labels[j]
        tab['i'][i, HITS] += 1
        tab['i'][i, LAST] = t
        det_track[j] = i
    nt = nt0
    for j in range(n):
        if j in pairs:
            continue
        if nt >= cap:
            tab['counts'][1] += 1
            continue
        tab['boxes'][nt] = det_boxes[j]
        tab['f'][nt] = det_scores[j]
        tab['i'][nt] = (det_labels[j], t, t, 1, 1)
        det_track[j] = nt
        nt += 1
    tab['counts'][0] = nt
    if max_age >= 0:
        for i in range(nt):
            if tab['i'][i, ALIVE] != 0 and t - int(tab['i'][i, LAST]) > max_age:
                tab['i'][i, ALIVE] = 0
    return det_track


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all() if a.dtype == np.float32 else np.array_equal(a, b)


def check(label, before, after, det_track, cap, t, iou, m, det_boxes, det_scores, det_labels, iou_thr=IOU_THR, same_class=False, max_age=-1,
          det_track_before=None):
    """`after` and det_track (what an implementation made of `before`) against update_spec over `iou`: det_track, counts, every field of
    every slot below the new n_tracks, and -- bit for bit what `before` held -- every slot at or above it with the sentinel tails;
    det_track may be longer than n: the tail must equal det_track_before's.  -> (the table the spec makes, its det_track)"""
    want = copy_table(before)
    ids = update_spec(want, cap, t, iou, m, det_boxes, det_scores, det_labels, iou_thr, same_class, max_age)
    n = len(ids)
    got_ids = np.asarray(det_track).reshape(-1)
    assert got_ids[:n].tolist() == ids.tolist(), f'{label}: det_track {got_ids[:n].tolist()} != {ids.tolist()}'
    if det_track_before is not None:
        assert np.array_equal(got_ids[n:], np.asarray(det_track_before).reshape(-1)[n:]), f'{label}: det_track was written behind its {n} rows'
    assert after['counts'][:2].tolist() == want['counts'][:2].tolist(), f"{label}: counts {after['counts'][:2].tolist()} != {want['counts'][:2].tolist()}"
    assert _same(after['counts'][2:], before['counts'][2:]), f'{label}: the tail of counts was written'
    nt = int(want['counts'][0])
    names = dict(boxes=['box'], f=['score', 'label_score'], i=['label', 'first_seen', 'last_seen', 'hits', 'alive'])
    for k in ('boxes', 'f', 'i'):
        assert after[k].shape == before[k].shape
        for s in range(nt):
            if not _same(after[k][s], want[k][s]):
                bad = [names[k][c if k != 'boxes' else 0] for c in range(after[k].shape[1]) if not _same(after[k][s, c:c + 1], want[k][s, c:c + 1])]
                raise AssertionError(f'{label}: slot {s}: {sorted(set(bad))} = {after[k][s].tolist()}, the spec makes {want[k][s].tolist()}')
        assert _same(after[k][nt:], before[k][nt:]), f'{label}: {k}: a slot at or above n_tracks = {nt} (or the tail) was written'
    return want, ids


# ------------------------------------------------------------------------------------------------------------------ populations
T_FRAMES, N_OBJECTS, N_CLASSES = 5, 14, 5


def walk(seed):
    """a walk of T = 5 frames past 14 objects -> a list of dict(boxes (n,9) f32, scores (n) f32, labels (n) int32) per frame.
    Object o is visible from frame ceil((o - 3) / 3); objects 1 and 3 stand 0.35 x size beside objects 0 and 2 (two overlapping neighbour
    pairs); object 5 is missed at t = 2, 3; every fourth object is detected twice on odd frames; 2 random false positives per frame;
    a detection = the object with centre jitter N(0, 0.07 x size) per axis, size x U(0.9, 1.1), angles +- 0.05; 85 % of the detections
    carry the object's class; scores U(0.2, 1) f32; the rows of a frame are permuted."""
    rng = np.random.default_rng(7000 + seed)
    grid = rng.permutation(16)[:N_OBJECTS]                         # objects on a 4 x 4 grid of 2.5 m cells: apart unless made neighbours
    cen = np.stack([(grid % 4) * 2.5 + rng.uniform(-.4, .4, N_OBJECTS), (grid // 4) * 2.5 + rng.uniform(-.4, .4, N_OBJECTS),
                    rng.uniform(0.4, 1.2, N_OBJECTS)], 1)
    size = rng.uniform(0.5, 1.2, (N_OBJECTS, 3))
    ang = np.stack([rng.uniform(-math.pi, math.pi, N_OBJECTS), rng.uniform(-.2, .2, N_OBJECTS), rng.uniform(-.2, .2, N_OBJECTS)], 1)
    for a, b in ((0, 1), (2, 3)):
        size[b] = size[a] * rng.uniform(0.95, 1.05, 3)
        ang[b] = ang[a]
        cen[b] = cen[a] + np.array([0.35 * size[a, 0] * math.cos(ang[a, 0]), 0.35 * size[a, 0] * math.sin(ang[a, 0]), 0.0])
    cls = rng.integers(0, N_CLASSES, N_OBJECTS)
    frames = []
    for t in range(T_FRAMES):
        boxes, labels = [], []
        for o in range(N_OBJECTS):
            if t < max(math.ceil((o - 3) / 3), 0) or (o == 5 and t in (2, 3)):
                continue
            for _ in range(2 if (o % 4 == 0 and t % 2 == 1) else 1):
                boxes.append(np.concatenate([cen[o] + rng.normal(0, 1, 3) * 0.07 * size[o], size[o] * rng.uniform(0.9, 1.1, 3),
                                             ang[o] + rng.uniform(-.05, .05, 3)]))
                labels.append(cls[o] if rng.random() < 0.85 else rng.integers(0, N_CLASSES))
        for _ in range(2):
            boxes.append(np.concatenate([rng.uniform(-1, 9, 2), rng.uniform(0.3, 1.5, 1), rng.uniform(0.4, 1.2, 3),
                                         [rng.uniform(-math.pi, math.pi)], rng.uniform(-.2, .2, 2)]))
            labels.append(rng.integers(0, N_CLASSES))
        n = len(boxes)
        perm = rng.permutation(n)
        frames.append(dict(boxes=np.asarray(boxes, np.float32)[perm], scores=rng.uniform(0.2, 1.0, n).astype(np.float32),
                           labels=np.asarray(labels, np.int32)[perm]))
    return frames


def oracle_matrix(det_boxes, tab):
    """the f64 matrix of oracle.grounding.box3d_iou (the detection first) against the slots below n_tracks; dead slots stay 0: no rule
    reads them"""
    from oracle import grounding as OG
    nt = int(tab['counts'][0])
    out = np.zeros((len(det_boxes), nt))
    for i in range(nt):
        if tab['i'][i, ALIVE] == 0:
            continue
        b = tab['boxes'][i].astype(np.float64)
        for j, d in enumerate(det_boxes):
            out[j, i] = OG.box3d_iou(d.astype(np.float64), b)
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(seed, cap=64, iou_thr=IOU_THR, same_class=False, max_age=1):
    """the spec over the oracle's matrices along walk(seed) -> a tuple per frame of (iou64 (n, n_tracks before), table before, table
    after, det_track); a few hundred Python clippings, computed once per process and left unchanged"""
    tab, out = new_table(cap), []
    for t, fr in enumerate(walk(seed)):
        iou = oracle_matrix(fr['boxes'], tab)
        before = copy_table(tab)
        ids = update_spec(tab, cap, t, iou, cap, fr['boxes'], fr['scores'], fr['labels'], iou_thr, same_class, max_age)
        for a in (iou, ids) + tuple(before.values()):
            a.setflags(write=False)
        out.append((iou, before, copy_table(tab), ids))
    return tuple(out)


def conditions(seed, cap=64, iou_thr=IOU_THR, same_class=False, max_age=1):
    """what makes the spec over the oracle's f64 matrices a valid reference for a kernel that compares f32-rounded IoUs: along the walk
    no oracle IoU of a (detection, live track) pair within 1e-5 of the threshold, no two candidates that share a row or a column within
    1e-5 of each other (the margin tests/scene_filter_spec.py takes over the 1e-6 at which tests/test_gpu_ground_kernels.py holds
    es_box3d_iou to the oracle) -- and, so that the runs test something, at least one CONTESTED detection (the track of its highest
    candidate goes to another row) and, at max_age = 1, at least one death.
    -> dict(thr_gap, pair_gap, contested, deaths, rounds (the most mutual-best rounds of a frame), births)"""
    thr = float(np.float32(iou_thr))
    thr_gap = pair_gap = math.inf
    contested = deaths = births = rounds = 0
    for t, (iou, before, after, ids) in enumerate(oracle_run(seed, cap, iou_thr, same_class, max_age)):
        fr = walk(seed)[t]
        nt0 = int(before['counts'][0])
        live = [i for i in range(nt0) if before['i'][i, ALIVE] != 0]
        if live and len(iou):
            thr_gap = min(thr_gap, float(np.abs(iou[:, live] - thr).min()))
        cand = candidates(before, iou, cap, fr['labels'], iou_thr, same_class)
        for a in range(len(cand)):
            for b in range(a + 1, len(cand)):
                if cand[a][0] == cand[b][0] or cand[a][1] == cand[b][1]:
                    pair_gap = min(pair_gap, abs(float(iou[cand[a]]) - float(iou[cand[b]])))
        r = []
        assert mutual_best_match(iou, cand, r) == greedy_match(iou, cand)
        rounds = max(rounds, r[0])
        for j in {p[0] for p in cand}:
            best = max((p for p in cand if p[0] == j), key=lambda p: float(iou[p]))
            contested += int(ids[j] != best[1])
        births += int(after['counts'][0]) - nt0
        deaths += int((before['i'][:nt0, ALIVE] != 0).sum() - (after['i'][:nt0, ALIVE] != 0).sum())
    assert thr_gap > 1e-5, f'seed {seed}: an oracle IoU of a live pair lies {thr_gap:.2e} from the threshold'
    assert pair_gap > 1e-5, f'seed {seed}: two candidates that share a row or a column lie {pair_gap:.2e} apart'
    assert contested >= 1, f'seed {seed}: no contested detection'
    assert max_age != 1 or deaths >= 1, f'seed {seed}: no death at max_age = 1'
    return dict(thr_gap=thr_gap, pair_gap=pair_gap, contested=contested, deaths=deaths, rounds=rounds, births=births)
