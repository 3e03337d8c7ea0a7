"""es_track_assign (csrc/ground.hip) and embodiedscan_amd.tracks.TrackTable held to tests/track_spec.py.

On the walk populations (5 frames, 6 .. 18 detections, seeds track_spec.SEEDS; max_age = 1) the ids and the whole table after every
frame equal (a) the spec over the matrix es_box3d_iou itself returns -- bit for bit the values the kernel compares -- and (b) the spec
over the oracle's f64 matrix, an independent reference under track_spec.conditions().  Synthetic matrices go straight to
es_track_assign (no geometry; reference: the spec over the same matrix): n in {0, 1, 63, 64, 65} x m in {0, 1, 63, 64, 65, 257} with
ld = m + 3 and 0.99 in the padding columns, the 40-step staircase (one pair per round), all entries tied, an entry equal to
f32(iou_thr), NaN entries, 0.99 in a column at or above counts[0] and in a dead track's column, same_class on and off, a full table
(cap = 8, 11 births), the ageing at its edge, equal scores in the label rule.  Every buffer carries a sentinel tail that must survive,
the slots at and above n_tracks hold sentinels that must survive, the inputs are unchanged, the refusals write nothing, two runs are
bit-equal.

Every body is a function of `dev`: tests/test_emu_tracks.py runs the same bodies on the CPU emulator."""
import numpy as np
import pytest
import torch

import track_spec as S

pytestmark = pytest.mark.gpu

SENT_F, SENT_I, PAD = -7.25e5, -9, 3
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _hip():
    from embodiedscan_amd import hip
    return hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def device_iou(dev, a, b):
    """the (n, m) f32 matrix es_box3d_iou(a, n, b, m) stores, as numpy"""
    hip = _hip()
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return np.zeros((n, m), np.float32)
    ta, tb = (torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in (a, b))
    out = torch.empty((n, m), dtype=torch.float32, device=dev)
    hip.call('es_box3d_iou', hip.P(ta), n, hip.P(tb), m, hip.P(out), _st())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _dets(n, seed=0, n_labels=3):
    rng = np.random.default_rng(100 + seed)
    boxes = rng.uniform(-1, 1, (n, 9)).astype(np.float32)
    return boxes, rng.uniform(0.1, 1, n).astype(np.float32), rng.integers(0, n_labels, n).astype(np.int32)


def table_of(cap, m, seed=0, dead=(), t=0):
    """a table of capacity cap with PAD sentinel rows behind it and sentinels in every slot: m tracks born at frame t (by the spec),
    those of `dead` killed"""
    tab = S.new_table(cap, PAD, SENT_F, SENT_I)
    S.update_spec(tab, cap, t, None, 0, *_dets(m, seed + 50))
    for i in dead:
        tab['i'][i, S.ALIVE] = 0
    return tab


def run_assign(dev, tab, iou, m, dets, cap, t, iou_thr=S.IOU_THR, same_class=False, max_age=-1, expect=0, n=None, ld=None):
    """one call of es_track_assign on device copies of `tab` (with its tails), iou (n, ld) and the detections, each input and det_track
    behind a sentinel tail -> (the table after, det_track with its tail, det_track before).  Asserts the status, that the inputs and
    their tails are unchanged and that a refused call wrote nothing."""
    hip = _hip()
    P = hip.P
    boxes, scores, labels = dets
    n = len(scores) if n is None else n
    iou = np.zeros((max(n, 0), 0), np.float32) if iou is None else np.ascontiguousarray(iou, dtype=np.float32)
    ld = iou.shape[1] if ld is None else ld

    def padded(a, dtype, sent):
        a = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).reshape(-1)
        return torch.cat([a, torch.full((PAD,), sent, dtype=dtype)]).to(dev)
    d_iou, d_b, d_s = padded(iou, torch.float32, SENT_F), padded(boxes, torch.float32, SENT_F), padded(scores, torch.float32, SENT_F)
    d_l = padded(labels, torch.int32, SENT_I)
    d_tab = {k: torch.from_numpy(tab[k].copy()).to(dev) for k in S.FIELDS}
    d_ids = torch.full((max(n, 0) + PAD,), SENT_I, dtype=torch.int32, device=dev)
    ins = [x.clone() for x in (d_iou, d_b, d_s, d_l)]
    rc = hip.raw('es_track_assign')(P(d_iou), n, m, ld, P(d_b), P(d_s), P(d_l), P(d_tab['boxes']), P(d_tab['f']), P(d_tab['i']), P(d_tab['counts']),
                                    cap, t, iou_thr, int(same_class), max_age, P(d_ids), _st())
    torch.cuda.synchronize()
    assert rc == expect, f'status {rc}, expected {expect}'
    for name, x, x0 in zip(('iou', 'det_boxes', 'det_scores', 'det_labels'), (d_iou, d_b, d_s, d_l), ins):
        assert torch.equal(x.view(torch.int32), x0.view(torch.int32)), f'{name}: an input (or its tail) was written'
    after = {k: d_tab[k].cpu().numpy() for k in S.FIELDS}
    ids = d_ids.cpu().numpy()
    if rc != 0:
        assert all(np.array_equal(after[k].view(np.int32), tab[k].view(np.int32)) for k in S.FIELDS) and bool((ids == SENT_I).all()), 'a refused call wrote something'
    return after, ids, np.full(len(ids), SENT_I, np.int32)


def assign_case(dev, label, tab, iou, m, dets, cap, t, ld=None, **kw):
    """run_assign twice (bit-equal) and S.check against the spec over the same matrix -> (the table after, det_track (n))"""
    after, ids, ids0 = run_assign(dev, tab, iou, m, dets, cap, t, ld=ld, **kw)
    S.check(label, tab, after, ids, cap, t, iou, m, *dets, det_track_before=ids0, **kw)
    again, ids2, _ = run_assign(dev, tab, iou, m, dets, cap, t, ld=ld, **kw)
    assert np.array_equal(ids, ids2) and all(np.array_equal(after[k].view(np.int32), again[k].view(np.int32)) for k in S.FIELDS), f'{label}: two runs differ'
    return after, ids[:len(dets[1])]


# ------------------------------------------------------------------------------------------------------------------ the walks
def walk_case(dev, seed, cap=64, max_age=1):
    from embodiedscan_amd.structures import InstanceData
    from embodiedscan_amd.tracks import TrackTable
    c = S.conditions(seed, cap=cap, max_age=max_age)
    table = TrackTable(dev, capacity=cap, max_age=max_age)

    def snapshot():
        return {k: getattr(table, k).cpu().numpy().copy() for k in S.FIELDS}          # (a copy: on the emulator .cpu() is the table itself)
    err = 0.0
    for t, (fr, (iou64, before64, after64, ids64)) in enumerate(zip(S.walk(seed), S.oracle_run(seed, cap=cap, max_age=max_age))):
        before = snapshot()
        nt0 = int(before['counts'][0])
        assert nt0 <= table._bound <= cap, 'the host bound is not an upper bound'
        iou32 = device_iou(dev, fr['boxes'], before['boxes'][:nt0])
        inst = InstanceData(bboxes_3d=torch.from_numpy(fr['boxes']).to(dev), scores_3d=torch.from_numpy(fr['scores']).to(dev),
                            labels_3d=torch.from_numpy(fr['labels']).long().to(dev))
        ids = table.update(inst)
        assert ids.dtype == torch.int64 and ids.device.type == dev.type and table.t == t
        after = snapshot()
        S.check(f'seed {seed} frame {t}, own matrix', before, after, ids.cpu().numpy(), cap, t, iou32, cap, fr['boxes'], fr['scores'], fr['labels'], max_age=max_age)
        S.check(f'seed {seed} frame {t}, oracle matrix', before64, after, ids.cpu().numpy(), cap, t, iou64, cap, fr['boxes'], fr['scores'], fr['labels'], max_age=max_age)
        assert ids.cpu().tolist() == ids64.tolist()
        live = [i for i in range(nt0) if before['i'][i, S.ALIVE] != 0]
        if live:
            err = max(err, float(np.abs(iou32[:, live].astype(np.float64) - iou64[:, live]).max()))
        hits, first = table.lookup(ids)
        assert hits.cpu().tolist() == after['i'][ids.cpu().numpy(), S.HITS].tolist() and first.cpu().tolist() == after['i'][ids.cpu().numpy(), S.FIRST].tolist()
    print(f'seed {seed}: {c["births"]} births, {c["deaths"]} deaths, {c["contested"]} contested rows, at most {c["rounds"]} rounds; '
          f'es_box3d_iou against the oracle on live pairs: max abs err {err:.1e}')
    # the inventory: the one read-back, which also makes the host's bound exact
    nt = int(after['counts'][0])
    for kw in (dict(), dict(min_hits=2), dict(alive_only=False), dict(min_hits=3, alive_only=False)):
        inv = table.inventory(**kw)
        rows = after['i'][:nt]
        want = [i for i in range(nt) if rows[i, S.HITS] >= kw.get('min_hits', 1) and (rows[i, S.ALIVE] != 0 or not kw.get('alive_only', True))]
        assert inv.track_ids.dtype == torch.int64 and inv.track_ids.cpu().tolist() == want and 0 < len(want)
        assert np.array_equal(inv.bboxes_3d.tensor.cpu().numpy(), after['boxes'][want]) and np.array_equal(inv.scores_3d.cpu().numpy(), after['f'][want, 0])
        for name, col in (('labels_3d', S.LABEL), ('hits', S.HITS), ('first_seen', S.FIRST), ('last_seen', S.LAST)):
            assert getattr(inv, name).cpu().tolist() == rows[want, col].tolist(), name
    assert table._bound == nt and table.dropped == 0
    return table


@pytest.mark.parametrize('seed', S.SEEDS)
def test_walks_against_own_and_oracle_matrix(dev, seed):
    walk_case(dev, seed)


def test_track_table_interface(dev):
    from embodiedscan_amd.structures import InstanceData
    from embodiedscan_amd.tracks import TrackTable
    table = walk_case(dev, S.SEEDS[0])
    assert table.state_bytes() >= 64 * (9 + 2 + 5) * 4 + 8
    fr = S.walk(S.SEEDS[0])[0]
    inst = InstanceData(bboxes_3d=torch.from_numpy(fr['boxes']).to(dev), scores_3d=torch.from_numpy(fr['scores']).to(dev),
                        labels_3d=torch.from_numpy(fr['labels']).long().to(dev))
    snap = [x.clone() for x in (table.boxes, table.f, table.i, table.counts)]
    for t in (4, 3, -1):
        with pytest.raises(ValueError, match='must increase'):
            table.update(inst, t=t)
    big = InstanceData(bboxes_3d=torch.zeros((2049, 9), device=dev), scores_3d=torch.zeros(2049, device=dev), labels_3d=torch.zeros(2049, dtype=torch.long, device=dev))
    with pytest.raises(ValueError, match='2048'):
        table.update(big)
    with pytest.raises(ValueError, match=r'boxes \(n, 9\)'):
        table.update(InstanceData(bboxes_3d=inst.bboxes_3d, scores_3d=inst.scores_3d[:2], labels_3d=inst.labels_3d))
    if dev.type == 'cuda':
        with pytest.raises(ValueError, match='scores on cpu'):
            table.update(InstanceData(bboxes_3d=inst.bboxes_3d, scores_3d=inst.scores_3d.cpu(), labels_3d=inst.labels_3d))
    assert all(torch.equal(a, b) for a, b in zip(snap, (table.boxes, table.f, table.i, table.counts))) and table.t == 4, 'a refused update changed the table'
    for kw in (dict(capacity=0), dict(capacity=4097), dict(iou_thr=-0.1), dict(iou_thr=NAN)):
        with pytest.raises(ValueError):
            TrackTable(dev, **kw)
    ids = table.update(inst, t=9)                              # a gap in t is fine; every track but the matched ones is long dead
    assert table.t == 9 and len(ids) == len(fr['scores'])
    empty = InstanceData(bboxes_3d=inst.bboxes_3d[:0], scores_3d=inst.scores_3d[:0], labels_3d=inst.labels_3d[:0])
    assert table.update(empty).shape == (0,) and table.t == 10
    assert table.inventory().last_seen.cpu().tolist() == [9] * len(ids), 'only the tracks of frame 9 are alive (max_age = 1)'
    assert table.update(empty).shape == (0,) and len(table.inventory().track_ids) == 0, 'an empty frame still ages the table'
    table.reset()
    assert table.t is None and int(table.counts[0]) == 0 and len(table.inventory(alive_only=False).track_ids) == 0
    assert table.update(inst).cpu().tolist() == list(range(len(fr['scores']))), 'after reset the ids start again at 0'


# ------------------------------------------------------------------------------------------------------------------ synthetic matrices
def random_matrix(n, m, seed, thr=S.IOU_THR):
    """(n, m + 3) f32: a few levels (exact ties), NaNs, entries equal to f32(thr); 0.99 in the three padding columns"""
    rng = np.random.default_rng(300 + seed)
    levels = np.array([0, 0, 0, 0.1, np.float32(thr), 0.3, 0.5, 0.5, 0.7, NAN], np.float32)
    iou = np.full((n, m + 3), 0.99, np.float32)
    iou[:, :m] = levels[rng.integers(0, len(levels), (n, m))]
    return iou


def size_case(dev, n, m, same_class=False):
    cap = 330
    dead = [i for i in range(m) if i % 7 == 3]
    tab = table_of(cap, m, seed=n, dead=dead)
    iou = random_matrix(n, m, 1000 * n + m)
    if m > 3 and n > 0:
        iou[:, 3] = 0.99                                       # a dead track's column
    after, ids = assign_case(dev, f'n = {n}, m = {m}', tab, iou, m, _dets(n, n + m), cap, 1, same_class=same_class, max_age=0, ld=m + 3)
    assert not any(i in dead for i in ids.tolist()), 'a dead track was matched'
    if n >= 63 and m >= 63:
        matched = int((ids < m).sum())
        assert 10 < matched, 'the case matches almost nothing'
    return ids


@pytest.mark.parametrize('n', [0, 1, 63, 64, 65])
def test_sizes_around_the_wave(dev, n):
    for m in (0, 1, 63, 64, 65, 257):
        size_case(dev, n, m, same_class=(n + m) % 2 == 1)


def test_staircase_takes_one_pair_per_round(dev):
    n = 40
    iou = np.zeros((n, n), np.float32)
    for j in range(n):
        iou[j, j] = 0.9 - 0.02 * j
        if j + 1 < n:
            iou[j + 1, j] = 0.89 - 0.02 * j
    cand = [(j, i) for j in range(n) for i in range(n) if iou[j, i] > np.float32(0.05)]
    r = []
    S.mutual_best_match(iou, cand, r)
    assert r == [n]
    _, ids = assign_case(dev, 'staircase', table_of(64, n), iou, n, _dets(n, 1), 64, 1, iou_thr=0.05)
    assert ids.tolist() == list(range(n))


def test_rules_at_their_edges(dev):
    cap = 16
    # every entry tied: j <-> j, the surplus rows are born
    tab = table_of(cap, 5)
    _, ids = assign_case(dev, 'ties', tab, np.full((7, 5), 0.5, np.float32), 5, _dets(7, 2), cap, 1)
    assert ids.tolist() == [0, 1, 2, 3, 4, 5, 6]
    _, ids = assign_case(dev, 'ties, wide', tab, np.full((3, 5), 0.5, np.float32), 5, _dets(3, 2), cap, 1)
    assert ids.tolist() == [0, 1, 2]
    # an entry equal to f32(iou_thr) is no candidate, the next f32 above it is; NaN is none
    thr = np.float32(S.IOU_THR)
    iou = np.array([[thr, 0, 0, 0, 0], [0, np.nextafter(thr, np.float32(1)), 0, 0, 0], [0, 0, NAN, 0, 0], [NAN, NAN, NAN, NAN, NAN]], np.float32)
    _, ids = assign_case(dev, 'threshold', tab, iou, 5, _dets(4, 3), cap, 1)
    assert ids.tolist() == [5, 1, 6, 7]
    # 0.99 in the columns at and above counts[0] (the host's bound m overshoots) and in a dead track's column: all ignored
    tab = table_of(cap, 5, dead=(2,))
    iou = np.zeros((3, 9), np.float32)
    iou[:, 5:] = 0.99
    iou[:, 2] = 0.99
    iou[1, 4] = 0.4
    after, ids = assign_case(dev, 'bound', tab, iou, 9, _dets(3, 4), cap, 1)
    assert ids.tolist() == [5, 4, 6] and after['counts'][:2].tolist() == [7, 0]
    # ... and a bound BELOW counts[0] hides the columns above it but the births still go behind counts[0]
    iou = np.full((2, 5), 0.9, np.float32)
    _, ids = assign_case(dev, 'low bound', table_of(cap, 5), iou, 3, _dets(2, 4), cap, 1)
    assert ids.tolist() == [0, 1]
    _, ids = assign_case(dev, 'zero bound', table_of(cap, 5), iou, 0, _dets(2, 4), cap, 1)
    assert ids.tolist() == [5, 6]
    # same_class on and off
    tab = table_of(cap, 2)
    tab['i'][:2, S.LABEL] = (1, 2)
    iou = np.array([[0.9, 0.5], [0.6, 0.8]], np.float32)
    b, s, _ = _dets(2, 5)
    l = np.array([2, 2], np.int32)
    assert assign_case(dev, 'any class', tab, iou, 2, (b, s, l), cap, 1)[1].tolist() == [0, 1]
    assert assign_case(dev, 'same class', tab, iou, 2, (b, s, l), cap, 1, same_class=True)[1].tolist() == [2, 1]
    # equal scores in the label rule: >= takes the detection's label, a lower score leaves it
    tab = table_of(cap, 2)
    tab['f'][:2, 1] = (0.5, 0.5)
    tab['i'][:2, S.LABEL] = (7, 7)
    s = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0))], np.float32)
    after, ids = assign_case(dev, 'label rule', tab, np.eye(2, dtype=np.float32), 2, (b, s, np.array([1, 2], np.int32)), cap, 1)
    assert ids.tolist() == [0, 1] and after['i'][:2, S.LABEL].tolist() == [1, 7] and after['f'][:2].tolist() == [[s[0], s[0]], [s[1], np.float32(0.5)]]


def test_a_full_table_drops_births(dev):
    cap = 8
    tab = table_of(cap, 2)
    iou = np.zeros((13, 2), np.float32)
    iou[4, 1] = 0.6
    iou[9, 0] = 0.7
    after, ids = assign_case(dev, 'full', tab, iou, 2, _dets(13, 6), cap, 1, max_age=0)
    assert ids.tolist() == [2, 3, 4, 5, 1, 6, 7, -1, -1, 0, -1, -1, -1] and after['counts'][:2].tolist() == [8, 5]
    # the issue's case: 11 births into 8 free slots: 3 ids of -1, dropped = 3, nothing written past slot 7 (the sentinel rows behind)
    tab = S.new_table(cap, PAD, SENT_F, SENT_I)
    after, ids = assign_case(dev, '11 births', tab, None, 0, _dets(11, 7), cap, 0)
    assert ids.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, -1, -1, -1] and after['counts'][:2].tolist() == [8, 3]
    after2, ids = assign_case(dev, 'full again', after, np.zeros((2, 8), np.float32), 8, _dets(2, 8), cap, 1)
    assert ids.tolist() == [-1, -1] and after2['counts'][:2].tolist() == [8, 5]


def test_ageing_at_its_edge(dev):
    cap = 8
    tab = table_of(cap, 4, t=0)
    tab['i'][:4, S.LAST] = (0, 1, 2, 3)
    iou = np.zeros((1, 4), np.float32)
    iou[0, 0] = 0.9                                            # track 0 is matched: it stays whatever its age was
    for max_age, alive in ((2, [1, 0, 1, 1]), (0, [1, 0, 0, 0]), (-1, [1, 1, 1, 1]), (3, [1, 1, 1, 1])):
        after, ids = assign_case(dev, f'max_age {max_age}', tab, iou, 4, _dets(1, 9), cap, 4, max_age=max_age)
        assert ids.tolist() == [0] and after['i'][:4, S.ALIVE].tolist() == alive, f'max_age = {max_age}: t - last_seen == max_age stays, + 1 dies'
    after, ids = assign_case(dev, 'n = 0 ages', tab, None, 4, _dets(0), cap, 4, ld=4, max_age=1)
    assert after['i'][:4, S.ALIVE].tolist() == [0, 0, 0, 1] and after['counts'][:2].tolist() == [4, 0]


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(dev):
    cap = 16
    tab = table_of(cap, 5)
    iou = np.full((4, 8), 0.9, np.float32)
    d = _dets(4, 10)
    for kw in (dict(n=-1), dict(n=2049), dict(cap=0), dict(cap=4097), dict(m=-1), dict(m=17), dict(ld=4), dict(iou_thr=-0.01), dict(iou_thr=NAN)):
        a = dict(dict(n=4, cap=cap, m=5, ld=8, iou_thr=S.IOU_THR), **kw)
        run_assign(dev, tab, iou, a['m'], d, a['cap'], 1, iou_thr=a['iou_thr'], expect=-4, n=a['n'], ld=a['ld'])
