"""es_box3d_iou_filter (csrc/ground.hip) and embodiedscan_amd.inference.filter_instances held to tests/scene_filter_spec.py.

On the clustered populations (96 boxes, seeds scene_filter_spec.SEEDS) at quotas 10, 3 and 1 the kept rows equal, row for row and in
order, (a) the Python greedy over the matrix es_box3d_iou itself returns -- bit for bit the values the kernel compares -- and (b) the
greedy over the oracle's f64 matrix, an independent reference under scene_filter_spec.conditions().  Edge cases (reference (a)):
n in {0, 1, 255, 256, 257, 300}, all rows under the score threshold, one class with a quota of 1, labels outside the range, zero-volume
boxes (NaN IoU), exact duplicates, a score equal to f32(score_thr).  Every buffer carries a sentinel tail that must survive, keep_idx
stays untouched behind keep_cnt, the refusals write nothing, two runs are bit-equal.

Every body is a function of `dev`: tests/test_emu_scene_filter.py runs the same bodies on the CPU emulator."""
import numpy as np
import pytest
import torch

import scene_filter_spec as S

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = -7.25e5, -9


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _hip():
    from embodiedscan_amd import hip
    return hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def _padded(dev, a, dtype, sent, pad=8):
    """a contiguous copy of `a` followed by `pad` sentinels -> (view of the copy, whole buffer)"""
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).reshape(-1)
    buf = torch.full((t.numel() + pad,), sent, dtype=dtype)
    buf[:t.numel()] = t
    buf = buf.to(dev)
    return buf[:t.numel()], buf


def device_iou(dev, boxes):
    """the (n, n) f32 matrix es_box3d_iou(boxes, n, boxes, n) stores, as numpy"""
    hip = _hip()
    n = len(boxes)
    if n == 0:
        return np.zeros((0, 0), np.float32)
    b = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32)).to(dev)
    out = torch.empty((n, n), dtype=torch.float32, device=dev)
    hip.call('es_box3d_iou', hip.P(b), n, hip.P(b), n, hip.P(out), _st())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_filter(dev, boxes, scores, labels, n_classes, iou_thr=S.IOU_THR, score_thr=S.SCORE_THR, topk=10, expect=0):
    """es_topk_sorted + es_box3d_iou_filter on buffers with sentinel tails -> (keep_idx (n) numpy, keep_cnt, status).  Asserts the
    tails of every buffer, the inputs themselves and keep_idx behind keep_cnt."""
    hip = _hip()
    P = hip.P
    n = len(scores)
    b, bb = _padded(dev, np.asarray(boxes, np.float32).reshape(n, 9), torch.float32, SENT_F)
    s, sb = _padded(dev, np.asarray(scores, np.float32), torch.float32, SENT_F)
    l, lb = _padded(dev, np.asarray(labels, np.int32), torch.int32, SENT_I)
    o, ob = _padded(dev, np.full(n, SENT_I), torch.int32, SENT_I)
    ki, kb = _padded(dev, np.full(n, SENT_I), torch.int32, SENT_I)
    kc, cb = _padded(dev, np.full(1, SENT_I), torch.int32, SENT_I)
    if 0 < n <= 16384:
        hip.call('es_topk_sorted', P(s), 1, n, 0, n, P(o), _st())
        torch.cuda.synchronize()
        assert o.cpu().tolist() == S.order_of(np.asarray(scores, np.float32)), 'es_topk_sorted: not the stable descending order'
    before = [t.clone() for t in (bb, sb, lb, ob)]
    rc = hip.raw('es_box3d_iou_filter')(P(b), P(s), P(l), P(o), n, n_classes, iou_thr, score_thr, topk, P(ki), P(kc), _st())
    torch.cuda.synchronize()
    assert rc == expect, f'status {rc}, expected {expect}'
    for name, t, t0 in zip(('boxes', 'scores', 'labels', 'order'), (bb, sb, lb, ob), before):
        assert torch.equal(t, t0), f'{name}: an input (or its tail) was written'
    assert bool((kb[n:] == SENT_I).all()) and bool((cb[1:] == SENT_I).all()), 'a launch wrote past the end of an output'
    if rc != 0:
        assert bool((kb == SENT_I).all()) and bool((cb == SENT_I).all()), 'a refused call wrote something'
        return None, None, rc
    cnt = int(kc.item())
    assert 0 <= cnt <= n
    assert bool((ki[cnt:] == SENT_I).all()), 'keep_idx was written beyond keep_cnt'
    return ki.cpu().numpy(), cnt, rc


def sized(n, seed=11, n_classes=5):
    """the first n rows of a clustered population of at least n rows"""
    pop = S.clustered(seed, n_clusters=max((n + 7) // 8, 1), n_classes=n_classes)
    return {k: (v[:n] if k != 'n_classes' else v) for k, v in pop.items()}


def against_own_matrix(dev, label, pop, **kw):
    iou = device_iou(dev, pop['boxes'])
    ki, cnt, _ = run_filter(dev, pop['boxes'], pop['scores'], pop['labels'], pop['n_classes'], **kw)
    want = S.check(label, ki, cnt, iou, pop['scores'], pop['labels'], pop['n_classes'], **kw)
    return want, iou


# ------------------------------------------------------------------------------------------------------------------ the populations
def population_case(dev, seed):
    pop = S.clustered(seed)
    iou64 = S.oracle_iou(seed)
    gap = S.conditions(pop, iou64)
    iou32 = device_iou(dev, pop['boxes'])
    err = float(np.abs(iou32.astype(np.float64) - iou64).max())
    print(f'seed {seed}: {int((iou64 > np.float32(S.IOU_THR)).sum() - len(iou64))} pairs above the threshold, nearest off-diagonal IoU '
          f'{gap:.1e} away; es_box3d_iou against the oracle: max abs err {err:.1e}')
    for topk in S.TOPKS:
        ki, cnt, _ = run_filter(dev, pop['boxes'], pop['scores'], pop['labels'], pop['n_classes'], topk=topk)
        a = S.check(f'seed {seed} topk {topk}, own matrix', ki, cnt, iou32, pop['scores'], pop['labels'], pop['n_classes'], topk=topk)
        b = S.check(f'seed {seed} topk {topk}, oracle matrix', ki, cnt, iou64, pop['scores'], pop['labels'], pop['n_classes'], topk=topk)
        assert a == b
        print(f'  topk {topk}: {cnt} kept')
        ki2, cnt2, _ = run_filter(dev, pop['boxes'], pop['scores'], pop['labels'], pop['n_classes'], topk=topk)
        assert cnt2 == cnt and np.array_equal(ki, ki2), 'two runs differ'


@pytest.mark.parametrize('seed', S.SEEDS)
def test_clustered_population_against_own_and_oracle_matrix(dev, seed):
    population_case(dev, seed)


# ------------------------------------------------------------------------------------------------------------------ edges
def size_case(dev, n):
    """no quota (topk = n), so that rows are kept down to the score threshold: at n = 300 the walk finds kept rows beyond the first
    256 sorted positions, the width of the workgroup's search"""
    pop = sized(n)
    want, _ = against_own_matrix(dev, f'n = {n}', pop, topk=max(n, 1))
    assert (len(want) > 0) == (n > 0 and bool((pop['scores'] >= np.float32(S.SCORE_THR)).any()))
    if n >= 255:
        assert 8 < len(want) < n, 'the case does not exercise the suppression'
    if n == 300:
        pos = {r: p for p, r in enumerate(S.order_of(pop['scores']))}
        assert max(pos[r] for r in want) >= 256, 'no kept row beyond the first 256 sorted positions'
    return want


@pytest.mark.parametrize('n', [0, 1, 255, 256, 257, 300])
def test_sizes_around_the_workgroup(dev, n):
    size_case(dev, n)


def test_rules_at_their_edges(dev):
    """all rows under the threshold; one class with a quota of 1; labels outside the range; a score equal to f32(score_thr)"""
    pop = sized(40, seed=12)
    low = dict(pop, scores=pop['scores'] * np.float32(0.07))
    want, _ = against_own_matrix(dev, 'all under the threshold', low)
    assert want == []
    one = dict(pop, labels=np.zeros(40, np.int32), n_classes=1)
    want, _ = against_own_matrix(dev, 'one class, quota 1', one, topk=1)
    assert want == [S.order_of(pop['scores'])[0]]
    lab = pop['labels'].copy()
    lab[::3] = -1
    lab[1::5] = 5
    lab[7] = -2 ** 31
    lab[8] = 2 ** 31 - 1
    want, _ = against_own_matrix(dev, 'labels outside the range', dict(pop, labels=lab), topk=40, iou_thr=2.0)
    assert want and all(0 <= lab[i] < 5 for i in want) and len(want) == int(((lab >= 0) & (lab < 5) & (pop['scores'] >= np.float32(S.SCORE_THR))).sum())
    sthr = np.float32(S.SCORE_THR)
    sc = pop['scores'].copy()
    sc[3], sc[4], sc[5] = sthr, np.nextafter(sthr, np.float32(0)), np.nextafter(sthr, np.float32(1))
    want, _ = against_own_matrix(dev, 'a score at the threshold', dict(pop, scores=sc), topk=40, iou_thr=2.0)
    assert 3 in want and 5 in want and 4 not in want


def test_degenerate_boxes(dev):
    """zero-volume boxes: the IoU of two of them is 0 / 0 = NaN, which must not suppress; exact duplicates: IoU 1, the highest score
    stays and on a tie the lower row"""
    pop = sized(24, seed=13)
    boxes = pop['boxes'].copy()
    boxes[2, 3:6] = 0
    boxes[9] = boxes[2]                                        # two identical zero-volume boxes
    boxes[11, 5] = 0                                           # a plate inside the population
    boxes[15] = boxes[4]
    boxes[20] = boxes[4]                                       # three copies of one box
    sc = pop['scores'] * np.float32(0.9)                       # (rows 15 and 20 below are the two highest scores, tied)
    sc[[2, 9, 11]] = (0.9, 0.8, 0.7)
    sc[[4, 15, 20]] = (0.6, 0.95, 0.95)
    want, iou = against_own_matrix(dev, 'degenerate', dict(pop, boxes=boxes, scores=sc), topk=24)
    assert np.isnan(iou[9, 2]) and np.isnan(iou[2, 9]) and np.isnan(iou[2, 2]), 'the case holds no NaN pair'
    assert 2 in want and 9 in want, 'a NaN IoU suppressed a row'
    assert 15 in want and 20 not in want and 4 not in want, 'duplicates: the first of the tied rows stays'


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(dev):
    pop = sized(16, seed=14)
    for kw in (dict(n_classes=0), dict(n_classes=4097), dict(topk=0), dict(topk=-3)):
        args = dict(dict(n_classes=5, topk=10), **kw)
        run_filter(dev, pop['boxes'], pop['scores'], pop['labels'], args['n_classes'], topk=args['topk'], expect=-4)
    n = 16385
    run_filter(dev, np.zeros((n, 9), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32), 5, expect=-4)


# ------------------------------------------------------------------------------------------------------------------ the public interface
def test_filter_instances_and_overlaps(dev):
    from embodiedscan_amd import inference
    from embodiedscan_amd.structures import EulerDepthInstance3DBoxes, InstanceData
    pop = S.clustered(S.SEEDS[0])
    boxes = torch.from_numpy(pop['boxes']).to(dev)
    iou = device_iou(dev, pop['boxes'])
    got = EulerDepthInstance3DBoxes.overlaps(EulerDepthInstance3DBoxes(boxes), boxes[:7])
    assert got.shape == (96, 7) and np.array_equal(got.cpu().numpy(), iou[:, :7], equal_nan=True)
    inst = InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(boxes), scores_3d=torch.from_numpy(pop['scores']).to(dev),
                        labels_3d=torch.from_numpy(pop['labels']).long().to(dev))
    for kw in (dict(), dict(topk_per_class=3, n_classes=5), dict(iou_thr=0.4, score_thr=0.3, topk_per_class=2, n_classes=284)):
        out = inference.filter_instances(inst, **kw)
        want = S.greedy(iou, pop['scores'], pop['labels'], kw.get('n_classes', 5), kw.get('iou_thr', S.IOU_THR), kw.get('score_thr', S.SCORE_THR),
                        kw.get('topk_per_class', 10))
        assert out.keep.dtype == torch.int64 and out.keep.cpu().tolist() == want
        assert torch.equal(out.bboxes_3d.tensor, boxes[out.keep]) and torch.equal(out.scores_3d, inst.scores_3d[out.keep])
        assert torch.equal(out.labels_3d, inst.labels_3d[out.keep]) and out.labels_3d.dtype == torch.int64
    empty = InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(boxes[:0]), scores_3d=inst.scores_3d[:0], labels_3d=inst.labels_3d[:0])
    out = inference.filter_instances(empty)
    assert len(out.keep) == 0 and out.bboxes_3d.tensor.shape == (0, 9)
    with pytest.raises(ValueError, match='16384'):
        inference.filter_instances(InstanceData(bboxes_3d=torch.zeros((16385, 9), device=dev), scores_3d=torch.zeros(16385, device=dev),
                                                labels_3d=torch.zeros(16385, dtype=torch.long, device=dev)))
    with pytest.raises(ValueError, match='n_classes'):
        inference.filter_instances(inst, n_classes=5000)
    if dev.type == 'cuda':
        with pytest.raises(ValueError, match='scores on cpu'):
            inference.filter_instances(InstanceData(bboxes_3d=inst.bboxes_3d, scores_3d=inst.scores_3d.cpu(), labels_3d=inst.labels_3d))
