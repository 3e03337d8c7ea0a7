"""Generate tests/golden/ground_metric.npz and tests/golden/occ_metric.npz by running the REFERENCE's own GroundingMetric.ground_eval and
OccupancyMetric.process + compute_metrics (embodiedscan/eval/metrics/grounding_metric.py, occupancy_metric.py).

Needs the reference checkout beside the repository's oracle stubs:   python tools/make_golden_eval_metrics.py [reference root]
TEST INFRASTRUCTURE (mechanism: tools/make_golden_det_metric.py).  Under oracle/_ref_stubs mmengine's BaseMetric is an inert base
class, so `results` and `dataset_meta` are set by hand; EulerInstance3DBoxes.overlaps (pytorch3d, un-vendored) is bound to
oracle.grounding.overlaps; AsciiTable / print_log of the imported modules are replaced by inert stand-ins.

Grounding cases (each a list of samples (boxes, target scores, gt boxes, (view_dep, hard, unique))): `generic` (12 samples, all eight
flag combinations) and one per quirk -- slot10_hit, rank11_miss, few_queries, no_gt, three_gt_last, mid_iou, empty_category,
single_sample.  Occupancy cases (each a list of (pred, gt list, mask or None) on an 8 x 8 x 4 volume with 5 classes): generic,
duplicates, no_mask, all_hidden (the reference divides by zero there: recorded as `raised` with an empty dict), gt_only_pred_only
(with a class in neither), pred_label_ge_C."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLASSES = ['floor', 'wall', 'chair', 'table', 'lamp']
SHAPE = (8, 8, 4)


def _cube(x, y=0.0, z=0.0, s=1.0):
    return [x, y, z, s, s, s, 0.0, 0.0, 0.0]


def _far(n, start=10.0):
    """n unit cubes that overlap nothing near the origin"""
    return [_cube(start + 3.0 * k, 20.0) for k in range(n)]


def _scores(n, best):
    """n distinct scores; `best` lists the indices that take the highest ones, in rank order"""
    s = np.zeros(n, np.float32)
    rest = [i for i in range(n) if i not in best]
    for r, i in enumerate(list(best) + rest):
        s[i] = 0.95 - 0.03 * r
    return s


def ground_cases():
    """-> {name: (samples, iou_thr)}.  Unit cubes shifted by d along x have IoU (1 - d) / (1 + d): 0.1 -> 0.818, 0.4 -> 0.429,
    0.8 -> 0.111."""
    f = lambda rows: np.array(rows, np.float32).reshape(-1, 9)
    out = {}
    g = np.random.default_rng(20251019)
    samples = []
    for s in range(12):
        n_gt = 1 + s % 2
        gt = np.concatenate([np.stack([3.0 * np.arange(n_gt), np.zeros(n_gt), np.zeros(n_gt)], 1), g.uniform(0.6, 1.4, (n_gt, 3)),
                             g.uniform(-3.1, 3.1, (n_gt, 3))], 1).astype(np.float32)
        Q = 14
        boxes = gt[g.integers(0, n_gt, Q)].copy()
        boxes[:, :3] += g.uniform(-0.35, 0.35, (Q, 3)).astype(np.float32) * (1.0 if s % 3 else 2.5)
        boxes[:, 3:6] *= g.uniform(0.6, 1.5, (Q, 3)).astype(np.float32)
        boxes[:, 6:] += g.uniform(-0.3, 0.3, (Q, 3)).astype(np.float32)
        scores = (g.permutation(Q).astype(np.float32) + 1) / np.float32(Q + 1)
        samples.append((boxes, scores, gt, (bool(s & 1), bool(s & 2), bool(s & 4))))
    out['generic'] = (samples, [0.25, 0.5])
    one = f([_cube(0.0)])
    # 12 queries; the only overlapping box has the 10th highest score (the last slot that counts) / the 11th (the first that does not)
    for name, rank in (('slot10_hit', 9), ('rank11_miss', 10)):
        order = list(range(1, 12))
        order.insert(rank, 0)
        out[name] = ([(f([_cube(0.1)] + _far(11)), _scores(12, order), one, (False, False, True))], [0.25, 0.5])
    out['few_queries'] = ([(f([_cube(9.0), _cube(0.1), _cube(6.0)]), _scores(3, [0, 2, 1]), one, (True, False, False))], [0.25, 0.5])
    out['no_gt'] = ([(f([_cube(0.0)] + _far(11)), _scores(12, range(12)), f([]), (False, True, False)),
                     (f([_cube(0.1)] + _far(10)), _scores(11, range(11)), one, (False, True, False))], [0.25, 0.5])
    out['three_gt_last'] = ([(f(_far(12) + [_cube(0.1)]), _scores(13, [12, 0, 1]), f([_cube(40.0), _cube(50.0), _cube(0.0)]),
                              (True, True, True))], [0.25, 0.5])
    out['mid_iou'] = ([(f([_cube(0.4)] + _far(10)), _scores(11, range(11)), one, (False, False, False))], [0.25, 0.5])
    # three view-independent samples: View-Dep is empty (0.0); one of them is hard (a category with one sample: found / (1e-14 + 1))
    trio = [(f([_cube(0.1)] + _far(10)), _scores(11, range(11)), one, (False, False, True)),
            (f([_cube(0.1)] + _far(10)), _scores(11, range(11)), one, (False, True, True)),
            (f([_cube(0.8)] + _far(10)), _scores(11, range(11)), one, (False, False, True))]
    out['empty_category'] = (trio, [0.25, 0.5])
    out['single_sample'] = ([trio[1]], [0.25])
    return out


def occ_cases():
    """-> {name: samples}; a sample is (pred (X,Y,Z) int64, gt list (M,4) int64, mask (X,Y,Z) bool or None)"""
    g = np.random.default_rng(20251020)
    X, Y, Z = SHAPE
    n = X * Y * Z
    C = len(CLASSES) + 1

    def random_sample(with_mask=True, dup=0):
        flat = g.permutation(n)[:90]
        lab = g.integers(1, C, len(flat))
        lst = np.stack([flat // (Y * Z), (flat // Z) % Y, flat % Z, lab], 1)
        if dup:                                             # the first `dup` voxels again, at the end, with another label
            again = lst[:dup].copy()
            again[:, 3] = again[:, 3] % (C - 1) + 1
            lst = np.concatenate([lst, again])
        dense = np.zeros(n, np.int64)
        for x, y, z, c in lst:
            dense[(x * Y + y) * Z + z] = c
        pred = dense.copy()
        noise = g.random(n) < 0.3
        pred[noise] = g.integers(0, C, int(noise.sum()))
        mask = (g.random(SHAPE) < 0.8) if with_mask else None
        return pred.reshape(SHAPE), lst.astype(np.int64), mask
    out = {}
    out['generic'] = [random_sample(), random_sample()]
    out['duplicates'] = [random_sample(dup=20)]
    out['no_mask'] = [random_sample(with_mask=False), random_sample()]
    p, lst, _ = random_sample()
    out['all_hidden'] = [(p, lst, np.zeros(SHAPE, bool))]
    # class 1 in the ground truth only, class 2 in the prediction only, class 3 in both, classes 4 and 5 in neither (dropped)
    lst = np.array([[0, 0, 0, 1], [0, 0, 1, 1], [1, 0, 0, 3], [1, 1, 0, 3], [1, 2, 0, 3]], np.int64)
    pred = np.zeros(SHAPE, np.int64)
    pred[2, 0, 0] = pred[2, 1, 0] = 2
    pred[1, 0, 0] = pred[1, 1, 0] = pred[3, 3, 3] = 3
    out['gt_only_pred_only'] = [(pred, lst, None)]
    # labels >= C that are not 255: they count in the geometry row only, in the prediction and in the ground truth alike
    p, lst, m = random_sample()
    p = p.copy()
    p.reshape(-1)[::7] = 9
    p.reshape(-1)[3::11] = 255
    lst = lst.copy()
    lst[::9, 3] = 7
    out['pred_label_ge_C'] = [(p, lst, m)]
    return out


class _Table:
    def __init__(self, data):
        self.table = ''


def run_ground(samples, iou_thr):
    from oracle import grounding as OG
    import embodiedscan.eval.metrics.grounding_metric as GM
    import embodiedscan.structures.bbox_3d.euler_box3d as EB
    from embodiedscan.structures import EulerDepthInstance3DBoxes

    def overlaps(cls, boxes1, boxes2, mode='iou', eps=1e-4):
        return OG.overlaps(boxes1.tensor, boxes2.tensor)
    EB.EulerInstance3DBoxes.overlaps = classmethod(overlaps)
    GM.AsciiTable = _Table
    GM.print_log = lambda *a, **k: None
    metric = GM.GroundingMetric(iou_thr=iou_thr)
    box = lambda b: EulerDepthInstance3DBoxes(torch.from_numpy(np.asarray(b, np.float32).reshape(-1, 9)))
    gt = [dict(gt_bboxes_3d=box(s[2]), is_view_dep=s[3][0], is_hard=s[3][1], is_unique=s[3][2]) for s in samples]
    det = [dict(bboxes_3d=box(s[0]), target_scores_3d=torch.from_numpy(np.asarray(s[1], np.float32))) for s in samples]
    return metric.ground_eval(gt, det)


def run_occ(samples):
    import embodiedscan.eval.metrics.occupancy_metric as OM
    OM.AsciiTable = _Table
    OM.print_log = lambda *a, **k: None
    metric = OM.OccupancyMetric()
    metric.results = []
    metric.dataset_meta = dict(classes=CLASSES)
    batch = []
    for pred, lst, mask in samples:
        d = dict(pred_occupancy=torch.from_numpy(np.asarray(pred, np.int64)), gt_occupancy=torch.from_numpy(np.asarray(lst, np.int64)))
        if mask is not None:
            d['gt_occupancy_masks'] = torch.from_numpy(np.asarray(mask, bool))
        batch.append(d)
    metric.process({}, batch)
    try:
        with np.errstate(all='ignore'):
            return metric.compute_metrics(metric.results), 0
    except ZeroDivisionError:                               # no class kept: `sum(res) / len(res)` of the mean's table row
        return {}, 1


def main(reference_root=None, out_dir=None):
    """Two npz files of f64 / int64 tables with the case index in column 0 (the f32 inputs are exact in f64).
    ground_metric.npz: samples (case, sample, view_dep, hard, unique), boxes (case, sample, target score, 9 box), gt (case, sample, 9
    box), thr (case, threshold), keys beside vals (case, value).
    occ_metric.npz: dims (case, sample, X, Y, Z, has_mask), pred / mask: the samples' volumes flattened one after the other in the
    order of dims (mask: ones where a sample has none), gt_list (case, sample, x, y, z, label), keys beside vals (case, value), raised
    (per case: 1 where the reference divided by zero)."""
    from oracle import _ref_stubs
    _ref_stubs.install(*([reference_root] if reference_root else []))
    out_dir = out_dir or os.path.join(ROOT, 'tests', 'golden')
    rows, boxes, gt, thrs, keys, vals = [], [], [], [], [], []
    for k, (name, (samples, thr)) in enumerate(ground_cases().items()):
        ret = run_ground(samples, thr)
        for s, (b, sc, g, fl) in enumerate(samples):
            rows.append([k, s, *[int(v) for v in fl]])
            boxes += [[k, s, np.float32(sc[i]), *np.asarray(b, np.float32)[i]] for i in range(len(sc))]
            gt += [[k, s, *np.asarray(g, np.float32)[j]] for j in range(len(g))]
        thrs += [[k, t] for t in thr]
        keys += list(ret)
        vals += [[k, ret[key]] for key in ret]
        print(name, ret)
    path = os.path.join(out_dir, 'ground_metric.npz')
    np.savez_compressed(path, names=np.array(list(ground_cases())), samples=np.array(rows, np.int64), boxes=np.array(boxes, np.float64),
                        gt=np.array(gt, np.float64), thr=np.array(thrs, np.float64), keys=np.array(keys), vals=np.array(vals, np.float64))
    print('wrote', path, os.path.getsize(path), 'bytes')
    dims, pred, mask, lists, keys, vals, raised = [], [], [], [], [], [], []
    for k, (name, samples) in enumerate(occ_cases().items()):
        ret, rz = run_occ(samples)
        raised.append(rz)
        for s, (p, lst, m) in enumerate(samples):
            dims.append([k, s, *np.asarray(p).shape, int(m is not None)])
            pred.append(np.asarray(p, np.int64).reshape(-1))
            mask.append(np.asarray(m, np.uint8).reshape(-1) if m is not None else np.ones(np.asarray(p).size, np.uint8))
            lists += [[k, s, *row] for row in np.asarray(lst, np.int64).tolist()]
        keys += list(ret)
        vals += [[k, float(ret[key])] for key in ret]
        print(name, 'raised' if rz else {key: round(float(v), 4) for key, v in ret.items()})
    path = os.path.join(out_dir, 'occ_metric.npz')
    np.savez_compressed(path, names=np.array(list(occ_cases())), classes=np.array(CLASSES), dims=np.array(dims, np.int64),
                        pred=np.concatenate(pred), mask=np.concatenate(mask), gt_list=np.array(lists, np.int64), keys=np.array(keys),
                        vals=np.array(vals, np.float64).reshape(-1, 2), raised=np.array(raised, np.int64))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(*sys.argv[1:2])
