"""Generate tests/golden/det_metric.npz by running the REFERENCE's own indoor_eval / eval_map_recall (embodiedscan/eval/indoor_eval.py).

Needs the reference checkout beside the repository's oracle stubs:   python tools/make_golden_det_metric.py [reference root]
TEST INFRASTRUCTURE (mechanism: oracle/make_golden_ground.py).  EulerInstance3DBoxes.overlaps (pytorch3d, un-vendored) is bound to
oracle.grounding.overlaps; AsciiTable / print_log of the imported module are replaced by inert stand-ins (the tables of
classes_split are recorded from the stand-in: the reference only prints them).  eval_map_recall is wrapped to record the per-class
recall / precision arrays it returns.

Cases (each a list of scenes): `generic` (3 scenes, 5 classes, jittered copies of the ground truth) and one per quirk of the
evaluator -- pred_only, gt_only, pred_in_scene_without_gt, three_on_one, mid_iou, thin_clamp, identical_gt, classes_split."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLASSES = ['chair', 'table', 'lamp', 'sofa', 'shelf']


def _box(c, s, r=(0.0, 0.0, 0.0)):
    return [*c, *s, *r]


def cases():
    """-> {name: (scenes, iou_thr, classes_split)}; scene = (pred boxes, scores, labels, gt boxes, gt labels)"""
    f = lambda rows: np.array(rows, np.float32).reshape(-1, 9)
    out = {}
    g = np.random.default_rng(20251018)
    scenes = []
    for s in range(3):
        n_gt = 6 + s
        gb = np.concatenate([g.uniform(-3, 3, (n_gt, 3)), g.uniform(0.4, 1.5, (n_gt, 3)), g.uniform(-3.1, 3.1, (n_gt, 3))], 1).astype(np.float32)
        gl = g.integers(0, 5, n_gt)
        src = g.integers(0, n_gt, 14)
        pb = gb[src].copy()
        pb[:, :3] += g.normal(0, 0.12, (14, 3)).astype(np.float32)
        pb[:, 3:6] *= g.uniform(0.8, 1.25, (14, 3)).astype(np.float32)
        pb[:, 6:] += g.normal(0, 0.15, (14, 3)).astype(np.float32)
        pl = np.where(g.random(14) < 0.8, gl[src], g.integers(0, 5, 14))
        scenes.append((pb, g.permutation(14 * 3)[:14].astype(np.float32) / 50 + s * 0.003, pl, gb, gl))
    out['generic'] = (scenes, [0.25, 0.5], None)
    out['classes_split'] = (scenes[:2], [0.25, 0.5], ([0, 3], [1], [2, 4]))
    unit = (1.0, 1.0, 1.0)
    # class 3 has predictions and no ground truth anywhere: NaN in the reference, dropped
    out['pred_only'] = ([(f([_box((0, 0, 0), unit), _box((5, 0, 0), unit)]), [0.9, 0.8], [0, 3], f([_box((0.1, 0, 0), unit)]), [0])], [0.25, 0.5], None)
    # class 2 has ground truth and no prediction: AP 0, recall 0 (and the mean turns f64)
    out['gt_only'] = ([(f([_box((0, 0, 0), unit)]), [0.9], [0], f([_box((0.1, 0, 0), unit), _box((4, 0, 0), unit)]), [0, 2])], [0.25, 0.5], None)
    # class 1: ground truth in scene 0 only, predictions in both scenes (scene 1's have nothing to look at: -inf)
    out['pred_in_scene_without_gt'] = ([(f([_box((0, 0, 0), unit)]), [0.5], [1], f([_box((0.05, 0, 0), unit)]), [1]),
                                        (f([_box((0, 0, 0), unit), _box((2, 0, 0), unit)]), [0.9, 0.7], [1, 1], f([_box((0, 0, 0), unit)]), [0])],
                                       [0.25, 0.5], None)
    # three detections on one box: the highest score takes it, the others are false positives
    out['three_on_one'] = ([(f([_box((0.1, 0, 0), unit), _box((0, 0.05, 0), unit), _box((0, 0, 0.2), unit), _box((3, 0, 0), unit)]),
                             [0.6, 0.9, 0.3, 0.5], [0, 0, 0, 0], f([_box((0, 0, 0), unit), _box((3.1, 0, 0), unit)]), [0, 0])], [0.25, 0.5], None)
    # best IoU 0.6 / 1.4 = 0.43: a true positive at 0.25, a false positive at 0.5
    out['mid_iou'] = ([(f([_box((0.4, 0, 0), unit, (0, 0, 0))]), [0.9], [0], f([_box((0, 0, 0), unit)]), [0])], [0.25, 0.5], None)
    # a 1 x 1 x 1e-4 prediction on a 1 x 1 x 0.02 slab: IoU 0.005 as given, 1.0 after the clamp to 2e-2; the second prediction's
    # faces are all >= 2e-4 (0.05 x 0.05 x 0.004 has one of 2e-4: not below) so it is NOT clamped
    out['thin_clamp'] = ([(f([_box((0, 0, 0), (1, 1, 1e-4)), _box((3, 0, 0), (0.05, 0.05, 0.004))]), [0.9, 0.8], [0, 0],
                           f([_box((0, 0, 0), (1, 1, 0.02)), _box((3, 0, 0), (0.05, 0.05, 0.02))]), [0, 0])], [0.25, 0.5], None)
    # two identical boxes: both predictions pick the first, so the second prediction is a false positive and recall stays 1/2
    out['identical_gt'] = ([(f([_box((0.05, 0, 0), unit), _box((0, 0.05, 0), unit)]), [0.9, 0.8], [0, 0],
                             f([_box((0, 0, 0), unit), _box((0, 0, 0), unit)]), [0, 0])], [0.25, 0.5], None)
    return out


class _Table:
    made = []

    def __init__(self, data):
        self.table = ''
        _Table.made.append(data)


def run_reference(scenes, iou_thr, classes_split):
    from oracle import grounding as OG
    import embodiedscan.eval.indoor_eval as IE
    import embodiedscan.structures.bbox_3d.euler_box3d as EB
    from embodiedscan.structures import EulerDepthInstance3DBoxes
    from embodiedscan.structures.bbox_3d.box_3d_mode import Box3DMode

    def overlaps(cls, boxes1, boxes2, mode='iou', eps=1e-4):
        return OG.overlaps(boxes1.tensor, boxes2.tensor)
    EB.EulerInstance3DBoxes.overlaps = classmethod(overlaps)
    IE.AsciiTable = _Table
    IE.print_log = lambda *a, **k: None
    curves = {}
    if not hasattr(IE, '_plain_eval_map_recall'):
        IE._plain_eval_map_recall = IE.eval_map_recall

    def recording(pred, gt, ovthresh=None):
        rec, prec, ap = IE._plain_eval_map_recall(pred, gt, ovthresh)
        curves['rec'], curves['prec'], curves['ap'] = rec, prec, ap
        return rec, prec, ap
    IE.eval_map_recall = recording
    _Table.made.clear()
    gt_annos = [dict(gt_bboxes_3d=EulerDepthInstance3DBoxes(torch.from_numpy(np.array(s[3], np.float32))), gt_labels_3d=np.asarray(s[4], np.int64))
                for s in scenes]
    dt_annos = [dict(bboxes_3d=EulerDepthInstance3DBoxes(torch.from_numpy(np.array(s[0], np.float32))),
                     scores_3d=torch.tensor(np.asarray(s[1], np.float32)), labels_3d=torch.tensor(np.asarray(s[2], np.int64))) for s in scenes]
    with np.errstate(all='ignore'):
        ret = IE.indoor_eval(gt_annos, dt_annos, iou_thr, CLASSES, box_mode_3d=Box3DMode.EULER_DEPTH, classes_split=classes_split)
    return ret, curves, [t for t in _Table.made]


def main(reference_root=None, out_dir=None):
    """One npz for all cases (few entries: every zip member costs more than these arrays): f64 tables with the case index in
    column 0 -- pred (case, scene, label, score, 9 box), gt (case, scene, label, 9 box), curves (case, threshold index, label,
    recall, precision) row by row in rank order, vals (case, value) beside keys; the f32 inputs are exact in f64."""
    from oracle import _ref_stubs
    _ref_stubs.install(*([reference_root] if reference_root else []))
    out_dir = out_dir or os.path.join(ROOT, 'tests', 'golden')
    pred, gt, curves, keys, vals, thrs, splits, tables = [], [], [], [], [], [], [], []
    for k, (name, (scenes, thr, split)) in enumerate(cases().items()):
        ret, cur, tabs = run_reference(scenes, thr, split)
        for s, (pb, ps, pl, gb, gl) in enumerate(scenes):
            pred += [[k, s, pl[i], np.float32(ps[i]), *np.asarray(pb, np.float32)[i]] for i in range(len(pl))]
            gt += [[k, s, gl[i], *np.asarray(gb, np.float32)[i]] for i in range(len(gl))]
        for t in range(len(thr)):
            thrs.append([k, thr[t]])
            for lab in cur['rec'][t]:
                curves += [[k, t, int(lab), r, p] for r, p in zip(cur['rec'][t][lab], cur['prec'][t][lab])]
        keys += list(ret)
        vals += [[k, ret[key]] for key in ret]
        if split is not None:
            splits += [[k, j, lab] for j in range(3) for lab in split[j]]
            tables += [[str(k)] + [str(v) for v in row] for tab in tabs[1:] for row in (tab[0], tab[-1])]
        print(name, {key: round(v, 4) for key, v in ret.items() if key.startswith('m')})
    path = os.path.join(out_dir, 'det_metric.npz')
    np.savez_compressed(path, classes=np.array(CLASSES), names=np.array(list(cases())), pred=np.array(pred, np.float64),
                        gt=np.array(gt, np.float64), curves=np.array(curves, np.float64), keys=np.array(keys), vals=np.array(vals, np.float64),
                        thr=np.array(thrs, np.float64), splits=np.array(splits, np.int64), split_tables=np.array(tables))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(*sys.argv[1:2])
