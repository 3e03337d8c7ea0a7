"""Indoor 3-D detection evaluation (9-DoF AP / AR) on the device: embodiedscan/eval/indoor_eval.py:8-377.

The reference walks class x scene x prediction in Python and runs a CPU IoU on every (prediction, ground truth) pair of a scene
and class.  Here the predictions never leave the device: three entry points of csrc/ground.hip do the work,

  es_det_best_gt   best ground-truth box of every prediction inside its (scene, class) group (rules 1, 2 below),
  es_det_mark      true-positive flags per IoU threshold from one integer atomicMin per (threshold, prediction) (rule 4),
  es_det_ap        cumulative TP / FP, precision envelope and its area per (class, threshold) (rule 5),

with es_sort_u64 for the ranking (rule 3) and torch index arithmetic for the grouping.  One device-to-host copy at the end
carries (T, C) APs and TP totals.

Semantics (eval_det_cls / eval_map_recall / indoor_eval of the reference):
 1. a prediction with one of dx*dy, dx*dz, dz*dy (f32 products) below 2e-4 has its three sizes clamped to >= 2e-2 before the IoU;
    ground-truth boxes are never clamped;
 2. a prediction of class c in scene s looks at the ground-truth boxes of class c in s in the scene's order: none -> iou_max =
    -inf (a false positive at every threshold); otherwise the f64 polyhedral IoU rounded to f32, the FIRST index attaining the
    maximum wins;
 3. within a class the predictions are ranked by descending score.  TIES: the reference leaves them to numpy's unstable argsort;
    this project defines them -- equal scores rank by (scene index, position in the scene's prediction list), and -0.0 ties
    with +0.0;
 4. at threshold t a prediction is a true positive iff iou_max > t (f32 compare) and it has the lowest rank among the predictions
    with iou_max > t that point at the same ground-truth box (= the reference's walk down the ranks with a `claimed` flag);
 5. recall = cumsum(tp) / npos, precision = cumsum(tp) / max(cumsum(tp) + cumsum(fp), eps); AP = area under the right-to-left
    monotone envelope of precision over the distinct recalls (0 prepended, (1, 0) appended), summed in f64, stored as f32;
 6. a class with ground truth but no prediction has AP 0 and recall 0; a class with predictions but no ground truth (NaN in the
    reference) is dropped from every output;
 7. keys: `{class}_AP_{t:.2f}`, `mAP_{t:.2f}`, `{class}_rec_{t:.2f}` (last recall), `mAR_{t:.2f}`; the means run over the kept
    classes in the reference's dictionary order (first appearance scene by scene, predictions before ground truth), mAP in f32 and
    mAR in f64 as numpy forms them there;
 8. with classes_split = (head, common, tail) the per-split means are printed (plain text) and returned beside the dict; a split
    without a kept class is skipped."""
import numpy as np
import torch

SPLITS = ('head', 'common', 'tail')


def _boxes(x):
    t = x.tensor if hasattr(x, 'tensor') else torch.as_tensor(x)
    t = t.to(torch.float32).reshape(-1, t.shape[-1] if t.dim() > 1 else 9)
    if t.shape[1] != 9:
        raise ValueError(f'9-DoF boxes expected, got {tuple(t.shape)}')
    return t


def _vec(x, dtype):
    return torch.as_tensor(x).reshape(-1).to(dtype)


def _pick_device(tensors, device):
    if device is not None:
        return torch.device(device)
    for t in tensors:
        if t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError('the detection metric runs on the GPU (there is no host fall-back): no device available')
    return torch.device('cuda', torch.cuda.current_device())


def flatten_annos(gt_annos, dt_annos, device=None):
    """per-scene lists -> flat device tensors: (pred boxes (P,9), scores (P), labels (P), scene (P)), (gt boxes (G,9), labels (G),
    scene (G)).  The scene's own order is kept inside every scene."""
    assert len(gt_annos) == len(dt_annos)
    pb = [_boxes(d['bboxes_3d']) for d in dt_annos]
    ps = [_vec(d['scores_3d'], torch.float32) for d in dt_annos]
    pl = [_vec(d['labels_3d'], torch.int64) for d in dt_annos]
    gb = [_boxes(g['gt_bboxes_3d']) for g in gt_annos]
    gl = [_vec(g['gt_labels_3d'], torch.int64) for g in gt_annos]
    dev = _pick_device(pb, device)
    for s, (b, sc, lb, g, glb) in enumerate(zip(pb, ps, pl, gb, gl)):
        if not (b.shape[0] == sc.shape[0] == lb.shape[0]) or g.shape[0] != glb.shape[0]:
            raise ValueError(f'scene {s}: boxes, scores and labels disagree in length')

    def cat(parts, dtype, tail=()):
        parts = [p.to(dev) for p in parts]
        return torch.cat(parts).contiguous() if parts else torch.zeros((0,) + tail, dtype=dtype, device=dev)

    def scene_ids(parts):
        n = torch.tensor([p.shape[0] for p in parts], dtype=torch.int64)
        return torch.repeat_interleave(torch.arange(len(parts), dtype=torch.int64), n).to(dev)
    return (cat(pb, torch.float32, (9,)), cat(ps, torch.float32), cat(pl, torch.int64), scene_ids(pb)), \
           (cat(gb, torch.float32, (9,)), cat(gl, torch.int64), scene_ids(gb))


def score_rank_keys(scores, labels):
    """64-bit keys whose ascending unsigned order is (class ascending, score descending): the high word is the class, the low word
    the complement of the order-preserving integer image of the f32 score (-0.0 mapped onto +0.0)."""
    bits = scores.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    bits = torch.where(bits == 0x80000000, torch.zeros_like(bits), bits)
    up = torch.where((bits & 0x80000000) != 0, ~bits & 0xffffffff, bits | 0x80000000)
    return (labels.to(torch.int64) << 32) | (~up & 0xffffffff)


def evaluate_device(pred, gt, n_classes, iou_thr):
    """The device pipeline on flat tensors (flatten_annos).  -> dict of device tensors:
    iou_max (P) f32, gt_best (P) int32: ORIGINAL ground-truth row (-1: none), order (P) int32: prediction at each rank,
    tp (T,P) u8 by rank, cls_off (C+1), npos (C), ap (T,C) f32, tp_total (T,C) int32."""
    from .. import hip
    from ..hip import P as ptr, call
    pb, ps, pl, pscene = pred
    gb, gl, gscene = gt
    dev, C, T = pb.device, int(n_classes), len(iou_thr)
    n_pred, n_gt = pb.shape[0], gb.shape[0]
    i32 = torch.int32
    for name, lab in (('prediction', pl), ('ground-truth', gl)):
        if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= C):
            raise ValueError(f'{name} label outside 0 .. {C - 1}')
    st = hip.stream()
    # ---- grouping: (scene, class) groups with at least one ground-truth box; rows stably ordered by group
    gkey, gperm = torch.sort(gscene * C + gl, stable=True)
    gsorted = gb[gperm].contiguous()
    grp_keys, counts = torch.unique_consecutive(gkey, return_counts=True)
    n_grp = grp_keys.numel()
    grp_off = torch.zeros(n_grp + 1, dtype=i32, device=dev)
    grp_off[1:] = torch.cumsum(counts, 0)
    if n_grp and n_pred:
        pkey = pscene * C + pl
        pos = torch.searchsorted(grp_keys, pkey)
        hit = (pos < n_grp) & (grp_keys[pos.clamp(max=n_grp - 1)] == pkey)
        pred_grp = torch.where(hit, pos, torch.full_like(pos, -1)).to(i32)
    else:
        pred_grp = torch.full((n_pred,), -1, dtype=i32, device=dev)
    # ---- best ground-truth box of every prediction
    iou_max = torch.empty(n_pred, dtype=torch.float32, device=dev)
    best_sorted = torch.empty(n_pred, dtype=i32, device=dev)
    call('es_det_best_gt', ptr(pb), n_pred, ptr(pred_grp), ptr(gsorted), ptr(grp_off), n_grp, ptr(iou_max), ptr(best_sorted), st)
    # ---- ranking: stable sort of (class, descending score); equal scores keep the (scene, position) order
    order = torch.empty(n_pred, dtype=i32, device=dev)
    if n_pred:
        keys = score_rank_keys(ps, pl)
        src = torch.arange(n_pred, dtype=i32, device=dev)
        nb = int(hip.raw('es_sort_scratch_bytes')(n_pred))
        scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
        out_keys = torch.empty(n_pred, dtype=torch.int64, device=dev)
        call('es_sort_u64', ptr(keys), ptr(src), n_pred, ptr(scratch), nb, ptr(out_keys), ptr(order), st)
    cls_off = torch.zeros(C + 1, dtype=i32, device=dev)
    cls_off[1:] = torch.cumsum(torch.bincount(pl, minlength=C), 0)
    npos = torch.bincount(gl, minlength=C).to(i32)
    # ---- marking and curves
    claim = torch.empty((T, max(n_gt, 1)), dtype=i32, device=dev)
    tp = torch.zeros((T, n_pred), dtype=torch.uint8, device=dev)
    call('es_det_mark', ptr(iou_max), ptr(best_sorted), ptr(order), n_pred, hip.farr(iou_thr), T, n_gt, ptr(claim), ptr(tp), st)
    ap = torch.empty((T, C), dtype=torch.float32, device=dev)
    tp_total = torch.empty((T, C), dtype=i32, device=dev)
    call('es_det_ap', ptr(tp), n_pred, ptr(cls_off), ptr(npos), C, T, ptr(ap), ptr(tp_total), st)
    if n_gt:
        gt_best = torch.where(best_sorted >= 0, gperm[best_sorted.clamp(min=0).long()].to(i32), best_sorted)
    else:
        gt_best = best_sorted
    return dict(iou_max=iou_max, gt_best=gt_best, order=order, tp=tp, cls_off=cls_off, npos=npos, ap=ap, tp_total=tp_total)


def class_order(pred, gt, n_classes):
    """classes in the order the reference's dictionaries meet them: scene by scene, a scene's predictions before its ground truth"""
    (_, _, pl, pscene), (_, gl, gscene) = pred, gt
    big = pl.numel() + gl.numel() + 1
    first = torch.full((n_classes,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=pl.device)
    first.scatter_reduce_(0, pl, (pscene * 2) * big + torch.arange(pl.numel(), device=pl.device), 'amin')
    first.scatter_reduce_(0, gl, (gscene * 2 + 1) * big + torch.arange(gl.numel(), device=gl.device), 'amin')
    return torch.argsort(first, stable=True)


def summarise(ap, tp_total, npos, npred, order, iou_thr, label2cat, classes_split=None):
    """host arrays ap (T,C) f32, tp_total (T,C), npos (C), npred (C), order (C) -> (result dict, split results, table text).
    A class without predictions enters the reference's mean as an f64 zero, every other AP as an f32 array: np.mean over the
    list of them is formed the same way here."""
    kept = [int(c) for c in order if npos[int(c)] > 0]
    ret, rows = {}, [[label2cat[c]] for c in kept] + [['Overall']]
    header = ['classes']
    for i, t in enumerate(iou_thr):
        aps = [np.array([ap[i, c]], dtype=np.float32) if npred[c] > 0 else np.zeros(1) for c in kept]
        recs = [np.float64(tp_total[i, c]) / float(npos[c]) for c in kept]
        for c, a in zip(kept, aps):
            ret[f'{label2cat[c]}_AP_{t:.2f}'] = float(a[0])
        ret[f'mAP_{t:.2f}'] = _mean(aps)
        for c, r in zip(kept, recs):
            ret[f'{label2cat[c]}_rec_{t:.2f}'] = float(r)
        ret[f'mAR_{t:.2f}'] = _mean(recs)
        header += [f'AP_{t:.2f}', f'AR_{t:.2f}']
        for row, a, r in zip(rows, [float(a[0]) for a in aps] + [ret[f'mAP_{t:.2f}']], [float(r) for r in recs] + [ret[f'mAR_{t:.2f}']]):
            row += [f'{a:.4f}', f'{r:.4f}']
    text = _table([header] + rows)
    splits = {}
    if classes_split is not None:
        for name, labels in zip(SPLITS, classes_split):
            mine = [int(c) for c in labels if int(c) in kept]
            if not mine:
                continue
            res = dict(classes=[label2cat[c] for c in mine])
            for i, t in enumerate(iou_thr):
                res[f'AP_{t:.2f}'] = float(np.mean([float(ap[i, c]) for c in mine]))
                res[f'AR_{t:.2f}'] = float(np.mean([np.float64(tp_total[i, c]) / float(npos[c]) for c in mine]))
            splits[name] = res
            text += '\n' + _table([[f'{name}_classes'] + header[1:], ['Overall'] + [f'{res[h]:.4f}' for h in header[1:]]])
    return ret, splits, text


def _mean(values):
    """np.mean as the reference calls it; NaN (its value there, with a warning) when no class is kept"""
    return float(np.mean(values)) if len(values) else float('nan')


def _table(rows):
    width = [max(len(str(r[k])) for r in rows) for k in range(len(rows[0]))]
    return '\n'.join('  '.join(str(v).ljust(w) for v, w in zip(r, width)) for r in rows)


def indoor_eval_full(gt_annos, dt_annos, metric, label2cat, classes_split=None, device=None):
    """-> (result dict, split results, table text, device intermediates)"""
    iou_thr = [float(t) for t in metric]
    pred, gt = flatten_annos(gt_annos, dt_annos, device)
    C = len(label2cat)
    out = evaluate_device(pred, gt, C, iou_thr)
    order = class_order(pred, gt, C)
    ap, tot, npos, off, order = (x.cpu().numpy() for x in (out['ap'], out['tp_total'], out['npos'], out['cls_off'], order))
    ret, splits, text = summarise(ap, tot, npos, np.diff(off), order, iou_thr, label2cat, classes_split)
    return ret, splits, text, out


def indoor_eval(gt_annos, dt_annos, metric, label2cat, logger=None, box_mode_3d=None, classes_split=None, device=None):
    """The reference's indoor_eval (eval/indoor_eval.py:224-377) on the device.

    gt_annos: per scene dict(gt_bboxes_3d, gt_labels_3d); dt_annos: per scene dict(bboxes_3d, scores_3d, labels_3d); boxes are
    EulerDepthInstance3DBoxes or plain (n, 9) tensors (Euler-Depth is the only box mode; box_mode_3d is accepted and unused).
    metric: IoU thresholds; label2cat: class names by label.  Predictions of equal score inside a class rank by (scene index,
    position in the scene's prediction list) -- the reference leaves that order to numpy's unstable argsort.
    Returns the reference's dict; the tables (and the per-split means of classes_split) go to `logger` or to stdout."""
    ret, _, text, _ = indoor_eval_full(gt_annos, dt_annos, metric, label2cat, classes_split, device)
    _log(text, logger)
    return ret


def _log(text, logger):
    if logger is not None and hasattr(logger, 'info'):
        logger.info('\n' + text)
    else:
        print(text)
