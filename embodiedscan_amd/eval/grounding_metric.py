"""GroundingMetric (embodiedscan/eval/metrics/grounding_metric.py:14-190) on the device.

The reference keeps every sample's 256 boxes on the host and runs a CPU IoU on the ten best of them at the end.  Here `process`
reduces a batch on the device to four bytes and one flag byte per sample,

  es_topk_sorted   the ten highest target scores of every sample, sorted (rule 1),
  es_ground_hits   their IoU with the sample's ground-truth boxes and one hit bit per threshold (rules 2, 3),

and `evaluate` gathers those rows over the ranks and counts them in one launch of es_ground_tally (rule 4); one device-to-host copy
carries the (T, 7, 2) counts.  `process` never synchronises with the device: the host-side facts of a batch (row offsets, lengths
and the three booleans of every sample) go up as one small tensor.

Semantics (ground_eval of the reference):
 1. per sample the 10 highest `target_scores_3d` are taken, all Q of them when Q < 10.  TIES: the reference leaves them to an
    unstable argsort; this project defines them as es_topk_sorted does -- the lower query index first, and -0.0 ties with +0.0;
 2. the IoU of each of those boxes with every box of `eval_ann_info['gt_bboxes_3d']` is the f64 polyhedral IoU rounded to f32.
    There is NO thin-box clamp (the reference calls `overlaps` directly here).  G may be 0, 1 or more;
 3. found[t] = any(iou > t), an f32 compare over the (<= 10) x G matrix; with G = 0 or Q = 0 nothing is found;
 4. every sample counts in Overall and in exactly one type of each pair View-Dep / View-Indep, Hard / Easy, Unique / Multi, by
    `is_view_dep`, `is_hard`, `is_unique` of its eval_ann_info;
 5. value = found_count / max(denominator, 1), the denominator formed as the reference forms it: an f64 that starts at 1e-14 and has
    1.0 added once per sample, one addition after the other, on the host.  A type with one sample scores just under 1, an empty one
    0.0;
 6. keys are f'{type}@{t}' with str(t), types in the order Easy, Hard, View-Dep, View-Indep, Unique, Multi, Overall; one table per
    threshold goes to the log as plain text;
 7. with format_only the 20 boxes and scores of highest `scores_3d` (same tie rule) of every sample are written as lists to
    result_dir/test_results.json and {} is returned."""
import json
import os

import numpy as np
import torch

from ..registry import METRICS
from .indoor_eval import _boxes, _log, _table, _vec
from .protocol import RowMetric, device_of, field, upload

TYPES = ('Easy', 'Hard', 'View-Dep', 'View-Indep', 'Unique', 'Multi', 'Overall')
TOP_K = 10
SAVE_K = 20


def _padded(score_list, dev):
    """(S, L) f32 with every sample's scores in the front of its row, L = the longest (at least 1)"""
    L = max([int(s.shape[0]) for s in score_list] + [1])
    if all(int(s.shape[0]) == L for s in score_list):
        return torch.stack(score_list).contiguous(), L
    vals = torch.zeros((len(score_list), L), dtype=torch.float32, device=dev)
    for i, s in enumerate(score_list):
        vals[i, :s.shape[0]] = s
    return vals, L


def sorted_topk(score_list, vlen, k, dev):
    """es_topk_sorted on ragged scores -> (S, k) int32 rows local to the sample, -1 where the sample has fewer than k"""
    from .. import hip
    from ..hip import P, call
    vals, L = _padded(score_list, dev)
    idx = torch.empty((len(score_list), k), dtype=torch.int32, device=dev)
    call('es_topk_sorted', P(vals), len(score_list), L, P(vlen), k, P(idx), hip.stream())
    return idx


def ground_hits(boxes, scores, gts, iou_thr, flags=None, device=None):
    """One batch on the device.  boxes: per sample (Q,9); scores: per sample (Q) target scores; gts: per sample (G,9); flags: per
    sample bit triple (bit 0 view-dependent, 1 hard, 2 unique) or None.
    -> dict of device tensors idx (S,10) int32, hit (S) int32, iou_top (S,10) f32, flags (S) uint8.  No synchronisation."""
    from .. import hip
    from ..hip import P, call
    S = len(boxes)
    boxes = [_boxes(b) for b in boxes]
    gts = [_boxes(g) for g in gts]
    scores = [_vec(s, torch.float32) for s in scores]
    dev = device_of(boxes + scores, device)
    for s, (b, sc) in enumerate(zip(boxes, scores)):
        if b.shape[0] != sc.shape[0]:
            raise ValueError(f'sample {s}: {b.shape[0]} boxes and {sc.shape[0]} target scores')
    lens = [int(b.shape[0]) for b in boxes]
    box_off = np.concatenate([[0], np.cumsum(lens)]).tolist()
    gt_off = np.concatenate([[0], np.cumsum([int(g.shape[0]) for g in gts])]).tolist()
    meta = upload(torch.tensor(box_off + gt_off + lens + list(flags if flags is not None else [0] * S), dtype=torch.int32), dev)
    box_off_d, gt_off_d, vlen, flags_d = meta[:S + 1], meta[S + 1:2 * S + 2], meta[2 * S + 2:3 * S + 2], meta[3 * S + 2:]
    hit = torch.empty(S, dtype=torch.int32, device=dev)
    iou_top = torch.empty((S, TOP_K), dtype=torch.float32, device=dev)
    if S == 0:
        return dict(idx=torch.empty((0, TOP_K), dtype=torch.int32, device=dev), hit=hit, iou_top=iou_top, flags=flags_d.to(torch.uint8))
    idx = sorted_topk([upload(s, dev) for s in scores], vlen, TOP_K, dev)
    all_boxes = torch.cat([upload(b, dev) for b in boxes]).contiguous()
    if all(not g.is_cuda for g in gts):                  # annotations still on the host: one upload for the batch
        all_gt = upload(torch.cat(gts), dev).contiguous()
    else:
        all_gt = torch.cat([upload(g, dev) for g in gts]).contiguous()
    call('es_ground_hits', P(all_boxes), P(box_off_d), P(idx), S, TOP_K, P(all_gt), P(gt_off_d), hip.farr(iou_thr), len(iou_thr),
         P(hit), P(iou_top), hip.stream())
    return dict(idx=idx, hit=hit, iou_top=iou_top, flags=flags_d.to(torch.uint8))


def ground_tally(hit, flags, T):
    """hit (N) int32, flags (N) uint8 on the device -> counts (T,7,2) int32 [found, samples] on the device"""
    from .. import hip
    from ..hip import P, call
    counts = torch.empty((T, len(TYPES), 2), dtype=torch.int32, device=hit.device)
    call('es_ground_tally', P(hit.contiguous()), P(flags.contiguous()), hit.shape[0], T, P(counts), hip.stream())
    return counts


def denominator(n):
    """rule 5: 1e-14 + 1.0 + 1.0 + ... (n additions, in that order; numpy's accumulate adds one after the other)"""
    return float(np.add.accumulate(np.concatenate([[1e-14], np.ones(int(n))]))[-1])


def ground_dict(counts, iou_thr):
    """host counts (T,7,2) -> (the reference's dict, the tables as text)"""
    ret, text = {}, []
    for t, thr in enumerate(iou_thr):
        row = ['results']
        for k, name in enumerate(TYPES):
            value = int(counts[t, k, 0]) / max(denominator(counts[t, k, 1]), 1)
            ret[name + '@' + str(thr)] = value
            row.append(f'{value:.4f}')
        text.append(_table([['Type'] + list(TYPES), row]))
    return ret, '\n'.join(text)


@METRICS.register_module()
class GroundingMetric(RowMetric):
    """Language grounding metric: the share of samples whose ten best-aligned boxes hold one with IoU above each threshold, overall
    and by Easy / Hard, View-Dep / View-Indep, Unique / Multi.  Between batches a sample is an int32 bit mask over the thresholds
    and a flag byte (with format_only: its 20 best boxes and scores).  Ties between equal scores: rule 1 of the module docstring."""

    def __init__(self, iou_thr=[0.25, 0.5], collect_device='cpu', prefix=None, format_only=False, result_dir='', device=None, **kwargs):
        self.iou_thr = [iou_thr] if isinstance(iou_thr, float) else list(iou_thr)
        self.format_only = format_only
        self.result_dir = result_dir
        self.dataset_meta = kwargs.pop('dataset_meta', None)
        self._setup(collect_device, prefix, device)

    def process(self, data_batch, data_samples):
        preds = [field(s, 'pred_instances_3d') for s in data_samples]
        boxes = [_boxes(field(p, 'bboxes_3d')) for p in preds]
        if self.format_only:
            scores = [_vec(field(p, 'scores_3d'), torch.float32) for p in preds]
            dev = device_of(boxes + scores, self.device)
            if not preds:
                return
            vlen = upload(torch.tensor([int(s.shape[0]) for s in scores], dtype=torch.int32), dev)
            idx = sorted_topk([upload(s, dev) for s in scores], vlen, SAVE_K, dev)
            for i, (b, s) in enumerate(zip(boxes, scores)):
                rows = idx[i, :min(int(s.shape[0]), SAVE_K)].long()
                self.results.append((upload(b, dev)[rows], upload(s, dev)[rows]))
            return
        anns = [field(s, 'eval_ann_info') for s in data_samples]
        flags = [(1 if field(a, 'is_view_dep') else 0) | (2 if field(a, 'is_hard') else 0) | (4 if field(a, 'is_unique') else 0) for a in anns]
        out = ground_hits(boxes, [field(p, 'target_scores_3d') for p in preds], [field(a, 'gt_bboxes_3d') for a in anns],
                          self.iou_thr, flags, self.device)
        for i in range(len(preds)):
            self.results.append((out['hit'][i:i + 1], out['flags'][i:i + 1]))

    def compute_metrics(self, results):
        if self.format_only:
            saved = [dict(bboxes_3d=b.cpu().tolist(), scores_3d=s.cpu().tolist()) for b, s in results]
            if self.result_dir:
                os.makedirs(self.result_dir, exist_ok=True)
            with open(os.path.join(self.result_dir, 'test_results.json'), 'w') as f:
                json.dump(saved, f)
            return {}
        T = len(self.iou_thr)
        if results:
            dev = device_of([r[0] for r in results], self.device)
            counts = ground_tally(torch.cat([r[0].to(dev) for r in results]), torch.cat([r[1].to(dev) for r in results]), T)
            counts = counts.cpu().numpy()
        else:
            counts = np.zeros((T, len(TYPES), 2), np.int32)
        ret, text = ground_dict(counts, self.iou_thr)
        _log(text, None)
        return ret
