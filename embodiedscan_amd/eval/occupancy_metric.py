"""OccupancyMetric (embodiedscan/eval/metrics/occupancy_metric.py:17-178) on the device.

The reference keeps one dense int64 ground-truth volume and one prediction per sample until the end (about 200 KB each for the
40 x 40 x 16 volume) and then walks the classes with masked comparisons on the host.  Here `process` reduces every sample on the
device to its (1, 3C) int32 confusion row,

  es_occ_targets (ratio 1)   the dense ground truth from the (M, 4) list and the visibility mask (rule 1),
  es_occ_confusion           the per-class counts over the voxels that are not ignored (rule 2),

and only that row is stored and gathered.  `evaluate` cuts the gathered rows to `size` BEFORE summing them (in int64), so padded
duplicates of the last batch never count -- what the reference's collect_results achieves -- and makes one device-to-host copy.
`process` never synchronises with the device.

Semantics (process / compute_metrics of the reference):
 1. the dense ground truth comes from the (M, 4) list {x, y, z, label}: the LAST occurrence of a voxel wins (the effect of the
    reference's sequential index_put), voxels outside `gt_occupancy_masks` become 255.  Indices outside the volume are a caller
    error (the reference raises or wraps them); here such rows are dropped, as es_occ_targets drops them;
 2. with C = len(classes) + 1, over the voxels with gt != 255 every class j >= 1 counts [gt == j and pred == j, gt == j, pred == j];
    row 0, the geometry row named `empty`, counts the same with `!= 0` in place of `== j`.  A label >= C that is not 255 counts in
    row 0 only, in gt and in pred alike;
 3. IoU_j = tp / (g + p - tp) in f64.  A class whose union is 0 (NaN in the reference) is left out of the dict.  The mean over the
    kept classes is logged, NOT returned.  Where no class is kept (every voxel ignored, or nothing processed) the reference divides
    by zero; here no mean is logged and {} is returned;
 4. batchwise_anns=True (continuous occupancy) keeps everything gathered instead of cutting to `size`."""
import numpy as np
import torch

from ..registry import METRICS
from .indoor_eval import _log, _table
from .protocol import RowMetric, device_of, field, upload

OCC_MAX_CLASSES = 256          # OCC_MAXC of csrc/occ.hip


def occ_confusion(pred, gt_list, mask, n_rows, device=None, out=None):
    """One sample on the device: pred (X,Y,Z) integer labels, gt_list (M,4) {x, y, z, label}, mask (X,Y,Z) bool or None
    -> (3 * n_rows,) int32 confusion counts (written into `out` when given).  No synchronisation."""
    from .. import hip
    from ..hip import P, call
    dev = device_of([pred], device)
    pred = upload(torch.as_tensor(pred).to(torch.int64), dev).contiguous()
    if pred.dim() != 3:
        raise ValueError(f'a (X, Y, Z) prediction expected, got {tuple(pred.shape)}')
    X, Y, Z = pred.shape
    occ = upload(torch.as_tensor(gt_list).to(torch.int32), dev).reshape(-1, 4).contiguous()
    m = None
    if mask is not None:
        m = upload(torch.as_tensor(mask).to(torch.uint8), dev).contiguous()
        if tuple(m.shape) != (X, Y, Z):
            raise ValueError(f'mask {tuple(m.shape)} does not match the prediction {(X, Y, Z)}')
    n = X * Y * Z
    scratch = torch.empty(n, dtype=torch.int32, device=dev)
    gt = torch.empty(n, dtype=torch.int32, device=dev)
    if out is None:
        out = torch.empty(3 * n_rows, dtype=torch.int32, device=dev)
    st = hip.stream()
    call('es_occ_targets', P(occ), occ.shape[0], 1, X, Y, Z, P(m), P(scratch), P(gt), st)
    call('es_occ_confusion', P(pred), P(gt), n, n_rows, P(out), st)
    return out


def occ_dict(counts, classes):
    """host counts (C,3) -> (the reference's dict, the table as text)"""
    score = np.asarray(counts, np.float64)
    ret, rows = {}, [['classes', 'IoU']]
    with np.errstate(all='ignore'):
        for i in range(len(classes) + 1):
            tp, p, g = score[i]
            value = tp / (p + g - tp)
            if np.isnan(value):                      # empty union: the class is in neither the ground truth nor the predictions
                continue
            name = 'empty' if i == 0 else classes[i - 1]
            ret[name] = float(value)
            rows.append([name, f'{ret[name]:.5f}'])
    if ret:
        vals = list(ret.values())
        rows.append(['mean', f'{sum(vals) / len(vals):.5f}'])
    return ret, _table(rows)


@METRICS.register_module()
class OccupancyMetric(RowMetric):
    """Occupancy metric: the IoU of every class, and of the geometry (`empty`: occupied against free), over the visible voxels.
    dataset_meta: dict(classes=[...]) -- needed by `process`, which reduces every sample to its (1, 3 * (len(classes) + 1)) int32
    confusion row.  batchwise_anns: the samples of a batch carry their own annotations (continuous occupancy), so `evaluate` keeps
    everything gathered instead of cutting to the dataset length."""

    def __init__(self, collect_device='cpu', prefix=None, batchwise_anns=False, device=None, **kwargs):
        self.batchwise_anns = batchwise_anns
        self.dataset_meta = kwargs.pop('dataset_meta', None)
        self._setup(collect_device, prefix, device)

    def _classes(self):
        meta = self.dataset_meta
        if not meta or 'classes' not in meta:
            raise RuntimeError('OccupancyMetric: set dataset_meta = dict(classes=[...]) before process(): a sample is reduced to its '
                               'per-class counts as it is processed')
        if len(meta['classes']) + 1 > OCC_MAX_CLASSES:
            raise ValueError(f'OccupancyMetric: at most {OCC_MAX_CLASSES - 1} classes')
        return list(meta['classes'])

    def process(self, data_batch, data_samples):
        C = len(self._classes()) + 1
        if not data_samples:
            return
        dev = device_of([field(s, 'pred_occupancy') for s in data_samples], self.device)
        rows = torch.empty((len(data_samples), 3 * C), dtype=torch.int32, device=dev)
        for i, s in enumerate(data_samples):
            occ_confusion(field(s, 'pred_occupancy'), field(s, 'gt_occupancy'), field(s, 'gt_occupancy_masks'), C, dev, rows[i])
            self.results.append((rows[i:i + 1],))

    def compute_metrics(self, results):
        classes = self._classes()
        C = len(classes) + 1
        if results:
            total = torch.cat([r[0] for r in results]).to(torch.int64).sum(0).cpu().numpy().reshape(C, 3)
        else:
            total = np.zeros((C, 3), np.int64)
        ret, text = occ_dict(total, classes)
        _log(text, None)
        return ret
