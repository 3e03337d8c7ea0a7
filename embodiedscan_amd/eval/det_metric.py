"""IndoorDetMetric (embodiedscan/eval/metrics/det_metric.py:20-162) with the predictions kept on the device between batches.

`process` appends device tensors and never synchronises; `evaluate` gathers over the ranks (when torch.distributed runs with
more than one), computes on rank 0 through eval/indoor_eval.py and broadcasts the dict -- the protocol of mmengine's BaseMetric."""
from itertools import zip_longest

import torch

from ..registry import METRICS
from .indoor_eval import _boxes, _log, _vec, indoor_eval_full


def gather_results(results, size=None, group=None):
    """All-gather of ragged results.  results: this rank's list of tuples of tensors -- the same arity, dtypes and trailing shapes
    on every rank, dim 0 free.  Returns, on EVERY rank, the results of all ranks interleaved rank by rank (rank 0's first, rank 1's
    first, ..., rank 0's second, ...; a rank that has run out is passed over) and cut to `size` (None: everything gathered) --
    what mmengine's collect_results does with the padded samples of the last batch.
    Variable lengths travel as one size exchange (all_gather_object of a few integers) and one padded all_gather per slot."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    nccl = dist.get_backend(group) == 'nccl'
    dev = torch.device('cuda', torch.cuda.current_device()) if nccl else torch.device('cpu')
    n_local = len(results)
    arity = len(results[0]) if n_local else 0
    meta = dict(n=n_local, arity=arity, tot=[sum(r[k].shape[0] for r in results) for k in range(arity)],
                dtype=[results[0][k].dtype for k in range(arity)], tail=[tuple(results[0][k].shape[1:]) for k in range(arity)])
    metas = [None] * world
    dist.all_gather_object(metas, meta, group=group)
    full = next((m for m in metas if m['n']), None)
    if full is None:
        return []
    arity = full['arity']
    n_max = max(m['n'] for m in metas)
    lens = torch.zeros((n_max, arity), dtype=torch.int64, device=dev)
    if n_local:
        lens[:n_local] = torch.tensor([[r[k].shape[0] for k in range(arity)] for r in results], dtype=torch.int64)
    all_lens = [torch.zeros_like(lens) for _ in range(world)]
    dist.all_gather(all_lens, lens, group=group)
    parts = [[[] for _ in range(m['n'])] for m in metas]
    for k in range(arity):
        tot_max = max(m['tot'][k] if m['n'] else 0 for m in metas)
        buf = torch.zeros((tot_max,) + full['tail'][k], dtype=full['dtype'][k], device=dev)
        if n_local and meta['tot'][k]:
            buf[:meta['tot'][k]] = torch.cat([r[k].to(dev) for r in results])
        bufs = [torch.zeros_like(buf) for _ in range(world)]
        dist.all_gather(bufs, buf, group=group)
        for r, m in enumerate(metas):
            pieces = torch.split(bufs[r][:m['tot'][k]] if m['n'] else bufs[r][:0], all_lens[r][:m['n'], k].tolist())
            for i, piece in enumerate(pieces):
                parts[r][i].append(piece)
    ordered = [tuple(x) for row in zip_longest(*parts) for x in row if x is not None]
    return ordered if size is None else ordered[:size]


@METRICS.register_module()
class IndoorDetMetric:
    """Indoor 3-D detection metric: per-class and mean AP / AR of 9-DoF boxes at the IoU thresholds `iou_thr`.

    dataset_meta: dict(classes=[...], classes_split=(head, common, tail) label lists (optional), box_type_3d (optional)).
    batchwise_anns: the samples of a batch carry their own annotations (continuous detection), so `evaluate` keeps everything
    gathered instead of cutting to the dataset length.  Ties between equal scores: see eval/indoor_eval.py rule 3."""
    default_prefix = None

    def __init__(self, iou_thr=[0.25, 0.5], collect_device='cpu', prefix=None, batchwise_anns=False, device=None, **kwargs):
        self.iou_thr = [iou_thr] if isinstance(iou_thr, float) else list(iou_thr)
        self.collect_device = collect_device
        self.prefix = prefix or self.default_prefix
        self.batchwise_anns = batchwise_anns
        self.device = device
        self.dataset_meta = kwargs.pop('dataset_meta', None)
        self.results = []
        self.split_results = {}

    @staticmethod
    def _field(obj, key):
        if isinstance(obj, dict):
            return obj.get(key)
        return getattr(obj, key, None)

    def process(self, data_batch, data_samples):
        """keeps (gt boxes, gt labels, boxes, scores, labels) of every sample as tensors where they are: no copy to the host, no
        synchronisation"""
        for sample in data_samples:
            pred = self._field(sample, 'pred_instances_3d')
            ann = self._field(sample, 'eval_ann_info')
            if ann is not None:
                gb, gl = self._field(ann, 'gt_bboxes_3d'), self._field(ann, 'gt_labels_3d')
            else:
                gt = self._field(sample, 'gt_instances_3d')
                gb, gl = self._field(gt, 'bboxes_3d'), self._field(gt, 'labels_3d')
            self.results.append((_boxes(gb), _vec(gl, torch.int64), _boxes(self._field(pred, 'bboxes_3d')),
                                 _vec(self._field(pred, 'scores_3d'), torch.float32), _vec(self._field(pred, 'labels_3d'), torch.int64)))

    def compute_metrics(self, results):
        meta = self.dataset_meta or {}
        gt_annos = [dict(gt_bboxes_3d=r[0], gt_labels_3d=r[1]) for r in results]
        dt_annos = [dict(bboxes_3d=r[2], scores_3d=r[3], labels_3d=r[4]) for r in results]
        ret, self.split_results, text, _ = indoor_eval_full(gt_annos, dt_annos, self.iou_thr, meta['classes'],
                                                            meta.get('classes_split'), self.device)
        _log(text, None)
        return ret

    def evaluate(self, size):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            results = gather_results(self.results, None if self.batchwise_anns else size)
            box = [self._prefixed(self.compute_metrics(results)) if dist.get_rank() == 0 else None]
            dist.broadcast_object_list(box, 0)
            metrics = box[0]
        else:
            results = self.results if self.batchwise_anns else self.results[:size]
            metrics = self._prefixed(self.compute_metrics(results))
        self.results.clear()
        return metrics

    def _prefixed(self, metrics):
        return {'/'.join((self.prefix, k)): v for k, v in metrics.items()} if self.prefix else metrics
