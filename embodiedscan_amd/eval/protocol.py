"""What GroundingMetric and OccupancyMetric share with IndoorDetMetric's protocol (mmengine's BaseMetric): `evaluate(size)` gathers
the per-sample rows over the ranks, cuts them to `size`, computes on rank 0, broadcasts the dict, clears `results`; `prefix` is
applied to the keys."""
import torch


def field(obj, key):
    if isinstance(obj, dict):
        return obj.get(key)
    return getattr(obj, key, None)


def device_of(tensors, device=None):
    """the device the kernels run on: `device`, else the first device tensor's, else the current GPU (there is no host fall-back)"""
    if device is not None:
        return torch.device(device)
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError('the metric runs on the GPU (there is no host fall-back): no device available')
    return torch.device('cuda', torch.cuda.current_device())


def upload(t, dev):
    """`t` on `dev` without synchronising the stream: a host tensor goes through pinned memory and an asynchronous copy (a plain
    `.to(device)` of pageable memory waits for everything queued before it)"""
    if t.device == dev:
        return t
    if dev.type == 'cuda' and not t.is_cuda and t.numel():
        return t.pin_memory().to(dev, non_blocking=True)
    return t.to(dev)


class RowMetric:
    """`results` holds one tuple of small tensors per sample (dim 0 free, as gather_results wants them)"""
    default_prefix = None
    batchwise_anns = False

    def _setup(self, collect_device, prefix, device):
        self.collect_device = collect_device
        self.prefix = prefix or self.default_prefix
        self.device = device
        self.results = []

    def evaluate(self, size):
        import torch.distributed as dist
        from .det_metric import gather_results
        cut = None if self.batchwise_anns else size
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            results = gather_results(self.results, cut)
            box = [self._prefixed(self.compute_metrics(results)) if dist.get_rank() == 0 else None]
            dist.broadcast_object_list(box, 0)
            metrics = box[0]
        else:
            metrics = self._prefixed(self.compute_metrics(self.results if cut is None else self.results[:cut]))
        self.results.clear()
        return metrics

    def _prefixed(self, metrics):
        return {'/'.join((self.prefix, k)): v for k, v in metrics.items()} if self.prefix else metrics
