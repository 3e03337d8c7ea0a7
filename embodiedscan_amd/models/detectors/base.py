"""What every detector of this package shares with mmengine's BaseModel protocol: parameter arena binding, reference-named
state dicts, train / eval switching, `forward(inputs, data_samples, mode)` dispatch, the eval + tape-off bracket of `predict`, and
`train_step(data, optim_wrapper)`: preprocess -> forward(mode='loss') -> reverse replay of the tape with the data-parallel gradient
buckets -> optimiser update.  A detector states its modules in `_children()`, records gradient parts with `tape_part()` and may
override `_backward_head` (the two-stream replay of the sparse fusion family) and the `_pf_take` / `_pf_done` prefetch hooks."""
import contextlib

import torch
from ... import engine as E
from ... import hip
from ...parallel import BucketedGradReducer, is_dist
from ...params import ParamArena


@contextlib.contextmanager
def predict_guard(det):
    """context: `det` in eval mode + tape off; the `training` flag and engine.TAPE.enabled are restored on exit"""
    was = det.training
    det.train(False)
    try:
        with E.no_tape():
            yield
    finally:
        det.train(was)


class DetectorBase:
    _version = 2

    def _init_base(self, specs, device, seed, data_preprocessor):
        from ...registry import MODELS
        self.device = torch.device(device)
        self.data_preprocessor = MODELS.build(data_preprocessor, device=self.device) if data_preprocessor else None
        self.arena = ParamArena(specs, seed=seed)
        self.training = True
        self._bound = False

    def _children(self):
        """[(module, arena prefix)] -- every module with a bind(arena, prefix)"""
        raise NotImplementedError

    def to(self, device):
        self.device = torch.device(device)
        self.arena.to(self.device)
        if self.data_preprocessor is not None:
            self.data_preprocessor.to(self.device)
        self._bound = False
        return self

    def _bind(self):
        if not self._bound:
            if self.arena.data.device != self.device:
                self.arena.to(self.device)
            E.begin_bind(id(self))               # conv kernels of an earlier bind of this detector are dropped
            try:
                for m, prefix in self._children():
                    m.bind(self.arena, prefix)
            finally:
                E.end_bind()
            self._bound = True

    def __del__(self):
        try:
            E.release(id(self))
        except Exception:
            pass

    def state_dict(self):
        return self.arena.state_dict()

    def load_state_dict(self, sd, strict=False, tap_order=None):
        """reference-named state dict -> arena; returns (missing, unexpected) keys like torch.nn.Module does"""
        res = self.arena.load_state_dict(sd, strict=strict, tap_order=tap_order)
        E.WEIGHT_VERSION[0] += 1                 # bf16 weight copies are stale
        if self._bound:
            for m, _ in self._children():
                if hasattr(m, 'refresh'):
                    m.refresh()                  # (the image backbone re-folds its frozen BatchNorm2d statistics)
        return res

    def train(self, mode=True):
        self.training = mode
        for m, _ in self._children():
            if hasattr(m, 'training'):
                m.training = mode
        return self

    def forward(self, inputs, data_samples=None, mode='tensor', **kwargs):
        hip.refresh_stream()                     # launches follow torch's CURRENT stream of this call
        if mode == 'loss':
            return self.loss(inputs, data_samples, **kwargs)
        elif mode == 'predict':
            return self.predict(inputs, data_samples, **kwargs)
        raise RuntimeError(f'Invalid mode "{mode}". Only supports loss, predict and tensor mode')

    __call__ = forward

    def _predict_guard(self):
        """context: eval mode + tape off"""
        return predict_guard(self)

    # data-parallel gradient buckets (parallel.BucketedGradReducer): name-prefix groups + the implicit last part; a
    # detector's forward records (tape index, part) pairs in `_tape_parts`: when the reverse replay of the tape has passed
    # the index, every gradient of that part is complete and its all-reduce starts under the rest of the backward pass
    _bucket_groups = (('backbone.',), ('backbone_3d.',))
    _tape_parts = ()

    def start_tape_parts(self):
        """called where a loss forward starts recording: forget the parts of the forward before"""
        self._tape_parts = []

    def tape_part(self, part):
        """called in forward: everything recorded on the tape from here on belongs to gradient part `part` (or later ones)"""
        self._tape_parts.append((len(E.TAPE.fns), part))

    def _backward(self, red):
        """Run the tape in reverse.  `red` (data parallel only) all-reduces each part of the gradient arena as soon as it is
        complete: the recorded parts from the back, then `_backward_head` for what lies in front of the first of them."""
        fns = E.TAPE.fns
        hi = len(fns)
        done = set()
        for idx, part in sorted(self._tape_parts, reverse=True):
            for fn in reversed(fns[idx:hi]):
                fn()
            hi = idx
            if red is not None:
                E.join_wgrad_streams(final=False)
                red.launch(part)
                done.add(part)
        self._backward_head(fns[:hi], red, done)
        E.TAPE.clear()

    def _backward_head(self, fns, red, done):
        """the closures in front of the first recorded part, the final join, and every part not in `done`"""
        for fn in reversed(fns):
            fn()
        E.join_wgrad_streams()
        if red is not None:
            for part in range(len(red.parts)):
                if part not in done:
                    red.launch(part)

    # next-batch prefetch hooks of _train_step (the sparse fusion family implements them)
    def _pf_take(self, data):
        """the preprocessed batch prepared ahead if `data` is the object prefetch() returned, else None"""
        return None

    def _pf_done(self):
        """hold the prefetched tensors until the prefetch stream has seen this step's end event"""

    # engine.mark names of a step: they are the keys of `stage_ms` in the benchmark's output
    _stages = ('data (caller)', 'forward + losses', 'backward', 'all-reduce + clip + AdamW')

    def train_step(self, data, optim_wrapper):
        """mmengine BaseModel.train_step: preprocess, loss forward, backward, update."""
        return self._train_step(data, optim_wrapper, lambda inputs, samples: self.forward(inputs, samples, mode='loss'))

    def _train_step(self, data, optim_wrapper, loss_fn):
        """the body of train_step with the loss forward as a callable (inputs, data_samples) -> loss dict (the grounder's
        train_step_shared passes loss_shared)"""
        E.settle_gc(self)                        # (the collector's generations are frozen once the warm-up steps are through)
        E.TAPE.clear()
        hip.refresh_stream()
        E.mark(self._stages[0])                  # whatever the caller queued before train_step (pipeline.make_batch)
        pre = self._pf_take(data)
        if pre is not None:
            data = pre
        elif self.data_preprocessor is not None:
            data = self.data_preprocessor(data, True)
        self._bind()
        self.arena.grad.zero_()
        E.new_grad_epoch()                       # first weight-gradient launch per weight overwrites, later ones add
        losses = loss_fn(data['inputs'], data['data_samples'])
        E.mark(self._stages[1])
        red = None
        if is_dist():
            # bucketed gradient all-reduce overlapped with backward: a part is launched when the tape (run in reverse) has
            # passed its mark
            if getattr(self.arena, 'reducer', None) is None:
                self.arena.reducer = BucketedGradReducer(self.arena, groups=self._bucket_groups)
            red = self.arena.reducer
        self._backward(red)
        E.mark(self._stages[2])
        optim_wrapper.update_params(self.arena)
        E.mark(self._stages[3])
        self._pf_done()
        return losses
