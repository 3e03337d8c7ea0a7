"""Operator layer of the MI355X path: thin Python drivers around the C-ABI kernels plus a
minimal reverse-mode tape (HIP launches in, HIP launches out -- no torch.autograd, no CPU path).

torch is used for device memory (caching allocator) and the current HIP stream only.
Every forward function registers one closure on the tape; `TAPE.backward()` replays them in
reverse.  Gradients w.r.t. parameters accumulate straight into the flat gradient arena.
"""
import os
from collections import namedtuple

import torch
from . import hip
from .hip import P, call, iarr

_C = hip.CONSTS             # the flag values of the C ABI by their names (include/es_hip.h)


def _stream():
    return hip.stream()


def _switch(env):
    """an A/B switch as a one-element list (tests and tools set X[0]): on unless the environment says ES_X=0"""
    return [os.environ.get(env, '1') != '0']


def instrumented(fwd=True):
    """Per-launch instrumentation is on: a profile (hip.PROFILE), a record hook of BACKWARD launches (DEBUG_CONV / DEBUG_GRADS / DEBUG_OPS) or,
    with fwd, the hook of forward launches (DEBUG_FWD).  graphed() asks with DEBUG_FWD: a replayed forward would record nothing;
    _f32_grad_rows_wanted() without: a forward record reads no gradient rows, so it has no say in how they are stored."""
    return (hip.PROFILE is not None or DEBUG_CONV is not None or DEBUG_GRADS is not None or DEBUG_OPS is not None
            or (fwd and DEBUG_FWD is not None))


_NEW_VARS = None            # list while graphed() captures a segment


class Var:
    """A row matrix (N, C) f32 on the device with an optional gradient (and lazily made bf16 shadows of both, the
    gather sources of the bf16 convolution kernels)."""
    __slots__ = ('d', 'g', 'rg', 'dh', 'gh', 'gate', 'gated', 'fresh', 'gsh', 'fold')

    def __init__(self, d, rg=True):
        self.d, self.g, self.rg = d, None, rg
        self.dh = self.gh = None
        if _NEW_VARS is not None:
            _NEW_VARS.append(self)     # a segment is being captured: its Vars are reset before every replay (graphed())
        self.fresh = False      # True between conv() and the norm() that consumes its output (nobody else sees this Var)
        self.gate = None        # folded-BN scale of the fused conv+BN+ReLU that produced this Var (see conv_affine)
        self.gated = False      # True: .g already is the gradient w.r.t. the producer's (pre-BN) conv output
        self.gsh = False        # True: the backward of the conv() that produced this Var reads .g through its bf16 shadow alone
        self.fold = None        # folded-BN scale of the conv + BN (no activation) that produced this Var, when that layer's backward can take
                                # the gradient of its conv output as pre-rounded bf16 rows (conv_affine: the downsample of a residual join)

    def shadow(self):
        if self.dh is None:
            self.dh = self.d if self.d.dtype == torch.bfloat16 else _cast_rows(self.d)     # bf16 rows are their own shadow
        return self.dh

    def grad_shadow(self):
        if self.gh is None:
            self.gh = _cast_rows(self.g)
        return self.gh

    @property
    def shape(self):
        return self.d.shape


class Param:
    """View into the parameter / gradient arenas (+ lazily refreshed bf16 copies for the bf16 MFMA path)."""
    __slots__ = ('d', 'g', 'bf_n', 'bf_t', 'bf_step', 'owner')

    def __init__(self, d, g=None):
        self.d, self.g = d, g
        self.bf_n = self.bf_t = None
        self.bf_step = -1
        self.owner = _OWNER[0]
        if d.dim() == 3 and d.is_cuda:
            CONV_PARAMS.setdefault(d.device, []).append(self)

    def bf16(self):
        """(natural [K][Cin][Cout], transposed [K][Cout][Cin]) bf16 copies, re-made when the weights changed.
        All conv kernels registered for this device are refreshed together by ONE table-driven launch."""
        if self.bf_step != WEIGHT_VERSION[0]:
            dev = self.d.device
            tab = _CAST_TABLE.get(dev)
            if tab is None or self.bf_n is None or self not in tab['set']:
                tab = _build_cast_table(dev)
            call('es_cast_weights_table', P(tab['dev']), tab['n'], tab['tiles'], _stream())
            for p in tab['params']:
                p.bf_step = WEIGHT_VERSION[0]
        return self.bf_n, self.bf_t


def refresh_weight_copies():
    """bf16 mode: bring the bf16 copies of every registered conv kernel up to date now (one launch on the current
    stream) instead of lazily at the first convolution that needs them."""
    if PRECISION[0] != 'bf16':
        return
    dev = torch.device('cuda', torch.cuda.current_device())
    ps = CONV_PARAMS.get(dev)
    if ps:
        ps[-1].bf16()


# Registry of the conv kernels (3-D Params) living on each GPU, the input of the one-launch bf16 weight cast.  Entries are
# tagged with the owner that was binding when they were made (a detector passes id(self) to begin_bind()); re-binding or
# releasing an owner drops its old entries, so a process that builds several detectors neither leaks their arenas nor
# keeps re-casting stale weights, and the tables of different devices never mix pointers.
_GC_FROZEN = [False]
CONV_PARAMS = {}          # torch.device -> [Param]
_CAST_TABLE = {}          # torch.device -> dict(dev=table tensor, n, tiles, params, set)
_OWNER = [None]


def begin_bind(owner):
    """drop every conv Param `owner` registered earlier and tag the ones created from now on with it"""
    release(owner)
    _OWNER[0] = owner


def end_bind():
    _OWNER[0] = None


def release(owner):
    """forget what detector `owner` registered here; objects frozen out of the collector's sight by settle_gc (gc.freeze at the
    detector's 6th step: everything alive then, the dropped detector's graph included) are handed back to it"""
    if _GC_FROZEN[0]:
        import gc
        gc.unfreeze()
        _GC_FROZEN[0] = False
    for dev in list(CONV_PARAMS):
        keep = [p for p in CONV_PARAMS[dev] if p.owner != owner]
        if len(keep) != len(CONV_PARAMS[dev]):
            CONV_PARAMS[dev] = keep
            _CAST_TABLE.pop(dev, None)
        if not keep:
            CONV_PARAMS.pop(dev, None)


def _build_cast_table(dev):
    ps = [p for p in CONV_PARAMS.get(dev, ()) if p.d.dim() == 3]
    rows, tiles = [], 0
    for p in ps:
        K, a, b = p.d.shape
        if p.bf_n is None:
            p.bf_n = torch.empty((K, a, b), dtype=torch.bfloat16, device=dev)
            p.bf_t = torch.empty((K, b, a), dtype=torch.bfloat16, device=dev)
        rows.append([p.d.data_ptr(), p.bf_n.data_ptr(), p.bf_t.data_ptr(), K, a, b, tiles])
        tiles += K * ((a + 63) // 64) * ((b + 63) // 64)
    tab = _CAST_TABLE[dev] = dict(dev=torch.tensor(rows, dtype=torch.int64).to(dev), n=len(rows), tiles=tiles, params=ps,
                                  set=set(ps))
    return tab


PRECISION = ['f32']       # 'f32': exact-f32 MFMA everywhere; 'bf16': bf16 MFMA (f32 accumulate) for conv fwd / dgrad / wgrad;
                          # the gathers read bf16 shadow copies of activations / gradients where the fast kernel takes the shape
WEIGHT_VERSION = [0]      # bumped by the optimiser: invalidates the bf16 weight copies


class Tape:
    def __init__(self):
        self.fns = []
        self.enabled = True
        self.epoch = 0                  # bumped whenever the tape is emptied (graphed(): one replay of a segment per epoch)

    def add(self, fn):
        if self.enabled:
            self.fns.append(fn)

    def backward(self):
        for fn in reversed(self.fns):
            fn()
        join_wgrad_streams()
        self.fns = []
        self.epoch += 1

    def clear(self):
        self.fns = []
        self.epoch += 1


TAPE = Tape()


class no_tape:
    """with no_tape(): ... -- nothing is recorded on the tape; TAPE.enabled is restored on exit, exceptions included"""

    def __enter__(self):
        self.prev, TAPE.enabled = TAPE.enabled, False

    def __exit__(self, *exc):
        TAPE.enabled = self.prev


# ------------------------------------------------------------------ captured launch sequences (hipGraph)
# The image backbone's forward is ~65 launches with static shapes, static addresses and no host round trip, but queuing them
# costs the host ~4 ms per step -- during which the point branch (whose kernels the image branch is meant to run under) has not
# even been issued (profiles/r3s_timeline.txt: main stream idle for the first 4 ms of every step).  graphed() captures such
# a sequence once into a hipGraph (torch.cuda.CUDAGraph: activations live in the graph's private pool) and replays it with ONE
# launch per step; the backward closures the sequence put on the tape are kept and re-registered at every replay (they run
# eagerly, on the same buffers), the gradient fields of the sequence's Vars are reset first.
GRAPHS = _switch('ES_GRAPHS')
GRAPH_STATS = dict(captured=0, replayed=0, eager=0, failed=0)


class _Segment:
    __slots__ = ('graph', 'outs', 'fns', 'vars', 'calls', 'failed', 'epoch')

    def __init__(self):
        self.graph = self.outs = None
        self.fns, self.vars, self.calls, self.failed, self.epoch = [], [], 0, False, -1


def reset_graphs(cache):
    """forget captured sequences (kernel-selection options or folded constants changed)"""
    cache.clear()


def graphed(cache, key, fn):
    """outs = fn(), through a hipGraph from the third call with the same key on (1st call: eager -- lazily built maps and
    shadows; 2nd: captured, then replayed).  Eager whenever per-launch instrumentation is on, on the default stream (capture
    needs a non-default stream: the side stream of the two-stream schedule), or after a failed capture."""
    global _NEW_VARS
    if not GRAPHS[0] or instrumented() or _NEW_VARS is not None or \
            torch.cuda.current_stream() == torch.cuda.default_stream():
        GRAPH_STATS['eager'] += 1
        return fn()
    seg = cache.get(key)
    if seg is None:
        if len(cache) > 8:
            cache.clear()
        seg = cache[key] = _Segment()
    seg.calls += 1
    # a replay hands out the SAME Vars and closures as the one before: two of them on one tape (the sequence run twice before a
    # backward pass) would double-count gradients, so the second run in a tape epoch is eager
    if seg.failed or seg.calls == 1 or (TAPE.enabled and seg.epoch == TAPE.epoch):
        GRAPH_STATS['eager'] += 1
        return fn()
    seg.epoch = TAPE.epoch
    if seg.graph is None:
        n0 = len(TAPE.fns)
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        _NEW_VARS = []
        try:
            g.capture_begin(capture_error_mode='thread_local')
            try:
                outs = fn()
            finally:
                g.capture_end()
        except Exception as e:                                  # leave the eager path in charge
            _NEW_VARS = None
            seg.failed = True
            GRAPH_STATS['failed'] += 1
            del TAPE.fns[n0:]
            import warnings
            warnings.warn(f'hipGraph capture of {key} failed ({e!r}): running this sequence eagerly')
            torch.cuda.synchronize()
            return fn()
        seg.vars, _NEW_VARS = _NEW_VARS, None
        seg.graph, seg.outs = g, outs
        seg.fns = TAPE.fns[n0:]
        del TAPE.fns[n0:]
        GRAPH_STATS['captured'] += 1
    for v in seg.vars:
        v.g = v.gh = None
        v.gated = False
    seg.graph.replay()
    GRAPH_STATS['replayed'] += 1
    if TAPE.enabled:
        TAPE.fns.extend(seg.fns)
    return seg.outs


# ------------------------------------------------------------------ side stream
# Independent branches of the step (image branch vs. point branch, samples of the loss) are issued on two HIP streams so
# that under-filled launches overlap.  Discipline that keeps the caching allocator safe without record_stream():
# (1) the side stream always starts ordered after everything queued on the main stream (fork event), (2) the main stream
# joins before it touches anything the side stream produced, (3) tensors crossing streams stay referenced until the
# join, so a block is only recycled by its own stream after the other stream's readers were ordered before it.
TWO_STREAMS = _switch('ES_TWO_STREAMS')
_SIDE = {}


class side_stream:
    """with side_stream(): ... -- run the enclosed launches on the side stream.  fork=True (default): ordered after
    everything queued on the current stream so far; fork=False: just continue on the side stream."""

    def __init__(self, fork=True):
        self.fork = fork

    def __enter__(self):
        if not _SIDE:
            _SIDE.update(s=torch.cuda.Stream(), fork=torch.cuda.Event(), join=torch.cuda.Event())
        if self.fork:
            _SIDE['fork'].record(hip.stream_obj())
            _SIDE['s'].wait_event(_SIDE['fork'])
        self.ctx = torch.cuda.stream(_SIDE['s'])
        self.ctx.__enter__()
        hip.refresh_stream()
        return self

    def __exit__(self, *exc):
        _SIDE['join'].record(_SIDE['s'])
        r = self.ctx.__exit__(*exc)
        hip.refresh_stream()
        return r


def join_side():
    """the current (main) stream waits for everything issued on the side stream so far"""
    if _SIDE:
        hip.stream_obj().wait_event(_SIDE['join'])


# Weight gradients hang off the backward chain (nothing downstream reads them before the optimiser), so they are
# launched on a second stream paired with the compute stream: the chain of data-gradient launches does not wait for them
# and under-filled launches of both kinds overlap.
WGRAD_ASYNC = _switch('ES_WGRAD_ASYNC')
_WGRAD_STREAMS = {}     # compute-stream handle -> dict(s=torch Stream, h=handle, fork=Event, join=Event, used=bool)
_KEEP = []              # temporaries read by queued weight-gradient launches; released by the final join


def _wgrad_rec():
    """the weight-gradient stream record of the current compute stream (created on first use)"""
    h = _stream()
    ws = _WGRAD_STREAMS.get(h)
    if ws is None:
        st = torch.cuda.Stream()
        ws = _WGRAD_STREAMS[h] = dict(s=st, h=st.cuda_stream, fork=torch.cuda.Event(), join=torch.cuda.Event(), used=False)
    return ws


def _wgrad_stream(*keep):
    """handle of the weight-gradient stream of the current compute stream, made to wait for everything queued on the
    compute stream so far; `keep`: tensors the launch reads that nobody else references."""
    if not WGRAD_ASYNC[0]:
        return _stream()
    ws = _wgrad_rec()
    ws['fork'].record(hip.stream_obj())
    ws['s'].wait_event(ws['fork'])
    ws['used'] = True
    _KEEP.extend(keep)
    return ws['h']


def wgrad_stream_obj():
    """the torch Stream that carries the weight-gradient launches of the current compute stream (created on first use) -- idle during
    the forward pass, so small independent forward-time work (the grounder's frozen text encoder) can ride on it instead of opening
    one more stream: a process has four hardware queues, and a fifth, sixth ... stream ends up sharing one with a stream it was meant to
    overlap (bench.py copy_stream: ~ 10 - 18 % per step when that happens)"""
    return _wgrad_rec()['s']


def join_wgrad_streams(final=True):
    """make the current stream wait for every queued weight-gradient launch (before the gradients are reduced or
    consumed by the optimiser)"""
    cur = hip.stream_obj()
    for ws in _WGRAD_STREAMS.values():
        if ws['used']:
            ws['join'].record(ws['s'])
            cur.wait_event(ws['join'])
            ws['used'] = False
    if final:
        _KEEP.clear()


# ------------------------------------------------------------------ per-stream workspaces
# One buffer per (tag, stream), grown on demand and reused by every launch of that stream that names the tag: the launches of a
# stream are ordered, so the reuse is race free.  Scratch tags: 'wgrad' (partial tensors of the weight-gradient row splits), 'dense'
# (partial tiles of split dense launches).  Zeroed tags -- kernels that reduce per-workgroup partials in their last workgroup
# (csrc/common.h es_last_block) keep a ticket counter at the head that is 0 before and after every launch: 'ticket', 'split', 'colsum'
# and 'topk' (es_topk_mask_ws also keeps its selection state there).
_ZEROED = ('ticket', 'split', 'colsum', 'topk')
_WS = {tag: {} for tag in ('wgrad', 'dense') + _ZEROED}      # tag -> {stream handle: tensor}
_WGRAD_WS = _WS['wgrad']


def stream_ws(stream, tag, floats, like):
    """(tensor, floats): the f32 workspace `tag` of stream handle `stream`, at least `floats` long, on like.device"""
    table = _WS[tag]
    ws = table.get(stream)
    if ws is None or ws.numel() < floats or ws.device != like.device:     # (a buffer of another device is never handed out)
        if ws is not None:
            _KEEP.append(ws)                     # launches already queued on `stream` may still use the old buffer
        if tag in _ZEROED:
            ws = torch.zeros(max(int(floats), 1 << 16), dtype=torch.float32, device=like.device)
            if stream != _stream():              # the zero fill was queued on the current stream: order it before the first launch
                ev = torch.cuda.Event()          # on `stream` that reads the ticket
                ev.record(hip.stream_obj())
                hip._stream_of(stream).wait_event(ev)
        else:
            ws = torch.empty(max(int(floats), 1 << 22), dtype=torch.float32, device=like.device)
        table[stream] = ws
    return ws, ws.numel()


def ticket_ws(floats, like, tag='ticket'):
    """zero-initialised workspace of a last-block reduction on the current stream (see stream_ws)"""
    assert tag in _ZEROED, tag
    return stream_ws(_stream(), tag, floats, like)


# The first weight-gradient launch a weight receives in a step OVERWRITES its slot of the gradient arena (a plain store: the
# read-modify-write of a 1 GB gradient made the wide occupancy layers wait on 128 dependent loads per thread); later launches of
# the same step (shared modules, the 8 taps of a transposed convolution have their own slots) accumulate.  Keyed by the slot's
# device pointer, so aliases of one tensor share the stamp.  new_grad_epoch() is called where the arena is zeroed.
GRAD_EPOCH = [1]
_GRAD_STAMP = {}


def new_grad_epoch():
    GRAD_EPOCH[0] += 1
    if len(_GRAD_STAMP) > 1 << 16:
        _GRAD_STAMP.clear()


def _first_write(ptr):
    """0 (overwrite) for the first gradient written to `ptr` in this epoch, 1 (accumulate) afterwards"""
    acc = 1 if _GRAD_STAMP.get(ptr) == GRAD_EPOCH[0] else 0
    _GRAD_STAMP[ptr] = GRAD_EPOCH[0]
    return acc


def _written(ptr):
    """what _first_write(ptr) would return, without stamping (for a launch that may still decline its operands)"""
    return 1 if _GRAD_STAMP.get(ptr) == GRAD_EPOCH[0] else 0


def _wgrad(name, sw, dW, *args, like=None, acc=None):
    """launch a weight-gradient entry point (`args` = everything between the function name and dW) on stream `sw` with the
    workspace its row split asks for (that stream's 'wgrad' buffer); like: a tensor on the launch's device (None: the current GPU,
    for callers that hold raw pointers only); acc: the accumulate flag (None: _first_write(dW))"""
    f32 = _C['ES_ROWS_F32']        # (the workspace query takes the operand kinds of the _src form; the other two entry points read f32 rows)
    X, xh, ldx, dY, yh, ldy, nbr, *shape = args if name == 'es_spconv_wgrad_bf16_src' else (args[0], f32, args[1], args[2], f32, *args[3:])
    need = hip.raw('es_spconv_wgrad_workspace_floats')(int(name != 'es_spconv_wgrad'), X, xh, ldx, dY, yh, ldy, *shape)
    if like is None:
        like = torch.empty(0, device=torch.device('cuda', torch.cuda.current_device()))
    ws, nf = stream_ws(sw, 'wgrad', need, like) if need else (None, 0)
    call(name, *args, dW, _first_write(dW) if acc is None else acc, P(ws), nf, sw)


IMG_WGRAD = _switch('ES_IMG_WGRAD')     # round 6: 3x3 image weight gradients on csrc/imgwgrad.hip (A/B switch)
# stride-2 data gradients of the image backbone by address arithmetic (csrc/imgconv.hip: es_img_dgrad3_s2_bf16 / es_img_dgrad1_s2_bf16),
# bit-identical to the map-kernel launches they replace (A/B switch and the way back)
IMG_STRIDED_DGRAD = _switch('ES_IMG_STRIDED_DGRAD')
# FCAF3D head backward without the work its result does not need (A/B switch; off: exactly the launches before it existed): the 8 taps of a
# generative transposed convolution's weight gradient in one launch (es_gen_transpose_wgrad_bf16), the head gradient matrix cleared by the
# focal-loss launch instead of a zero fill (es_focal_loss_clear, models/dense_heads/fcaf3d_head.py)
HEAD_BWD_FUSED = _switch('ES_HEAD_BWD_FUSED')


# Python's cyclic collector and the train loop (round 5, profiles/r5d / r5f_bench_grounding_diag.json: `gc_collections`): a generation-2
# collection walks every live container of the process -- model, configs, the frozen text encoder's module tree, torch's own tables
# -- and costs 110-170 ms of host time whenever the allocation counters trip it (every ~20-25 steps: the 3.5x step-time outliers of
# rounds 3-4).  A step leaves no cyclic garbage (sparse.CoordSet caches are weak), so after a few steps everything alive is long-lived:
# it is moved to the permanent generation once (gc.freeze) and later collections only look at what was allocated since (measured on
# this image: a full collection of 10^6 tracked objects 180 ms -> 0.0 ms after the freeze).  ES_GC_FREEZE=0 turns this off; a process
# that drops a detector and builds another should gc.unfreeze() + gc.collect() in between (bench.py release_frozen).
GC_SETTLE_STEP = 6
_HOST_SETTLED = [False]


def settle_host_threads(force=False):
    """Once per process (first train step): cap torch's intra-op (OpenMP) pool.  torch sizes it by the CPUs it SEES (128 threads on
    the GPU boxes); the cgroup GRANTS 16 cores there, and after any CPU-side tensor operation of a step the idle workers spin before
    they sleep -- together they exhaust the quota and the kernel throttles the whole process, the thread that queues the GPU's work
    included: every ~9th occupancy step was 12 - 27 ms longer with the device idle (cpu.stat nr_throttled 28 -> 59 over two 60-step runs,
    none with one thread: profiles/r5w_*).  A training step has no CPU tensor work worth a pool: a quarter of the granted cores per local
    rank (ES_HOST_THREADS=n overrides, 0 leaves torch alone)."""
    if _HOST_SETTLED[0] and not force:
        return
    _HOST_SETTLED[0] = True
    want = os.environ.get('ES_HOST_THREADS', 'auto')
    if want == '0':
        return
    if want == 'auto':
        from .datasets.loader import effective_cpus
        local = max(1, int(os.environ.get('LOCAL_WORLD_SIZE', '1') or 1))
        n = max(1, effective_cpus() // 4 // local)
    else:
        n = max(1, int(want))
    if torch.get_num_threads() > n:
        torch.set_num_threads(n)


def settle_gc(det):
    """called at the top of every train_step: freezes the collector's generations when `det` reaches its GC_SETTLE_STEP-th step
    (and, at the process's first step, caps the host thread pool: settle_host_threads)"""
    settle_host_threads()
    n = getattr(det, '_steps_done', 0) + 1
    det._steps_done = n
    if n == GC_SETTLE_STEP and _switch('ES_GC_FREEZE')[0]:
        import gc
        gc.collect()
        gc.freeze()
        _GC_FROZEN[0] = True                     # (release() unfreezes)


def reset_tickets():
    """re-zero the ticket heads of every cached election workspace (on the current stream).  A launch that faulted inside an
    in-launch reduction leaves its ticket non-zero; the step that saw the fault has already raised HipError, a caller that
    catches it and continues must call this (after synchronising) before the next step."""
    for tag in _ZEROED:
        for ws in _WS[tag].values():
            ws[:min(ws.numel(), 2048)].zero_()


def drop_caches():
    """forget every per-stream workspace / kept temporary (tests that switch between devices or libraries in one process)"""
    for table in _WS.values():
        table.clear()
    _KEEP.clear()


MARKS = None            # bench.py sets a list: stage boundaries as (name, event) recorded on the current stream
HOST_MARKS = None       # tools/host_profile.py sets a list: (name, host perf_counter) at the same stage boundaries


def mark(name):
    """stage boundary for the per-stage timing of bench.py (SURVEY 8d "Reporting"); free when MARKS is None"""
    if HOST_MARKS is not None:
        import time
        HOST_MARKS.append((name, time.perf_counter()))
    if MARKS is not None:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(hip.stream_obj())
        MARKS.append((name, ev))


DEBUG_GRADS = None      # tools/debug_grads.py sets a dict: id(Var) -> snapshot of its gradient when consumed
DEBUG_CONV = None       # tests/test_gpu_insitu.py sets a list: one record per convolution backward of the step (operands as the
                        # launches saw them + the data gradient this launch produced), for the in-situ check of every
                        # weight- / data-gradient launch against its arithmetic specification
DEBUG_OPS = None        # ... and a list for the other backward launches with parameters or matrix-core arithmetic: attention
                        # (kind 'attn'), LayerNorm ('ln'), ContrastiveEmbed ('contrastive', appended by GroundingHead)
DEBUG_FWD = None        # ... and for the forward launches (fwd_record): a list, or a callable that receives each record at once (a check
                        # on the spot: nothing accumulates over a config-scale step)


def fwd_record(kind, entry, **ops):
    """DEBUG_FWD: one record of the forward launch that has just been queued -- `entry`: the entry point that took it; `ops`: its
    operands and outputs, cloned here on the launch's stream (later in-place writers -- relu_, upsample_add_ -- cannot change them).
    A Param / ParamSlice operand is recorded as its f32 values plus (`<name>_h`) the bf16 copy a bf16 launch read."""
    rec = dict(kind=kind, entry=entry, precision=PRECISION[0])
    for k, v in ops.items():
        if isinstance(v, (Param, ParamSlice)):
            rec[k] = v.d.clone()
            if PRECISION[0] == 'bf16' and v.d.dim() == 3:
                rec[k + '_h'] = v.bf16()[1].clone()
        elif isinstance(v, torch.Tensor):
            rec[k] = v.clone()
        else:
            rec[k] = v
    if callable(DEBUG_FWD):
        DEBUG_FWD(rec)
    else:
        DEBUG_FWD.append(rec)


def _cast_rows(t):
    n, C = t.shape
    h = torch.empty((n, C), dtype=torch.bfloat16, device=t.device)
    call('es_cast_rows_bf16', P(t), t.stride(0), n, C, P(h), _stream())
    return h


GEN_FUSED = _switch('ES_GEN_FUSED')        # generative transposed conv: 8 taps in one launch per direction (round 4:
                                           # run on hardware, forward bit-identical, step -0.6 ms; profiles/r4a_*)


def _split_ws(n_out, K, cin, cout, like):
    """workspace for the deterministic tap split of an under-filled bf16 conv launch (size from the library's own rule,
    es_spconv_split_workspace_floats): (tensor or None, floats).  Its head holds the tile tickets of the in-kernel reduction (zero
    before and after every launch), so it is the stream's persistent zero-initialised ticket workspace (ticket_ws), not a fresh
    allocation: the split launches of a stream are ordered, each has read its partial tiles before the next one starts."""
    if K <= 1 or n_out <= 0:
        return None, 0
    nf = int(hip.raw('es_spconv_split_workspace_floats')(n_out, K, cin, cout))
    if nf == 0:
        return None, 0
    return ticket_ws(nf, like, tag='split')


def _fwd_bf16(X, x_is_bf16, ldx, Wp, nbr, n_out, n_in, K, cin, cout, bias_p, Y, ldy, acc, like):
    """es_spconv_fwd_bf16 with the deterministic-split workspace when the launch would split its tap list -> the entry point taken"""
    ws, nf = _split_ws(n_out, K, cin, cout, like)
    entry, ws_args = ('es_spconv_fwd_bf16', ()) if ws is None else ('es_spconv_fwd_bf16_ws', (P(ws), nf))
    call(entry, X, x_is_bf16, ldx, Wp, nbr, n_out, n_in, K, cin, cout, bias_p, Y, ldy, acc, *ws_args, _stream())
    return entry


def _use_shadow(n_rows, C, K, cin, cout):
    """bf16 shadow pays when the rows are gathered several times (K > 1) and the fast kernel takes the shape"""
    return K > 1 and hip.raw('es_spconv_bf16_is_fast')(n_rows, C, K, cin, cout) == 1


def _grad_shadow_only(x, w, n_out, need_dx, bf, gate=None, ldg=None):
    """the backward of this convolution takes the bf16 shadow of its output gradient (leading dimension ldg; None: contiguous rows)
    for both of its launches: _conv_wgrad and _conv_dgrad gather gh, and the f32 rows are read by a bias column sum at most"""
    K, cin, cout = w.d.shape
    return bool(bf and cout >= 16 and need_dx and x.rg and gate is None and (ldg is None or ldg == cout)
                and _use_shadow(n_out, cout, K, cout, cin))


# Gradient rows that only bf16 readers see are written once, in bf16 (A/B switch; 0: exactly the launches before it existed).  The
# gradient a train-mode norm hands to the convolution that produced its input is such a matrix when that convolution's backward gathers
# the shadow for both launches (_grad_shadow_only) and has no bias: es_norm_bwd then writes the shadow alone (dx = NULL), and the
# convolution's .g IS that bf16 matrix.  The per-launch instrumentation records and reads the f32 rows: with any of it on they are written.
GRAD_ROWS_BF16 = _switch('ES_GRAD_ROWS_BF16')


def _f32_grad_rows_wanted():
    return instrumented(fwd=False)


# ------------------------------------------------------------------ halo-tile K = 27 convolutions (round 6, csrc/halo.hip)
HALO = _switch('ES_HALO')
if os.environ.get('ES_HALO_MIN_WGS') is not None:
    hip.raw('es_halo_set_option')(30, int(os.environ['ES_HALO_MIN_WGS']))
if os.environ.get('ES_HALO_PLAN_BITMAP') is not None:       # A/B switch of the bitmap halo plan (default: on; 0: hash-and-rank)
    hip.raw('es_halo_set_option')(32, int(os.environ['ES_HALO_PLAN_BITMAP']))


def _is_mirror(inv):
    """inv is a sparse.MirrorInv handle: "the inverse map is the forward map inv.nbr with its taps mirrored" (no inverse map tensor exists)"""
    return inv is not None and not isinstance(inv, torch.Tensor)


def _halo_ok(nbr, n_out, n_in, ldx, K, cin, cout):
    return (HALO[0] and K == 27 and nbr is not None
            and hip.raw('es_spconv_halo_supported')(n_out, n_in, ldx, K, cin, cout) == 1)


def halo_plan(nbr):
    """(loc, hrows, hcnt) of a kernel map: per 256-row tile the sorted distinct source rows and the 16-bit positions of every
    (row, tap) neighbour in that list (es_halo_plan).  Built on the current stream at first use and kept ON the map tensor, so it
    lives and dies with the map's cache entry (sparse.CoordSet.kernel_map / inverse_map)."""
    plan = getattr(nbr, '_halo', None)
    if plan is None:
        n_out, K = nbr.shape
        rows = int(hip.raw('es_halo_plan_rows')(n_out))
        loc = torch.empty((rows, K), dtype=torch.int16, device=nbr.device)
        hrows = torch.empty((rows // 256, 256 * K), dtype=torch.int32, device=nbr.device)
        hcnt = torch.empty((rows // 256,), dtype=torch.int32, device=nbr.device)
        call('es_halo_plan', P(nbr), n_out, K, P(loc), P(hrows), P(hcnt), _stream())
        plan = nbr._halo = (loc, hrows, hcnt)
        if hip.PROFILE is not None:
            hip.PAIRS[loc.data_ptr()] = (nbr >= 0).sum()
    return plan


def _halo_launch(Xh, ldx, Wp, nbr, n_out, n_in, K, cin, cout, bias_p, Y, ldy, acc):
    """nbr: the launch's gather map.  The INVERSE map of a stride-1 convolution on one coordinate set is its forward map with the
    taps mirrored (sparse.CoordSet.inverse_map marks it `_mirror_of`): such a data gradient runs on the forward map's plan."""
    fwd = nbr.nbr if _is_mirror(nbr) else getattr(nbr, '_mirror_of', None)
    loc, hrows, hcnt = halo_plan(fwd if fwd is not None else nbr)
    return hip.try_call('es_spconv_halo_bf16', Xh, ldx, Wp, P(loc), P(hrows), P(hcnt), n_out, n_in, K, cin, cout, bias_p, Y, ldy, acc,
                        int(fwd is not None), _stream())


def empty(shape, like, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


def zeros(shape, like, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype, device=like.device)


def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1, 'row matrices must be contiguous along channels'
    return t.stride(0)


def _grad_target(v, shape_like):
    """(tensor, accumulate flag) for writing the gradient of v."""
    v.gh = None                                       # whatever shadow of the gradient exists is about to go stale
    # (a bf16 .g is the only copy of a gradient whose producer promised a single consumer -- norm() on a fresh conv output, a join on
    # its downsample identity: a second consumer would write f32 rows into it)
    assert v.g is None or v.g.dtype == torch.float32, 'a second consumer accumulates into gradient rows that were written in bf16'
    if v.g is None:
        v.g = torch.empty(shape_like.shape, dtype=torch.float32, device=shape_like.device)    # gradients are f32 rows
        return v.g, 0
    return v.g, 1


def _grad_ptr(v):
    """_grad_target as (pointer, accumulate flag) for a launch with optional outputs: (0, 0) for no Var or one that takes no gradient"""
    if v is None or not v.rg:
        return 0, 0
    t, acc = _grad_target(v, v.d)
    return P(t), acc


def _grad_give(v, t, alias=True):
    """give the f32 row matrix `t` to v as its gradient: v has none yet -> t itself where the caller says v may alias it (nobody else keeps
    or writes t), else a copy -> True; v has one -> added to it (es_axpy2d) -> False.  The same guards as _grad_target."""
    v.gh = None
    assert v.g is None or v.g.dtype == torch.float32, 'a second consumer accumulates into gradient rows that were written in bf16'
    if v.g is None:
        v.g = t if alias else t.clone()
        return True
    call('es_axpy2d', P(v.g), _ld(v.g), P(t), _ld(t), t.shape[0], t.shape[1], 1.0, 1, _stream())
    return False


# ------------------------------------------------------------------ dense-volume convolutions (round 5, csrc/dconv.hip)
# nn.Conv3d on a dense (B, X, Y, Z) grid by address arithmetic: no neighbour map.  `dense` = (B, X, Y, Z, ksize, stride, pad) of the
# INPUT grid; a convolution that passes it runs on the dense engine wherever the library takes the shape (bf16 mode, reduction
# channels % 64, output channels % 256; the data gradient for stride 1) and falls back to the map kernels elsewhere -- `maps` is then
# a callable returning (nbr, inv), so the maps of a layer the dense engine covers completely are never built.
# Z = 0 names a FLAT grid: nn.Conv2d on (B, X, Y) images (the FPN's 3x3 output convolutions); a bias is pre-filled, the launch accumulates.
DENSE = _switch('ES_DENSE')


def _dense_geom(dense):
    return iarr(dense) if dense is not None else None


def dense_ok(dense, mode, cin, cout):
    """the dense engine takes this shape (es_dconv_supported: for fresh contiguous operands -- the launch itself answers for the
    caller's, _dense_launch / _dense_wgrad return False where it does not take them)"""
    if not (DENSE[0] and dense is not None and PRECISION[0] == 'bf16'):
        return False
    if mode == 2 and dense[4] == 1 and (cin // 256) * (cout // 256) < 48:
        # weight gradient of a 1x1x1 convolution: one workgroup per 256 x 256 channel tile walking every row -- the neck's 768 -> 1536
        # down-sample would launch 18 of them (134 us against the map kernel's row-split 49 us, profiles/r5p_occ_launches.jsonl)
        return False
    return hip.raw('es_dconv_supported')(_dense_geom(dense), mode, cin, cout) == 1


def _dense_launch(Xh, ldx, Wp, dense, mode, cin, cout, Y, ldy, acc, like):
    g = _dense_geom(dense)
    s = _stream()
    need = int(hip.raw('es_dconv_workspace_floats')(g, mode, cin, cout))
    ws, nf = stream_ws(s, 'dense', need, like) if need else (None, 0)
    return hip.try_call('es_dconv_fwd_bf16', Xh, ldx, Wp, g, mode, cin, cout, Y, ldy, acc, P(ws), nf, s)


def _dense_wgrad(xh, ldx, gh, ldy, dense, transposed, cin, cout, dW, acc, sw, like):
    """weight gradient on the dense engine, on the weight-gradient stream `sw`; launches of few tiles over many rows (the 2-D 3x3
    layers) slice the rows through that stream's workspace"""
    g = _dense_geom(dense)
    need = int(hip.raw('es_dconv_wgrad_workspace_floats')(g, transposed, cin, cout))
    ws, nf = stream_ws(sw, 'dense', need, like) if need else (None, 0)
    return hip.try_call('es_dconv_wgrad_ws_bf16', xh, ldx, gh, ldy, g, transposed, cin, cout, dW, acc, P(ws), nf, sw)


class _Maps:
    """(nbr, inv) of a convolution, built on first use"""
    __slots__ = ('fn', 'val')

    def __init__(self, fn):
        self.fn, self.val = fn, None

    def get(self):
        if self.val is None:
            self.val = self.fn()
        return self.val


# ------------------------------------------------------------------ convolution
def conv(x, w, nbr, inv, n_out, bias=None, need_dx=True, bias_from=0, dense=None, maps=None):
    """y[j] = sum_k x[nbr[j,k]] @ w[k] (+bias).  w.d: (K,Cin,Cout).  nbr None -> identity (K=1).
    bias_from: first output column whose bias is trainable (earlier columns keep a zero bias).
    dense / maps: see "dense-volume convolutions" above (nbr / inv are then taken from maps() where a map kernel runs)."""
    K, cin, cout = w.d.shape
    n_in = x.d.shape[0]
    bias_p = P(bias.d) if bias else 0
    y = Var(empty((n_out, cout), x.d))
    bf = PRECISION[0] == 'bf16' and cin >= 16
    if maps is not None:
        maps = _Maps(maps) if not isinstance(maps, _Maps) else maps
    x16 = x.d.dtype == torch.bfloat16                  # bf16 activation rows (the image backbone's outputs): their own shadow
    if x16:
        assert bf and _ld(x.d) == cin, 'bf16 input rows need the bf16 kernels and contiguous rows'
        x.dh = x.d
    dn = bf and _ld(x.d) == cin and dense_ok(dense, 0, cin, cout)
    if dn and bias:                               # rows pre-filled with the bias, the launch accumulates (the tile's accumulators fill the
        y.d.copy_(bias.d.expand_as(y.d))          # register file: an epilogue that also held the bias spilled)
    if dn and _dense_launch(P(x.shadow()), cin, P(w.bf16()[1]), dense, 0, cin, cout, P(y.d), cout, 1 if bias else 0, x.d):
        entry, gathered = 'es_dconv_fwd_bf16', True
    else:
        if maps is not None:
            nbr, inv = maps.get()
        gathered = bool(bf and (x16 or (_ld(x.d) == cin and _use_shadow(n_in, cin, K, cin, cout))))    # the launch gathers x's bf16 shadow
        if gathered:                               # (False: it reads the f32 rows)
            if (_halo_ok(nbr, n_out, n_in, cin, K, cin, cout)
                    and _halo_launch(P(x.shadow()), cin, P(w.bf16()[1]), nbr, n_out, n_in, K, cin, cout, bias_p, P(y.d), cout, 0)):
                entry = 'es_spconv_halo_bf16'
            else:
                entry = _fwd_bf16(P(x.shadow()), 1, cin, P(w.bf16()[1]), P(nbr), n_out, n_in, K, cin, cout, bias_p, P(y.d), cout, 0, x.d)
        elif bf:
            entry = _fwd_bf16(P(x.d), 0, _ld(x.d), P(w.bf16()[1]), P(nbr), n_out, n_in, K, cin, cout, bias_p, P(y.d), cout, 0, x.d)
        else:
            call('es_spconv_fwd', P(x.d), _ld(x.d), P(w.d), P(nbr), n_out, n_in, K, cin, cout, bias_p, P(y.d), cout, 0, 0, _stream())
            entry = 'es_spconv_fwd'
    if DEBUG_FWD is not None:
        if maps is not None:
            nbr, inv = maps.get()
        fwd_record('conv', entry, x=x.d, xh=x.dh if gathered else None, w=w, nbr=nbr, n_out=n_out, bias=bias.d if bias else None,
                   round=bool(bf), y=y.d)

    def bwd():
        if y.g is None:
            return
        if DEBUG_GRADS is not None:
            DEBUG_GRADS[id(y)] = y.g.clone()
        _conv_backward(x, w, nbr, inv, n_out, y, y.g, bias, bias_from, need_dx, bf, dense=dense, maps=maps)
    TAPE.add(bwd)
    x.fresh = False
    y.fresh = True
    y.gsh = TAPE.enabled and bias is None and _grad_shadow_only(x, w, n_out, need_dx, bf)
    return y


# The storage form of a convolution's output gradient: decided ONCE, by _conv_backward, and handed to _conv_wgrad / _conv_dgrad as a _Gy
# (shadow: the bf16 matrix the gathering launches read -- SHADOWED, BF16 -- else None); an entry point's integers are made where it is called.
F32, SHADOWED, BF16, PRE16 = 'f32 rows', 'f32 rows + cast shadow', 'bf16 rows of es_norm_bwd, their own shadow', 'pre-rounded bf16 rows of a join'
_GY_F32 = (F32, SHADOWED)                          # the forms whose .rows are f32
_Gy = namedtuple('_Gy', 'rows form shadow')
# dy_half of es_spconv_wgrad_bf16_src for the matrix it is given (the shadow where there is one, else the rows)
_DY_HALF = {F32: _C['ES_ROWS_F32'], SHADOWED: _C['ES_ROWS_BF16'], BF16: _C['ES_ROWS_BF16'], PRE16: _C['ES_ROWS_PRE16']}
Img = namedtuple('Img', 'n_img H W stride')        # the image grid of a conv_affine layer; callers may pass a plain 4-tuple


def _conv_backward(x, w, nbr, inv, n_out, y, gy, bias, bias_from, need_dx, bf, gate=None, dense=None, maps=None, img=None, pre16=False):
    """wgrad (+ bias grad) and dgrad of a convolution whose output gradient is the row matrix `gy`.
    gate: folded-BN scale of x's producer -- the dgrad launch then also applies that layer's ReLU mask and BN scale
    (x is its only consumer), leaving x.g as the gradient of the producer's raw conv output.
    pre16: gy holds the PRE-ROUNDED bf16 rows of an f32 matrix that was never stored (conv_affine's joins, GRAD_ROWS_BF16): the K = 1
    launches take them in place of that matrix, on its tiles and slices; whoever chose the bf16 rows has checked that they can."""
    K, cin, cout = w.d.shape
    rec = None
    # dense engine: weight gradient / data gradient by address arithmetic where the library takes the shape
    dn_ok = bf and dense is not None and gate is None and _ld(gy) == cout and _ld(x.d) == cin
    dn_w = dense if (dn_ok and w.g is not None and dense_ok(dense, 2, cin, cout)) else None
    dn_d = dense if (dn_ok and need_dx and x.rg and dense_ok(dense, 1, cin, cout)) else None
    if maps is not None and (DEBUG_CONV is not None or (w.g is not None and dn_w is None) or (need_dx and x.rg and dn_d is None)):
        nbr, inv = maps.get()
    if DEBUG_CONV is not None:
        rec = dict(x=x.d, w=w, nbr=nbr, n_out=n_out, gy=gy.clone(), bf=bool(bf), gate=gate, need_dx=bool(need_dx and x.rg),
                   before=(x.g.clone() if (x.g is not None and need_dx and x.rg) else None), bias=bias, bias_from=bias_from)
        DEBUG_CONV.append(rec)
    # bf16 shadow of the output gradient: gather source of the data-gradient launch and, with the input's shadow from
    # the forward pass, of the weight-gradient launch (made here, before the weight-gradient stream forks)
    img = None if img is None else Img(*img)
    g = _Gy(gy, F32, None)
    if gy.dtype == torch.bfloat16:               # bf16 gradient rows (GRAD_ROWS_BF16: nothing reads this gradient in f32) are their own
        assert bf and _ld(gy) == cout and bias is None              # shadow: no cast launch
        if pre16:
            assert K == 1 and x.d.dtype == torch.bfloat16
            g = _Gy(gy, PRE16, None)
        else:                                    # from norm(): both launches gather the shadow anyway
            assert gy is y.g and _grad_shadow_only(x, w, n_out, need_dx, bf, gate)
            g = _Gy(gy, BF16, gy)
            y.gh = gy
    elif dn_w is not None or dn_d is not None or _grad_shadow_only(x, w, n_out, need_dx, bf, gate, _ld(gy)):
        g = _Gy(gy, SHADOWED, y.grad_shadow() if gy is y.g else _cast_rows(gy))
    if dn_w is not None:
        x.shadow()                               # (made by the forward launch; never on the weight-gradient stream)
    if w.g is not None or (bias is not None and bias.g is not None):
        sw = _wgrad_stream(gy, x.d, g.shadow, x.dh)
    if w.g is not None:
        _conv_wgrad(x, w, nbr, n_out, g, bf, dn_w, maps, img, sw)
    if bias is not None and bias.g is not None:
        # column sums of gy (round 4: one deterministic launch on the weight-gradient stream; was an f32 GEMM against a column of ones)
        nb, dst = cout - bias_from, bias.g.data_ptr() + 4 * bias_from
        ws, nf = stream_ws(sw, 'colsum', int(hip.raw('es_colsum_workspace_floats')(n_out, nb)), gy)
        call('es_colsum', gy.data_ptr() + 4 * bias_from, _ld(gy), n_out, nb, dst, _first_write(dst), P(ws), nf, sw)
    if need_dx and x.rg:
        _conv_dgrad(x, w, inv, n_out, g, bf, dn_d, maps, gate, img)
    if rec is not None and rec['need_dx']:
        rec['after'] = x.g.clone()               # (gradient buffer after this launch; `before` = what it accumulated onto)


def _conv_wgrad(x, w, nbr, n_out, g, bf, dn_w, maps, img, sw):
    """the weight-gradient launch of a convolution on stream `sw`: the first candidate that takes it (a fast path's launcher has the
    last word on the operands: ES_DECLINED passes on to the next candidate).  g: the output gradient (_Gy)"""
    K, cin, cout = w.d.shape
    n_in = x.d.shape[0]
    gy, gh = g.rows, g.shadow
    acc = _first_write(P(w.g))
    xh_f32 = bf and x.dh is not None and g.form in _GY_F32              # bf16 activation rows against f32 gradient rows
    if dn_w is not None:                         # dense engine (dense_ok)
        if _dense_wgrad(P(x.dh), cin, P(gh), cout, dn_w, 0, cin, cout, P(w.g), acc, sw, gh):
            return
        if maps is not None:                     # the maps are built on the compute stream: fork the weight-gradient stream again
            nbr, _ = maps.get()
            sw = _wgrad_stream()
    # 3x3 / pad 1 image layers, C -> C channels, by address arithmetic on the image grid (csrc/imgwgrad.hip)
    if IMG_WGRAD[0] and xh_f32 and img is not None and K == 9 and cin == cout:
        nf = int(hip.raw('es_img_wgrad9_workspace_floats')(img.n_img, img.H, img.W, cin, img.stride))
        if nf:
            ws, nf = stream_ws(sw, 'wgrad', nf, gy)
            if hip.try_call('es_img_wgrad9_bf16', P(x.dh), _ld(x.dh), P(gy), _ld(gy), img.n_img, img.H, img.W, cin, img.stride, P(w.g),
                            acc, P(ws), nf, sw):
                return
    # 1x1 layers on contiguous rows (identity map): streaming kernel (csrc/imgwgrad.hip)
    if (xh_f32 or (g.form == PRE16 and x.dh is not None)) and K == 1 and nbr is None and n_in == n_out:
        nf = int(hip.raw('es_rows_wgrad1_workspace_floats')(n_out, cin, cout))
        if nf:
            ws, nf = stream_ws(sw, 'wgrad', nf, gy)
            if hip.try_call('es_rows_wgrad1_bf16', P(x.dh), _ld(x.dh), P(gy), _ld(gy), n_out, cin, cout, P(w.g),
                            acc | (_C['ES_ACC_ROWS_BF16'] if g.form == PRE16 else 0), P(ws), nf, sw):
                return
    # map kernels: gathering from the bf16 shadows where they exist (bf16 activation rows are their own shadow)
    if bf and (gh is not None or x.dh is not None or x.d.dtype == torch.bfloat16):
        xs, ys = x.dh if x.dh is not None else x.d, gh if gh is not None else gy
        _wgrad('es_spconv_wgrad_bf16_src', sw, P(w.g), P(xs), int(x.dh is not None), _ld(xs), P(ys), _DY_HALF[g.form], _ld(ys), P(nbr),
               n_out, n_in, K, cin, cout, like=gy, acc=acc)
        return
    assert x.d.dtype == torch.float32, 'bf16 activation rows reach the weight gradient through their shadow (x.dh)'
    _wgrad('es_spconv_wgrad_bf16' if bf else 'es_spconv_wgrad', sw, P(w.g), P(x.d), _ld(x.d), P(gy), _ld(gy), P(nbr), n_out, n_in, K,
           cin, cout, like=gy, acc=acc)


def _conv_dgrad(x, w, inv, n_out, g, bf, dn_d, maps, gate, img):
    """the data-gradient launch of a convolution into x.g: the first candidate that takes it (as _conv_wgrad).  gate: see _conv_backward;
    g: the output gradient (_Gy)"""
    K, cin, cout = w.d.shape
    n_in = x.d.shape[0]
    gy, gh, s = g.rows, g.shadow, _stream()
    x16 = x.d.dtype == torch.bfloat16
    if gate is not None:
        assert x.g is None and bf, 'gated dgrad: x must have exactly one consumer'
        x.g, x.gated = torch.empty(x.d.shape, dtype=torch.float32, device=x.d.device), True
        gated, wn = _C['ES_ACT_GATE'], P(w.bf16()[0])
        im3 = img is not None and K == 9 and cin == cout and x16 and g.form in _GY_F32       # a 3x3 image layer (csrc/imgconv.hip)
        # ... of stride 1 by address arithmetic (mode 1)
        if (im3 and img.stride == 1 and _ld(x.d) == cin and hip.raw('es_img_conv3_supported')(img.n_img, img.H, img.W, cin, 1, 1) == 1
                and hip.try_call('es_img_conv3_bf16', P(gy), _ld(gy), wn, img.n_img, img.H, img.W, cin, 1, 1, P(gate), 0, P(x.d), _ld(x.d),
                                 gated, P(x.g), _C['ES_ROWS_F32'], _ld(x.g), s)):
            return
        # ... of stride 2: only the taps of each pixel's parity class (k_img_dgrad3_s2)
        if (im3 and img.stride == 2 and IMG_STRIDED_DGRAD[0] and hip.raw('es_img_dgrad3_s2_supported')(img.n_img, img.H, img.W, cin) == 1
                and hip.try_call('es_img_dgrad3_s2_bf16', P(gy), _ld(gy), wn, img.n_img, img.H, img.W, cin, P(gate), P(x.d), _ld(x.d),
                                 P(x.g), _ld(x.g), s)):
            return
        if _is_mirror(inv):                      # the fused-epilogue entry points have no mirrored tap walk: the real inverse map
            inv = inv.real()
        if x16:                                  # the gate operand is the bf16 activation (only its sign is read); gy's rows as they are stored
            call('es_spconv_fwd_bf16_io', P(gy), _C['ES_ROWS_F32' if g.form in _GY_F32 else 'ES_ROWS_BF16'], _ld(gy), wn, P(inv), n_in, n_out,
                 K, cout, cin, P(gate), 0, P(x.d), _C['ES_ROWS_BF16'], _ld(x.d), gated, P(x.g), _C['ES_ROWS_F32'], _ld(x.g), s)
        else:
            call('es_spconv_fwd_bf16_affine', P(gy), _ld(gy), wn, P(inv), n_in, n_out, K, cout, cin, P(gate), 0, P(x.d), _ld(x.d), gated,
                 P(x.g), _ld(x.g), s)
        return
    dx, acc = _grad_target(x, x.d)
    # 1x1 / stride-2 image layer (downsample.0): a row GEMM over the gradient rows only, stored to the even pixels (k_img_dgrad1_s2)
    if (IMG_STRIDED_DGRAD[0] and img is not None and K == 1 and img.stride == 2 and bf and g.form in (F32, PRE16) and dn_d is None
            and n_in == img.n_img * img.H * img.W and hip.raw('es_img_dgrad1_s2_supported')(img.n_img, img.H, img.W, cout, cin) == 1
            and hip.try_call('es_img_dgrad1_s2_bf16', P(gy), _ld(gy), P(w.bf16()[0]), img.n_img, img.H, img.W, cout, cin, P(dx), _ld(dx),
                             acc | (_C['ES_ACC_ROWS_BF16'] if g.form == PRE16 else 0), s)):
        return
    # pre-rounded rows reach an ungated data gradient only where that launch takes them (_pre16_ok, checked before they were chosen)
    assert g.form != PRE16, 'pre-rounded gradient rows were chosen for a layer whose data gradient cannot take them'
    if dn_d is not None:                         # dense engine (dense_ok)
        if _dense_launch(P(gh), cout, P(w.bf16()[0]), dn_d, 1, cin, cout, P(dx), _ld(dx), acc, gh):
            return
        if maps is not None:
            _, inv = maps.get()
    if gh is not None and _halo_ok(inv, n_in, n_out, cout, K, cout, cin) and \
            _halo_launch(P(gh), cout, P(w.bf16()[0]), inv, n_in, n_out, K, cout, cin, 0, P(dx), _ld(dx), acc):
        return
    if _is_mirror(inv):                          # gather kernels on the forward map with the taps mirrored: same bits as on the inverse
        inv, acc = inv.nbr, acc | _C['ES_ACC_MIRROR']                                                # map, which is never built
    if gh is not None or (bf and cout >= 16):    # the gather reads the shadow where there is one (contiguous rows)
        src, kind = (gy, _C['ES_ROWS_F32']) if gh is None else (gh, _C['ES_ROWS_BF16'])
        _fwd_bf16(P(src), kind, _ld(src), P(w.bf16()[0]), P(inv), n_in, n_out, K, cout, cin, 0, P(dx), _ld(dx), acc, src)
    else:
        call('es_spconv_fwd', P(gy), _ld(gy), P(w.d), P(inv), n_in, n_out, K, cout, cin, 0, P(dx), _ld(dx), 1, acc, s)


def _pre16_ok(x, w, nbr, n_in, n_out, need_dx, gate, img):
    """every backward launch of this K = 1 layer of the image backbone takes the gradient of its conv output as pre-rounded bf16 rows and
    gives the bits of the f32 rows (GRAD_ROWS_BF16).  The conditions imply the launchers' acceptance -- there is no way back to f32 rows once
    the join has written bf16: bf16 activation rows (never the small-linear weight-gradient plan, which reads f32), cout % 8 on fresh
    contiguous rows (the alignment ES_ROWS_PRE16 and the stride-2 kernel ask for), and a data gradient that is the gated K = 1 row GEMM, the
    stride-2 image kernel on a grid it supports, or absent."""
    K, cin, cout = w.d.shape
    if not (K == 1 and x.d.dtype == torch.bfloat16 and _ld(x.d) == cin and cout % 8 == 0):
        return False
    if not (need_dx and x.rg):
        return True
    if gate is not None:
        return nbr is None and n_in == n_out
    return bool(IMG_STRIDED_DGRAD[0] and img is not None and img.stride == 2 and n_in == img.n_img * img.H * img.W
                and hip.raw('es_img_dgrad1_s2_supported')(img.n_img, img.H, img.W, cout, cin) == 1)


def conv_affine(x, w, nbr, inv, n_out, scale, shift, act=1, res=None, need_dx=True, sole_consumer=False, out_bf16=False, img=None,
                res_sole=False):
    """conv -> frozen-BN affine (+ residual) (+ ReLU) of the 2-D backbone.  In bf16 mode this is ONE launch (affine
    fused into the conv epilogue); in f32 mode conv() followed by affine_act().
    sole_consumer: promise that x feeds nothing but this conv; if x itself came out of a fused conv+BN+ReLU, its
    ReLU/BN backward is then folded into this conv's data-gradient launch.
    out_bf16: store the output rows in bf16 (the image backbone's activations); x / res may themselves be bf16 row matrices.
    img: (n_img, H, W, stride) when the map is a 3x3 / pad 1 (or 1x1 / pad 0) image-grid map: the weight gradient (csrc/imgwgrad.hip) and
    the data gradient (csrc/imgconv.hip) may then run by address arithmetic instead of through the map.
    res_sole: promise that res feeds nothing but this layer (the downsample identity of a bottleneck): where res came out of a conv + BN
    without activation, the join's backward then writes the gradient of THAT conv output itself (GRAD_ROWS_BF16)."""
    K, cin, cout = w.d.shape
    n_in = x.d.shape[0]
    if PRECISION[0] != 'bf16':
        return affine_act(conv(x, w, nbr, inv, n_out, need_dx=need_dx), scale, shift, act=act, res=res)
    img = None if img is None else Img(*img)
    h16 = torch.bfloat16
    y16 = bool(out_bf16 and cout % 4 == 0)
    x16, r16 = x.d.dtype == h16, (res is not None and res.d.dtype == h16)
    y = Var(empty((n_out, cout), x.d, dtype=h16 if y16 else torch.float32))
    res_p, ldr = (P(res.d), _ld(res.d)) if res is not None else (0, 0)
    # round 6: 3x3 layers on an image grid by address arithmetic (csrc/imgconv.hip) where the library takes the shape
    ic = (img is not None and K == 9 and x16 and res is None and act in (0, 1) and cin == cout and _ld(x.d) == cin
          and hip.raw('es_img_conv3_supported')(img.n_img, img.H, img.W, cin, img.stride, 0) == 1)
    if ic and hip.try_call('es_img_conv3_bf16', P(x.d), cin, P(w.bf16()[1]), img.n_img, img.H, img.W, cin, img.stride, 0, P(scale), P(shift),
                           0, 0, act, P(y.d), int(y16), cout, _stream()):
        entry = 'es_img_conv3_bf16'             # (declined: the launcher did not take the operands -- the map kernels below)
    elif x16 or r16 or y16:                     # (int(.16): ES_ROWS_F32 / ES_ROWS_BF16)
        call('es_spconv_fwd_bf16_io', P(x.d), int(x16), _ld(x.d), P(w.bf16()[1]), P(nbr), n_out, n_in, K, cin, cout, P(scale), P(shift),
             res_p, int(r16), ldr, act, P(y.d), int(y16), cout, _stream())
        entry = 'es_spconv_fwd_bf16_io'
    else:
        call('es_spconv_fwd_bf16_affine', P(x.d), _ld(x.d), P(w.bf16()[1]), P(nbr), n_out, n_in, K, cin, cout, P(scale), P(shift), res_p,
             ldr, act, P(y.d), cout, _stream())
        entry = 'es_spconv_fwd_bf16_affine'
    if y16:
        y.dh = y.d                              # bf16 rows are their own gather shadow
    if x16:
        x.dh = x.d
    if DEBUG_FWD is not None:
        fwd_record('conv_affine', entry, x=x.d, w=w, nbr=nbr, n_out=n_out, round=True, scale=scale, shift=shift,
                   res=res.d if res is not None else None, act=act, y=y.d)

    if act == 1 and res is None:
        y.gate = scale
    gate = x.gate if sole_consumer else None
    if act == 0 and res is None and y16 and TAPE.enabled and _pre16_ok(x, w, nbr, n_in, n_out, need_dx, gate, img):
        y.fold = scale

    def bwd():
        if y.g is None:
            return
        if DEBUG_GRADS is not None:
            DEBUG_GRADS[id(y)] = y.g.clone()
        if y.gated:                             # the consumer's launch already applied mask and scale (a gated dgrad; a join: bf16 rows)
            gconv = y.g
        else:
            # residual joins of the image backbone (conv3 + bn3 + identity -> ReLU, bf16 activations): both readers of the conv-output
            # gradient -- conv3's gated K = 1 data gradient and its weight gradient -- round it to bf16 on load, so it is written in
            # bf16 here (GRAD_ROWS_BF16; same es_pack_bf16, the gradients keep their bits).  Other layers: f32 rows as before.
            rows16 = (GRAD_ROWS_BF16[0] and res is not None and y.d.dtype == h16 and act in (0, 1) and not _f32_grad_rows_wanted()
                      and _pre16_ok(x, w, nbr, n_in, n_out, need_dx, gate, img))
            # ... and on a downsample block, where the identity is a conv + BN output nothing else reads, the gradient of that conv
            # output too (dz * its fold, what its own act = 0 backward launch would make of an f32 dres): no dres, no such launch
            two = rows16 and res_sole and res.fold is not None and res.rg and res.g is None and res.d.shape == y.d.shape
            gconv = torch.empty((n_out, cout), dtype=h16 if rows16 else torch.float32, device=y.d.device)   # gradient w.r.t. the conv output
            if two:
                res.g, res.gated = torch.empty((n_out, cout), dtype=h16, device=y.d.device), True
                call('es_affine_act_bwd_yh_xh2', P(y.g), P(y.d), P(scale), P(res.fold), n_out, cout, act, P(gconv), P(res.g), _stream())
            else:
                gr, accr = _grad_ptr(res)
                if rows16:
                    call('es_affine_act_bwd_yh_xh', P(y.g), P(y.d), P(scale), n_out, cout, act, P(gconv), gr, accr, _stream())
                else:
                    call('es_affine_act_bwd_yh' if y.d.dtype == h16 else 'es_affine_act_bwd', P(y.g), P(y.d), P(scale), n_out, cout,
                         act, P(gconv), 0, gr, accr, _stream())
        _conv_backward(x, w, nbr, inv, n_out, y, gconv, None, 0, need_dx, True, gate, img=img, pre16=gconv.dtype == h16)
    TAPE.add(bwd)
    return y


def gen_conv_transpose(x, w):
    """MinkowskiGenerativeConvolutionTranspose(k=2,s=2): y[8i+k] = x[i] @ w[k]; 8 row GEMMs into the
    (N, 8*Cout) view of the output."""
    K, cin, cout = w.d.shape
    n = x.d.shape[0]
    y = Var(empty((n * 8, cout), x.d))
    s = _stream()
    bf = PRECISION[0] == 'bf16'
    fused = (bf and GEN_FUSED[0] and x.d.dtype == torch.float32      # all eight taps in one launch (declined: the per-tap launches)
             and hip.try_call('es_gen_transpose_fwd_bf16', P(x.d), _ld(x.d), P(w.bf16()[1]), n, cin, cout, P(y.d), s))
    for k in range(0 if not fused else 8, 8):
        if bf:
            call('es_spconv_fwd_bf16', P(x.d), 0, _ld(x.d), w.bf16()[1].data_ptr() + 2 * k * cin * cout, 0, n, n, 1, cin,
                 cout, 0, y.d.data_ptr() + 4 * k * cout, 8 * cout, 0, s)
        else:
            call('es_spconv_fwd', P(x.d), _ld(x.d), w.d.data_ptr() + 4 * k * cin * cout, 0, n, n, 1, cin, cout, 0,
                 y.d.data_ptr() + 4 * k * cout, 8 * cout, 0, 0, s)
    if DEBUG_FWD is not None:
        fwd_record('gen_transpose', 'es_gen_transpose_fwd_bf16' if fused else ('es_spconv_fwd_bf16' if bf else 'es_spconv_fwd'),
                   x=x.d, w=w, round=bf, y=y.d)

    def bwd():
        if y.g is None:
            return
        s = _stream()
        recs = None
        if DEBUG_CONV is not None:                     # the 8 taps as 8 identity-map K = 1 records sharing one data gradient
            before = x.g.clone() if (x.rg and x.g is not None) else None
            recs = [dict(x=x.d, w=ParamSlice(w, k), nbr=None, n_out=n, gy=y.g.view(n, 8, cout)[:, k].clone(), bf=bool(bf), gate=None,
                         need_dx=bool(x.rg), before=before, bias=None, bias_from=0, group=id(y), group_size=8) for k in range(8)]
            DEBUG_CONV.extend(recs)
        g, acc = _grad_target(x, x.d) if x.rg else (None, 0)
        sw = _wgrad_stream(y.g, x.d) if w.g is not None else s
        dfused = (g is not None and bf and GEN_FUSED[0] and y.g.is_contiguous()      # (n * 8, cout) rows = (n, 8 cout)
                  and hip.try_call('es_gen_transpose_dgrad_bf16', P(y.g), P(w.bf16()[0]), n, cin, cout, P(g), _ld(g), acc, s))
        wfused = False
        slots = [w.g.data_ptr() + 4 * k * cin * cout for k in range(8)] if w.g is not None else []
        if (w.g is not None and bf and GEN_FUSED[0] and HEAD_BWD_FUSED[0] and y.g.is_contiguous() and x.d.dtype == torch.float32
                and len({_written(q) for q in slots}) == 1):        # all eight taps' weight gradients in one launch
            need = hip.raw('es_gen_transpose_wgrad_workspace_floats')(P(x.d), _ld(x.d), P(y.g), n, cin, cout)
            ws, nf = stream_ws(sw, 'wgrad', need, y.g) if need else (None, 0)
            wfused = hip.try_call('es_gen_transpose_wgrad_bf16', P(x.d), _ld(x.d), P(y.g), n, cin, cout, P(w.g), _written(slots[0]), P(ws),
                                  nf, sw)                           # (declined: nothing launched -- the per-tap launches)
            if wfused:
                for q in slots:
                    _first_write(q)
        for k in range(8):
            gy = y.g.data_ptr() + 4 * k * cout
            if w.g is not None and not wfused:
                _wgrad('es_spconv_wgrad_bf16' if bf else 'es_spconv_wgrad', sw,
                       w.g.data_ptr() + 4 * k * cin * cout, P(x.d), _ld(x.d), gy, 8 * cout, 0, n, n, 1, cin, cout, like=y.g)
            if dfused:
                continue
            if g is not None and bf:
                call('es_spconv_fwd_bf16', gy, 0, 8 * cout, w.bf16()[0].data_ptr() + 2 * k * cin * cout, 0, n, n, 1, cout,
                     cin, 0, P(g), _ld(g), 1 if (acc or k > 0) else 0, s)
            elif g is not None:
                call('es_spconv_fwd', gy, 8 * cout, w.d.data_ptr() + 4 * k * cin * cout, 0, n, n, 1, cout, cin, 0,
                     P(g), _ld(g), 1, 1 if (acc or k > 0) else 0, s)
        if recs is not None and x.rg:
            recs[-1]['after'] = x.g.clone()          # (after all eight taps)
    TAPE.add(bwd)
    return y


def _required(taken):
    if not taken:
        raise hip.HipError('the dense engine did not take the operands of a launch that has no other path (status -4)')


def conv_transpose_dense(x, w, dense):
    """nn.ConvTranspose3d(k=2, s=2) on a dense (B, X, Y, Z) grid (dense = (B, X, Y, Z, 2, 2, 0)): y (B*2X*2Y*2Z, Cout) in DENSE row order
    by the parity-class launch of the dense engine (csrc/dconv.hip mode 3) -- no generative-layout intermediate, no row permutation;
    backward: data gradient (mode 4: 8 taps gathered at 2 r + p) and weight gradient (mode 5).  Caller checks dense_ok(dense, 3 / 4 / 5)."""
    K, cin, cout = w.d.shape
    n = x.d.shape[0]
    y = Var(empty((n * 8, cout), x.d))
    _required(_dense_launch(P(x.shadow()), cin, P(w.bf16()[1]), dense, 3, cin, cout, P(y.d), cout, 0, x.d))
    if DEBUG_FWD is not None:
        fwd_record('transpose_dense', 'es_dconv_fwd_bf16', x=x.d, xh=x.dh, w=w, dense=tuple(dense), round=True, y=y.d)

    def bwd():
        if y.g is None:
            return
        gh = y.grad_shadow()
        rec_before = x.g.clone() if (DEBUG_CONV is not None and x.rg and x.g is not None) else None
        if w.g is not None:
            x.shadow()
            sw = _wgrad_stream(y.g, x.d, gh, x.dh)
            _required(_dense_wgrad(P(x.dh), cin, P(gh), cout, dense, 1, cin, cout, P(w.g), _first_write(P(w.g)), sw, gh))
        if x.rg:
            g, acc = _grad_target(x, x.d)
            _required(_dense_launch(P(gh), cout, P(w.bf16()[0]), dense, 4, cin, cout, P(g), _ld(g), acc, gh))
        if DEBUG_CONV is not None:                     # the 8 taps as 8 identity-map K = 1 records sharing one data gradient (as gen_conv_transpose)
            B, X, Y, Z = dense[:4]
            gv = y.g.view(B, X, 2, Y, 2, Z, 2, cout)
            recs = [dict(x=x.d, w=ParamSlice(w, k), nbr=None, n_out=n, gy=gv[:, :, k >> 2, :, (k >> 1) & 1, :, k & 1].reshape(n, cout).clone(),
                         bf=True, gate=None, need_dx=bool(x.rg), before=rec_before, bias=None, bias_from=0, group=id(y), group_size=8)
                    for k in range(8)]
            if x.rg:
                recs[-1]['after'] = x.g.clone()
            DEBUG_CONV.extend(recs)
    TAPE.add(bwd)
    return y


# ------------------------------------------------------------------ norms
def norm(x, weight, bias, seg_off, eps, act=0, res=None, running=None, momentum=0.1):
    """Train-mode batch norm (seg_off=[0,N]) / instance norm (seg_off=batch offsets) with fused
    residual add and activation (0 none, 1 ReLU, 2 ELU)."""
    n, C = x.d.shape
    nseg = len(seg_off) - 1
    so = iarr(seg_off)
    ws_n = hip.raw('es_norm_workspace_floats')(n, C, so, nseg) + 2 * nseg * C
    ws = empty((ws_n,), x.d)
    mean, invstd = empty((nseg, C), x.d), empty((nseg, C), x.d)
    y = Var(empty((n, C), x.d))
    rm, rv = (running if running is not None else (None, None))
    # bf16 mode: the apply passes also write the bf16 gather shadows their consumers would otherwise make with a cast launch
    # each (forward: of y, for the next convolution; backward: of the gradient handed to the producing convolution, when this
    # norm is that Var's only consumer) -- bit-identical to the casts they replace
    fuse = PRECISION[0] == 'bf16' and C >= 16 and C % 8 == 0
    private, x.fresh = bool(x.fresh), False
    if fuse:
        y.dh = empty((n, C), x.d, dtype=torch.bfloat16)
    run0 = (rm.clone(), rv.clone()) if (DEBUG_FWD is not None and rm is not None) else (None, None)
    call('es_norm_fwd', P(x.d), _ld(x.d), n, C, so, nseg, float(eps), P(weight.d), P(bias.d),
         P(res.d) if res is not None else 0, _ld(res.d) if res is not None else 0, act, P(rm), P(rv), float(momentum),
         P(mean), P(invstd), P(ws), P(y.d), C, P(y.dh) if fuse else 0, _stream())
    if DEBUG_FWD is not None:
        fwd_record('norm', 'es_norm_fwd', x=x.d, w=weight.d, b=bias.d, seg_off=list(seg_off), eps=float(eps), act=act,
                   res=res.d if res is not None else None, rm0=run0[0], rv0=run0[1], rm1=rm, rv1=rv, momentum=float(momentum),
                   mean=mean, invstd=invstd, y=y.d, yh=y.dh if fuse else None)

    def bwd():
        if y.g is None:
            return
        s = _stream()
        if DEBUG_GRADS is not None:
            DEBUG_GRADS[id(y)] = y.g.clone()
        ws2 = empty((ws_n,), x.d)
        if GRAD_ROWS_BF16[0] and fuse and private and x.gsh and x.g is None and not _f32_grad_rows_wanted():
            # the producing convolution's backward gathers the shadow only: no f32 rows (GRAD_ROWS_BF16)
            x.g = gh = empty((n, C), x.d, dtype=torch.bfloat16)
            g, ldg, acc = None, C, 0
        else:
            g, acc = _grad_target(x, x.d)
            ldg = _ld(g)
            gh = empty((n, C), x.d, dtype=torch.bfloat16) if (fuse and private and ldg == C) else None
        call('es_norm_bwd', P(y.g), _ld(y.g), P(y.d), C, P(x.d), _ld(x.d), n, C, so, nseg, P(mean), P(invstd),
             P(weight.d), act, P(weight.g), P(bias.g), P(ws2), P(g), ldg, acc, P(gh), s)
        x.gh = gh
        if DEBUG_GRADS is not None:
            DEBUG_GRADS[('norm', id(y))] = dict(dx=g.clone(), dz=y.g.clone(), mean=mean.clone(), invstd=invstd.clone(),
                                                x=x.d.clone(), yd=y.d.clone(), acc=acc, n=n, C=C, act=act)
        if res is not None and res.rg:          # y.g now holds dz == gradient of the residual input
            _grad_give(res, y.g)
    TAPE.add(bwd)
    return y


def affine_act(x, scale, shift, act=1, res=None, need_dx=True):
    """frozen-BN affine (+residual) (+ReLU) for the 2-D backbone."""
    n, C = x.d.shape
    y = Var(empty((n, C), x.d))
    call('es_affine_act_fwd', P(x.d), P(scale), P(shift), P(res.d) if res is not None else 0, n, C, act, P(y.d),
         _stream())
    if DEBUG_FWD is not None:
        fwd_record('affine_act', 'es_affine_act_fwd', x=x.d, scale=scale, shift=shift, res=res.d if res is not None else None,
                   act=act, y=y.d)

    def bwd():
        if y.g is None:
            return
        (gx, accx), (gr, accr) = _grad_ptr(x if need_dx else None), _grad_ptr(res)
        if gx or gr:
            call('es_affine_act_bwd', P(y.g), P(y.d), P(scale), n, C, act, gx, accx, gr, accr, _stream())
    TAPE.add(bwd)
    return y


# ------------------------------------------------------------------ pooling / row moves
def maxpool(x, nbr, n_out, need_dx=True):
    C = x.d.shape[1]
    K = nbr.shape[1]
    y = Var(empty((n_out, C), x.d))
    arg = empty((n_out, C), x.d, torch.int32)
    call('es_maxpool_fwd', P(x.d), _ld(x.d), P(nbr), n_out, K, C, P(y.d), P(arg), _stream())
    if DEBUG_FWD is not None:
        fwd_record('maxpool', 'es_maxpool_fwd', x=x.d, nbr=nbr, y=y.d, arg=arg)

    def bwd():
        if y.g is None or not (need_dx and x.rg):
            return
        if x.g is None:
            x.g = torch.zeros_like(x.d)
        call('es_maxpool_bwd', P(y.g), P(arg), n_out, C, P(x.g), _ld(x.g), _stream())
    TAPE.add(bwd)
    return y


def gather_rows(x, idx):
    """y = x[idx] (MinkowskiPruning with idx = kept rows)."""
    n, C = idx.shape[0], x.d.shape[1]
    y = Var(empty((n, C), x.d))
    call('es_row_move', P(y.d), C, P(x.d), _ld(x.d), P(idx), n, C, 0, _stream())

    def bwd():
        if y.g is None or not x.rg:
            return
        if x.g is None:
            x.g = torch.zeros_like(x.d)
        call('es_row_move', P(x.g), _ld(x.g), P(y.g), _ld(y.g), P(idx), n, C, 1, _stream())
    TAPE.add(bwd)
    return y


def gather_rows_shared(x, idx, P_, Q, r0=0, L=None):
    """y (P_*Q, C) = x[r0 + idx] for P_ prompts' (P_, Q) int32 row choices among ONE scene's rows [r0, r0 + L) of x (default: all of x):
    different prompts select overlapping rows, so the backward is es_rows_scatter_sum (per row the prompts' gradients added in ascending
    prompt order, no atomics) instead of es_row_move's plain `+=`.  The indices of one prompt must be distinct (es_topk_sorted
    guarantees it)."""
    C = x.d.shape[1]
    L = x.d.shape[0] - r0 if L is None else L
    n = P_ * Q
    assert idx.dtype == torch.int32 and idx.numel() == n and idx.is_contiguous() and 0 <= r0 and r0 + L <= x.d.shape[0]
    y = Var(empty((n, C), x.d))
    xs = x.d[r0:r0 + L]
    call('es_row_move', P(y.d), C, P(xs), _ld(x.d), P(idx), n, C, 0, _stream())

    def bwd():
        if y.g is None or not x.rg:
            return
        if x.g is None:
            x.g = torch.zeros_like(x.d)         # (the scenes of a batch write disjoint row ranges; rows between them stay zero)
        x.gh = None
        g = x.g[r0:r0 + L]
        nws = int(hip.raw('es_rows_scatter_sum_workspace_ints')(P_, L))
        ws = torch.empty(max(nws, 1), dtype=torch.int32, device=x.d.device)
        rec = None
        if DEBUG_OPS is not None:
            rec = dict(kind='scatter_sum', dy=y.g.clone(), idx=idx.clone(), P=P_, Q=Q, L=L, C=C, acc=1, dx0=g.clone())
            DEBUG_OPS.append(rec)
        call('es_rows_scatter_sum', P(y.g), _ld(y.g), P(idx), P_, Q, L, C, P(g), _ld(g), 1, P(ws), nws, _stream())
        if rec is not None:
            rec['dx1'] = g.clone()
    TAPE.add(bwd)
    return y


def concat_rows(vs):
    """the rows of the Vars `vs` (same width) one after the other; each input's gradient is its row range of the result's"""
    if len(vs) == 1:
        return vs[0]
    y = Var(torch.cat([v.d for v in vs]))
    offs = [0]
    for v in vs:
        offs.append(offs[-1] + v.d.shape[0])

    def bwd():
        if y.g is None:
            return
        for i, v in enumerate(vs):
            if v.rg:
                _grad_give(v, y.g[offs[i]:offs[i + 1]])
    TAPE.add(bwd)
    return y


def union_add(a, b, pos_a, pos_b, n):
    """sparse a + b on the coordinate union (rows pos_a / pos_b of the result)."""
    C = a.d.shape[1]
    y = Var(zeros((n, C), a.d))
    s = _stream()
    call('es_row_move', P(y.d), C, P(a.d), _ld(a.d), P(pos_a), a.d.shape[0], C, 2, s)
    call('es_row_move', P(y.d), C, P(b.d), _ld(b.d), P(pos_b), b.d.shape[0], C, 1, s)

    def bwd():
        if y.g is None:
            return
        s = _stream()
        for v, pos in ((a, pos_a), (b, pos_b)):
            if not v.rg:
                continue
            m = v.d.shape[0]
            t = empty((m, C), a.d)
            call('es_row_move', P(t), C, P(y.g), _ld(y.g), P(pos), m, C, 0, s)
            _grad_give(v, t)
    TAPE.add(bwd)
    return y


def copy_cols(dst, col, src):
    """dst[:, col:col+C] = src (raw tensors)."""
    n, C = src.shape
    call('es_axpy2d', dst.data_ptr() + 4 * col, dst.stride(0), P(src), src.stride(0), n, C, 1.0, 0, _stream())


def add_into(dst, src):
    n, C = src.shape
    call('es_axpy2d', P(dst), dst.stride(0), P(src), src.stride(0), n, C, 1.0, 1, _stream())


def add(a, b):
    """y = a + b of two row matrices of the same shape (dense residual / lateral sums)."""
    n, C = a.d.shape
    y = Var(empty((n, C), a.d))
    s = _stream()
    call('es_axpy2d', P(y.d), C, P(a.d), _ld(a.d), n, C, 1.0, 0, s)
    call('es_axpy2d', P(y.d), C, P(b.d), _ld(b.d), n, C, 1.0, 1, s)

    def bwd():
        if y.g is None:
            return
        for v in (a, b):
            if v.rg:
                _grad_give(v, y.g, alias=v is a and not b.rg)         # (y.g serves one input at most: later consumers add into theirs)
    TAPE.add(bwd)
    return y


def upsample_add_(fine, coarse, n_img, Hf, Wf, Hc, Wc):
    """mmdet.FPN top-down step, in place: fine += nearest_upsample(coarse, size=(Hf, Wf)).  `fine` keeps its identity
    (its producer's backward sees the same gradient); the gradient reaching `coarse` is accumulated when the tape passes
    this point, i.e. after every later consumer of `fine` has contributed."""
    C = fine.d.shape[1]
    call('es_upsample_nearest_add_fwd', P(fine.d), P(coarse.d), n_img, Hf, Wf, Hc, Wc, C, _stream())

    def bwd():
        if fine.g is None or not coarse.rg:
            return
        g, acc = _grad_target(coarse, coarse.d)
        call('es_upsample_nearest_add_bwd', P(fine.g), P(g), n_img, Hf, Wf, Hc, Wc, C, acc, _stream())
    TAPE.add(bwd)
    return fine


# ------------------------------------------------------------------ transformer operators (grounding decoder, A19)
class ParamSlice:
    """tap j of a (K, Cin, Cout) Param as a (1, Cin, Cout) kernel of its own (the q / k / v blocks of an attention
    in-projection): shares storage, gradient and the parent's bf16 copies"""
    __slots__ = ('parent', 'j', 'd', 'g')

    def __init__(self, parent, j):
        self.parent, self.j = parent, j
        self.d = parent.d[j:j + 1]
        self.g = parent.g[j:j + 1] if parent.g is not None else None

    def bf16(self):
        n, t = self.parent.bf16()
        return n[self.j:self.j + 1], t[self.j:self.j + 1]


def linear(x, w, b=None, need_dx=True):
    """y = x @ W + b as a row GEMM on the convolution engine (w: Param / ParamSlice (1, Cin, Cout))"""
    return conv(x, w, None, None, x.d.shape[0], bias=b, need_dx=need_dx)


def relu_(x):
    """in-place ReLU on x.d; the gradient of x is masked in place when the tape passes here"""
    call('es_relu_fwd', P(x.d), x.d.numel(), _stream())

    def bwd():
        if x.g is not None:
            call('es_relu_bwd', P(x.g), P(x.d), x.d.numel(), _stream())
    TAPE.add(bwd)
    return x


def layernorm(x, w, b, res=None, eps=1e-5):
    """y = LayerNorm(x (+ res)) over channels; w, b: Params (C,)"""
    n, C = x.d.shape
    assert x.d.is_contiguous() and (res is None or res.d.is_contiguous())
    y = Var(empty((n, C), x.d))
    z = empty((n, C), x.d) if res is not None else x.d
    mean, rstd = empty((n,), x.d), empty((n,), x.d)
    call('es_layernorm_fwd', P(x.d), P(res.d) if res is not None else 0, n, C, P(w.d), P(b.d), float(eps), P(y.d),
         P(z) if res is not None else 0, P(mean), P(rstd), _stream())
    if DEBUG_FWD is not None:
        fwd_record('layernorm', 'es_layernorm_fwd', x=x.d, res=res.d if res is not None else None, w=w.d, b=b.d, eps=float(eps), y=y.d,
                   z=z if res is not None else None, mean=mean, rstd=rstd)

    def bwd():
        if y.g is None:
            return
        s = _stream()
        tgt = [v for v in ((x, res) if res is not None else (x,)) if v.rg]
        dz = torch.empty_like(y.d)
        ws, nws = ticket_ws(hip.raw('es_layernorm_bwd_workspace_floats')(n, C), y.d)
        rec = None
        if DEBUG_OPS is not None:
            rec = dict(kind='ln', dy=y.g.clone(), z=z.clone(), w=w.d.clone(), mean=mean.clone(), rstd=rstd.clone(), n=n, C=C,
                       wp=w, bp=b, dw0=w.g.clone(), db0=b.g.clone())
            DEBUG_OPS.append(rec)
        call('es_layernorm_bwd', P(y.g), P(z), n, C, P(w.d), P(mean), P(rstd), P(dz), 0, P(w.g), P(b.g), P(ws), nws, s)
        if rec is not None:
            rec.update(dz=dz.clone(), dw1=w.g.clone(), db1=b.g.clone())
        owned = False                            # dz may be handed to exactly one input as its gradient buffer
        for v in tgt:
            owned |= _grad_give(v, dz, alias=not owned)
    TAPE.add(bwd)
    return y


def attention(q, k, v, B, H, Lq, Lk, klen=None):
    """softmax(q k^T / sqrt(32)) v per (sample, head); q (B*Lq, H*32), k / v (B*Lk, H*32) projected row matrices (Vars,
    possibly column slices of wider buffers); klen: device int32 (B,) valid key counts or None"""
    bf = 1 if PRECISION[0] == 'bf16' else 0
    o = Var(empty((B * Lq, H * 32), q.d))
    lse = empty((B * H * Lq,), q.d)
    call('es_attn_fwd', P(q.d), _ld(q.d), P(k.d), _ld(k.d), P(v.d), _ld(v.d), B, H, Lq, Lk, P(klen), P(o.d), H * 32, P(lse), bf,
         _stream())
    if DEBUG_FWD is not None:
        fwd_record('attention', 'es_attn_fwd', q=q.d, k=k.d, v=v.d, B=B, H=H, Lq=Lq, Lk=Lk, klen=klen, bf=bf, o=o.d, lse=lse)

    def bwd():
        if o.g is None:
            return
        delta = empty((B * H * Lq,), q.d)
        gs = []
        for t in (q, k, v):
            if t.g is None:
                t.g = torch.empty_like(t.d)
                gs.append(0)
            else:
                gs.append(1)
        assert gs[0] == gs[1] == gs[2], 'attention inputs must be fresh projections (single consumer)'
        rec = None
        if DEBUG_OPS is not None:
            rec = dict(kind='attn', q=q.d.clone(), k=k.d.clone(), v=v.d.clone(), o=o.d.clone(), do=o.g.clone(), lse=lse.clone(),
                       klen=None if klen is None else klen.clone(), B=B, H=H, Lq=Lq, Lk=Lk, bf=bf, acc=gs[0],
                       before=[t.g.clone() for t in (q, k, v)] if gs[0] else None)
            DEBUG_OPS.append(rec)
        call('es_attn_bwd', P(q.d), _ld(q.d), P(k.d), _ld(k.d), P(v.d), _ld(v.d), P(o.d), H * 32, P(o.g), _ld(o.g), P(lse), B, H,
             Lq, Lk, P(klen), P(delta), P(q.g), _ld(q.g), P(k.g), _ld(k.g), P(v.g), _ld(v.g), gs[0], bf, _stream())
        if rec is not None:
            rec.update(delta=delta.clone(), dq=q.g.clone(), dk=k.g.clone(), dv=v.g.clone())
    TAPE.add(bwd)
    return o


# ---- one scene, many prompts: forward only for SparseFeatureFusion3DGrounder.ground (nothing on the tape), taped for loss_shared
# backward of the taped attention_kv: es_attn_kv_bwd (the query side converted once per call, the workgroup's key tile resident) or
# es_attn_bwd with B = 1 -- the same function (A/B switch; the default follows the decision in DESIGN section 3c, tools/bench_shared_train.py)
ATTN_KV_BWD = _switch('ES_ATTN_KV_BWD')


class PreparedKV:
    """the projected keys / values of one cross-attention layer in the operand image es_attn_kv_fwd consumes (csrc/transformer.hip),
    built once per scene; k / v: the f32 projections, kept only when DEBUG_FWD was set at build time (the forward record needs them).
    Taped form (attention_kv_prepare(..., src=...)): kvar / vvar are the projection Vars the scene's rows [r0, r0 + Lk) were taken from
    and `group` the state the scenes of one layer share (their gradient buffers are made once, by whichever scene's backward runs first)"""
    __slots__ = ('kv', 'H', 'Lk', 'bf', 'k', 'v', 'kvar', 'vvar', 'r0', 'group')


def attention_kv_prepare(k, v, H, Lk, src=None):
    """k / v: Vars (Lk, H*32), the projected point tokens of one scene -> PreparedKV in the precision of the current mode.
    src = (kvar, vvar, r0, group): k / v are rows [r0, r0 + Lk) of these projection Vars (several scenes' padded rows), which receive the
    gradients of a taped attention_kv; group: a dict shared by the scenes of one layer"""
    bf = 1 if PRECISION[0] == 'bf16' else 0
    pk = PreparedKV()
    pk.H, pk.Lk, pk.bf = H, Lk, bf
    pk.kv = torch.empty(int(hip.raw('es_attn_kv_bytes')(H, Lk, bf)), dtype=torch.uint8, device=k.d.device)
    call('es_attn_kv_prepare', P(k.d), _ld(k.d), P(v.d), _ld(v.d), H, Lk, bf, P(pk.kv), _stream())
    pk.k, pk.v = (k.d, v.d) if (DEBUG_FWD is not None or src is not None) else (None, None)
    pk.kvar, pk.vvar, pk.r0, pk.group = src if src is not None else (None, None, 0, None)
    return pk


def attention_kv(q, pk, Lq):
    """softmax(q k^T / sqrt(32)) v per head of Lq query rows (any number of prompts' queries) over the ONE prepared key / value set.
    pk may be a list of PreparedKV, one per scene: q then holds Lq rows per scene, scene after scene, and each block attends to its own
    scene.  With the tape on, a q that requires a gradient and PreparedKVs that kept their projection Vars, the backward is recorded: dQ
    and each scene's rows of dK / dV by es_attn_kv_bwd (ATTN_KV_BWD off: es_attn_bwd with B = 1) on the f32 projections, same rounding
    points as the forward."""
    pks = list(pk) if isinstance(pk, (list, tuple)) else [pk]
    H = pks[0].H
    n = len(pks) * Lq
    taped = TAPE.enabled and q.rg and all(k_.kvar is not None for k_ in pks)
    o = Var(empty((n, H * 32), q.d), rg=taped)
    lse = empty((len(pks), H * Lq), q.d)
    for s_, k_ in enumerate(pks):
        qs, os_ = q.d[s_ * Lq:(s_ + 1) * Lq], o.d[s_ * Lq:(s_ + 1) * Lq]
        call('es_attn_kv_fwd', P(qs), _ld(q.d), P(k_.kv), H, Lq, k_.Lk, P(os_), H * 32, P(lse[s_]), k_.bf, _stream())
        if DEBUG_FWD is not None:
            if k_.k is None:
                raise RuntimeError('DEBUG_FWD: this scene encoding was built without it (the record needs the f32 projections): rebuild it')
            fwd_record('attention', 'es_attn_kv_fwd', q=qs, k=k_.k, v=k_.v, B=1, H=H, Lq=Lq, Lk=k_.Lk, klen=None, bf=k_.bf, o=os_, lse=lse[s_])
    if not taped:
        return o

    def bwd():
        if o.g is None:
            return
        assert q.g is None, 'attention_kv: q must be a fresh projection (single consumer)'
        q.g = torch.empty_like(q.d)
        delta = empty((len(pks), H * Lq), q.d)
        for s_, k_ in enumerate(pks):
            kvar, vvar, r0, group, Lk = k_.kvar, k_.vvar, k_.r0, k_.group, k_.Lk
            if not group.get('made'):
                # the scenes of a layer write disjoint row ranges of the projections' gradients; the padded rows between them stay zero
                assert kvar.g is None and vvar.g is None, 'attention_kv: k / v must be fresh projections (single consumer)'
                kvar.g, vvar.g = torch.zeros_like(kvar.d), torch.zeros_like(vvar.d)
                kvar.gh = vvar.gh = None
                group['made'] = True
            sl = slice(s_ * Lq, (s_ + 1) * Lq)
            qs, os_, dos, dq = q.d[sl], o.d[sl], o.g[sl], q.g[sl]
            dk, dv = kvar.g[r0:r0 + Lk], vvar.g[r0:r0 + Lk]
            rec = None
            if DEBUG_OPS is not None:
                rec = dict(kind='attn', q=qs.clone(), k=k_.k.clone(), v=k_.v.clone(), o=os_.clone(), do=dos.clone(), lse=lse[s_].clone(),
                           klen=None, B=1, H=H, Lq=Lq, Lk=Lk, bf=k_.bf, acc=0, before=None, shared=True,
                           entry='es_attn_kv_bwd' if ATTN_KV_BWD[0] else 'es_attn_bwd')
                DEBUG_OPS.append(rec)
            if ATTN_KV_BWD[0]:
                nws = int(hip.raw('es_attn_kv_bwd_workspace_bytes')(H, Lq, k_.bf))
                ws = torch.empty(nws, dtype=torch.uint8, device=q.d.device)
                call('es_attn_kv_bwd', P(qs), _ld(q.d), P(k_.k), _ld(k_.k), P(k_.v), _ld(k_.v), P(os_), H * 32, P(dos), _ld(o.g), P(lse[s_]), H,
                     Lq, Lk, P(delta[s_]), P(ws), nws, P(dq), _ld(q.g), P(dk), _ld(kvar.g), P(dv), _ld(vvar.g), 0, k_.bf, _stream())
            else:
                call('es_attn_bwd', P(qs), _ld(q.d), P(k_.k), _ld(k_.k), P(k_.v), _ld(k_.v), P(os_), H * 32, P(dos), _ld(o.g), P(lse[s_]), 1, H,
                     Lq, Lk, 0, P(delta[s_]), P(dq), _ld(q.g), P(dk), _ld(kvar.g), P(dv), _ld(vvar.g), 0, k_.bf, _stream())
            if rec is not None:
                rec.update(delta=delta[s_].clone(), dq=dq.clone(), dk=dk.clone(), dv=dv.clone())
    TAPE.add(bwd)
    return o


def contrastive_shared(v, L, text, n_prompts, T, tlen, bias, want_logits=False, want_max=True):
    """ContrastiveEmbed of one scene's rows v (L, C) against n_prompts text blocks (n_prompts*T, C) -> (logits (n_prompts*L, T) or None,
    rowmax (n_prompts*L,) or None); raw tensors"""
    C = v.shape[1]
    logits = torch.empty((n_prompts * L, T), dtype=torch.float32, device=v.device) if want_logits else None
    rowmax = torch.empty(n_prompts * L, dtype=torch.float32, device=v.device) if want_max else None
    call('es_contrastive_shared_fwd', P(v), L, P(text), n_prompts, T, C, P(tlen), P(bias), P(logits), T, P(rowmax), _stream())
    if DEBUG_FWD is not None:                    # the replicated reading: what es_contrastive_fwd computes on n_prompts copies of the rows
        fwd_record('contrastive', 'es_contrastive_shared_fwd', v=v.repeat(n_prompts, 1), text=text, B=n_prompts, L=L, T=T, tlen=tlen,
                   vlen=None, bias=bias, logits=logits, rowmax=rowmax)
    return logits, rowmax
