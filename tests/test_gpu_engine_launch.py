"""The engine's launch door and gradient hand-over on small operands (bodies written once, taking a device; tests/test_emu_engine_launch.py
runs them on the CPU emulator):
 - gen_conv_transpose in bf16 mode asks the fused entry points through hip.try_call: a declined direction (ES_GEN_DECLINED) is followed by
   the eight per-tap launches and gives the bits of the GEN_FUSED = off step; a served one is the fused launch alone; any other status raises
   and nothing further is queued;
 - add / concat_rows / union_add / layernorm(res) / norm(res) hand their gradient over through one helper: a bf16 .g is refused ("second
   consumer"), a stale .gh is dropped, the gradient is the handed tensor itself or g0 + it, bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _bits(t):
    return t.contiguous().view(torch.int32)


def _conv_param(dev, d, g):
    """a (K, Cin, Cout) Param on dev with current bf16 copies (one es_cast_weight_bf16 launch: the registry of the one-launch cast is keyed by
    CUDA devices)"""
    from embodiedscan_amd import engine as E, hip
    p = E.Param(d.to(dev), g.to(dev))
    K, a, b = d.shape
    p.bf_n, p.bf_t = (torch.empty(s, dtype=torch.bfloat16, device=dev) for s in ((K, a, b), (K, b, a)))
    hip.call('es_cast_weight_bf16', hip.P(p.d), K, a, b, hip.P(p.bf_n), hip.P(p.bf_t), hip.stream())
    p.bf_step = E.WEIGHT_VERSION[0]
    return p


class _Recorder:
    """names of everything that goes through engine.call / hip.try_call (a declined try_call as '<name> refused')"""

    def __enter__(self):
        from embodiedscan_amd import engine as E
        self.E, self.names, self.real = E, [], (E.call, E.hip.try_call)
        real_call, real_try = self.real

        def call(fn, *args):
            self.names.append(fn)
            return real_call(fn, *args)

        def try_call(fn, *args):
            ok = real_try(fn, *args)
            self.names.append(fn if ok else fn + ' refused')
            return ok
        E.call, E.hip.try_call = call, try_call
        return self.names

    def __exit__(self, *exc):
        self.E.call, self.E.hip.try_call = self.real


def _gen_step(dev, cin, cout, fused, n=5):
    from embodiedscan_amd import engine as E
    g = torch.Generator().manual_seed(100 * cin + cout)
    x = E.Var(torch.randn(n, cin, generator=g).to(dev))
    w = _conv_param(dev, torch.randn(8, cin, cout, generator=g) / cin ** 0.5, torch.zeros(8, cin, cout))
    dy = torch.randn(8 * n, cout, generator=g).to(dev)
    old = E.PRECISION[0], E.GEN_FUSED[0]
    E.PRECISION[0], E.GEN_FUSED[0] = 'bf16', fused
    E.TAPE.clear()
    E.new_grad_epoch()
    try:
        with _Recorder() as fwd:
            y = E.gen_conv_transpose(x, w)
        y.g = dy
        with _Recorder() as bwd:
            E.TAPE.backward()
    finally:
        E.PRECISION[0], E.GEN_FUSED[0] = old
    return fwd, bwd, dict(y=y.d.clone(), dx=x.g.clone(), dw=w.g.clone())


def gen_transpose_door_case(dev, cin, cout, fwd_served, dgrad_served):
    f0, b0, off = _gen_step(dev, cin, cout, False)
    f1, b1, on = _gen_step(dev, cin, cout, True)
    assert f0 == ['es_spconv_fwd_bf16'] * 8 and not [n for n in b0 if n.startswith('es_gen_transpose')], (f0, b0)
    assert b0.count('es_spconv_fwd_bf16') == 8 and b0.count('es_spconv_wgrad_bf16') == 8, b0
    # forward: the fused name alone, or the refused fused name followed by the per-tap launches
    assert f1 == (['es_gen_transpose_fwd_bf16'] if fwd_served else ['es_gen_transpose_fwd_bf16 refused'] + ['es_spconv_fwd_bf16'] * 8), f1
    # backward: the data gradient is asked first, then the weight gradient, then whatever per-tap launches are left
    d_name = 'es_gen_transpose_dgrad_bf16' + ('' if dgrad_served else ' refused')
    assert b1[0] == d_name and b1[1] in ('es_gen_transpose_wgrad_bf16', 'es_gen_transpose_wgrad_bf16 refused'), b1
    wgrad_served = b1[1] == 'es_gen_transpose_wgrad_bf16'
    assert b1[2:].count('es_spconv_fwd_bf16') == (0 if dgrad_served else 8), b1
    assert b1[2:].count('es_spconv_wgrad_bf16') == (0 if wgrad_served else 8), b1
    assert len(b1) == 2 + (0 if dgrad_served else 8) + (0 if wgrad_served else 8), b1
    assert all(float(v.abs().max()) > 0 for v in off.values())
    for key, served in (('y', fwd_served), ('dx', dgrad_served), ('dw', wgrad_served)):
        if not served:                           # the same launches as with the switch off: the same bits
            assert torch.equal(_bits(off[key]), _bits(on[key])), key


@pytest.mark.parametrize('cin,cout,fwd_served,dgrad_served', [(32, 32, True, True), (16, 32, True, False), (8, 24, False, False)])
def test_gen_conv_transpose_asks_the_fused_entries_through_the_door(dev, cin, cout, fwd_served, dgrad_served):
    gen_transpose_door_case(dev, cin, cout, fwd_served, dgrad_served)


def gen_transpose_error_case(dev, monkeypatch):
    from embodiedscan_amd import engine as E, hip
    monkeypatch.setitem(hip._fn, 'es_gen_transpose_fwd_bf16', lambda *a: -1)
    x = E.Var(torch.randn(5, 32).to(dev))
    w = _conv_param(dev, torch.randn(8, 32, 32), torch.zeros(8, 32, 32))
    old = E.PRECISION[0], E.GEN_FUSED[0]
    E.PRECISION[0], E.GEN_FUSED[0] = 'bf16', True
    E.TAPE.clear()
    try:
        with _Recorder() as names:
            with pytest.raises(hip.HipError, match='es_gen_transpose_fwd_bf16 failed with status -1'):
                E.gen_conv_transpose(x, w)
    finally:
        E.PRECISION[0], E.GEN_FUSED[0] = old
        E.TAPE.clear()
    assert names == [], names                    # (the error left try_call before the recorder saw a result; no per-tap launch followed)


def test_a_failed_fused_launch_raises_and_queues_nothing_more(dev, monkeypatch):
    gen_transpose_error_case(dev, monkeypatch)


# ---------------------------------------------------------------------------------------------- gradient hand-over
N, C = 4, 16


def _handover_ops(dev):
    """name -> build(a, b) -> (y, [(input Var, the tensor handed to it, read after the backward)])"""
    from embodiedscan_amd import engine as E
    pos_a = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device=dev)
    pos_b = torch.tensor([2, 3, 4, 5], dtype=torch.int32, device=dev)
    vec = lambda v: E.Param(torch.full((C,), v, device=dev), torch.zeros(C, device=dev))

    def add(a, b):
        y = E.add(a, b)
        return y, [(a, lambda: y.g), (b, lambda: y.g)]

    def concat_rows(a, b):
        y = E.concat_rows([a, b])
        return y, [(a, lambda: y.g[:N]), (b, lambda: y.g[N:])]

    def union_add(a, b):
        y = E.union_add(a, b, pos_a, pos_b, 6)
        return y, [(a, lambda: y.g[pos_a.long()]), (b, lambda: y.g[pos_b.long()])]

    def layernorm(a, b):                          # both inputs receive dz, which only the launch knows: the first run's gradient is the reference
        y = E.layernorm(a, vec(1.5), vec(0.25), res=b)
        return y, [(a, None), (b, None)]

    def norm(a, b):                               # es_norm_bwd leaves dz in y.g: that is what the residual input receives
        y = E.norm(a, vec(1.5), vec(0.25), [0, N], 1e-5, res=b)
        return y, [(b, lambda: y.g)]
    return dict(add=add, concat_rows=concat_rows, union_add=union_add, layernorm=layernorm, norm=norm)


def _handover_run(dev, build, prior, bf16_on=None):
    """one forward + backward; prior: give every receiving input a gradient g0 and a stale .gh first -> [(g0, .g after, handed, .gh after)]"""
    from embodiedscan_amd import engine as E
    g = torch.Generator().manual_seed(7)
    a, b = (E.Var(torch.randn(N, C, generator=g).to(dev)) for _ in range(2))
    E.TAPE.clear()
    y, targets = build(a, b)
    y.g = torch.randn(*y.d.shape, generator=g).to(dev)
    g0s = []
    for i, (v, _) in enumerate(targets):
        v.gh = torch.zeros(N, C, dtype=torch.bfloat16, device=dev)
        g0s.append(torch.randn(N, C, generator=g).to(dev) if prior else None)
        v.g = None if g0s[-1] is None else g0s[-1].clone()
        if bf16_on == i:
            v.g = torch.zeros(N, C, dtype=torch.bfloat16, device=dev)
    try:
        E.TAPE.backward()
    finally:
        E.TAPE.clear()
    return [(g0, v.g.clone(), None if t is None else t().clone(), v.gh) for g0, (v, t) in zip(g0s, targets)]


def handover_case(dev, name):
    build = _handover_ops(dev)[name]
    first = _handover_run(dev, build, False)
    for _, got, handed, gh in first:
        assert gh is None and got.dtype == torch.float32 and float(got.abs().max()) > 0
        if handed is not None:
            assert torch.equal(_bits(got), _bits(handed))                 # the handed tensor itself (or its copy)
    if name == 'layernorm':
        assert torch.equal(_bits(first[0][1]), _bits(first[1][1]))        # dz and its clone
    for (g0, got, handed, gh), ref in zip(_handover_run(dev, build, True), first):
        assert gh is None
        assert torch.equal(_bits(got), _bits(g0 + (handed if handed is not None else ref[1])))       # g0 + y.g: one f32 add per element
    for i in range(len(first)):
        with pytest.raises(AssertionError, match='second consumer'):
            _handover_run(dev, build, True, bf16_on=i)


@pytest.mark.parametrize('name', ['add', 'concat_rows', 'union_add', 'layernorm', 'norm'])
def test_gradient_hand_over(dev, name):
    handover_case(dev, name)
