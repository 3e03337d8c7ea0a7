"""engine.GRAD_ROWS_BF16 on the CPU emulator (tests/emu): a MinkResNet basic block (conv K = 27 -> norm -> conv K = 27 -> norm + identity)
in bf16 mode, backward with the switch off and on.  Off: every es_norm_bwd launch is given f32 rows.  On: both are given none (each
convolution's backward gathers the bf16 shadow for both of its launches) and the convolution gradients -- weights, norm parameters, the
block input -- keep their bits.  With per-launch instrumentation on, or when the convolution has a bias, the f32 rows are written as
before.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import pytest
import torch

from test_emu_insitu import _param
from test_emu_product import _ListAsDict, emulated  # noqa: F401


def _block(E, sparse, switch, bias=False, debug=False):
    g = torch.Generator().manual_seed(11)
    pts = [torch.rand(3000, 3, generator=g) * 1.2]
    cs = sparse.voxelize(pts, 0.1)[0]
    n, C = cs.n, 64                               # (the fast bf16 kernel takes Cout % 64 == 0: both directions gather shadows)
    E.TAPE.clear()
    E.new_grad_epoch()
    E.GRAD_ROWS_BF16[0] = switch
    x = E.Var(torch.randn(n, C, generator=g))
    ps = dict(w1=torch.randn(27, C, C, generator=g) / (27 * C) ** 0.5, w2=torch.randn(27, C, C, generator=g) / (27 * C) ** 0.5,
              g1=torch.rand(C, generator=g) + 0.5, b1=torch.randn(C, generator=g) * 0.1, g2=torch.rand(C, generator=g) + 0.5,
              b2=torch.randn(C, generator=g) * 0.1, cb=torch.randn(C, generator=g) * 0.1)
    ps = {k: _param(v, torch.zeros_like(v)) for k, v in ps.items()}
    nbr, inv = cs.kernel_map(cs, 3), cs.self_inverse(3)
    o = E.conv(x, ps['w1'], nbr, inv, n, bias=ps['cb'] if bias else None)
    o = E.norm(o, ps['g1'], ps['b1'], cs.offsets(), 1e-5, act=1)
    o = E.conv(o, ps['w2'], nbr, inv, n)
    y = E.norm(o, ps['g2'], ps['b2'], cs.offsets(), 1e-5, act=1, res=x)
    y.g = torch.randn(n, C, generator=g)
    dx_args = []
    real = E.call

    def call(fn, *args):
        if fn == 'es_norm_bwd':
            dx_args.append(args[17])
        return real(fn, *args)
    E.call = call
    if debug:
        E.DEBUG_GRADS = {}
    try:
        E.TAPE.backward()
    finally:
        E.call, E.DEBUG_GRADS = real, None
    return n, dx_args, dict(x=x.g.clone(), **{k: p.g.clone() for k, p in ps.items()})


@pytest.fixture
def engine(emulated, monkeypatch):  # noqa: F811
    from embodiedscan_amd import engine as E, sparse
    monkeypatch.setitem(_ListAsDict(E.PRECISION), 0, 'bf16')
    monkeypatch.setitem(_ListAsDict(E.GRAD_ROWS_BF16), 0, True)
    return E, sparse


def _same(a, b):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_block_backward_without_f32_rows_keeps_every_gradient(engine):
    E, sparse = engine
    n, dx0, off = _block(E, sparse, False)
    _, dx1, on = _block(E, sparse, True)
    assert n > 500 and float(off['w1'].abs().max()) > 0 and float(off['x'].abs().max()) > 0
    assert len(dx0) == 2 and all(dx0), dx0
    assert dx1 == [0, 0], dx1
    _same(off, on)


def test_f32_rows_stay_for_a_biased_convolution_and_under_instrumentation(engine):
    E, sparse = engine
    _, dx, on = _block(E, sparse, True, bias=True)          # conv1's bias gradient sums the f32 rows
    assert dx[0] == 0 and dx[1] != 0, dx                    # (backward order: norm2 first)
    _, _, off = _block(E, sparse, False, bias=True)
    _same(off, on)
    _, dx, _ = _block(E, sparse, True, debug=True)
    assert len(dx) == 2 and all(dx), dx


def _join(E, switch, n=300):
    """the tail of an image-backbone bottleneck on bf16 activations: conv1 (1x1, 128 -> 32, BN, ReLU) -> conv3 (1x1, 32 -> 128, BN) + identity -> ReLU"""
    g = torch.Generator().manual_seed(21)
    E.TAPE.clear()
    E.new_grad_epoch()
    E.GRAD_ROWS_BF16[0] = switch
    cur = E.Var(torch.randn(n, 128, generator=g).to(torch.bfloat16))
    w1 = _param(torch.randn(1, 128, 32, generator=g) / 128 ** 0.5, torch.zeros(1, 128, 32))
    w3 = _param(torch.randn(1, 32, 128, generator=g) / 32 ** 0.5, torch.zeros(1, 32, 128))
    s1, t1 = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.2
    s3, t3 = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.2
    o = E.conv_affine(cur, w1, None, None, n, s1, t1, act=1, out_bf16=True)
    y = E.conv_affine(o, w3, None, None, n, s3, t3, act=1, res=cur, sole_consumer=True, out_bf16=True)
    y.g = torch.randn(n, 128, generator=g)
    names = []
    real = E.call

    def call(fn, *args):
        names.append(fn)
        return real(fn, *args)
    E.call = call
    try:
        E.TAPE.backward()
    finally:
        E.call = real
    return names, dict(cur=cur.g.clone(), w1=w1.g.clone(), w3=w3.g.clone())


def test_residual_join_writes_bf16_rows_and_keeps_every_gradient(engine):
    E, _ = engine
    n0, off = _join(E, False)
    n1, on = _join(E, True)
    assert n0.count('es_affine_act_bwd_yh') == 1 and 'es_affine_act_bwd_yh_xh' not in n0, n0
    assert n1.count('es_affine_act_bwd_yh_xh') == 1 and 'es_affine_act_bwd_yh' not in n1 and 'es_cast_rows_bf16' not in n1, n1
    assert float(off['w3'].abs().max()) > 0 and float(off['w1'].abs().max()) > 0 and float(off['cur'].abs().max()) > 0
    _same(off, on)


def _downsample_block(E, switch, H=8, W=6):
    """the first bottleneck of a stage without its 3x3 layer: conv1 (1x1, 64 -> 32) -> conv3 (1x1, 32 -> 128) + downsample (1x1 / stride 2,
    64 -> 128, BN, no activation) -> ReLU; conv1 runs on the stride-2 rows here so that every layer stays a 1x1 one"""
    from embodiedscan_amd.models.backbones.resnet2d import _Grid
    g = torch.Generator().manual_seed(31)
    E.TAPE.clear()
    E.new_grad_epoch()
    E.GRAD_ROWS_BF16[0] = switch
    n_img = 2
    grid = _Grid(n_img, H, W, torch.device('cpu'))
    dn, di, n_out, _, _ = grid.conv_map(1, 2, 0)
    n_in = n_img * H * W
    cur = E.Var(torch.randn(n_in, 64, generator=g).to(torch.bfloat16))
    half = E.Var(torch.randn(n_out, 64, generator=g).to(torch.bfloat16))
    w1 = _param(torch.randn(1, 64, 32, generator=g) / 8, torch.zeros(1, 64, 32))
    w3 = _param(torch.randn(1, 32, 128, generator=g) / 32 ** 0.5, torch.zeros(1, 32, 128))
    wd = _param(torch.randn(1, 64, 128, generator=g) / 8, torch.zeros(1, 64, 128))
    fold = lambda c: (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2)
    (s1, t1), (s3, t3), (sd, td) = fold(32), fold(128), fold(128)
    o = E.conv_affine(half, w1, None, None, n_out, s1, t1, act=1, out_bf16=True)
    idt = E.conv_affine(cur, wd, dn, di, n_out, sd, td, act=0, out_bf16=True, img=(n_img, H, W, 2))
    y = E.conv_affine(o, w3, None, None, n_out, s3, t3, act=1, res=idt, sole_consumer=True, out_bf16=True, res_sole=True)
    y.g = torch.randn(n_out, 128, generator=g)
    names = []
    real, real_try = E.call, E.hip.try_call

    def call(fn, *args):
        names.append(fn)
        return real(fn, *args)

    def try_call(fn, *args):
        ok = real_try(fn, *args)
        names.append(fn if ok else fn + ' refused')
        return ok
    E.call, E.hip.try_call = call, try_call
    try:
        E.TAPE.backward()
    finally:
        E.call, E.hip.try_call = real, real_try
    return names, dict(cur=cur.g.clone(), half=half.g.clone(), w1=w1.g.clone(), w3=w3.g.clone(), wd=wd.g.clone())


def test_downsample_join_writes_both_gradients_and_no_dres(engine):
    E, _ = engine
    n0, off = _downsample_block(E, False)
    n1, on = _downsample_block(E, True)
    assert n0.count('es_affine_act_bwd_yh') == 2 and n0.count('es_img_dgrad1_s2_bf16') == 1, n0      # the join, then the downsample's BN
    assert n1.count('es_affine_act_bwd_yh_xh2') == 1 and n1.count('es_img_dgrad1_s2_bf16') == 1, n1
    assert not [n for n in n1 if n in ('es_affine_act_bwd_yh', 'es_affine_act_bwd_yh_xh', 'es_cast_rows_bf16')], n1
    assert all(float(v.abs().max()) > 0 for v in off.values())
    _same(off, on)


def test_downsample_on_an_odd_grid_keeps_f32_rows(engine):
    E, _ = engine
    n0, off = _downsample_block(E, False, H=9, W=7)
    n1, on = _downsample_block(E, True, H=9, W=7)           # the stride-2 kernel does not take odd grids: the join keeps dres,
    assert n1.count('es_affine_act_bwd_yh_xh') == 1 and n1.count('es_affine_act_bwd_yh') == 1, n1      # the downsample its f32 rows
    assert 'es_affine_act_bwd_yh_xh2' not in n1
    _same(off, on)


def test_second_consumer_of_bf16_gradient_rows_fails_loudly(engine):
    E, _ = engine
    v = E.Var(torch.zeros(4, 16))
    v.g = torch.zeros(4, 16, dtype=torch.bfloat16)
    with pytest.raises(AssertionError, match='second consumer'):
        E._grad_target(v, v.d)
