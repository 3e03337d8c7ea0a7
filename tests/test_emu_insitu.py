"""The forward in-situ gate (tests/fwd_spec.py, the checker tests/test_gpu_insitu.py runs on every forward launch of a real bf16 step)
in the CPU suite: engine operators in bf16 mode on the emulated library (tests/emu) with engine.DEBUG_FWD set -- the fused conv +
BN (+ residual) + ReLU epilogue with bf16 residual and output rows and a ragged tail, a K = 27 convolution through the map kernel,
train-mode norm with its fused shadow, the fused generative transposed convolution, max pooling, LayerNorm, attention -- each record
must pass.  Then mutated copies of those records, and a record of a real stale shadow, must each be rejected, with a message that
names the defect: the gate has teeth without a GPU.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import copy

import numpy as np
import pytest
import torch

import fwd_spec as FS
from test_emu_product import _ListAsDict, emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


def _param(d, g=None):
    """a conv Param whose bf16 copies are made by one cast launch (the GPU registry is keyed by CUDA devices)"""
    from embodiedscan_amd import engine as E, hip
    p = E.Param(d.clone(), g)
    if d.dim() == 3:
        K, a, b = d.shape
        p.bf_n, p.bf_t = torch.empty((K, a, b), dtype=torch.bfloat16), torch.empty((K, b, a), dtype=torch.bfloat16)
        hip.call('es_cast_weight_bf16', hip.P(p.d), K, a, b, hip.P(p.bf_n), hip.P(p.bf_t), 0)
        p.bf_step = E.WEIGHT_VERSION[0]
    return p


def _map(rng, n_out, n_in, K, fill=0.5, spread=30):
    nbr = np.full((n_out, K), -1, np.int32)
    for k in range(K):
        m = rng.random(n_out) < fill
        src = np.clip(np.arange(n_out) * n_in // n_out + rng.integers(-spread, spread + 1, n_out), 0, n_in - 1)
        nbr[m, k] = src[m]
    return torch.from_numpy(nbr)


@pytest.fixture
def bf16_records(emulated, monkeypatch):
    """one record of each operator class, made by the engine on the emulated library in bf16 mode"""
    from embodiedscan_amd import engine as E
    monkeypatch.setitem(_ListAsDict(E.PRECISION), 0, 'bf16')
    monkeypatch.setitem(_ListAsDict(E.HALO), 0, False)                    # (the K = 27 case runs through the map kernel)
    monkeypatch.setattr(E, 'DEBUG_FWD', [])
    g = torch.Generator().manual_seed(5)
    rng = np.random.default_rng(5)
    E.TAPE.clear()
    out = {}
    # conv_affine: f32 input rows, bf16 residual and output rows, 300 rows (a ragged last tile), K = 27, ReLU
    n, cin, cout = 300, 32, 64
    x = E.Var(torch.randn(n, cin, generator=g), rg=False)
    w = _param(torch.randn(27, cin, cout, generator=g) / (27 * cin) ** 0.5)
    res = E.Var((torch.randn(n, cout, generator=g) * 0.5).to(torch.bfloat16), rg=False)
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    E.conv_affine(x, w, _map(rng, n, n, 27), None, n, scale, shift, act=1, res=res, out_bf16=True)
    out['conv_affine'] = E.DEBUG_FWD[-1]
    # K = 27 convolution through the gather-map kernel, bias, 37 -> 300 rows
    n_in = 270
    x = E.Var(torch.randn(n_in, cin, generator=g), rg=False)
    w = _param(torch.randn(27, cin, cout, generator=g) / (27 * cin) ** 0.5)
    b = _param(torch.randn(cout, generator=g))
    E.conv(x, w, _map(rng, n, n_in, 27), None, n, bias=b)
    out['conv'] = E.DEBUG_FWD[-1]
    # train-mode batch norm (running statistics, fused bf16 shadow) and instance norm over two segments with a residual
    x = E.Var(torch.randn(200, 32, generator=g) * 2 + 1, rg=False)
    wn, bn = _param(torch.rand(32, generator=g) + 0.5), _param(torch.randn(32, generator=g) * 0.1)
    rm, rv = torch.zeros(32), torch.ones(32)
    E.norm(x, wn, bn, [0, 200], 1e-5, act=1, running=(rm, rv))
    out['norm'] = E.DEBUG_FWD[-1]
    E.norm(x, wn, bn, [0, 120, 200], 1e-5, act=2, res=E.Var(torch.randn(200, 32, generator=g), rg=False))
    out['norm_seg'] = E.DEBUG_FWD[-1]
    # fused generative transposed convolution (8 taps, one launch)
    x = E.Var(torch.randn(90, 64, generator=g), rg=False)
    E.gen_conv_transpose(x, _param(torch.randn(8, 64, 32, generator=g) / 8))
    out['gen_transpose'] = E.DEBUG_FWD[-1]
    # max pooling over 8 taps with absent neighbours
    x = E.Var(torch.randn(200, 16, generator=g), rg=False)
    E.maxpool(x, _map(rng, 60, 200, 8, fill=0.6), 60)
    out['maxpool'] = E.DEBUG_FWD[-1]
    # LayerNorm with its residual input
    E.layernorm(E.Var(torch.randn(40, 256, generator=g), rg=False), _param(torch.rand(256, generator=g) + 0.5),
                _param(torch.randn(256, generator=g) * 0.1), res=E.Var(torch.randn(40, 256, generator=g), rg=False))
    out['layernorm'] = E.DEBUG_FWD[-1]
    # attention: 2 samples x 2 heads, 20 queries over 40 keys, the second sample's keys cut at 25
    B, H, Lq, Lk = 2, 2, 20, 40
    q = E.Var(torch.randn(B * Lq, H * 32, generator=g) * 2, rg=False)
    k = E.Var(torch.randn(B * Lk, H * 32, generator=g) * 2, rg=False)
    v = E.Var(torch.randn(B * Lk, H * 32, generator=g), rg=False)
    E.attention(q, k, v, B, H, Lq, Lk, klen=torch.tensor([40, 25], dtype=torch.int32))
    out['attention'] = E.DEBUG_FWD[-1]
    E.TAPE.clear()
    return out


def test_forward_records_of_engine_operators_pass_the_checker(bf16_records):
    want = dict(conv_affine='es_spconv_fwd_bf16_io', conv='es_spconv_fwd_bf16_ws', norm='es_norm_fwd', norm_seg='es_norm_fwd',
                gen_transpose='es_gen_transpose_fwd_bf16', maxpool='es_maxpool_fwd', layernorm='es_layernorm_fwd',
                attention='es_attn_fwd')
    stats = FS.Stats('emulated')
    for name, rec in bf16_records.items():
        assert rec['entry'] == want[name], (name, rec['entry'])        # (conv: an under-filled launch takes the deterministic tap split)
        FS.check(rec, torch.device('cpu'), stats)
    assert bf16_records['conv']['xh'] is not None                 # the map kernel gathered the bf16 shadow ...
    assert bf16_records['norm']['yh'] is not None                 # ... and norm wrote one
    assert bf16_records['conv_affine']['y'].dtype == torch.bfloat16 and bf16_records['conv_affine']['res'].dtype == torch.bfloat16
    print(stats.report())


def _rejected(rec, match):
    with pytest.raises(AssertionError, match=match):
        FS.check(rec, torch.device('cpu'), FS.Stats('mutated'))


def _bf16_step(t, steps):
    """t (bf16) moved by `steps` ulps"""
    return (t.view(torch.int16) + steps).view(torch.bfloat16)


def _affine_parts(rec):
    x, w = FS._r(rec['x']), FS._r(rec['w'])
    conv = FS.gather_gemm(x, w, rec['nbr'], rec['n_out'])
    return conv * rec['scale'].double(), rec['shift'].double(), rec['res'].double()


def test_checker_rejects_an_output_two_ulp_off(bf16_records):
    rec = copy.deepcopy(bf16_records['conv_affine'])
    i = int(torch.argmax(rec['y'].float().abs()))
    rec['y'].view(-1)[i] = _bf16_step(rec['y'].view(-1)[i:i + 1], 2)[0]
    _rejected(rec, r'per-element bound exceeded')


def test_checker_rejects_a_dropped_residual_row(bf16_records):
    rec = copy.deepcopy(bf16_records['conv_affine'])
    sc, sh, res = _affine_parts(rec)
    row = int(torch.argmax(res.abs().sum(1)))
    rec['y'][row] = (sc[row] + sh).clamp(min=0).to(torch.bfloat16)
    _rejected(rec, r'per-element bound exceeded.*the residual dropped')


def test_checker_rejects_a_dropped_shift_column(bf16_records):
    rec = copy.deepcopy(bf16_records['conv_affine'])
    sc, sh, res = _affine_parts(rec)
    col = int(torch.argmax(sh.abs()))
    rec['y'][:, col] = (sc[:, col] + res[:, col]).clamp(min=0).to(torch.bfloat16)
    _rejected(rec, r'per-element bound exceeded.*the shift dropped')


def test_checker_rejects_a_stale_shadow(emulated, monkeypatch):
    """a real one: the rows change in place after their bf16 shadow was made (what relu_ / upsample_add_ / add_into / copy_cols do
    to Var.d without touching Var.dh); the convolution then gathers the stale shadow"""
    from embodiedscan_amd import engine as E
    monkeypatch.setitem(_ListAsDict(E.PRECISION), 0, 'bf16')
    monkeypatch.setitem(_ListAsDict(E.HALO), 0, False)
    monkeypatch.setattr(E, 'DEBUG_FWD', [])
    g = torch.Generator().manual_seed(9)
    n, cin, cout = 300, 32, 64
    x = E.Var(torch.randn(n, cin, generator=g), rg=False)
    x.shadow()
    x.d[7] += 1.0                                                 # in-place write after the shadow was made
    E.conv(x, _param(torch.randn(27, cin, cout, generator=g) / 30), _map(np.random.default_rng(9), n, n, 27), None, n)
    E.TAPE.clear()
    rec = E.DEBUG_FWD[-1]
    assert rec['xh'] is not None
    _rejected(rec, r'stale shadow')


def test_checker_rejects_norm_statistics_of_the_wrong_segment(bf16_records):
    rec = copy.deepcopy(bf16_records['norm_seg'])
    rec['mean'] = rec['mean'].flip(0)
    rec['invstd'] = rec['invstd'].flip(0)
    _rejected(rec, r'norm mean of segment 0')


def test_checker_rejects_a_bias_gradient_off_in_one_column(emulated, monkeypatch):
    """the backward gate's per-element bias bound: a column whose exact sum cancels (the attention key-projection bias) is held to
    G u sqrt(rows) sum |gy|, where the relative-L2 tolerance TOL + 1e-5 sum|gy| / |want| lets anything pass"""
    import test_gpu_insitu as TI
    from embodiedscan_amd import engine as E
    monkeypatch.setitem(_ListAsDict(E.PRECISION), 0, 'bf16')
    monkeypatch.setattr(E, 'DEBUG_CONV', [])
    g = torch.Generator().manual_seed(11)
    n, cin, cout = 64, 32, 32
    w = _param(torch.randn(1, cin, cout, generator=g) / 6, torch.zeros(1, cin, cout))
    b = _param(torch.zeros(cout), torch.zeros(cout))
    E.TAPE.clear()
    y = E.linear(E.Var(torch.randn(n, cin, generator=g)), w, b)
    gy = torch.randn(n, cout, generator=g, dtype=torch.float64)
    gy = (gy - gy.mean(0)).float()                                # every column sum cancels to ~ eps * sum |gy|
    y.g = gy.clone()
    E.TAPE.backward()
    recs = E.DEBUG_CONV
    TI._check_conv_records(recs, 'emulated linear', torch.device('cpu'))
    mag = gy.double().abs().sum(0)
    b.g[3] += float(100 * FS.G * FS.U * n ** 0.5 * mag[3])
    with pytest.raises(AssertionError, match=r'bias gradient column 3: per-element bound exceeded'):
        TI._check_conv_records(recs, 'emulated linear', torch.device('cpu'))


def test_checker_rejects_a_weight_gradient_missing_one_pair(emulated, monkeypatch):
    """the backward gate's per-element weight-gradient bound: a K = 27 layer whose centre tap has 40 pairs on rows of their own with
    small output gradients (the rest ~ 3 000 pairs each).  One of those 40 pairs dropped from the launch's result moves that tap's
    elements by several per cent and the whole tensor by < 2e-4 relative L2: the old assertion passes it, the new one does not"""
    import test_gpu_insitu as TI
    from embodiedscan_amd import engine as E
    monkeypatch.setitem(_ListAsDict(E.PRECISION), 0, 'bf16')
    monkeypatch.setitem(_ListAsDict(E.HALO), 0, False)
    monkeypatch.setattr(E, 'DEBUG_CONV', [])
    g = torch.Generator().manual_seed(13)
    rng = np.random.default_rng(13)
    n, cin, cout = 4096, 32, 32
    nbr = _map(rng, n, n, 27, fill=0.73)
    nbr[:, 13] = -1
    own = torch.from_numpy(rng.choice(n, size=40, replace=False))
    nbr[own] = -1
    nbr[own, 13] = torch.from_numpy(rng.integers(0, n, size=40).astype(np.int32))
    w = _param(torch.randn(27, cin, cout, generator=g) / 30, torch.zeros(27, cin, cout))
    E.TAPE.clear()
    x = E.Var(torch.randn(n, cin, generator=g), rg=False)
    y = E.conv(x, w, nbr, None, n)
    gy = torch.randn(n, cout, generator=g)
    gy[own] /= 64
    y.g = gy.clone()
    E.TAPE.backward()
    recs = E.DEBUG_CONV
    assert len(recs) == 1 and recs[0]['w'] is w
    n_dw, _, _, _ = TI._check_conv_records(recs, 'emulated K = 27 layer', torch.device('cpu'))
    assert n_dw == 1
    row = int(own[7])
    pair = torch.outer(FS._r(x.d[int(nbr[row, 13])]), FS._r(gy[row]))
    good = w.g.clone()
    w.g[13] -= pair.float()
    rel = TI._rel(w.g, good)
    assert rel < TI.TOL, rel                                      # what the relative L2 alone sees of it
    with pytest.raises(AssertionError, match=r'weight gradient K=27 32->32 \(1 launch\(es\)\): per-element bound exceeded at dw\[13\]'):
        TI._check_conv_records(recs, 'emulated K = 27 layer', torch.device('cpu'))
