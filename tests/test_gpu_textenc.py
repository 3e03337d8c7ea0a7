"""The frozen text encoder on the project's own kernels (text.HipTextEncoder, SparseFeatureFusion3DGrounder(text_encoder_impl='hip')).
Kernel level: es_text_attn_fwd, es_text_embed_ln and es_bias_gelu held to the f64 specifications of tests/textenc_spec.py at every
shape edge (both sides of the 16-query tile, of the 64-key LDS-resident limit and of the 64-key streaming step; operands are column
slices of wider buffers that hold a sentinel everywhere else).  Model level: the whole encoder against the transformers module in f64,
gated by that module's OWN f32 / bf16 error on the same input.  Detector level: the two implementations behind one constructor argument.

Every body is a function of `dev`: tests/test_emu_textenc.py runs the kernel bodies and the tiny f32 model on the CPU emulator
(dev.type == 'cpu' selects the reduced grid there)."""
import contextlib
import copy
import functools
import math
import os
import warnings

import pytest
import torch

import textenc_spec as S
from test_gpu_ground_kernels import SENT, Cols, _flat, _hip, _rc, _small, _st, _tail_ok

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


@contextlib.contextmanager
def precision(mode):
    from embodiedscan_amd import engine as E
    prev = E.PRECISION[0]
    E.PRECISION[0] = mode
    try:
        yield
    finally:
        E.PRECISION[0] = prev


# ------------------------------------------------------------------------------------------------------------------ attention
REGIMES = ('flat', 'peaked', 'ascending')
ATTN_T = (1, 15, 16, 17, 33, 64, 65, 130)
ATTN_BH = ((1, 1), (3, 2), (2, 3))
MASKS = ('null', 'prefix', 'hole', 'dead')


def text_attn_inputs(regime, B, H, T, seed):
    """the packed (B T, 3 H 64) projection, the three value regimes of test_gpu_ground_kernels.attn_inputs at head dimension 64.
    'flat': small scores, a near-uniform softmax.  'peaked': q scaled so that max |S| = 25.  'ascending': keys and queries share a
    +-1 direction per head and key j carries it j / 64 times, so the row maximum rises at every 64-key step (the online-softmax rescale
    matters) and the scores reach a large magnitude at T = 512"""
    g = torch.Generator().manual_seed(seed)
    E = H * 64
    q, k, v = (torch.randn(B * T, E, generator=g) for _ in range(3))
    if regime == 'flat':
        q = q * 0.05
    elif regime == 'peaked':
        Sm = (S._heads(q.double() * S.SCALE, B, T, H) @ S._heads(k.double(), B, T, H).transpose(-1, -2)).abs().max()
        q = q * float(25.0 / Sm)
    else:
        d = (torch.randint(0, 2, (1, E), generator=g) * 2 - 1).float()
        a = math.sqrt(3.0 / 8.0)                                   # (q / 8) . k rises by 3 per 64 keys
        j = (torch.arange(B * T) % T).float()[:, None]
        k = d * a * (j / 64.0) + 0.02 * k
        q = d * a + 0.1 * q
    return torch.cat([q, k, v], 1)


def text_mask(kind, B, T, seed):
    """None; prefix lengths [T, 1, ...]; an interior hole (sample 0) and scattered masked keys (the others; key 0 stays live: <s>);
    one sample (the last) without a live key"""
    if kind == 'null':
        return None
    g = torch.Generator().manual_seed(seed)
    m = torch.ones((B, T), dtype=torch.int32)
    if kind == 'prefix':
        for b, n in enumerate(([T, 1] + [max(1, (T * (b + 1)) // (B + 1)) for b in range(B)])[:B]):
            m[b, n:] = 0
    elif kind == 'hole':
        m[0, T // 3:(2 * T) // 3] = 0
        if B > 1:
            m[1:] = (torch.rand((B - 1, T), generator=g) < 0.5).int()
            m[1:, 0] = 1
    else:
        m[B - 1] = 0
        if B > 1:
            m[0, (T + 1) // 2:] = 0
    return m


def text_attn_case(dev, stats, bf, regime, B, H, T, kind, seed):
    """one es_text_attn_fwd launch (twice: the two outputs must be bit-identical) on a column slice of a wider buffer"""
    hip = _hip()
    E = H * 64
    qkv = text_attn_inputs(regime, B, H, T, seed)
    mask = text_mask(kind, B, T, seed + 1)
    md = None if mask is None else mask.to(dev)
    X = Cols(dev, B * T, 3 * E, 3 * E + 8, 4, qkv)
    outs = [Cols(dev, B * T, E, E + 4 * (i + 1), 4 * i) for i in range(2)]
    for O in outs:
        hip.call('es_text_attn_fwd', X.ptr(), X.ld, B, H, T, hip.P(md), O.ptr(), O.ld, bf, _st())
    torch.cuda.synchronize()
    label = f'text attention {regime} bf16={bf} B={B} H={H} T={T} mask={kind}'
    for O in outs:
        O.untouched_outside(label)
    assert torch.equal(outs[0].v, outs[1].v), f'{label}: two runs differ'
    S.check_text_attention(dict(B=B, H=H, T=T, bf=bf, qkv=X.v, mask=md, o=outs[0].v), dev, stats)


@pytest.mark.parametrize('bf', [0, 1])
def test_text_attention_on_the_tile_edge_grid(dev, bf):
    stats = S.Stats(f'text attention bf16={bf}')
    small = _small(dev)
    i = 0
    for T in ATTN_T:
        for (B, H) in ATTN_BH:
            for kind in MASKS:
                for regime in REGIMES:
                    i += 1
                    if small and (i % 3 != T % 3 or (B, H) == (3, 2)):      # the emulator's reduced grid: every T, mask and regime stays
                        continue
                    text_attn_case(dev, stats, bf, regime, B, H, T, kind, 100 + i)
    if not small:
        for kind, regime in (('hole', 'ascending'), ('prefix', 'peaked')):
            text_attn_case(dev, stats, bf, regime, 2, 2, 512, kind, 7)
    print(stats.report())


def test_text_attention_refusals_leave_the_output_untouched(dev):
    """T = 0 and T = 513, a leading dimension below 3 H 64 or not a multiple of 4, a misaligned slice, NULL operands"""
    B, H, T = 1, 1, 4
    X = Cols(dev, B * 520, 192, 200, 4, torch.zeros(520, 192))
    O = Cols(dev, B * 520, 64, 68, 4)
    for args in ((X.ptr(), 200, B, H, 0), (X.ptr(), 200, B, H, 513), (X.ptr(), 188, B, H, T), (X.ptr(), 198, B, H, T),
                 (X.ptr() + 4, 200, B, H, T), (0, 200, B, H, T)):
        assert _rc('es_text_attn_fwd', *args, 0, O.ptr(), 68, 1, _st()) == -4, args
    assert _rc('es_text_attn_fwd', X.ptr(), 200, B, H, T, 0, O.ptr(), 60, 1, _st()) == -4
    assert _rc('es_text_attn_fwd', X.ptr(), 200, B, H, T, 0, 0, 68, 1, _st()) == -4
    torch.cuda.synchronize()
    assert bool((O.buf == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ embedding
VOCAB, MAX_POS, PAD = 100, 40, 1


def embed_tables(C, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(word=torch.randn(VOCAB, C, generator=g), pos=torch.randn(MAX_POS, C, generator=g) * 0.5, type0=torch.randn(1, C, generator=g) * 0.2,
                w=torch.rand(C, generator=g) + 0.5, b=torch.randn(C, generator=g) * 0.1)


def embed_ids(T, seed):
    """five rows: no pad; pads at the end; a pad in the middle (the rule skips it); all pads; one id equal to the vocabulary size"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, VOCAB, (5, T), generator=g)
    ids[:, 0] = 0
    ids[1, (T + 1) // 2:] = PAD
    ids[2, T // 2] = PAD
    ids[3] = PAD
    ids[4, T - 1] = VOCAB
    return ids


def embed_case(dev, stats, C, T, eps, seed):
    hip = _hip()
    P = hip.P
    tab = {k: v.to(dev) for k, v in embed_tables(C, seed).items()}
    ids = embed_ids(T, seed + 1).to(dev)
    B = ids.shape[0]
    y, ybuf = _flat(dev, torch.zeros(B * T, C))
    p, pbuf = _flat(dev, torch.zeros(B * T, dtype=torch.int32))
    hip.call('es_text_embed_ln', P(ids), B, T, PAD, P(tab['word']), P(tab['pos']), P(tab['type0']), C, VOCAB, MAX_POS, P(tab['w']), P(tab['b']),
             eps, P(y), P(p), _st())
    torch.cuda.synchronize()
    _tail_ok(ybuf, B * T * C, 'embedding y')
    _tail_ok(pbuf, B * T, 'embedding position ids')
    rec = dict(tab, ids=ids, pad_id=PAD, vocab=VOCAB, eps=eps, y=y, pos_ids=p)
    S.check_text_embed(rec, dev, stats)
    return rec


def test_text_embedding_positions_and_layernorm(dev):
    stats = S.Stats('text embedding')
    for C in (128, 768):
        for T in (1, 11, 38):
            for eps in (1e-12, 1e-5):
                embed_case(dev, stats, C, T, eps, 3 * C + T)
    print(stats.report())


def test_text_embedding_refuses_a_row_beyond_the_position_table(dev):
    """pad_id + T >= max_pos: T = 39 is refused, nothing is written; so are C > 1024 and a pad id outside the vocabulary"""
    hip = _hip()
    P = hip.P
    C, T = 128, 39
    tab = {k: v.to(dev) for k, v in embed_tables(C, 5).items()}
    ids = torch.full((2, T), 7, dtype=torch.long, device=dev)
    y, ybuf = _flat(dev, torch.zeros(2 * T, C))
    y.fill_(SENT)
    args = lambda T_, C_, pad: (P(ids), 2, T_, pad, P(tab['word']), P(tab['pos']), P(tab['type0']), C_, VOCAB, MAX_POS, P(tab['w']), P(tab['b']), 1e-5,
                                P(y), 0, _st())
    assert _rc('es_text_embed_ln', *args(39, C, PAD)) == -4
    assert _rc('es_text_embed_ln', *args(11, 1025, PAD)) == -4
    assert _rc('es_text_embed_ln', *args(11, C, VOCAB)) == -4
    torch.cuda.synchronize()
    assert bool((ybuf == SENT).all())
    assert _rc('es_text_embed_ln', *args(38, C, PAD)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ GELU
def gelu_case(dev, stats, n, C, seed):
    hip = _hip()
    g = torch.Generator().manual_seed(seed)
    x = (torch.linspace(-12, 12, n * C)[torch.randperm(n * C, generator=g)]).view(n, C).clone()
    bias = torch.randn(C, generator=g) * 0.5
    x[0, :8] = -bias[:8]                                     # z = 0 exactly
    x[n - 1, C - 1] = 12.0 - float(bias[C - 1])
    X = Cols(dev, n, C, C + 8, 4, x)
    x0 = X.v.clone()
    bd = bias.to(dev)
    hip.call('es_bias_gelu', X.ptr(), X.ld, n, C, hip.P(bd), _st())
    torch.cuda.synchronize()
    X.untouched_outside(f'bias + GELU ({n}, {C})')
    assert bool((X.v[0, :8] == 0).all()), 'gelu(0) must be 0'
    S.check_bias_gelu(dict(x=x0, bias=bd, y=X.v), dev, stats)


def test_bias_gelu_exact_erf_form(dev):
    stats = S.Stats('bias + GELU')
    for n, C in ((1, 128), (37, 3072)):
        gelu_case(dev, stats, n, C, n + C)
    assert _rc('es_bias_gelu', 0, 128, 1, 128, 0, _st()) == -4
    print(stats.report())


# ------------------------------------------------------------------------------------------------------------------ model
TINY = dict(vocab_size=100, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, max_position_embeddings=40)
WIDE = dict(vocab_size=100, hidden_size=768, num_attention_heads=12, num_hidden_layers=1, intermediate_size=3072, max_position_embeddings=40)
CONFIGS = dict(tiny=TINY, wide=WIDE)


def ragged_ids(vocab, B=3, T=11, lens=(11, 4, 2), seed=9):
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((B, T), 1, dtype=torch.long)
    mask = torch.zeros((B, T), dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(3, vocab, (n,), generator=g)
        ids[b, 0], ids[b, n - 1] = 0, 2
        mask[b, :n] = 1
    return ids, mask


@functools.lru_cache(maxsize=None)
def model_case(name):
    """the seeded transformers module, the ragged input, its f64 output on the CPU and the errors of the module's own f32 and bf16
    evaluations against it (computed once, shared by every test of this process)"""
    from embodiedscan_amd.text import build_text_encoder
    model = build_text_encoder(CONFIGS[name], seed=5)
    ids, mask = ragged_ids(CONFIGS[name]['vocab_size'])
    with torch.no_grad():
        ref = copy.deepcopy(model).double()(input_ids=ids, attention_mask=mask).last_hidden_state
        f32 = model(input_ids=ids, attention_mask=mask).last_hidden_state.double()
        b16 = copy.deepcopy(model).bfloat16()(input_ids=ids, attention_mask=mask).last_hidden_state.double()
    return dict(model=model, ids=ids, mask=mask, ref=ref, err_f32=float((f32 - ref).abs().max()), max_bf16=float((b16 - ref).abs().max()),
                rms_bf16=float((b16 - ref).pow(2).mean().sqrt()))


def hip_model_output(dev, name, mode):
    from embodiedscan_amd.text import HipTextEncoder
    c = model_case(name)
    enc = HipTextEncoder.from_module(c['model'], dev)
    with precision(mode):
        out = enc(c['ids'].to(dev), c['mask'].to(dev))
    torch.cuda.synchronize()
    assert out.shape == c['ref'].shape and out.dtype == torch.float32
    return c, out.double().cpu()


def model_f32_case(dev, name):
    c, out = hip_model_output(dev, name, 'f32')
    err = float((out - c['ref']).abs().max())
    print(f'{name} f32: max |hip - f64| = {err:.3e}; the transformers module in f32 on the CPU: {c["err_f32"]:.3e} (gate: 4 x)')
    assert err <= 4 * c['err_f32']


@pytest.mark.parametrize('name', ['tiny', 'wide'])
def test_model_f32_within_four_times_the_modules_own_f32_error(dev, name):
    """both are f32 evaluations of one formula that differ only in summation order (4-wide MFMA k-steps and sequential chains against
    blocked CPU sums): the gate is 4 x the module's own max-abs error against f64, measured on the same input"""
    model_f32_case(dev, name)


@pytest.mark.parametrize('name', ['tiny', 'wide'])
def test_model_bf16_not_worse_than_the_bf16_module(dev, name):
    """the yardstick is the module converted with .bfloat16() on the CPU: the HIP path rounds a strict subset of what it rounds (its
    activations stay f32).  RMS error against f64 not above the bf16 module's, max-abs error not above twice the bf16 module's (the
    maximum of a few thousand elements is a noisy statistic)"""
    c, out = hip_model_output(dev, name, 'bf16')
    mx, rms = float((out - c['ref']).abs().max()), float((out - c['ref']).pow(2).mean().sqrt())
    print(f'{name} bf16: hip rms {rms:.3e} max {mx:.3e}; the bf16 module: rms {c["rms_bf16"]:.3e} max {c["max_bf16"]:.3e}')
    assert rms <= c['rms_bf16']
    assert mx <= 2 * c['max_bf16']


# ------------------------------------------------------------------------------------------------------------------ detector
class _Slot:
    pass


def _samples(texts):
    out = []
    for t in texts:
        s = _Slot()
        s.text, s.tokens_positive, s.gt_instances_3d = t, [[[0, 1]]], _Slot()
        out.append(s)
    return out


def tiny_grounder(dev, impl):
    """the small grounder of tests/test_gpu_grounding.py with the TINY text configuration (and a tokenizer of its vocabulary)"""
    from embodiedscan_amd.config import build_detector, load_config
    from embodiedscan_amd.text import HashTokenizer
    cfg = load_config(os.path.join(ROOT, 'configs', 'mv_grounding.py'))
    m = cfg['model']
    m['num_queries'] = 32
    m['decoder']['num_layers'] = 2
    m['decoder']['layer_cfg']['ffn_cfg']['feedforward_channels'] = 128
    m['neck_3d']['pts_prune_threshold'] = 300
    m['text_encoder_cfg'] = TINY
    m['tokenizer'] = HashTokenizer(TINY['vocab_size'])
    m['text_encoder_impl'] = impl
    return cfg, build_detector(cfg, device=dev, seed=0).to(dev)


def _encode(det, texts):
    from embodiedscan_amd import engine as E
    prev = E.TAPE.enabled
    E.TAPE.enabled = False
    try:
        det.encode_text(_samples(texts))
        torch.cuda.synchronize()
    finally:
        E.TAPE.enabled = prev
    return det.last_text['hidden'].float().clone()


def test_grounder_with_either_text_encoder(dev):
    from embodiedscan_amd import engine as E, pipeline
    from embodiedscan_amd.config import build_optim_wrapper
    from embodiedscan_amd.synth import make_grounding_sample, make_scan
    assert E.PRECISION[0] == 'f32'
    (cfg, dt), (_, dh) = tiny_grounder(dev, 'torch'), tiny_grounder(dev, 'hip')
    dt._bind()
    dh._bind()
    sdt, sdh = dt.state_dict(), dh.state_dict()
    assert list(sdt) == list(sdh)
    text_keys = [k for k in sdt if k.startswith('text_encoder.')]
    assert text_keys and all(torch.equal(sdt[k], sdh[k]) for k in text_keys)
    # the two encoders on the same prompts: within the f32 model gate (4 x the module's own f32 error against f64)
    texts = ['find the chair near the window', 'the lamp', 'a small round table between the sofa and the door of the room']
    ht, hh = _encode(dt, texts), _encode(dh, texts)
    ids, mask = dt.last_text['input_ids'].cpu(), dt.last_text['mask'].long().cpu()
    with torch.no_grad():
        cpu = copy.deepcopy(dt.text_encoder).cpu()
        ref = cpu.double()(input_ids=ids, attention_mask=mask).last_hidden_state
        own = float((copy.deepcopy(dt.text_encoder).cpu()(input_ids=ids, attention_mask=mask).last_hidden_state.double() - ref).abs().max())
    err = float((hh.double().cpu() - ref).abs().max())
    print(f'grounder text features: max |hip - f64| = {err:.3e}, the module in f32 on the CPU {own:.3e}; torch-on-device vs hip '
          f'{float((ht - hh).abs().max()):.3e}')
    assert hh.shape == ht.shape and err <= 4 * own
    # loading the torch build's dictionary with one encoder weight perturbed moves the text features of the hip build accordingly
    key = 'text_encoder.encoder.layer.1.attention.self.key.weight'
    sd2 = {k: v.clone() for k, v in sdt.items()}
    sd2[key] = sd2[key] + 0.05 * torch.randn(sd2[key].shape, generator=torch.Generator().manual_seed(1)).to(dev)
    dh.load_state_dict(sd2)
    dt.load_state_dict(sd2)
    assert torch.equal(dh.state_dict()[key], sd2[key])
    ht2, hh2 = _encode(dt, texts), _encode(dh, texts)
    assert float((hh2 - hh).abs().max()) > 1e-4, 'the loaded weight did not reach the kernels'
    assert float((hh2 - ht2).abs().max()) <= 1e-4, float((hh2 - ht2).abs().max())
    # twenty distinct (B, T) shapes in a row: no capture, no shape cache, no warning
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        for i in range(20):
            words = ' '.join(['word%d' % j for j in range(1 + (i * 7) % 31)])
            h = _encode(dh, [words] * (1 + i % 4))
            assert h.shape[:2] == (1 + i % 4, 3 + (i * 7) % 31) and bool(torch.isfinite(h).all())
    assert not getattr(dh, '_text_graphs', None), 'the hip encoder must not capture graphs'
    # one train step and one prediction
    scans = [make_scan(31 + i, n_views=3, height=120, width=160, img_size=(128, 128), n_points=12000, n_boxes=8) for i in range(2)]
    anns = [make_grounding_sample(s, seed=i) for i, s in enumerate(scans)]
    dscans = [pipeline.upload_scan(s, dev) for s in scans]
    losses = dh.train_step(pipeline.make_grounding_batch(dscans, anns), build_optim_wrapper(cfg))
    torch.cuda.synchronize()
    assert losses and all(math.isfinite(float(v)) for v in losses.values()), losses
    dh.train(False)
    data = dh.data_preprocessor(pipeline.make_grounding_batch(dscans, anns), False)
    res = dh.forward(data['inputs'], data['data_samples'], mode='predict')
    torch.cuda.synchronize()
    assert len(res) == 2
    for r in res:
        boxes = r.pred_instances_3d.bboxes_3d
        boxes = getattr(boxes, 'tensor', boxes)
        assert bool(torch.isfinite(boxes).all())
