"""tests/test_gpu_textenc.py on the CPU emulator (tests/emu): the kernel bodies on their reduced grid and the tiny f32 model, under the
`emulated` fixture of tests/test_emu_product.py (random thread schedule), the attention cases also under schedules 0 and 1.  Then the
checkers themselves: a correct output with ONE thing wrong must be rejected.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import pytest
import torch

import test_gpu_textenc as T
import textenc_spec as S
from test_emu_ground_kernels import _rejected, _schedule, launched  # noqa: F401
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


@pytest.mark.parametrize('bf', [0, 1])
def test_text_attention_on_the_tile_edge_grid(emulated, launched, bf):  # noqa: F811
    T.test_text_attention_on_the_tile_edge_grid(emulated, bf)
    assert f'k_text_attn_fwd<{"true" if bf else "false"}>' in launched()


@pytest.mark.parametrize('order', [0, 1])
def test_text_attention_under_other_schedules(emulated, order):  # noqa: F811
    """the ascending and the descending thread schedule (the fixture's default is the random one): the lanes of a wave exchange their
    tiles through LDS between barriers"""
    _schedule(order)
    stats = S.Stats(f'schedule {order}')
    for bf in (0, 1):
        T.text_attn_case(emulated, stats, bf, 'ascending', 2, 2, 130, 'hole', 60 + bf)
        T.text_attn_case(emulated, stats, bf, 'peaked', 2, 3, 17, 'prefix', 62 + bf)
    print(stats.report())


def test_text_attention_refusals(emulated):  # noqa: F811
    T.test_text_attention_refusals_leave_the_output_untouched(emulated)


def test_text_embedding(emulated, launched):  # noqa: F811
    T.test_text_embedding_positions_and_layernorm(emulated)
    T.test_text_embedding_refuses_a_row_beyond_the_position_table(emulated)
    assert 'k_text_embed_ln' in launched()


def test_bias_gelu(emulated, launched):  # noqa: F811
    T.test_bias_gelu_exact_erf_form(emulated)
    assert 'k_bias_gelu' in launched()


def test_tiny_model_f32(emulated, launched):  # noqa: F811
    T.model_f32_case(emulated, 'tiny')
    assert {'k_text_embed_ln', 'k_text_attn_fwd<false>', 'k_bias_gelu', 'k_text_add_ln'} <= launched()


# ------------------------------------------------------------------------------------------------------------ the checkers reject
@pytest.mark.parametrize('bf', [0, 1])
def test_checker_rejects_a_leaked_key_and_one_element_off(bf):
    """a masked key let through; one output element off by 2^-7 relative (bf16 mode) or by 64 u relative (f32 mode), at the element
    that cancels least (|o| / (P |v|) largest: the bound is relative to P |v|)"""
    dev = torch.device('cpu')
    B, H, Tn = 2, 2, 17
    mask = T.text_mask('prefix', B, Tn, 3)                       # lengths [17, 1]
    for regime in T.REGIMES:
        qkv = T.text_attn_inputs(regime, B, H, Tn, 11)
        good = S.text_attn_ref(qkv, mask, B, H, Tn, bf)
        rec = dict(B=B, H=H, T=Tn, bf=bf, qkv=qkv, mask=mask, o=good)
        S.check_text_attention(rec, dev, S.Stats('good'))
        bad = S.text_attn_ref(qkv, mask, B, H, Tn, bf, leak=(1, 5))
        _rejected(lambda: S.check_text_attention(dict(rec, o=bad), dev, S.Stats('leak')), f'a masked key let through ({regime}, bf16={bf})')
    # (the f32 bound is (16 + G sqrt(T)) u + 2 dS relative to P |v|: 64 u stands out of it for a short row with small scores)
    Tn = 4
    mask = T.text_mask('prefix', B, Tn, 3)                       # lengths [4, 1]
    qkv = T.text_attn_inputs('flat', B, H, Tn, 12)
    qkv[:, :H * 64] *= 0.01                                      # dS (the score GEMM's share of the bound) below 1 u
    good = S.text_attn_ref(qkv, mask, B, H, Tn, bf)
    rec = dict(B=B, H=H, T=Tn, bf=bf, qkv=qkv, mask=mask, o=good)
    S.check_text_attention(rec, dev, S.Stats('good'))
    off = good.clone()
    i = int(off[Tn:].abs().reshape(-1).argmax()) + Tn * H * 64      # sample 1 has ONE live key: o = v, nothing cancels
    off.view(-1)[i] *= 1 + (2.0 ** -7 if bf else 64 * S.U)
    _rejected(lambda: S.check_text_attention(dict(rec, o=off), dev, S.Stats('off')), f'one element off (bf16={bf})')


def test_checker_rejects_a_position_off_by_one_and_tanh_gelu():
    dev = torch.device('cpu')
    tab = T.embed_tables(128, 3)
    ids = T.embed_ids(11, 4)
    y, p = S.embed_ref(ids, T.PAD, T.VOCAB, tab['word'], tab['pos'], tab['type0'], tab['w'], tab['b'], 1e-5)
    rec = dict(tab, ids=ids, pad_id=T.PAD, vocab=T.VOCAB, eps=1e-5, y=y, pos_ids=p)
    S.check_text_embed(rec, dev, S.Stats('good'))
    p2 = p.clone()
    p2[2 * 11 + 7] += 1                                           # the token after the skipped pad
    _rejected(lambda: S.check_text_embed(dict(rec, pos_ids=p2), dev, S.Stats('pos')), 'a position id off by one')
    y2, _ = S.embed_ref(ids, T.PAD, T.VOCAB, tab['word'], tab['pos'].roll(1, 0), tab['type0'], tab['w'], tab['b'], 1e-5)
    _rejected(lambda: S.check_text_embed(dict(rec, y=y2), dev, S.Stats('row')), 'rows built from the neighbouring position')
    g = torch.Generator().manual_seed(2)
    x, bias = torch.linspace(-12, 12, 37 * 64).view(37, 64), torch.randn(64, generator=g) * 0.5
    S.check_bias_gelu(dict(x=x, bias=bias, y=S.gelu_ref(x, bias)), dev, S.Stats('good'))
    _rejected(lambda: S.check_bias_gelu(dict(x=x, bias=bias, y=S.gelu_ref(x, bias, tanh=True)), dev, S.Stats('tanh')), 'tanh-GELU')
