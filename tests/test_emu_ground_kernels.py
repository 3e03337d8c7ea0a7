"""tests/test_gpu_ground_kernels.py on the CPU emulator (tests/emu): the same bodies on their reduced grid (B <= 2, H <= 2, L <= 130,
every tile edge, all three softmax regimes, es_attn_bwd in both matrix-core modes, both LSA kernels, the top-k dynamic-LDS branch),
under the `emulated` fixture of tests/test_emu_product.py (random thread schedule); attention and LayerNorm backward also under
schedules 0 and 1.  Then the checker itself: mutated outputs -- each a correct output with ONE thing wrong -- must be rejected.
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import numpy as np
import pytest
import torch

import ground_spec as S
import test_gpu_ground_kernels as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


def _schedule(order):
    import build as emu_build
    lib = ctypes.CDLL(emu_build.build())
    lib.es_emu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    lib.es_emu_set_schedule(order, 4242)


@pytest.fixture
def launched(emulated):  # noqa: F811
    """the set of kernels launched since the previous call (the log is emptied first)"""
    import build as emu_build
    lib = ctypes.CDLL(emu_build.build())

    def take():
        buf = ctypes.create_string_buffer(1 << 22)
        lib.es_emu_take_launch_log(buf, len(buf))
        return {ln.split(' grid=')[0] for ln in buf.value.decode().splitlines()}
    take()
    return take


def test_attention_fwd_bwd_on_the_tile_edge_grid(emulated, launched):  # noqa: F811
    T.test_attention_fwd_bwd_on_the_tile_edge_grid(emulated)
    assert {f'k_attn_{k}<{m}>' for k in ('fwd', 'bwd_dq', 'bwd_dkv') for m in ('true', 'false')} | {'k_attn_delta'} <= launched()


@pytest.mark.parametrize('order', [0, 1])
def test_attention_and_layernorm_backward_under_other_schedules(emulated, order):  # noqa: F811
    """es_attn_bwd (both modes) and es_layernorm_bwd under the ascending and the descending thread schedule (the fixture's default is
    the random one)"""
    _schedule(order)
    stats = S.Stats(f'schedule {order}')
    for bf in (0, 1):
        T.attn_case(emulated, stats, bf, 'ascending', 2, 2, 65, 97, [97, 33], bf, 40 + bf)
    for n, C in ((33, 65), (70, 512)):
        T.ln_case(emulated, stats, n, C, 1, 1, 1, 1, 44)
    print(stats.report())


def test_attention_reference_alone_meets_the_bounds():
    T.test_attention_reference_alone_meets_the_bounds()


def test_attention_sample_without_valid_keys(emulated):  # noqa: F811
    T.test_attention_sample_without_valid_keys(emulated)


def test_attention_refuses_unaligned_leading_dimensions(emulated):  # noqa: F811
    T.test_attention_refuses_unaligned_leading_dimensions(emulated)


def test_layernorm_fwd_bwd_on_the_shape_grid(emulated):  # noqa: F811
    T.test_layernorm_fwd_bwd_on_the_shape_grid(emulated)


def test_layernorm_refusals_leave_the_outputs_untouched(emulated):  # noqa: F811
    T.test_layernorm_refusals_leave_the_outputs_untouched(emulated)


def test_contrastive_fwd_bwd_on_the_shape_grid(emulated):  # noqa: F811
    T.test_contrastive_fwd_bwd_on_the_shape_grid(emulated)


def test_contrastive_refuses_a_text_block_beyond_the_lds(emulated):  # noqa: F811
    T.test_contrastive_refuses_a_text_block_beyond_the_lds(emulated)


def test_contrastive_tout_below_the_token_count(emulated):  # noqa: F811
    T.test_contrastive_tout_below_the_token_count(emulated)
    T.test_contrastive_tout_at_least_t_is_unchanged(emulated)


def test_box_coders_at_the_clamp(emulated):  # noqa: F811
    T.test_box_coders_at_the_clamp(emulated)


def test_assignment_on_tied_costs_through_k_lsa_wave_and_k_lsa(emulated, launched):  # noqa: F811
    """Q up to 1024 through k_lsa_wave, Q = 1025 through the serial k_lsa"""
    T.test_assignment_on_tied_costs_through_both_solvers(emulated)
    assert {'k_ground_cost', 'k_lsa_wave', 'k_lsa'} <= launched()


def test_focal_loss_per_element(emulated):  # noqa: F811
    T.test_focal_loss_per_element(emulated)


def test_topk_sorted_on_the_length_grid(emulated):  # noqa: F811
    """es_topk_sorted up to L = 16384: the dynamic-LDS branch (L > 8192) included"""
    T.test_topk_sorted_on_the_length_grid(emulated)
    T.test_topk_sorted_treats_the_two_zeros_as_equal(emulated)


def test_box3d_iou_closed_form_quarter_turns_thin_boxes(emulated):  # noqa: F811
    T.test_box3d_iou_closed_form_quarter_turns_thin_boxes(emulated)


# ------------------------------------------------------------------------------------------------------------ the checker rejects
def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the checker accepted {what}')


@pytest.mark.parametrize('bf', [0, 1])
def test_checker_rejects_wrong_attention_gradients(bf):
    """a correct output (the f32 evaluation of the formula, which passes) with one thing wrong: dK with one 32-query step left out,
    delta taken from a different O, dQ without the final scale, one padded key given probability, one element of dV off by 2^-7
    relative"""
    dev = torch.device('cpu')
    B, H, Lq, Lk = 2, 2, 65, 70
    kl = torch.tensor([37, 70], dtype=torch.int32)
    for regime in T.REGIMES:
        q, k, v, do = T.attn_inputs(regime, B, H, Lq, Lk, 21)
        good = S.attn_ref(q, k, v, do, kl, B, H, Lq, Lk, bf)
        base = dict(B=B, H=H, Lq=Lq, Lk=Lk, bf=bf, q=q, k=k, v=v, klen=kl, o=good['o'], lse=good['lse'].reshape(-1), do=do, acc=0)
        S.check_attn_bwd(dict(base, dq=good['dq'], dk=good['dk'], dv=good['dv']), dev, S.Stats('good'))
        for mut in ('dk_skip_qstep', 'delta_other_o', 'dq_no_scale', 'pad_leak'):
            bad = S.attn_ref(q, k, v, do, kl, B, H, Lq, Lk, bf, mutate=mut, o=good['o'], lse=good['lse'])
            _rejected(lambda: S.check_attn_bwd(dict(base, dq=bad['dq'], dk=bad['dk'], dv=bad['dv']), dev, S.Stats(mut)), f'{mut} ({regime}, bf16={bf})')
    # one element of dV off by 2^-7 relative.  In bf16 mode the rounding of P legitimately moves dV by up to 2^-8 sum_q P |dO|, so the
    # error shows where |dV| > sum_q P |dO| / 2: with few queries per key (Lq = 3 here) and at the element that cancels least
    Lq = 3
    for regime in T.REGIMES:
        q, k, v, do = T.attn_inputs(regime, B, H, Lq, Lk, 22)
        good = S.attn_ref(q, k, v, do, kl, B, H, Lq, Lk, bf)
        base = dict(B=B, H=H, Lq=Lq, Lk=Lk, bf=bf, q=q, k=k, v=v, klen=kl, o=good['o'], lse=good['lse'].reshape(-1), do=do, acc=0)
        S.check_attn_bwd(dict(base, dq=good['dq'], dk=good['dk'], dv=good['dv']), dev, S.Stats('good'))
        P = torch.exp(torch.einsum('bhqd,bhkd->bhqk', S._heads(q, B, Lq, H) * S.S32, S._heads(k, B, Lk, H)) - good['lse'][..., None])
        mag = S._rows(P.transpose(-1, -2) @ S._heads(do, B, Lq, H).abs(), B, Lk, H)
        live = (torch.arange(Lk)[None, :] < kl[:, None]).reshape(-1, 1)
        i = int((good['dv'].abs() / mag.clamp(min=1e-30) * live).argmax())
        dv = good['dv'].clone()
        dv.view(-1)[i] *= 1 + 2.0 ** -7
        _rejected(lambda: S.check_attn_bwd(dict(base, dq=good['dq'], dk=good['dk'], dv=dv), dev, S.Stats('dv')), f'dV off by 2^-7 ({regime}, bf16={bf})')


def test_checker_rejects_wrong_layernorm_and_contrastive_sums():
    """dw missing one workgroup's partial (rows 32 .. 63); dtext with one visual row dropped"""
    dev = torch.device('cpu')
    g = torch.Generator().manual_seed(31)
    n, C = 100, 65
    z, dy, w = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g), torch.rand(C, generator=g) + .5
    mean = z.mean(1)
    rstd = 1 / torch.sqrt(z.var(1, unbiased=False) + 1e-5)
    dz, dw, db = S.ln_bwd_ref(dy, z, w, mean, rstd)
    zero = torch.zeros(C)
    rec = dict(dy=dy, z=z, w=w, mean=mean, rstd=rstd, dz=dz, dz0=None, dw0=zero, dw1=dw, db0=zero, db1=db)
    S.check_layernorm_bwd(rec, dev, S.Stats('good'))
    _, dw_bad, db_bad = S.ln_bwd_ref(dy, z, w, mean, rstd, skip_rows=(32, 64))
    _rejected(lambda: S.check_layernorm_bwd(dict(rec, dw1=dw_bad), dev, S.Stats('dw')), 'dw without one workgroup\'s partial')
    _rejected(lambda: S.check_layernorm_bwd(dict(rec, db1=db_bad), dev, S.Stats('db')), 'db without one workgroup\'s partial')
    B, L, Tt, Cc, Tout = 2, 20, 9, 100, 11
    v, text = torch.randn(B, L, Cc, generator=g), torch.randn(B, Tt, Cc, generator=g)
    tlen = torch.tensor([9, 5], dtype=torch.int32)
    dl = torch.randn(B, L, Tout, generator=g) * (torch.arange(Tout)[None, None, :] < tlen[:, None, None])
    dv, dt, dbias = S.contrastive_bwd_ref(dl, v, text, tlen, B, L, Tt, Cc, Tout)
    rec = dict(B=B, L=L, T=Tt, C=Cc, Tout=Tout, dl=dl, v=v, text=text, tlen=tlen, dv=dv, dv0=None, dtext0=torch.zeros(B, Tt, Cc), dtext1=dt,
               dbias0=torch.zeros(1), dbias1=dbias.reshape(1))
    S.check_contrastive_bwd(rec, dev, S.Stats('good'))
    _, dt_bad, _ = S.contrastive_bwd_ref(dl, v, text, tlen, B, L, Tt, Cc, Tout, drop_row=(1, 7))
    _rejected(lambda: S.check_contrastive_bwd(dict(rec, dtext1=dt_bad), dev, S.Stats('dtext')), 'dtext with one visual row dropped')


def test_checker_rejects_another_tie_resolution_and_swapped_ties():
    """an assignment of equal total cost but a different tie resolution; a top-k with two tied rows swapped"""
    cost = np.array([[[1.0, 1.0, 2.0, 5.0], [3.0, 3.0, 1.0, 5.0]]])
    col = S.lsa_port(cost[0])
    q2g = np.full((1, 4), -1)
    for r, c in enumerate(col):
        q2g[0, c] = r
    S.check_assignment('good', cost, [2], q2g)
    other = q2g.copy()
    other[0, [0, 1]] = other[0, [1, 0]]                        # row 0 moves to the other column of cost 1
    assert not np.array_equal(other, q2g)
    _rejected(lambda: S.check_assignment('ties', cost, [2], other), 'an optimal assignment with another tie resolution')
    twice = q2g.copy()
    twice[0, :] = [0, 0, 1, -1]
    _rejected(lambda: S.check_assignment('twice', cost, [2], twice), 'a box matched twice')
    worse = np.array([[-1, -1, 0, 1]])
    _rejected(lambda: S.check_assignment('worse', cost, [2], worse), 'a matching that is not optimal')
    vals = torch.tensor([[0.5, 2.0, 0.5, -1.0, 2.0]])
    good = torch.tensor([[1, 4, 0, 2, 3]], dtype=torch.int32)
    S.check_topk('good', vals, None, 5, good)
    _rejected(lambda: S.check_topk('swapped', vals, None, 5, torch.tensor([[4, 1, 0, 2, 3]], dtype=torch.int32)), 'a top-k with two tied rows swapped')
