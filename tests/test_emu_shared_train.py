"""tests/test_gpu_shared_train.py on the CPU emulator (tests/emu): the scatter-sum kernel on its reduced grid (random thread schedule, and once
each under the ascending and the descending one), its refusals, the token-level comparison of loss_shared_from_tokens with the oracle and with
`loss` on the replicated tokens, and the in-situ records of the shared path in both modes.  The model-level test needs the backbones and stays
on the GPU.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import pytest

import test_gpu_shared_train as T
from test_emu_ground_kernels import _schedule, launched  # noqa: F401
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)
from test_emu_shared_scene import emulated_bf16  # noqa: F401


def test_scatter_sum_on_the_shape_grid(emulated, launched):  # noqa: F811
    T.test_scatter_sum_on_the_shape_grid(emulated)
    assert {'k_scatter_table', 'k_scatter_sum<4>', } <= launched()


@pytest.mark.parametrize('order', [0, 1])
def test_scatter_sum_under_other_schedules(emulated, order):  # noqa: F811
    _schedule(order)
    for n, (L, P_, Q, C, acc, kind) in enumerate(((33, 5, 33, 4, 1, 'same'), (1029, 2, 33, 8, 0, 'common'), (5, 5, 4, 3, 1, 'random'))):
        T.scatter_case(emulated, L, P_, Q, C, acc, kind, 40 + n)


def test_scatter_sum_order_sensitive_triple_is_order_sensitive():
    T.test_scatter_sum_order_sensitive_triple_is_order_sensitive()


def test_scatter_sum_refusals_leave_the_outputs_untouched(emulated, launched):  # noqa: F811
    launched()
    T.test_scatter_sum_refusals_leave_the_outputs_untouched(emulated)
    assert 'k_scatter_sum<1>' in launched()


@pytest.mark.parametrize('bf', [0, 1])
def test_attention_kv_bwd_on_the_tile_edge_grid(emulated, launched, bf):  # noqa: F811
    launched()
    T.test_attention_kv_bwd_on_the_tile_edge_grid(emulated, bf)
    m = 'true' if bf else 'false'
    assert {f'k_attn_kv_bwd_prep<{m}>', f'k_attn_kv_bwd_dkv<{m}>', f'k_attn_bwd_dq<{m}>'} <= launched()


@pytest.mark.parametrize('order', [0, 1])
def test_attention_kv_bwd_under_other_schedules(emulated, order):  # noqa: F811
    import fwd_spec as F
    _schedule(order)
    stats = F.Stats(f'schedule {order}')
    for bf in (0, 1):
        T.attn_kv_bwd_case(emulated, stats, bf, 'ascending', 2, 99, 65, bf, 60 + bf)
        T.attn_kv_bwd_case(emulated, stats, bf, 'normal', 1, 129, 130, 1 - bf, 62 + bf)
    print(stats.report())


def test_attention_kv_bwd_reference_alone_meets_the_bounds():
    T.test_attention_kv_bwd_reference_alone_meets_the_bounds()


def test_attention_kv_bwd_refusals_leave_the_outputs_untouched(emulated):  # noqa: F811
    T.test_attention_kv_bwd_refusals_leave_the_outputs_untouched(emulated)


def test_oracle_skips_few_gradient_tensors_on_these_inputs():
    T.test_oracle_skips_few_gradient_tensors_on_these_inputs()


def test_loss_shared_from_tokens_one_scene_two_prompts(emulated):  # noqa: F811
    T.shared_from_tokens_vs_oracle(emulated, 'mv_grounding.py', 1, 2, [41])


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_shared_records_in_situ(emulated_bf16, mode):  # noqa: F811
    T.shared_records_in_situ(emulated_bf16, mode, S_=2, P_=2, lens=(33, 40))
