"""tests/test_gpu_shared_scene.py on the CPU emulator (tests/emu): the same bodies on their reduced grid under the `emulated` fixture of
tests/test_emu_product.py (random thread schedule); the prepared-operand attention also once each under the ascending and the
descending schedule; the decoder-level comparison with the oracle, the in-situ records in both modes, staleness and the empty
scene (whose ground() must launch nothing: the emulator's launch log is read).  The model-level test needs the backbones and stays on
the GPU.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import pytest
import torch

import fwd_spec as F
import test_gpu_shared_scene as T
from test_emu_ground_kernels import _schedule, launched  # noqa: F401
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


@pytest.fixture
def emulated_bf16(emulated, monkeypatch):  # noqa: F811
    """bf16 mode of a whole model on the emulator: the product's one-launch weight-cast registry is keyed by CUDA devices, so here
    a Param's bf16 copies are made by one es_cast_weight_bf16 launch each (as tests/test_emu_insitu.py does for its Params)"""
    from embodiedscan_amd import engine as E, hip

    def bf16(self):
        if self.bf_n is None or self.bf_step != E.WEIGHT_VERSION[0]:
            K, a, b = self.d.shape
            self.bf_n, self.bf_t = torch.empty((K, a, b), dtype=torch.bfloat16), torch.empty((K, b, a), dtype=torch.bfloat16)
            hip.call('es_cast_weight_bf16', hip.P(self.d), K, a, b, hip.P(self.bf_n), hip.P(self.bf_t), 0)
            self.bf_step = E.WEIGHT_VERSION[0]
        return self.bf_n, self.bf_t
    monkeypatch.setattr(E.Param, 'bf16', bf16)
    return emulated


def test_contrastive_shared_on_the_shape_grid(emulated, launched):  # noqa: F811
    T.test_contrastive_shared_on_the_shape_grid(emulated)
    assert {'k_contrastive_shared_fwd', 'k_contrastive_fwd'} <= launched()


def test_contrastive_shared_refusals_leave_the_outputs_untouched(emulated):  # noqa: F811
    T.test_contrastive_shared_refusals_leave_the_outputs_untouched(emulated)


def test_attention_kv_on_the_tile_edge_grid(emulated, launched):  # noqa: F811
    T.test_attention_kv_on_the_tile_edge_grid(emulated)
    assert {f'k_attn_kv_{k}<{m}>' for k in ('prepare', 'fwd') for m in ('true', 'false')} <= launched()


@pytest.mark.parametrize('order', [0, 1])
def test_attention_kv_under_other_schedules(emulated, order):  # noqa: F811
    _schedule(order)
    stats = F.Stats(f'schedule {order}')
    for bf in (0, 1):
        T.attn_kv_case(emulated, stats, bf, 'ascending', 2, 99, 97, 40 + bf)
        T.attn_kv_case(emulated, stats, bf, 'normal', 1, 129, 65, 42 + bf)
    print(stats.report())


def test_attention_kv_reference_alone_meets_the_bounds():
    T.test_attention_kv_reference_alone_meets_the_bounds()


def test_attention_kv_refuses_unaligned_leading_dimensions(emulated):  # noqa: F811
    T.test_attention_kv_refuses_unaligned_leading_dimensions(emulated)


def test_ground_on_tokens_vs_oracle_baseline_coder(emulated):  # noqa: F811
    T.ground_vs_oracle(emulated, 'mv_grounding.py')


def test_ground_on_tokens_vs_oracle_fcaf_coder(emulated):  # noqa: F811
    T.ground_vs_oracle(emulated, 'mv_grounding_fcaf.py')


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_ground_records_in_situ(emulated_bf16, mode):
    T.ground_records_in_situ(emulated_bf16, mode)


def test_stale_encodings_are_refused_and_the_edges(emulated_bf16, launched):
    det = T.staleness_and_edges(emulated_bf16)
    launched()
    T.empty_scene(emulated_bf16, det)
    assert launched() == set(), 'ground() on an empty scene must launch nothing'
