"""tests/test_gpu_rowops.py on the CPU emulator (tests/emu): the same bodies, every case below 2^17 rows, under the `emulated` fixture
of tests/test_emu_product.py (the product's host layer on the emulated library, random thread schedule).  Each case also asserts,
through es_emu_take_launch_log, which kernels its branch label names: the GPU has no launch log, so this is what keeps the GPU
module's labels true when a dispatch rule changes.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import pytest

import test_gpu_rowops as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


@pytest.fixture
def launched(emulated):  # noqa: F811
    """the kernels launched since the previous call (the log is emptied first)"""
    import build as emu_build
    lib = ctypes.CDLL(emu_build.build())

    def take():
        buf = ctypes.create_string_buffer(1 << 20)
        lib.es_emu_take_launch_log(buf, len(buf))
        return [ln.split(' grid=')[0] for ln in buf.value.decode().splitlines()]
    take()
    return take


def test_norm_one_launch_chunked_and_scalar_branches(emulated, launched):  # noqa: F811
    T.test_norm_every_branch(emulated, launched)


def test_norm_segments_empty_one_row_and_es_max_seg(emulated, launched):  # noqa: F811
    T.test_norm_segments(emulated, launched)


def test_norm_refuses_33_segments(emulated, launched):  # noqa: F811
    T.test_norm_refuses_33_segments(emulated, launched)


def test_norm_options_15_17_9(emulated, launched):  # noqa: F811
    T.test_norm_options_select_paths_that_all_meet_the_specification(emulated, launched)


def test_affine_act_float4_scalar_and_bf16_activation(emulated, launched):  # noqa: F811
    T.test_affine_act_every_branch(emulated, launched)


def test_maxpool_ties_missing_taps_empty_windows(emulated, launched):  # noqa: F811
    T.test_maxpool_ties_missing_taps_empty_windows(emulated, launched)


def test_minkresnet_pool_map_has_disjoint_windows(emulated):  # noqa: F811
    T.test_minkresnet_pool_map_has_disjoint_windows(emulated)


def test_row_move_axpy_relu(emulated, launched):  # noqa: F811
    T.test_row_move_axpy_relu(emulated, launched)


def test_upsample_nearest_add(emulated, launched):  # noqa: F811
    T.test_upsample_nearest_add(emulated, launched)


def test_reg_decode_on_the_head_layout(emulated, launched):  # noqa: F811
    T.test_reg_decode_on_the_head_layout(emulated, launched)


def test_interp_scores_row_max_argmax_bn_fold(emulated, launched):  # noqa: F811
    T.test_interp_scores_row_max_argmax_bn_fold(emulated, launched)
