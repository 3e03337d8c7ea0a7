"""tests/test_gpu_grad_rows_bf16_kernels.py on the CPU emulator (tests/emu): the same bodies under the `emulated` fixture of
tests/test_emu_product.py -- the join kernel with bf16 rows and its three readers, bit for bit against the f32-rows launches.
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import pytest

import test_gpu_grad_rows_bf16_kernels as T
from test_emu_product import emulated  # noqa: F401


@pytest.mark.parametrize('rows', [1, 5, 257, 4099])
def test_join_bf16_rows_are_the_rounded_f32_rows(emulated, rows):  # noqa: F811
    T.run_join(emulated, rows)


@pytest.mark.parametrize('n', [4096, 4161])
def test_rows_wgrad1_on_bf16_rows(emulated, n):  # noqa: F811
    T.run_rows_wgrad(emulated, n)


@pytest.mark.parametrize('n', [300, 5000])
def test_map_wgrad_on_pre_rounded_rows(emulated, n):  # noqa: F811
    T.run_map_wgrad(emulated, n)


@pytest.mark.parametrize('n', [257, 4099])
def test_gated_data_gradient_on_bf16_rows(emulated, n):  # noqa: F811
    T.run_gated_dgrad(emulated, n)


@pytest.mark.parametrize('H,W', [(10, 6), (18, 16), (9, 7)])
def test_stride2_data_gradient_on_bf16_rows(emulated, H, W):  # noqa: F811
    T.run_s2_dgrad(emulated, H, W)
