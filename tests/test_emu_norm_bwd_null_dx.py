"""tests/test_gpu_norm_bwd_null_dx.py on the CPU emulator (tests/emu): the same bodies under the `emulated` fixture of
tests/test_emu_product.py, each call also held to the kernels its path names (es_emu_take_launch_log) -- without dx the scalar path
launches no cast.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import pytest

import test_gpu_norm_bwd_null_dx as T
from test_emu_product import emulated  # noqa: F401
from test_emu_rowops import launched  # noqa: F401


@pytest.mark.parametrize('rows', T.ROWS)
def test_null_dx_keeps_every_other_output_bit_for_bit(emulated, launched, rows):  # noqa: F811
    T.run_rows(emulated, rows, launched)


def test_null_dx_on_the_scalar_path(emulated, launched):  # noqa: F811
    T.run_scalar(emulated, launched)


def test_null_dx_refused_without_bf16_rows_or_with_accumulate(emulated):  # noqa: F811
    T.run_refusals(emulated)
