"""The FCAF3D head's backward entry points under the CDNA emulator of tests/emu (two thread schedules): the generative transposed
convolution's weight gradient in one launch (es_gen_transpose_wgrad_bf16) against the eight per-tap launches, bit for bit; the focal loss
that clears the rest of its gradient rows (es_focal_loss_clear) against es_focal_loss.  The cases are those of
tests/test_gpu_head_backward.py (tests/head_backward_cases.py).  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import numpy as np
import pytest

import head_backward_cases as cases
from test_emu_kernels import emu  # noqa: F401  (the fixture)


class _Buf:
    def __init__(self, a):
        self.a = np.array(a, copy=True, order='C')
        self.ptr = self.a.ctypes.data
        assert self.ptr % 16 == 0

    def get(self):
        return self.a.copy()


class _Backend:
    def __init__(self, emu):
        self.emu = emu

    def fn(self, name):
        return self.emu.fns[name]

    def put(self, a):
        return _Buf(a)

    def launches(self):
        self.last_log = self.emu.launches()
        return self.last_log


@pytest.fixture
def be(emu):  # noqa: F811
    return _Backend(emu)


def test_fused_generative_weight_gradient_equals_the_per_tap_launches(be):
    todo = cases.gen_wgrad_cases(be)
    assert todo[2][0] > 1
    split = [cases.check_gen_wgrad(be, *c, seed=i) for i, c in enumerate(todo)]
    assert split[2] > 0                                      # the last case splits its rows through the workspace
    cases.check_gen_wgrad_unserved(be)


def test_fused_generative_weight_gradient_on_the_128_tile(be):
    """the kernel the up-sampling blocks of the detector run (k_spconv_wgrad_bf16_big<0, 0>; the small shapes above run the whole-stage
    64 x 64 kernel, switched off here by library option 24): one slice with accumulation, and rows split over two slices"""
    assert be.fn('es_set_option')(24, 0) == 0
    try:
        assert cases.check_gen_wgrad(be, 512, 128, 128, 0, 1, seed=10) == 0
        assert 'k_spconv_wgrad_bf16_big' in be.last_log[0]
        assert cases.check_gen_wgrad(be, 600, 256, 128, 8, 0, seed=11) > 0
        assert 'k_spconv_wgrad_bf16_big' in be.last_log[0]
    finally:
        be.fn('es_set_option')(24, 256)


@pytest.mark.parametrize('N', [5, 4 * 2048 + 3])
def test_focal_loss_clear_equals_focal_loss_and_clears_the_rest(be, N):
    cases.check_focal_clear(be, N)
