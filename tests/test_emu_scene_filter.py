"""tests/test_gpu_scene_filter.py on the CPU emulator (tests/emu): the same bodies under the `emulated` fixture of
tests/test_emu_product.py, with the ascending, the descending and the random thread schedule; k_box3d_iou_filter must appear in the
launch log.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import pytest

import scene_filter_spec as S
import test_gpu_scene_filter as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


def _lib():
    import build as emu_build
    return ctypes.CDLL(emu_build.build())


def _schedule(order):
    lib = _lib()
    lib.es_emu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    lib.es_emu_set_schedule(order, 4242)


@pytest.fixture
def launched(emulated):  # noqa: F811
    """the set of kernels launched since the previous call (the log is emptied first)"""
    lib = _lib()

    def take():
        buf = ctypes.create_string_buffer(1 << 22)
        lib.es_emu_take_launch_log(buf, len(buf))
        return {ln.split(' grid=')[0] for ln in buf.value.decode().splitlines()}
    take()
    return take


@pytest.mark.parametrize('order', [0, 1, 2])
def test_clustered_populations_under_every_schedule(emulated, launched, order):  # noqa: F811
    _schedule(order)
    T.population_case(emulated, S.SEEDS[order])
    assert {'k_box3d_iou_filter', 'k_box3d_iou', 'k_topk_sorted'} <= launched()


@pytest.mark.parametrize('order', [0, 1, 2])
def test_sizes_around_the_workgroup(emulated, order):  # noqa: F811
    _schedule(order)
    for n in (0, 1, 255, 256, 257, 300):
        T.size_case(emulated, n)


def test_rules_at_their_edges(emulated, launched):  # noqa: F811
    T.test_rules_at_their_edges(emulated)
    assert 'k_box3d_iou_filter' in launched()


@pytest.mark.parametrize('order', [0, 1, 2])
def test_degenerate_boxes(emulated, order):  # noqa: F811
    _schedule(order)
    T.test_degenerate_boxes(emulated)


def test_refusals_write_nothing(emulated, launched):  # noqa: F811
    T.test_refusals_write_nothing(emulated)
    assert 'k_box3d_iou_filter' not in launched(), 'a refused call launched the kernel'


def test_filter_instances_and_overlaps(emulated, launched):  # noqa: F811
    T.test_filter_instances_and_overlaps(emulated)
    assert 'k_box3d_iou_filter' in launched()
