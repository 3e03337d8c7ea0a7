"""tests/test_gpu_tracks.py on the CPU emulator (tests/emu): the same bodies under the `emulated` fixture of tests/test_emu_product.py,
with the ascending, the descending and the random thread schedule; k_track_assign must appear in the launch log, and after a refusal
it must not.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import pytest

import test_gpu_tracks as T
import track_spec as S
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
def test_walks_under_every_schedule(emulated, launched, order):  # noqa: F811
    _schedule(order)
    for seed in S.SEEDS[order::3]:
        T.walk_case(emulated, seed)
    assert {'k_track_assign', 'k_box3d_iou'} <= launched()


def test_track_table_interface(emulated, launched):  # noqa: F811
    T.test_track_table_interface(emulated)
    assert 'k_track_assign' in launched()


@pytest.mark.parametrize('order', [0, 1, 2])
def test_sizes_around_the_wave(emulated, order):  # noqa: F811
    _schedule(order)
    for n in (0, 1, 63, 64, 65):
        for m in (0, 1, 63, 64, 65, 257):
            T.size_case(emulated, n, m, same_class=(n + m) % 2 == 1)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_staircase_and_edges(emulated, launched, order):  # noqa: F811
    _schedule(order)
    T.test_staircase_takes_one_pair_per_round(emulated)
    T.test_rules_at_their_edges(emulated)
    T.test_a_full_table_drops_births(emulated)
    T.test_ageing_at_its_edge(emulated)
    assert 'k_track_assign' in launched()


def test_refusals_write_nothing(emulated, launched):  # noqa: F811
    T.test_refusals_write_nothing(emulated)
    assert 'k_track_assign' not in launched(), 'a refused call launched the kernel'
