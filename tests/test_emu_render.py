"""tests/test_gpu_render.py on the CPU emulator (tests/emu): the same bodies under the `emulated` fixture of tests/test_emu_product.py,
with the ascending, the descending and the random thread schedule; the three kernels must appear in the launch log and a refused call
must not.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import pytest

import test_gpu_render as T
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
def test_frame_shapes_and_layouts(emulated, launched, order):  # noqa: F811
    _schedule(order)
    for H, W in T.SHAPES:
        T.test_frame_shapes_and_layouts(emulated, H, W, order % 2)
    assert {'k_render_project', 'k_render_boxes'} <= launched()


@pytest.mark.parametrize('order', [0, 1, 2])
def test_counts_around_the_chunk(emulated, order):  # noqa: F811
    _schedule(order)
    for n in T.COUNTS:
        T.test_counts_around_the_chunk(emulated, n)


def test_line_widths_and_weights(emulated):  # noqa: F811
    for radius_q in (1, 4, 10):
        for alpha in (0, 192, 256):
            T.test_line_widths_and_weights(emulated, radius_q, alpha)


def test_in_place_and_population(emulated):  # noqa: F811
    T.test_in_place_on_hwc_frames(emulated)
    T.test_population_holds_every_kind(emulated)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_occupancy(emulated, launched, order):  # noqa: F811
    _schedule(order)
    for shape in T.GRIDS:
        T.test_occupancy_grids_and_cameras(emulated, shape)
    T.test_occupancy_odd_frames_and_weights(emulated)
    assert 'k_render_occupancy' in launched()


def test_refusals_write_nothing(emulated, launched):  # noqa: F811
    T.test_refusals_write_nothing(emulated)
    log = launched()
    assert 'k_render_project' in log and not {'k_render_boxes', 'k_render_occupancy'} & log, 'a refused call launched a kernel'


def test_render_module_against_the_spec(emulated, launched):  # noqa: F811
    T.test_render_module_against_the_spec(emulated)
    assert {'k_render_project', 'k_render_boxes', 'k_render_occupancy'} <= launched()
