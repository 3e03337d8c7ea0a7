"""tests/test_gpu_scene_map.py on the CPU emulator (tests/emu): the same bodies under the `emulated` fixture of tests/test_emu_product.py,
with the ascending, the descending and the random thread schedule; the four k_map_* kernels must appear in the launch log, a refused call
must launch nothing, and a run with map=None must launch none of them.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import pytest

import test_gpu_scene_map as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)

MAP_KERNELS = {'k_map_splat', 'k_map_resolve', 'k_map_project', 'k_map_occupancy'}


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
def test_depth_and_map_shapes(emulated, launched, order):  # noqa: F811
    _schedule(order)
    for H, W in T.DEPTHS:
        for Hm, Wm in T.MAPS:
            T.test_depth_and_map_shapes(emulated, H, W, Hm, Wm)
    assert {'k_map_splat', 'k_map_resolve'} <= launched()


def test_layouts_and_population(emulated):  # noqa: F811
    T.test_both_layouts_give_one_map(emulated)
    T.test_population_holds_every_kind(emulated)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_box_counts_and_footprints(emulated, launched, order):  # noqa: F811
    _schedule(order)
    for n in T.COUNTS:
        T.test_box_counts_and_footprints(emulated, n)
    assert {'k_map_project', 'k_render_boxes'} <= launched()


@pytest.mark.parametrize('order', [0, 1, 2])
def test_occupancy_top_surface(emulated, launched, order):  # noqa: F811
    _schedule(order)
    for shape in T.GRIDS:
        T.test_occupancy_top_surface(emulated, shape)
    assert 'k_map_occupancy' in launched()


def test_refusals_write_nothing(emulated, launched):  # noqa: F811
    T.test_refusals_write_nothing(emulated)
    assert not launched(), 'a refused call (or one with V = 0 / n = 0) launched a kernel'


def test_scene_map_module_against_the_spec(emulated, launched):  # noqa: F811
    T.test_scene_map_module_against_the_spec(emulated)
    assert MAP_KERNELS | {'k_render_boxes'} <= launched()


def test_run_scene_maps_a_given_prediction(emulated, launched, tmp_path_factory, tmp_path):  # noqa: F811
    """(the whole-model bodies of tests/test_gpu_scene_map.py need the MI355X: no whole model runs on the emulator in this suite)"""
    T.test_run_scene_maps_a_given_prediction(emulated, tmp_path_factory, tmp_path, launch_log=launched)


def test_walk_maps_grow_frame_by_frame(emulated, launched, tmp_path_factory, tmp_path):  # noqa: F811
    """walk_scene(map=) on a scripted session: cont-det3d without and with track=, an occupancy volume per frame, and map=None's launch log"""
    T.test_walk_maps_grow_frame_by_frame(emulated, tmp_path_factory, tmp_path, launch_log=launched)
