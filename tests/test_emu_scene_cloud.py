"""tests/test_gpu_scene_cloud.py on the CPU emulator (tests/emu): the same bodies under the `emulated` fixture of tests/test_emu_product.py,
with the ascending, the descending and the random thread schedule for the splat, label and face cases; the six k_cloud_* / k_occ_face_*
kernels must appear in the launch log, a refused call must launch nothing, and a run with cloud=None must launch none of them.  The
whole-model bodies are left to the MI355X.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import pytest

import test_gpu_scene_cloud as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)

CLOUD_KERNELS = {'k_cloud_splat', 'k_cloud_mask', 'k_cloud_points', 'k_cloud_label', 'k_occ_face_mask', 'k_occ_face_quads'}


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
def test_depth_shapes_and_cells(emulated, launched, order):  # noqa: F811
    _schedule(order)
    for H, W in T.DEPTHS:
        for cell in T.CELLS:
            T.test_depth_shapes_and_cells(emulated, H, W, cell)
    assert {'k_cloud_splat', 'k_cloud_mask', 'k_cloud_points'} <= launched()


@pytest.mark.parametrize('order', [0, 1, 2])
def test_orders_layouts_and_small_tables(emulated, launched, order):  # noqa: F811
    _schedule(order)
    T.test_both_layouts_give_one_cloud(emulated)
    T.test_one_cloud_any_order(emulated)
    for cap in (8, 128):
        T.test_a_table_that_is_too_small_reports_it(emulated, cap)
    assert 'k_cloud_splat' in launched()


@pytest.mark.parametrize('order', [0, 1, 2])
def test_labels_and_support(emulated, launched, order):  # noqa: F811
    _schedule(order)
    for m in T.COUNTS:
        for grow in (0.0, 0.05):
            T.test_labels_and_support(emulated, m, grow)
    assert 'k_cloud_label' in launched()


@pytest.mark.parametrize('order', [0, 1, 2])
def test_exposed_faces(emulated, launched, order):  # noqa: F811
    _schedule(order)
    for shape in T.GRIDS:
        T.test_exposed_faces(emulated, shape)
    assert {'k_occ_face_mask', 'k_occ_face_quads'} <= launched()


def test_an_empty_volume_launches_only_the_mask(emulated, launched):  # noqa: F811
    import numpy as np
    T.faces_case(emulated, np.zeros((3, 2, 5), np.uint8), np.zeros(3), np.ones(3), T.N_CLASSES)
    log = launched()
    assert 'k_occ_face_mask' in log and 'k_occ_face_quads' not in log


def test_refusals_write_nothing(emulated, launched):  # noqa: F811
    T.test_refusals_write_nothing(emulated)
    assert launched() <= {'k_cloud_splat'}, 'a refused call (or one with V = 0 / n = 0) launched a kernel'     # (the one legal splat of the body)


def test_scene_cloud_module_against_the_spec(emulated, launched):  # noqa: F811
    T.test_scene_cloud_module_against_the_spec(emulated)
    assert CLOUD_KERNELS <= launched()
    T.test_scene_cloud_full(emulated)


def test_run_scene_exports_a_given_prediction(emulated, launched, tmp_path_factory, tmp_path):  # noqa: F811
    """(the whole-model bodies of tests/test_gpu_scene_cloud.py need the MI355X: no whole model runs on the emulator in this suite)"""
    T.test_run_scene_exports_a_given_prediction(emulated, tmp_path_factory, tmp_path, launch_log=launched)


def test_walk_clouds_grow_frame_by_frame(emulated, launched, tmp_path_factory, tmp_path):  # noqa: F811
    """walk_scene(cloud=, cloud_every=1) on a scripted session: cont-det3d without and with track=, an occupancy volume per frame, and
    cloud=None's launch log"""
    T.test_walk_clouds_grow_frame_by_frame(emulated, tmp_path_factory, tmp_path, launch_log=launched)
