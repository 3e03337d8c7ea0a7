"""tests/test_gpu_det_metric.py on the CPU emulator (tests/emu): the whole pipeline of embodiedscan_amd/eval -- grouping, es_det_best_gt,
es_sort_u64, es_det_mark, es_det_ap -- through the `emulated` fixture of tests/test_emu_product.py (random thread schedule) against
tests/det_metric_spec.py, on the same shape grid and under the same asserted input conditions; the marking and the curves again under
thread schedules 0 and 1.  Then the checker itself: a correct output with ONE thing wrong (one TP flag, one gt_best, one AP off by two
ulp) must be rejected.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import numpy as np
import pytest

import det_metric_spec as S
import test_gpu_det_metric as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


def _lib():
    import build as emu_build
    lib = ctypes.CDLL(emu_build.build())
    lib.es_emu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    return lib


@pytest.fixture
def launched(emulated):  # noqa: F811
    lib = _lib()

    def take():
        buf = ctypes.create_string_buffer(1 << 22)
        lib.es_emu_take_launch_log(buf, len(buf))
        return {ln.split(' grid=')[0] for ln in buf.value.decode().splitlines()}
    take()
    return take


def test_registry_builds_the_metric_of_both_detection_configs():
    import embodiedscan_amd  # noqa: F401
    from embodiedscan_amd.registry import METRICS
    assert METRICS.build(dict(type='IndoorDetMetric')).batchwise_anns is False                 # mv-3ddet
    assert METRICS.build(dict(type='IndoorDetMetric', batchwise_anns=True)).batchwise_anns     # cont-det3d


def test_grid_against_the_specification(emulated, launched):  # noqa: F811
    T.body_grid(emulated)
    assert {'k_box3d_iou_best', 'k_det_claim', 'k_det_flag', 'k_det_ap'} <= launched()


@pytest.mark.parametrize('order', [0, 1])
def test_marking_and_curves_under_other_schedules(emulated, order):  # noqa: F811
    """the cases where threads of several waves meet: > 64 predictions on one box (atomicMin), a class segment of one scan chunk and
    of one more (block scan + suffix maximum), 284 classes x 3 thresholds"""
    _lib().es_emu_set_schedule(order, 4242)
    T.body_grid(emulated, pick=lambda name: name.startswith('one class') or name.startswith('P=257') or name == 'P=65')


def test_reference_cases_and_class_splits(emulated):  # noqa: F811
    T.body_golden(emulated)


def test_refusals_leave_the_outputs_untouched(emulated):  # noqa: F811
    T.body_refusals(emulated)


def test_metric_object_through_the_registry(emulated):  # noqa: F811
    T.body_metric_object(emulated)


def test_equal_scores_rank_by_scene_then_position(emulated):  # noqa: F811
    """the project's tie rule (the reference leaves ties to an unstable argsort): -0.0 ties with +0.0 too"""
    name, scenes, C, thr = T.grid_cases()[2]
    s = scenes[0]
    box = np.repeat(s[0], 3, 0)
    sc0 = (box, np.array([0.5, 0.0, 0.5], np.float32), np.zeros(3, np.int64), s[3], s[4])
    sc1 = (box, np.array([0.5, -0.0, 0.7], np.float32), np.zeros(3, np.int64), s[3], s[4])
    _, _, got = T.run_device([sc0, sc1], 1, [0.25], emulated)
    assert got['order'].tolist() == [5, 0, 2, 3, 1, 4]
    assert got['tp'][0].tolist() == [1, 1, 0, 0, 0, 0]          # one box per scene: the first of each scene at its rank


# ------------------------------------------------------------------------------------------------------------ the checker rejects
def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the checker accepted {what}')


def test_checker_rejects_one_wrong_flag_box_or_area():
    name, scenes, C, thr = T.grid_cases()[5]                    # P = 65
    ev = T.spec_of(name, scenes, C, thr)
    good = {k: np.array(ev[k]) for k in ('iou_max', 'gt_best', 'order', 'tp', 'tp_total', 'ap')}
    S.check_outputs(ev, good, 'good')
    bad = dict(good, tp=good['tp'].copy())
    bad['tp'][1, 7] ^= 1
    _rejected(lambda: S.check_outputs(ev, bad, 'tp'), 'one TP flag flipped')
    bad = dict(good, gt_best=good['gt_best'].copy())
    i = int(np.nonzero(good['gt_best'] >= 0)[0][3])
    bad['gt_best'][i] += 1
    _rejected(lambda: S.check_outputs(ev, bad, 'gt_best'), 'one gt_best moved to the next row')
    bad = dict(good, ap=good['ap'].copy())
    c = int(np.nonzero(good['ap'][0] > 0)[0][0])
    bad['ap'][0, c] = np.nextafter(np.nextafter(bad['ap'][0, c], np.float32(2)), np.float32(2))
    _rejected(lambda: S.check_outputs(ev, bad, 'ap'), 'one AP off by two ulp')
    one = dict(good, ap=good['ap'].copy())
    one['ap'][0, c] = np.nextafter(one['ap'][0, c], np.float32(0))
    S.check_outputs(ev, one, 'one ulp')                          # ... and one ulp is what the bound allows
    bad = dict(good, iou_max=good['iou_max'].copy())
    bad['iou_max'][i] += np.float32(3e-6)
    _rejected(lambda: S.check_outputs(ev, bad, 'iou'), 'one IoU off by 3e-6')
    want = S.result_dict(scenes, C, thr, [f'c{k}' for k in range(C)], ev)
    T.check_dict(dict(want), want)
    key = next(k for k in want if '_rec_' in k)
    _rejected(lambda: T.check_dict(dict(want, **{key: want[key] + 1e-12}), want), 'one recall off by 1e-12')


def test_conditions_reject_a_prediction_on_the_threshold():
    """the condition check itself: an IoU within 1e-5 of a threshold, two boxes within 1e-5 of each other, equal scores"""
    name, scenes, C, thr = T.grid_cases()[2]
    iou_max, gt_best, second = S.best_gt(scenes)
    ev = S.evaluate(scenes, C, thr, best=(iou_max, gt_best))
    S.check_conditions(scenes, thr, ev, second)
    _rejected(lambda: S.check_conditions(scenes, [float(iou_max[0]) + 5e-6], ev, second), 'an IoU 5e-6 from the threshold')
    _rejected(lambda: S.check_conditions(scenes, thr, ev, iou_max - np.float32(5e-6)), 'a second box 5e-6 below the best')
    s = scenes[0]
    two = [(np.repeat(s[0], 2, 0), np.array([0.5, 0.5], np.float32), np.zeros(2, np.int64), s[3], s[4])]
    b = S.best_gt(two)
    _rejected(lambda: S.check_conditions(two, thr, S.evaluate(two, C, thr, best=b[:2]), b[2]), 'equal scores in a class')
