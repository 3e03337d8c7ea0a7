"""tests/test_gpu_ground_answers.py on the CPU emulator (tests/emu): the same bodies under the `emulated` fixture of
tests/test_emu_product.py, with the ascending, the descending and the random thread schedule; k_ground_answers must appear in the
launch log (and must not after a refusal).  The figures ground_answers_spec.conditions() rests on are pinned here on the CPU.
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import pytest

import ground_answers_spec as G
import scene_filter_spec as F
import test_gpu_ground_answers as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)
from test_emu_scene_filter import _schedule, launched  # noqa: F401


def test_conditions_of_the_three_populations():
    """the table the thresholds (IoU 0.25, score 0.4, topk 96 / 8 / 1) were chosen by: f64 oracle matrix, labels ignored"""
    want = {1: (8.4e-4, 28, 57, 38, 2), 3: (3.6e-4, 34, 60, 44, 5), 4: (6.6e-4, 29, 53, 38, 3)}
    for seed in G.SEEDS:
        pop = G.population(seed)
        assert len(pop['scores']) == G.Q and int((pop['scores'] == 0.5).sum()) == 10
        c = G.conditions(pop, F.oracle_iou(seed))
        gap, full, no_sup, no_thr, tied = want[seed]
        assert abs(c['gap'] - gap) < 0.05e-4 and c['kept'] == {G.Q: full, 8: 8, 1: 1}
        assert (c['no_suppression'], c['no_score_thr'], c['tied_kept']) == (no_sup, no_thr, tied)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_three_prompts_under_every_schedule(emulated, launched, order):  # noqa: F811
    _schedule(order)
    T.three_references(emulated)
    # (k_box3d_iou, reference (a), runs once per process: the matrix is shared between the schedules)
    assert {'k_ground_answers', 'k_box3d_iou_filter', 'k_topk_sorted'} <= launched()


def test_sixty_four_prompts_in_one_launch(emulated, launched):  # noqa: F811
    T.many_prompts(emulated, (8,))
    assert 'k_ground_answers' in launched()


@pytest.mark.parametrize('order', [0, 1, 2])
def test_sizes_around_the_workgroup_and_the_limit(emulated, order):  # noqa: F811
    _schedule(order)
    for q in T.SIZES:
        T.size_case(emulated, q)


@pytest.mark.parametrize('order', [0, 1, 2])
def test_rules_at_their_edges(emulated, launched, order):  # noqa: F811
    _schedule(order)
    T.edge_cases(emulated)
    assert 'k_ground_answers' in launched()


def test_no_rows_and_no_prompts(emulated, launched):  # noqa: F811
    T.empty_cases(emulated)
    assert 'k_ground_answers' not in launched(), 'Q = 0 / P = 0 launched the selection kernel'


def test_refusals_write_nothing(emulated, launched):  # noqa: F811
    T.refusal_cases(emulated)
    assert launched() == set(), 'a refused call launched something'


def test_select_answers(emulated, launched, monkeypatch):  # noqa: F811
    T.select_answers_case(emulated, monkeypatch)
    assert 'k_ground_answers' in launched()
