"""tests/test_gpu_walk_step.py on the CPU emulator (tests/emu): the same bodies with smaller n (every T and C kept), under the `emulated`
fixture of tests/test_emu_product.py (random thread schedule) and under schedules 0 and 1.  Then the checker itself: a correct walk
with ONE thing wrong -- an nvalid off by one, a step whose add was skipped on a voxel with a hit, one step's rows shifted by one voxel
-- must be rejected.
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import pytest
import torch

import prefix_spec as S
import test_gpu_walk_step as T
import walk_spec as W
from test_emu_prefix_fusion import _rejected, _schedule
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


def test_walk_step_on_the_shape_grid(emulated):  # noqa: F811
    T.test_walk_step_on_the_shape_grid(emulated)


def test_walk_step_refusals_write_nothing(emulated):  # noqa: F811
    T.test_walk_step_refusals_write_nothing(emulated)


@pytest.mark.parametrize('order', [0, 1])
def test_walk_step_under_other_schedules(emulated, order):  # noqa: F811
    """under the ascending and the descending thread schedule (the fixture's default is the random one)"""
    _schedule(order)
    st = W.Stats(f'walk step, schedule {order}')
    for i, (V, C, n, B, blind, cluster, pad) in enumerate(((3, 40, 50, 1, 1, 20, 8), (10, 256, 37, 2, 2, 0, 0), (10, 512, 37, 1, 0, 0, 8))):
        T.walk_case(emulated, st, S.make_case(V, C, n, 5, 7, i % 2, 6500 + i, B=B, blind=blind, cluster=cluster), pad)
    print(st.report())


def test_checker_rejects_mutated_walks(emulated):  # noqa: F811
    """a correct walk (it passes) with one thing wrong"""
    dev = emulated
    case, steps = T.walk_case(dev, W.Stats('good'), S.make_case(4, 40, 50, 5, 7, 1, 6600, blind=1, cluster=20), 8)
    V, n = case['V'], case['n']

    def mutated(t, **kw):
        return [dict(s, **{k: f(s[k].clone()) for k, f in kw.items()}) if j == t else s for j, s in enumerate(steps)]

    i = int(torch.nonzero(steps[V - 1]['nvalid'] >= 2)[0])

    def up(c):
        c[i] += 1
        return c

    def down(c):
        c[i] -= 1
        return c
    _rejected(lambda: W.check_walk(case, mutated(V - 1, nvalid=up), dev, W.Stats('nvalid')), 'an nvalid one too high')
    if int(steps[V - 1]['nvalid'][i]) - 1 >= int(steps[V - 2]['nvalid'][i]):        # (keeps the steps legal: only the quotient is wrong)
        _rejected(lambda: W.check_walk(case, mutated(V - 1, nvalid=down), dev, W.Stats('nvalid')), 'an nvalid one too low')
    # a step whose add was skipped on a voxel with a hit: the output the kernel would have written from the sum WITHOUT that view's row
    t = 2
    hit = torch.nonzero((steps[t]['pix'] >= 0) & (steps[t]['nvalid'] > 0))
    j = int(hit[0])
    row = case['feats'].reshape(-1, case['Hf'] * case['Wf'], case['C'])[t, int(steps[t]['pix'][j])]
    assert float(row.abs().max()) > 0

    def skipped(o):
        o[j] -= row / float(steps[t]['nvalid'][j])
        return o
    _rejected(lambda: W.check_walk(case, mutated(t, out=skipped), dev, W.Stats('skip')), 'a step whose add was skipped on a voxel with a hit')
    _rejected(lambda: W.check_walk(case, mutated(t, out=lambda o: o.roll(1, 0)), dev, W.Stats('shift')), "one step's rows shifted by one voxel")
    W.check_walk(case, mutated(t), dev, W.Stats('unchanged'))
