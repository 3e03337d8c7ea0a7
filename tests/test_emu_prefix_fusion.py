"""tests/test_gpu_prefix_fusion.py on the CPU emulator (tests/emu): the same bodies with smaller n (every V and C kept), under the
`emulated` fixture of tests/test_emu_product.py (random thread schedule) and under schedules 0 and 1.  Then the checker itself:
correct outputs with ONE thing wrong -- a cnt off by one, one frame's rows shifted, one suffix term dropped -- must be rejected.
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import pytest
import torch

import prefix_spec as S
import test_gpu_prefix_fusion as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


def _schedule(order):
    import build as emu_build
    lib = ctypes.CDLL(emu_build.build())
    lib.es_emu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    lib.es_emu_set_schedule(order, 4242)


def test_prefix_fusion_on_the_shape_grid(emulated):  # noqa: F811
    T.test_prefix_fusion_on_the_shape_grid(emulated)


def test_prefix_forward_refusals_write_nothing(emulated):  # noqa: F811
    T.test_prefix_forward_refusals_write_nothing(emulated)


@pytest.mark.parametrize('order', [0, 1])
def test_prefix_fusion_under_other_schedules(emulated, order):  # noqa: F811
    """forward and backward under the ascending and the descending thread schedule (the fixture's default is the random one)"""
    _schedule(order)
    sf, sb = S.Stats(f'forward, schedule {order}'), S.Stats(f'backward, schedule {order}')
    for i, (V, C, n, B, blind, cluster, acc) in enumerate(((3, 40, 150, 1, 1, 70, 1), (10, 256, 37, 2, 2, 0, 0), (20, 32, 45, 1, 0, 0, 1))):
        rec = T.fwd_case(emulated, sf, S.make_case(V, C, n, 5, 7, i % 2, 3000 + i, B=B, blind=blind, cluster=cluster), 8)
        T.bwd_case(emulated, sb, rec, acc, 3100 + i)
    print(sf.report())
    print(sb.report())


def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the checker accepted {what}')


def test_checker_rejects_mutated_outputs(emulated):  # noqa: F811
    """a correct launch (it passes) with one thing wrong"""
    dev = emulated
    for acc in (0, 1):
        rec = T.fwd_case(dev, S.Stats('good'), S.make_case(4, 40, 150, 5, 7, 1, 4000, blind=1, cluster=70), 8)
        brec = T.bwd_case(dev, S.Stats('good'), rec, acc, 4100, old=False)
        V, n, C = rec['V'], rec['n'], rec['C']
        cnt = rec['cnt'].clone()
        i = int(torch.nonzero(cnt[V - 1] >= 2)[0])
        cnt[V - 1, i] += 1                                    # one cnt off by one (the step from the prefix before is then 2, too)
        _rejected(lambda: S.check_prefix_fwd(dict(rec, cnt=cnt), dev, S.Stats('cnt')), 'a cnt off by one')
        cnt = rec['cnt'].clone()
        cnt[V - 1, i] -= 1                                    # ... and one that keeps the steps legal: only the quotient is wrong
        if int(cnt[V - 1, i]) >= int(cnt[V - 2, i]):
            _rejected(lambda: S.check_prefix_fwd(dict(rec, cnt=cnt), dev, S.Stats('cnt')), 'a cnt one too low')
        out = rec['out'].clone()
        out[2 * n:3 * n] = out[2 * n:3 * n].roll(1, 0)        # one frame's rows shifted by one voxel
        _rejected(lambda: S.check_prefix_fwd(dict(rec, out=out), dev, S.Stats('shift')), 'the rows of one frame shifted')
        # one suffix term dropped: the contribution of prefix t = V - 1 to view v of one voxel taken out of its pixel
        pix = rec['pix']
        hit = torch.nonzero((pix[:, 1:V - 1] >= 0) & (rec['cnt'][V - 1] > 0)[:, None])[0]
        i, v = int(hit[0]), int(hit[1]) + 1
        term = brec['dout'][(V - 1) * n + i] / float(rec['cnt'][V - 1, i])
        df = brec['dfeats'].clone()
        df[v * rec['Hf'] * rec['Wf'] + int(pix[i, v])] -= term
        _rejected(lambda: S.check_prefix_bwd(dict(brec, dfeats=df), dev, S.Stats('suffix')), 'a gradient with one suffix term dropped')
