"""tests/test_gpu_window_fusion.py on the CPU emulator (tests/emu): the same bodies under the `emulated` fixture of
tests/test_emu_product.py (random thread schedule) and under the ascending and the descending schedule; the coverage the GPU grid
asserts is checked here first, on the same seeds.  Then the checker itself: a correct record with ONE thing wrong -- an in-window pix
turned to -1 in the adjoint's input, a beyond-window term added to a pixel, one row's gradient landed in the other image set, a cnt
off by one -- must be rejected.
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import pytest
import torch

import test_gpu_window_fusion as T
import window_spec as S
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


def _schedule(order):
    import build as emu_build
    lib = ctypes.CDLL(emu_build.build())
    lib.es_emu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    lib.es_emu_set_schedule(order, 4242)


def test_window_fusion_on_the_shape_grid(emulated):  # noqa: F811
    T.test_window_fusion_on_the_shape_grid(emulated)


def test_full_windows_are_the_existing_kernels_bit_for_bit(emulated):  # noqa: F811
    T.test_full_windows_are_the_existing_kernels_bit_for_bit(emulated)


def test_window_backward_cluster_two_sets_accumulate(emulated):  # noqa: F811
    T.test_window_backward_cluster_two_sets_accumulate(emulated)


def test_window_refusals_write_nothing(emulated):  # noqa: F811
    T.test_window_refusals_write_nothing(emulated)


@pytest.mark.parametrize('order', [0, 1])
def test_window_fusion_under_other_schedules(emulated, order):  # noqa: F811
    """forward and backward under the ascending and the descending thread schedule (the fixture's default is the random one)"""
    _schedule(order)
    sf, sb = S.Stats(f'forward, schedule {order}'), S.Stats(f'backward, schedule {order}')
    for i, (V, C, n, B, kind, n_sets, blind, cluster, acc, half) in enumerate(((3, 40, 400, 2, 'asc', 2, 1, 160, 1, 0), (10, 256, 17, 3, 'arb', 1, 2, 0, 0, 1),
                                                                               (64, 1, 150, 9, 'arb', 2, 0, 0, 1, 0))):
        case = S.make_case(V, C, n, 5, 7, i % 2, 4000 + i, B=B, kind=kind, n_sets=n_sets, blind=blind, cluster=cluster, empty=1 if B >= 3 else None)
        rec, _ = T.fwd_case(emulated, sf, case, half, ldo_pad=8)
        T.bwd_case(emulated, sb, rec, acc, 4100 + i)
    print(sf.report())
    print(sb.report())


def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the checker accepted {what}')


def test_checker_rejects_mutated_records(emulated):  # noqa: F811
    """a correct launch (it passes) with one thing wrong"""
    dev = emulated
    for acc in (0, 1):
        case = S.make_case(4, 40, 300, 5, 7, 1, 5000, B=4, kind='asc', n_sets=2, blind=1, cluster=70, empty=None)
        rec, _ = T.fwd_case(dev, S.Stats('good'), case, 0)
        brec = T.bwd_case(dev, S.Stats('good'), rec, acc, 5100)
        V, HW = rec['V'], rec['Hf'] * rec['Wf']
        win = rec['win'].long()
        b = rec['coords'][:, 0].long()
        s, w = win[b, 0], win[b, 1]
        pix, cnt = rec['pix'], rec['cnt']
        live = cnt > 0
        # an in-window pix turned to -1 in the adjoint's input: the specification then misses a term the kernel added
        hit = torch.nonzero((pix >= 0) & live[:, None])[0]
        i, v = int(hit[0]), int(hit[1])
        assert v < int(w[i])
        bad = pix.clone()
        bad[i, v] = -1
        _rejected(lambda: S.check_win_bwd(dict(brec, pix=bad), dev, S.Stats('pix')), 'an adjoint that ignores an in-window hit')
        # one beyond-window term added to a pixel: row i of a sample with w < V, the pixel a view beyond the window would have hit
        i = int(torch.nonzero(live & (w < V))[0])
        v = int(w[i])
        term = brec['dout'][i] / float(cnt[i])
        df = brec['dfeats'].clone()
        df[(int(s[i]) * V + v) * HW + 3] += term
        _rejected(lambda: S.check_win_bwd(dict(brec, dfeats=df), dev, S.Stats('beyond')), 'a gradient with a beyond-window term')
        # one row's gradient landed in the other image set
        hit = torch.nonzero((pix >= 0) & live[:, None])[-1]
        i, v = int(hit[0]), int(hit[1])
        term = brec['dout'][i] / float(cnt[i])
        df = brec['dfeats'].clone()
        df[(int(s[i]) * V + v) * HW + int(pix[i, v])] -= term
        df[((1 - int(s[i])) * V + v) * HW + int(pix[i, v])] += term
        _rejected(lambda: S.check_win_bwd(dict(brec, dfeats=df), dev, S.Stats('set')), 'a gradient row in the other image set')
        # one cnt off by one: the forward quotient and the adjoint's weight are both wrong
        i = int(torch.nonzero(cnt >= 2)[0])
        for d in (1, -1):
            c2 = cnt.clone()
            c2[i] += d
            if d == -1 or int(c2[i]) <= int(((pix[i] >= 0)).sum()):
                _rejected(lambda: S.check_win_fwd(dict(rec, cnt=c2), dev, S.Stats('cnt')), 'a cnt off by one (forward)')
            _rejected(lambda: S.check_win_bwd(dict(brec, cnt=c2), dev, S.Stats('cnt')), 'a cnt off by one (backward)')
