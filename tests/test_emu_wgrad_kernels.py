"""tests/test_gpu_wgrad_kernels.py on the CPU emulator (tests/emu): the same bodies on the same shapes under the `emulated` fixture of
tests/test_emu_product.py (random thread schedule), with the launch log compared against the restated plan's kernel and reducer names;
one case per tile kernel again under the ascending, the descending and another random schedule; the transposed-read tile in both
LDS-DMA delivery modes.  The three 35 k-row cases of the 256 x 256 tile run with two pairs per slice (its first and last row) here.
Then the specification alone: it rejects a correct weight gradient with ONE thing wrong (the first mutation passes the relative-L2
gate of tests/test_gpu_ops.py), and the restated plan sends every case of the grid to the kernel its name promises.
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_wgrad_kernels as T
import wgrad_spec as S
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)


def _lib():
    import build as emu_build
    lib = ctypes.CDLL(emu_build.build())
    lib.es_emu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    return lib


def _launches():
    """kernel expressions launched since the last call"""
    buf = ctypes.create_string_buffer(1 << 16)
    _lib().es_emu_take_launch_log(buf, len(buf))
    return [ln.split(' grid=')[0] for ln in buf.value.decode().splitlines()]


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\n' + T.STATS.report())


def _case(name):
    return next(c for c in T.CASES if c['name'] == name)


# ------------------------------------------------------------------------------------------------------------ the GPU bodies
@pytest.mark.parametrize('name', [c['name'] for c in T.CASES])
def test_weight_gradient_per_element(emulated, name):  # noqa: F811
    T.wgrad_case(emulated, _case(name), _launches)


@pytest.mark.parametrize('name', T.CONTRACT_CASES)
def test_weight_gradient_contracts(emulated, name):  # noqa: F811
    T.contracts_case(emulated, _case(name))


@pytest.mark.parametrize('n,C,ld,x_off', T.CAST_CASES)
def test_cast_rows_bf16_bit_exact(emulated, n, C, ld, x_off):  # noqa: F811
    T.cast_rows_case(emulated, n, C, ld, x_off, n + C)


# ------------------------------------------------------------------------------------------------------------ other schedules, DMA modes
SCHEDULE_CASES = ['f32-130to67-K27-n129-acc', 'narrow-n65', 'lin-64to64-n257', 'bf16-96to192-K3-x1y0', 'big-128to256-K8-6slices-x0y1',
                  'tr32-128to128-K8-n512', 'tr64-128to256-K8-6slices', 'reduce-65slices', 'reduce-513slices', 'reduce-11slices-dW-4bytes-off']


@pytest.mark.parametrize('order,seed', [(0, 1), (1, 1), (2, 99)])
def test_one_case_per_kernel_under_other_schedules(emulated, order, seed):  # noqa: F811
    """schedule 0 / 1: ascending / descending thread order between synchronisation points; 2: random with another seed"""
    _lib().es_emu_set_schedule(order, seed)
    for name in SCHEDULE_CASES:
        T.wgrad_case(emulated, _case(name), _launches)


@pytest.mark.parametrize('lazy', [0, 1])
def test_transposed_read_tile_in_both_dma_delivery_modes(emulated, lazy):  # noqa: F811
    _lib().es_emu_set_dma_mode(lazy)
    try:
        for name in ('tr32-128to256-K8-6slices', 'tr64-128to256-K8-6slices', 'tr32-128to128-K8-n512', 'tr64-128to128-K8-n512'):
            T.wgrad_case(emulated, _case(name), _launches)
    finally:
        _lib().es_emu_set_dma_mode(1)


# ------------------------------------------------------------------------------------------------------------ the specification alone
def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the specification accepted {what}')


def _problem(n_out, n_in, K, cin, cout, rps, splits, seed):
    rng = np.random.default_rng(seed)
    nbr = T.place_pairs(rng, n_out, n_in, K, rps, splits)
    x = torch.from_numpy(rng.standard_normal((n_in, cin)).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((n_out, cout)).astype(np.float32))
    return torch.from_numpy(nbr), x, dy


def test_specification_rejects_one_thing_wrong():
    """each mutation is a weight gradient a plausible kernel defect would produce; every one fails the per-element check"""
    # 1. one pair dropped at a slice edge of a tap with about 3 000 pairs: the relative L2 of tests/test_gpu_ops.py (< 5e-3) passes it
    n_out, n_in, K, cin, cout = 4096, 4096, 27, 32, 24
    rng = np.random.default_rng(3)
    nbr = torch.full((n_out, K), -1, dtype=torch.int32)
    for k in range(K):                                                                  # the shape of tests/test_gpu_ops.py: 27 taps of ~ 3 000 pairs
        rows = torch.from_numpy(np.union1d(rng.choice(n_out, size=2999, replace=False), [2048]))   # 2048: the first row of the second slice
        nbr[rows, k] = torch.from_numpy(rng.integers(0, n_in, size=len(rows)).astype(np.int32))
    x = torch.from_numpy(rng.standard_normal((n_in, cin)).astype(np.float32))
    dy = torch.from_numpy(rng.standard_normal((n_out, cout)).astype(np.float32))
    xr, yr = S.operand(x, True), S.operand(dy, True)
    want, A, nk = S.reference(xr, yr, nbr, n_out, n_in, K)
    assert 2900 <= int(nk[0]) <= 3000
    good = want.float()
    S.check('good', good, want, A, nk)
    dropped = nbr.clone()
    dropped[2048, 0] = -1
    one_short = S.reference(xr, yr, dropped, n_out, n_in, K)[0].float()
    rel = S.rel_l2(one_short, want)
    assert rel < 5e-3, rel                                                              # the old gate lets it through ...
    _rejected(lambda: S.check('pair', one_short, want, A, nk), 'one pair dropped at a slice edge')   # ... the per-element bound does not
    print(f'one of {int(nk[0])} pairs dropped: relative L2 {rel:.2e} (the old gate: < 5e-3)')
    # 2. one slice's partial tile missing
    half = nbr.clone()
    half[2048:, 0] = -1
    _rejected(lambda: S.check('slice', S.reference(xr, yr, half, n_out, n_in, K)[0].float(), want, A, nk), "one slice's partial tile missing")
    # 3. / 4. operands not rounded; dY rounded but X not
    exact = S.reference(S.operand(x, False), S.operand(dy, False), nbr, n_out, n_in, K)[0].float()
    _rejected(lambda: S.check('unrounded', exact, want, A, nk), 'operands not rounded')
    mixed = S.reference(S.operand(x, False), yr, nbr, n_out, n_in, K)[0].float()
    _rejected(lambda: S.check('mixed', mixed, want, A, nk), 'dY rounded but X not')
    # 5. a NaN (or anything but 0.0) left in a pair-less tap under accumulate = 0
    nbr3, x3, dy3 = _problem(600, 300, 4, 24, 40, 256, 3, 5)
    w3, A3, nk3 = S.reference(S.operand(x3, True), S.operand(dy3, True), nbr3, 600, 300, 4)
    assert int(nk3[2]) == 0 and bool((nk3[[0, 1, 3]] > 0).all())
    g3 = w3.float()
    S.check('good', g3, w3, A3, nk3)
    left = g3.clone()
    left[2, 3, 4] = float('nan')
    _rejected(lambda: S.check('nan', left, w3, A3, nk3), 'a NaN left in a pair-less tap')
    left[2, 3, 4] = 1e-30
    _rejected(lambda: S.check('tiny', left, w3, A3, nk3), 'a value other than 0.0 in a pair-less tap')
    # 6. the prior added twice (and: a pair-less tap must keep the prior bit for bit)
    prior = torch.from_numpy(np.random.default_rng(6).standard_normal(tuple(w3.shape)).astype(np.float32))
    acc = (w3 + prior.double()).float()
    S.check('good', acc, w3, A3, nk3, prior)
    _rejected(lambda: S.check('twice', (w3 + 2 * prior.double()).float(), w3, A3, nk3, prior), 'the prior added twice')
    nudged = acc.clone()
    nudged[2, 0, 0] = float(np.nextafter(np.float32(nudged[2, 0, 0]), np.float32(9)))
    _rejected(lambda: S.check('prior', nudged, w3, A3, nk3, prior), 'a prior one ulp off in a pair-less tap')
    # 7. a tap's tile written to the neighbouring tap
    moved = g3.clone()
    moved[[0, 1]] = moved[[1, 0]]
    _rejected(lambda: S.check('tap', moved, w3, A3, nk3), "a tap's tile written to the neighbouring tap")
    # 8. Cin / Cout transposed on a square layer
    nbr8, x8, dy8 = _problem(300, 300, 2, 32, 32, 300, 1, 8)
    w8, A8, nk8 = S.reference(S.operand(x8, True), S.operand(dy8, True), nbr8, 300, 300, 2)
    S.check('good', w8.float(), w8, A8, nk8)
    _rejected(lambda: S.check('transposed', w8.transpose(1, 2).contiguous().float(), w8, A8, nk8), 'Cin / Cout transposed')
    # 9. n_in ignored on the identity map (n_out > n_in: rows past n_in have no input row)
    x9, dy9 = torch.cat([x8[:200], torch.ones(100, 32)]), dy8
    w9, A9, nk9 = S.reference(S.operand(x9[:200], True), S.operand(dy9, True), None, 300, 200, 1)
    assert int(nk9[0]) == 200
    S.check('good', w9.float(), w9, A9, nk9)
    ignored = S.reference(S.operand(x9, True), S.operand(dy9, True), None, 300, 300, 1)[0].float()
    _rejected(lambda: S.check('n_in', ignored, w9, A9, nk9), 'n_in ignored on the identity map')


def test_restated_plan_sends_every_case_to_the_kernel_it_names():
    """no device, no emulator: every kind 0 .. 5, both transposed-read widths, the 256 x 256 tile and all four reducers are reached"""
    kernels, reducers, kinds = set(), set(), set()
    for c in T.CASES:
        p, kernel = T.restated_plan(c)
        T.promised(c, p, kernel)
        kinds.add(p.kind), kernels.add(kernel), reducers.add(p.reducer)
        if c['map'] == 'placed':
            assert p.rows_per_split * (p.splits - 1) < c['n_out'] <= p.rows_per_split * p.splits
    assert kinds == {0, 1, 2, 3, 4, 5}
    assert kernels == {'k_spconv_wgrad', 'k_spconv_narrow_wgrad<3>', 'k_lin_wgrad_small', 'k_spconv_wgrad_bf16', 'k_spconv_wgrad_bf16_big',
                       'k_spconv_wgrad_bf16_tr<32>', 'k_spconv_wgrad_bf16_tr<64>', 'k_spconv_wgrad_bf16_huge'}
    assert reducers == {None, 'k_wgrad_reduce', 'k_wgrad_reduce4', 'k_wgrad_reduce_ranges<16>', 'k_wgrad_reduce_ranges<64>'}
    by = {c['name']: T.restated_plan(c)[0] for c in T.CASES}
    assert by['huge-256to256-K27-36slices'].splits == 36 and by['huge-one-row-fewer'].kind == 2
    assert [by[f'reduce-{s}slices'].splits for s in (11, 64, 65, 511, 512, 513)] == [11, 64, 65, 511, 512, 513]
    assert by['narrow-385slices-acc'].splits == 385 and by['big-128to256-K8-6slices-x1y1'].splits == 6 and by['f32-24to72-K8-22slices-acc'].splits == 22
    # slice counts that are no multiple of 8 (the XCD remap pads gridDim.z) and a short last slice are both in the grid
    assert any(p.splits % 8 and p.splits > 8 for p in by.values())
    # the pair placement puts every count of COUNTS into some (tap, slice), pairs on both edges of a slice, an empty slice, an empty tap
    nbr = T.place_pairs(np.random.default_rng(1), 6 * 448 - 111, 900, 27, 448, 6)
    cnt = np.stack([(nbr[s * 448:(s + 1) * 448] >= 0).sum(0) for s in range(6)])
    assert set(cnt.reshape(-1).tolist()) >= {0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 448}
    assert not cnt[1].any() and not cnt[:, 13].any() and cnt[[0, 2, 3, 4, 5]][:, [k for k in range(27) if k != 13]].sum(1).all()
    assert nbr[-1, 0] >= 0 and nbr[0, 0] >= 0 and all((nbr[min((s + 1) * 448, len(nbr)) - 1] >= 0).any() for s in (0, 2, 3, 4, 5))
    # the even slices have a pair on their first row; the odd ones leave it without one in any tap and start on the second; X row 0 is unnamed
    assert all((nbr[s * 448] >= 0).any() for s in (0, 2, 4)) and all((nbr[s * 448] < 0).all() and (nbr[s * 448 + 1] >= 0).any() for s in (3, 5))
    assert (nbr != 0).all()
