"""The three bit-identity claims of the mirrored tap walk, k_focal_inflight and k_halo_plan_bitmap on the CPU emulation of the kernels
(tests/emu, see tests/test_emu_kernels.py for what the emulator does and does not pin): same entry points, host pointers, two thread
schedules.  The GPU versions with the full case tables are tests/test_gpu_mirror_taps.py, test_gpu_focal_inflight.py and
test_gpu_halo_plan_bitmap.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'emu'))
K = 27


@pytest.fixture(scope='module', params=['descending', 'random'])
def emu(request):
    import build as emu_build
    from embodiedscan_amd import hip
    lib = ctypes.CDLL(emu_build.build())
    lib.es_emu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    lib.es_emu_set_schedule(['ascending', 'descending', 'random'].index(request.param), 4321)
    fns = {}
    for name, (ret, at, _) in hip.PROTOS.items():
        f = getattr(lib, name, None)
        if f is not None:
            f.restype, f.argtypes = ret, at
            fns[name] = f

    def call(name, *args):
        rc = fns[name](*args)
        assert rc == 0, (name, rc)

    def launches():
        buf = ctypes.create_string_buffer(1 << 16)
        lib.es_emu_take_launch_log(buf, len(buf))
        return [ln.split(' grid=')[0] for ln in buf.value.decode().splitlines()]
    call.fns, call.launches = fns, launches
    return call


def P(a):
    return a.ctypes.data if a is not None else 0


def bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def test_focal_inflight_is_bit_identical_to_the_loop_kernel(emu):
    rng = np.random.default_rng(3)
    ld = 400
    try:
        for N, C in ((1, 1), (4, 64), (5, 65), (9, 284), (131, 320), (6, 321)):
            for lead, tail in ((13, 23), (0, 0)):
                for gamma in (2.0, 1.5):
                    for with_grad in (1, 0):
                        logits = (rng.standard_normal((N, ld)) * 3).astype(np.float32)
                        labels = rng.integers(-1, C + 2, N).astype(np.int32)
                        labels[0] = C - 1
                        avg = np.array([3.5], np.float32)
                        outs = []
                        for on in (0, 1):
                            emu('es_losses_set_option', 40, on)
                            grad = np.full((N, ld), 7.25, np.float32)
                            partial = np.full(2048, -1.0, np.float64)
                            loss = np.array([0.5], np.float32)
                            emu.launches()
                            emu('es_focal_loss_clear', P(logits) + 4 * 13, ld, P(labels), N, C, gamma, 0.25, P(avg), 0.7,
                                (P(grad) + 4 * 13) if with_grad else 0, ld, P(partial), P(loss), lead if with_grad else 0,
                                tail if with_grad else 0, 0)
                            assert ('k_focal_inflight' in emu.launches()[0]) == bool(on and C <= 320)
                            outs.append((grad, partial, loss))
                        for a, b in zip(*outs):
                            assert a.tobytes() == b.tobytes(), (N, C, lead, gamma, with_grad)
    finally:
        emu('es_losses_set_option', 40, 1)


def _plan(emu, nbr, on):
    n_out = nbr.shape[0]
    rows = emu.fns['es_halo_plan_rows'](n_out)
    loc = np.full((rows, K), 0x1234, np.uint16)
    hrows = np.full((rows // 256, 256 * K), -7, np.int32)
    hcnt = np.full(rows // 256, -7, np.int32)
    emu('es_halo_set_option', 32, on)
    try:
        emu.launches()
        emu('es_halo_plan', P(nbr), n_out, K, P(loc), P(hrows), P(hcnt), 0)
        assert ('k_halo_plan_bitmap' in emu.launches()[0]) == bool(on)
    finally:
        emu('es_halo_set_option', 32, 1)
    return loc, hrows, hcnt


def test_bitmap_halo_plan_equals_hash_and_rank_and_numpy(emu):
    rng = np.random.default_rng(5)
    cases = []
    for n_out in (1, 255, 257, 1000):
        base = np.arange(n_out)[:, None] + rng.integers(-300, 300, (n_out, K))
        cases.append(np.where(rng.random((n_out, K)) < 0.7, np.clip(base, 0, n_out + 200), -1).astype(np.int32))
    nbr = np.full((600, K), -1, np.int32)                         # an empty tile, a one-row tile, a scattered one (fallback)
    nbr[256:512] = 41
    nbr[512:] = rng.integers(0, (1 << 20) + 5, (88, K))
    cases.append(nbr)
    for span in ((1 << 19), (1 << 19) + 1):
        nbr = rng.integers(1000, 1000 + span, (256, K)).astype(np.int32)
        nbr[rng.random((256, K)) < 0.2] = -1
        nbr[0, 0], nbr[255, 26] = 1000, 1000 + span - 1
        cases.append(nbr)
    for ci, nbr in enumerate(cases):
        (l0, h0, c0), (l1, h1, c1) = _plan(emu, nbr, 0), _plan(emu, nbr, 1)
        assert np.array_equal(c0, c1) and np.array_equal(l0, l1), ci
        for t in range(len(c1)):
            assert np.array_equal(h0[t, :c0[t]], h1[t, :c0[t]]), (ci, t)
            blk = nbr[t * 256:(t + 1) * 256]
            u = np.unique(blk[blk >= 0])
            assert c1[t] == len(u) and np.array_equal(h1[t, :len(u)], u), (ci, t)
            want = np.where(blk >= 0, np.searchsorted(u, np.maximum(blk, 0)), 0xFFFF).astype(np.uint16)
            assert np.array_equal(l1[t * 256:t * 256 + len(blk)], want), (ci, t)


def test_mirrored_tap_walk_equals_the_inverse_map(emu):
    """every kernel family of the gather dispatch, on a symmetric 27-tap map of random voxels: launch on inv == launch on nbr with bit 1"""
    rng = np.random.default_rng(7)
    vox = np.unique(rng.integers(0, 9, (420, 3)), axis=0)[:300]
    n = len(vox)
    lut = {tuple(v): i for i, v in enumerate(vox)}
    offs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]
    nbr = np.full((n, K), -1, np.int32)
    for i, v in enumerate(vox):
        for k, o in enumerate(offs):
            nbr[i, k] = lut.get((v[0] + o[0], v[1] + o[1], v[2] + o[2]), -1)
    inv = np.full((n, K), -1, np.int32)
    emu('es_inverse_map', P(nbr), n, K, n, P(inv), 0)
    assert np.array_equal(inv, nbr[:, ::-1])
    seen = set()

    def bf16_case(cin, cout, x_bf16, rows, acc, split):
        x = rng.standard_normal((n, cin)).astype(np.float32)
        X = bf16_bits(x) if x_bf16 else x
        w = (rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)
        wt, wn = np.zeros((K, cout, cin), np.uint16), np.zeros((K, cin, cout), np.uint16)
        emu('es_cast_weight_bf16', P(w), K, cin, cout, P(wn), P(wt), 0)
        y0 = rng.standard_normal((rows, cout)).astype(np.float32)
        outs, kern = [], []
        for m, mp in ((0, inv), (2, nbr)):
            mp = np.ascontiguousarray(mp[:rows])
            y = y0.copy()
            emu.launches()
            if split:
                nf = int(emu.fns['es_spconv_split_workspace_floats'](rows, K, cin, cout))
                assert nf > 0
                ws = np.zeros(nf, np.float32)
                emu('es_spconv_fwd_bf16_ws', P(X), x_bf16, cin, P(wt), P(mp), rows, n, K, cin, cout, 0, P(y), cout, acc | m, P(ws), nf, 0)
            else:
                emu('es_spconv_fwd_bf16', P(X), x_bf16, cin, P(wt), P(mp), rows, n, K, cin, cout, 0, P(y), cout, acc | m, 0)
            kern.append(emu.launches())
            outs.append(y)
        assert kern[0] == kern[1] and outs[0].tobytes() == outs[1].tobytes(), (cin, cout, x_bf16, rows, acc, split)
        seen.update(k.split('<')[0].strip('(') for k in kern[0])
    try:
        for rows, acc in ((1, 0), (129, 1), (n, 0)):
            bf16_case(64, 128, 1, rows, acc, 0)
            bf16_case(24, 64, 0, rows, acc, 0)
            bf16_case(64, 64, 1, rows, acc, 1)
            emu('es_set_option', 11, 0)                          # the LDS-DMA kernel for every width
            bf16_case(64, 64, 1, rows, acc, 0)
            emu('es_set_option', 11, 768)
            for cin, cout, tw in ((20, 40, 1), (3, 64, 0)):
                x = rng.standard_normal((n, cin)).astype(np.float32)
                w = rng.standard_normal((K, cin, cout)).astype(np.float32)
                y0 = rng.standard_normal((rows, cout)).astype(np.float32)
                outs = []
                for m, mp in ((0, inv), (2, nbr)):
                    mp = np.ascontiguousarray(mp[:rows])
                    y = y0.copy()
                    emu.launches()
                    emu('es_spconv_fwd', P(x), cin, P(w), P(mp), rows, n, K, cin, cout, 0, P(y), cout, tw, acc | m, 0)
                    seen.update(k.split('<')[0].strip('(') for k in emu.launches())
                    outs.append(y)
                assert outs[0].tobytes() == outs[1].tobytes(), ('f32', cin, cout, rows, acc)
    finally:
        emu('es_set_option', 11, 768)
    assert {'k_spconv_bf16_fast', 'k_spconv_bf16_dma', 'k_spconv_bf16', 'k_spconv', 'k_spconv_narrow_fwd', 'k_sum_splits4'} <= seen, seen
    y = np.zeros((4, 64), np.float32)
    w8, m8 = np.zeros((8, 64, 64), np.uint16), np.zeros((4, 8), np.int32)
    assert emu.fns['es_spconv_fwd_bf16'](P(y), 0, 64, P(w8), P(m8), 4, 4, 8, 64, 64, 0, P(y), 64, 2, 0) == -3      # even K
    assert emu.fns['es_spconv_fwd_bf16'](P(y), 0, 64, P(w8), 0, 4, 4, 1, 64, 64, 0, P(y), 64, 2, 0) == -3          # no map
    assert emu.fns['es_spconv_fwd'](P(y), 64, P(y), 0, 4, 4, 1, 64, 64, 0, P(y), 64, 0, 3, 0) == -3
