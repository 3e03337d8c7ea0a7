"""The kernel-level cases of the FCAF3D head's backward entry points (es_gen_transpose_wgrad_bf16, es_focal_loss_clear), written once
against a small backend -- tests/test_emu_head_backward.py runs them on the CDNA emulator,
tests/test_gpu_head_backward.py on the device.  A backend has fn(name) -> the C entry point (returns its status) and put(array) -> a
buffer with .ptr (address) and .get() (its present content as a numpy array of the same shape and dtype).  Not a test module."""
import numpy as np


def bf16_round(x):
    """f32 -> nearest-even bf16, returned as f32 (v_cvt_pk_bf16_f32)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def split_rows(be, cin=128, cout=128):
    """the smallest n for which ONE tap's weight-gradient launch (K = 1, cin -> cout, the (n, 8 cout) gradient rows) splits its rows"""
    probe = be.put(np.zeros(64, np.float32))
    wsf = be.fn('es_spconv_wgrad_workspace_floats')
    for n in range(1, 4097):
        if wsf(1, probe.ptr, 0, cin, probe.ptr, 0, 8 * cout, n, n, 1, cin, cout):
            return n
    raise AssertionError('no row split below 4097 rows')


def gen_wgrad_cases(be):
    return [(1, 128, 128, 0, 0), (300, 256, 128, 8, 0), (split_rows(be), 128, 128, 0, 1)]       # n, Cin, Cout, ldx - Cin, accumulate


def check_gen_wgrad(be, n, cin, cout, ext, acc, seed=0):
    """the fused launch against the eight per-tap es_spconv_wgrad_bf16 launches (bits) and against f64 on the bf16-rounded operands; -> the
    workspace floats it asked for"""
    rng = np.random.default_rng(100 + seed)
    x = rng.standard_normal((n, cin + ext)).astype(np.float32)
    dy = rng.standard_normal((n, 8 * cout)).astype(np.float32)
    dw0 = rng.standard_normal((8, cin, cout)).astype(np.float32)
    X, DY = be.put(x), be.put(dy)
    ldx, ldy = cin + ext, 8 * cout
    # the per-tap launches, each with the workspace its own query asks for
    ref = be.put(dw0)
    nf1 = int(be.fn('es_spconv_wgrad_workspace_floats')(1, X.ptr, 0, ldx, DY.ptr, 0, ldy, n, n, 1, cin, cout))
    ws1 = be.put(np.full(max(nf1, 1), np.nan, np.float32))
    for k in range(8):
        rc = be.fn('es_spconv_wgrad_bf16')(X.ptr, ldx, DY.ptr + 4 * k * cout, ldy, 0, n, n, 1, cin, cout, ref.ptr + 4 * k * cin * cout, acc,
                                           ws1.ptr if nf1 else 0, nf1, 0)
        assert rc == 0, (k, rc)
    ref = ref.get()
    nf = int(be.fn('es_gen_transpose_wgrad_workspace_floats')(X.ptr, ldx, DY.ptr, n, cin, cout))
    assert nf == 8 * nf1, (nf, nf1)
    ws = be.put(np.full(max(nf, 1), np.nan, np.float32))
    outs = []
    for _ in range(2):                                       # two calls on the same workspace
        got = be.put(dw0)
        be.launches()
        rc = be.fn('es_gen_transpose_wgrad_bf16')(X.ptr, ldx, DY.ptr, n, cin, cout, got.ptr, acc, ws.ptr if nf else 0, nf, 0)
        assert rc == 0, rc
        log = be.launches()
        if log is not None:                                  # one kernel launch and at most one reduction launch
            assert len(log) == (2 if nf else 1) and 'wgrad' in log[0] and (not nf or 'reduce' in log[1]), log
        outs.append(got.get())
    assert np.array_equal(outs[0], ref), (n, cin, cout, float(np.abs(outs[0] - ref).max()))
    assert np.array_equal(outs[0], outs[1])
    xb, yb = bf16_round(x)[:, :cin].astype(np.float64), bf16_round(dy).astype(np.float64)
    want = np.stack([xb.T @ yb[:, k * cout:(k + 1) * cout] for k in range(8)]) + (dw0 if acc else 0)
    err = np.abs(outs[0] - want).max() / np.abs(want).max()
    print(f'gen wgrad n={n} {cin}->{cout}: rel err {err:.3g}, workspace floats {nf}')
    assert err <= 2e-6, (n, cin, cout, err)
    if nf:                                                   # a workspace that is too small
        got = be.put(dw0)
        assert be.fn('es_gen_transpose_wgrad_bf16')(X.ptr, ldx, DY.ptr, n, cin, cout, got.ptr, acc, ws.ptr, nf - 1, 0) == -5
        assert np.array_equal(got.get(), dw0)
    return nf


def check_gen_wgrad_unserved(be):
    """a shape outside the gate: returns 1, dW untouched"""
    n, cin, cout = 333, 64, 96
    rng = np.random.default_rng(7)
    X, DY = be.put(rng.standard_normal((n, cin)).astype(np.float32)), be.put(rng.standard_normal((n, 8 * cout)).astype(np.float32))
    dw0 = rng.standard_normal((8, cin, cout)).astype(np.float32)
    got, ws = be.put(dw0), be.put(np.zeros(1 << 16, np.float32))
    assert be.fn('es_gen_transpose_wgrad_workspace_floats')(X.ptr, cin, DY.ptr, n, cin, cout) == 0
    assert be.fn('es_gen_transpose_wgrad_bf16')(X.ptr, cin, DY.ptr, n, cin, cout, got.ptr, 0, ws.ptr, 1 << 16, 0) == 1
    assert np.array_equal(got.get(), dw0)


def check_focal_clear(be, N):
    """es_focal_loss_clear against es_focal_loss on the head's layout: (N, 320) rows, 13 lead columns, 284 classes, 23 padding columns"""
    C, ld, lead, tail = 284, 320, 13, 23
    rng = np.random.default_rng(N)
    ho = (2 * rng.standard_normal((N, ld))).astype(np.float32)
    labels = rng.choice(np.array([-1, 0, 283], np.int32), N).astype(np.int32)
    avg = np.array([3.0], np.float32)
    HO, LAB, AVG = be.put(ho), be.put(labels), be.put(avg)
    res = []
    for clear in (0, 1):
        g = be.put(np.full((N + 1, ld), np.nan, np.float32))
        part, loss = be.put(np.zeros(2048, np.float64)), be.put(np.array([0.25], np.float32))
        args = (HO.ptr + 4 * lead, ld, LAB.ptr, N, C, 2.0, 0.25, AVG.ptr, 0.5, g.ptr + 4 * lead, ld, part.ptr, loss.ptr)
        rc = be.fn('es_focal_loss_clear')(*args, lead, tail, 0) if clear else be.fn('es_focal_loss')(*args, 0)
        assert rc == 0, rc
        res.append((g.get(), loss.get()))
    (g0, l0), (g1, l1) = res
    assert np.isfinite(g0[:N, lead:lead + C]).all() and np.isnan(g0[:N, :lead]).all() and np.isnan(g0[:N, lead + C:]).all()
    assert np.array_equal(g1[:N, lead:lead + C].view(np.uint32), g0[:N, lead:lead + C].view(np.uint32))     # class block: the same bits
    assert np.array_equal(l1.view(np.uint32), l0.view(np.uint32)) and l0[0] != 0.25
    rest = np.concatenate([g1[:N, :lead], g1[:N, lead + C:]], 1)
    assert not rest.view(np.uint32).any()                                                                   # exactly +0.0
    assert np.isnan(g1[N]).all()                                                                            # the row behind the last one
