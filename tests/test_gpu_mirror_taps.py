"""Mirrored tap walk of the gather kernels (bit 1 of `accumulate` of es_spconv_fwd / es_spconv_fwd_bf16 / es_spconv_fwd_bf16_ws): a
coordinate set's own 3x3x3 map read with mirrored taps IS its inverse map (inv[i][k] == nbr[i][26 - k]), so a launch on the forward map
with the mirror bit must give the bits of the launch on the real inverse map -- on every kernel family the dispatch can take
(k_spconv_bf16_fast incl. the tap split and its k_sum_splits4 tail, k_spconv_bf16, k_spconv_bf16_dma, the f32 k_spconv and the
3-channel lane-per-output kernel), with and without accumulation, on ragged row counts.  Then the engine: engine.conv with the
sparse.MirrorInv handle in place of the inverse map gives the same data gradient and never launches es_inverse_map.

The set: a cluster of random voxels at ~30 % occupancy (most of the 26 neighbours of a row absent, a few present) plus scattered
isolated voxels, whose only present tap is the centre (the row itself: a set's own map always holds that one)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
K = 27


def _points(seed):
    g = torch.Generator().manual_seed(seed)
    dense = torch.rand(2600, 3, generator=g) * 0.8                      # 20^3 cells of 0.04: ~ 28 % occupied
    lone = torch.rand(400, 3, generator=g) * 40 + 5                      # isolated voxels
    return torch.cat([dense, lone])


def _set(dev, seed=0):
    from embodiedscan_amd import sparse
    cs, _ = sparse.voxelize([_points(seed).to(dev), _points(seed + 1)[:1700].to(dev)], 0.04)
    return cs


@pytest.fixture(scope='module')
def maps():
    dev = torch.device('cuda:0')
    cs = _set(dev)
    nbr, inv = cs.kernel_map(cs, 3), cs.inverse_map(cs, 3)
    torch.cuda.synchronize()
    present = (nbr >= 0).sum(1)
    assert 2000 <= cs.n <= 6000 and cs.n_batch == 2
    assert int(present.min()) == 1 and int((present == 1).sum()) >= 100, 'rows with no neighbour but themselves'
    assert 0.05 < float((nbr >= 0).float().mean()) < 0.6, 'many neighbours absent'
    assert torch.equal(inv, nbr.flip(1))
    return cs, nbr, inv


def _weights(g, cin, cout, dev, st):
    from embodiedscan_amd.hip import P, call
    w = (torch.randn(K, cin, cout, generator=g) / (K * cin) ** 0.5).to(dev)
    wn = torch.empty((K, cin, cout), dtype=torch.bfloat16, device=dev)
    wt = torch.empty((K, cout, cin), dtype=torch.bfloat16, device=dev)
    call('es_cast_weight_bf16', P(w), K, cin, cout, P(wn), P(wt), st)
    return w, wt


def _pair(launch, nbr, inv, rows, cout, y0):
    """the launch on the first `rows` rows of the real inverse map and of the forward map with the mirror bit, accumulate 0 and 1"""
    a, b = inv[:rows].contiguous(), nbr[:rows].contiguous()
    for acc in (0, 1):
        ya, yb = y0[:rows].clone(), y0[:rows].clone()
        launch(a, rows, ya, acc)
        launch(b, rows, yb, acc | 2)
        torch.cuda.synchronize()
        assert torch.equal(ya, yb), (rows, acc, float((ya - yb).abs().max()))
        assert not torch.equal(ya, y0[:rows]), 'the launch wrote nothing'


@pytest.mark.parametrize('shape', [(128, 128, 1), (64, 64, 1), (16, 64, 0)])
def test_bf16_entry_point_mirrored_equals_the_inverse_map(maps, shape):
    """es_spconv_fwd_bf16: 128 -> 128 and 64 -> 64 on bf16 shadow rows (k_spconv_bf16_fast), 16 -> 64 on f32 rows (below the 32-channel
    chunk of the fast kernels: k_spconv_bf16)"""
    from embodiedscan_amd import hip
    from embodiedscan_amd.hip import P, call
    cs, nbr, inv = maps
    cin, cout, shadow = shape
    dev, n = nbr.device, cs.n
    st = torch.cuda.current_stream().cuda_stream
    assert hip.raw('es_spconv_bf16_is_fast')(n, cin, K, cin, cout) == (1 if cin >= 32 else 0)
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(n, cin, generator=g).to(dev)
    X = x.bfloat16().contiguous() if shadow else x
    _, wt = _weights(g, cin, cout, dev, st)
    y0 = torch.randn(n, cout, generator=g).to(dev)

    def launch(mp, rows, y, acc):
        call('es_spconv_fwd_bf16', P(X), shadow, cin, P(wt), P(mp), rows, n, K, cin, cout, 0, P(y), cout, acc, st)
    for rows in (1, 127, 129, n):
        _pair(launch, nbr, inv, rows, cout, y0)


def test_tap_split_launch_mirrored_equals_the_inverse_map(maps):
    """es_spconv_fwd_bf16_ws on 300 rows, 512 -> 512: twelve workgroups, so the tap list is split over gridDim.z and the partial tiles
    are added by the second launch"""
    from embodiedscan_amd import hip
    from embodiedscan_amd.hip import P, call
    cs, nbr, inv = maps
    dev, n, rows, cin, cout = nbr.device, cs.n, 300, 512, 512
    st = torch.cuda.current_stream().cuda_stream
    nf = int(hip.raw('es_spconv_split_workspace_floats')(rows, K, cin, cout))
    assert nf > 0, 'the launch must split its taps'
    g = torch.Generator().manual_seed(7)
    xh = torch.randn(n, cin, generator=g).to(dev).bfloat16().contiguous()
    _, wt = _weights(g, cin, cout, dev, st)
    y0 = torch.randn(n, cout, generator=g).to(dev)
    ws = torch.zeros(nf, device=dev)

    def launch(mp, r, y, acc):
        call('es_spconv_fwd_bf16_ws', P(xh), 1, cin, P(wt), P(mp), r, n, K, cin, cout, 0, P(y), cout, acc, P(ws), nf, st)
    _pair(launch, nbr, inv, rows, cout, y0)


def test_dma_kernel_mirrored_equals_the_inverse_map(maps):
    """k_spconv_bf16_dma: the dispatch takes it for bf16 rows of a fast shape with option 10 != 0 and C_in >= option 11 (768 as shipped:
    both are set here to their shipped values, the shape is 768 -> 64)"""
    from embodiedscan_amd import hip
    from embodiedscan_amd.hip import P, call
    cs, nbr, inv = maps
    dev, n, cin, cout = nbr.device, cs.n, 768, 64
    st = torch.cuda.current_stream().cuda_stream
    opt = hip.raw('es_set_option')
    g = torch.Generator().manual_seed(9)
    xh = torch.randn(n, cin, generator=g).to(dev).bfloat16().contiguous()
    _, wt = _weights(g, cin, cout, dev, st)
    y0 = torch.randn(n, cout, generator=g).to(dev)
    assert opt(10, 2) == 0 and opt(11, 768) == 0 and cin >= 768                 # the gate of the DMA family ...
    assert hip.raw('es_spconv_bf16_is_fast')(n, cin, K, cin, cout) == 1         # ... and of the fast kernels it belongs to

    def launch(mp, rows, y, acc):
        call('es_spconv_fwd_bf16', P(xh), 1, cin, P(wt), P(mp), rows, n, K, cin, cout, 0, P(y), cout, acc, st)
    for rows in (1, 127, 129, n):
        _pair(launch, nbr, inv, rows, cout, y0)
    # the register-staged kernel on the same operands gives the DMA kernel's bits (tests/test_gpu_dma.py): mirrored too
    ya, yb = torch.empty(n, cout, device=dev), torch.empty(n, cout, device=dev)
    try:
        launch(nbr, n, ya, 2)
        opt(10, 0)
        launch(nbr, n, yb, 2)
        torch.cuda.synchronize()
    finally:
        opt(10, 2)
    assert torch.equal(ya, yb)


@pytest.mark.parametrize('shape', [(20, 40, 1), (20, 40, 0), (3, 64, 0)])
def test_f32_entry_point_mirrored_equals_the_inverse_map(maps, shape):
    """es_spconv_fwd: the tiled f32 kernel with transposed (data-gradient) and natural weights, and the 3 -> 64 lane-per-output kernel"""
    from embodiedscan_amd.hip import P, call
    cs, nbr, inv = maps
    cin, cout, trans_w = shape
    dev, n = nbr.device, cs.n
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(11 + cin)
    x = torch.randn(n, cin, generator=g).to(dev)
    w = torch.randn((K, cout, cin) if trans_w else (K, cin, cout), generator=g).to(dev)
    y0 = torch.randn(n, cout, generator=g).to(dev)

    def launch(mp, rows, y, acc):
        call('es_spconv_fwd', P(x), cin, P(w), P(mp), rows, n, K, cin, cout, 0, P(y), cout, trans_w, acc, st)
    for rows in (1, 127, 129, n):
        _pair(launch, nbr, inv, rows, cout, y0)


def test_mirror_bit_needs_an_odd_kernel_on_a_real_map(maps):
    from embodiedscan_amd import hip
    from embodiedscan_amd.hip import P
    cs, nbr, inv = maps
    dev = nbr.device
    st = torch.cuda.current_stream().cuda_stream
    x, y = torch.zeros(64, 64, device=dev), torch.zeros(64, 64, device=dev)
    w16 = torch.zeros(8, 64, 64, dtype=torch.bfloat16, device=dev)
    m8 = torch.zeros(64, 8, dtype=torch.int32, device=dev)
    ws = torch.zeros(4096, device=dev)
    assert hip.raw('es_spconv_fwd_bf16')(P(x), 0, 64, P(w16), P(m8), 64, 64, 8, 64, 64, 0, P(y), 64, 2, st) == -3
    assert hip.raw('es_spconv_fwd_bf16')(P(x), 0, 64, P(w16), 0, 64, 64, 1, 64, 64, 0, P(y), 64, 3, st) == -3
    assert hip.raw('es_spconv_fwd_bf16_ws')(P(x), 0, 64, P(w16), P(m8), 64, 64, 8, 64, 64, 0, P(y), 64, 2, P(ws), 4096, st) == -3
    assert hip.raw('es_spconv_fwd')(P(x), 64, P(x), P(m8), 64, 64, 8, 64, 8, 0, P(y), 64, 1, 2, st) == -3
    assert hip.raw('es_spconv_fwd')(P(x), 64, P(x), 0, 64, 64, 1, 64, 64, 0, P(y), 64, 1, 2, st) == -3
    torch.cuda.synchronize()
    assert not y.any()


@pytest.mark.parametrize('case', [('bf16', 64, 64), ('bf16', 64, 24), ('f32', 20, 40)])
def test_engine_conv_with_the_mirror_handle(case):
    """engine.conv + backward on a fresh set: the data gradient with sparse.MirrorInv equals the one with the real inverse map bit for
    bit (bf16 shadow rows, bf16 kernels on f32 gradient rows, f32), es_inverse_map is never launched on the way, and the set's strided
    map still gets its inverse map"""
    from embodiedscan_amd import engine as E, hip, sparse
    precision, cin, cout = case
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(13)
    calls = []
    orig = hip._fn['es_inverse_map']

    def spy(*a):
        calls.append(a[1:4])
        return orig(*a)
    saved = (E.PRECISION[0], sparse.MIRROR_TAPS[0])
    res = {}
    try:
        hip._fn['es_inverse_map'] = spy
        E.PRECISION[0] = precision
        for mirror in (True, False):
            sparse.MIRROR_TAPS[0] = mirror
            cs = _set(dev, seed=3)                               # (fresh: nothing cached)
            n = cs.n
            if mirror:
                xd = torch.randn(n, cin, generator=g).to(dev)
                wd = (torch.randn(K, cin, cout, generator=g) / (K * cin) ** 0.5).to(dev)
                gy = torch.randn(n, cout, generator=g).to(dev)
                g0 = torch.randn(n, cin, generator=g).to(dev)
            E.TAPE.clear()
            nbr, inv = cs.kernel_map(cs, 3), cs.self_inverse(3)
            assert isinstance(inv, sparse.MirrorInv) == mirror and (not mirror or inv.nbr is nbr)
            outs = []
            for first in (True, False):                          # the gradient's first write, then an accumulating one
                x = E.Var(xd.clone())
                if not first:
                    x.g = g0.clone()
                w = E.Param(wd.clone(), torch.zeros_like(wd))
                y = E.conv(x, w, nbr, inv, n)
                y.g = gy.clone()
                E.TAPE.backward()
                E.join_wgrad_streams()
                torch.cuda.synchronize()
                outs += [y.d.clone(), x.g.clone(), w.g.clone()]
                E.TAPE.clear()
            res[mirror] = (outs, list(calls))
            calls.clear()
            if mirror:
                down = cs.strided(2)
                cs.inverse_map(down, 3)
                assert len(calls) == 1 and calls[0][0] == down.n, 'the strided map keeps its inverse map'
                real = inv.real()                                # a launch that cannot mirror still gets the real thing
                assert len(calls) == 2 and torch.equal(real, nbr.flip(1)) and real._mirror_of is nbr
                calls.clear()
    finally:
        hip._fn['es_inverse_map'] = orig
        E.PRECISION[0], sparse.MIRROR_TAPS[0] = saved
        E.TAPE.clear()
    assert res[True][1] == [], res[True][1]
    assert len(res[False][1]) == 1
    for a, b in zip(res[True][0], res[False][0]):
        assert torch.equal(a, b), float((a - b).abs().max())
    assert float(res[True][0][1].abs().max()) > 0
