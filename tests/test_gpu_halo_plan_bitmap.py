"""es_halo_plan by bitmap (k_halo_plan_bitmap, es_halo_set_option 32 = 1, the default) against the hash-and-rank plan (32 = 0): `loc`,
`hcnt` and `hrows[:, :hcnt]` must be equal (entries of hrows past hcnt are unspecified) -- on a real Z-ordered set, on ragged row
counts, on tiles with no entry and with one distinct row, on a scattered map whose tiles span more than 2^19 source rows (they take the
hash-and-rank code inside the new kernel) and on two hand-built tiles at the span limit and one past it.  Both are also held to numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
K = 27


def _plan(nbr, on):
    from embodiedscan_amd import hip
    from embodiedscan_amd.hip import P, call
    n_out = nbr.shape[0]
    rows = int(hip.raw('es_halo_plan_rows')(n_out))
    loc = torch.full((rows, K), 0x1234, dtype=torch.int16, device=nbr.device)
    hrows = torch.full((rows // 256, 256 * K), -7, dtype=torch.int32, device=nbr.device)
    hcnt = torch.full((rows // 256,), -7, dtype=torch.int32, device=nbr.device)
    assert hip.raw('es_halo_set_option')(32, on) == 0
    try:
        call('es_halo_plan', P(nbr), n_out, K, P(loc), P(hrows), P(hcnt), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        hip.raw('es_halo_set_option')(32, 1)
    return loc.cpu().numpy().view(np.uint16), hrows.cpu().numpy(), hcnt.cpu().numpy()


def _check(nbr, tag):
    """-> hcnt; bitmap against hash-and-rank, and against numpy (sorted distinct rows per 256-row tile, positions in that list)"""
    (l0, h0, c0), (l1, h1, c1) = _plan(nbr, 0), _plan(nbr, 1)
    assert np.array_equal(c0, c1), tag
    assert np.array_equal(l0, l1), tag
    nb = nbr.cpu().numpy()
    for t in range(len(c0)):
        assert np.array_equal(h0[t, :c0[t]], h1[t, :c0[t]]), (tag, t)
        blk = nb[t * 256:(t + 1) * 256]
        u = np.unique(blk[blk >= 0])
        assert c1[t] == len(u) and np.array_equal(h1[t, :len(u)], u), (tag, t)
        want = np.where(blk >= 0, np.searchsorted(u, np.maximum(blk, 0)), 0xFFFF).astype(np.uint16)
        assert np.array_equal(l1[t * 256:t * 256 + len(blk)], want), (tag, t)
    assert (l1[nb.shape[0]:] == 0xFFFF).all(), tag
    return c1


@pytest.fixture(scope='module')
def zset():
    from embodiedscan_amd import sparse
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(21)
    pts = [(torch.rand(n, 3, generator=g) * torch.tensor([1.2, 1.0, 0.5])).to(dev) for n in (9000, 5000)]
    cs, _ = sparse.voxelize(pts, 0.04)
    nbr = cs.kernel_map(cs, 3)
    torch.cuda.synchronize()
    return nbr


def test_real_z_ordered_set(zset):
    hc = _check(zset, 'z-ordered')
    print(f'{zset.shape[0]} rows: halo per tile mean {hc.mean():.0f} max {hc.max()}')
    assert hc.max() > 256


@pytest.mark.parametrize('n_out', [1, 255, 256, 257, 1000])
def test_ragged_row_counts(zset, n_out):
    _check(zset[:n_out].contiguous(), n_out)


def test_empty_tile_one_row_tile_and_scattered_fallback():
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(22)
    n_in = (1 << 20) + 5
    nbr = torch.full((256 * 2 + 700, K), -1, dtype=torch.int32)
    nbr[256:512] = 41                                         # every entry of the tile names one row
    nbr[300:400, ::2] = -1
    nbr[512:] = torch.randint(0, n_in, (700, K), generator=g, dtype=torch.int32)
    nbr[512:][torch.rand(700, K, generator=g) < 0.3] = -1
    for t in range(2, 5):                                     # (the scattered tiles must take the fallback: span > 2^19)
        blk = nbr[t * 256:(t + 1) * 256]
        assert int(blk.max()) - int(blk[blk >= 0].min()) + 1 > (1 << 19)
    hc = _check(nbr.to(dev), 'empty / one row / scattered')
    assert hc[0] == 0 and hc[1] == 1 and hc[2] > 4000


@pytest.mark.parametrize('span', [1 << 19, (1 << 19) + 1])
def test_tiles_at_the_span_limit(span):
    """span exactly 2^19: the widest bitmap (all 16 384 words); 2^19 + 1: the first tile of the fallback"""
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(span % 1000)
    base = 777
    nbr = (torch.randint(0, span, (256, K), generator=g, dtype=torch.int32) + base)
    nbr[torch.rand(256, K, generator=g) < 0.2] = -1
    nbr[0, 0], nbr[255, 26] = base, base + span - 1          # the span's two ends are present
    nbr[17, 3], nbr[200, 9] = base + span - 1, base + 31     # (a duplicate of the last row; a row in the first word's top bit)
    hc = _check(nbr.to(dev), f'span {span}')
    assert hc[0] > 4000
