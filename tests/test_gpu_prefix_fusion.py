"""The prefix-fusion kernels (csrc/fusion.hip) held to tests/prefix_spec.py on the shape grid: V in {1, 2, 3, 10, 20}, C in {32, 40,
256, 512}, n with and without a multiple of 16, meta blocks with and without reverse-augmentation ops, leading views that see nothing
(cnt = 0 .. 0, 1, ..), voxels that are never valid, views without a pixel, a pixel with more than 64 hits, ldo > C with a guard band
that must keep its bits, accumulate 0 and 1, two samples in one launch (a workgroup that straddles the sample boundary reads its
meta block from global memory).

Forward: bit-equal to the V-call composition of es_point_sample_fwd_pts, and within the f64 bound.  Backward: within the derived
bound of the f64 adjoint, two runs bit-equal, and the V-call composition of es_point_sample_bwd (accumulate = 1) within its bound.

Every body is a function of `dev`: tests/test_emu_prefix_fusion.py runs the same bodies on the CPU emulator (dev.type == 'cpu'
selects smaller n there; every V and C is kept)."""
import pytest
import torch

import fusion_geom_spec as G
import prefix_spec as S

pytestmark = pytest.mark.gpu

SENT = -7.25e5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _hip():
    from embodiedscan_amd import hip
    return hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def _small(dev):
    return dev.type == 'cpu'


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _banded(dev, rows, C, ldo):
    """(rows, ldo) f32 buffer of sentinels (+ 8 past the end); returns (whole buffer, (rows, C) view of the first C columns)"""
    buf = torch.full((rows * ldo + 8,), SENT, dtype=torch.float32, device=dev)
    return buf, buf[:rows * ldo].view(rows, ldo)[:, :C]


def _band_ok(buf, rows, C, ldo, label):
    b = buf.clone()
    b[:rows * ldo].view(rows, ldo)[:, :C].fill_(SENT)
    assert bool((b == SENT).all()), f'{label}: a launch wrote outside columns [0, {C}) of its (rows {rows}, ld {ldo}) output'


def fwd_case(dev, stats, case, ldo_pad):
    """the prefix forward and the V-call composition on one case; returns the record (device tensors)"""
    hip = _hip()
    P = hip.P
    V, C, n, Hf, Wf, B = (case[k] for k in ('V', 'C', 'n', 'Hf', 'Wf', 'B'))
    assert (S.NOPS, S.OPS, S.ROTINV, S.PROJ) == tuple(hip.CONSTS[k] for k in ('ES_FUSE_NOPS', 'ES_FUSE_OPS', 'ES_FUSE_ROTINV', 'ES_FUSE_PROJ'))
    label = f'prefix fwd V={V} C={C} n={n} B={B} seed={case["seed"]}'
    coords, points, meta, feats = (case[k].to(dev) for k in ('coords', 'points', 'meta', 'feats'))
    ldo = C + ldo_pad
    obuf, out = _banded(dev, V * n, C, ldo)
    pix = torch.full((n * V + 8,), -77, dtype=torch.int32, device=dev)
    cnt = torch.full((V * n + 8,), -77, dtype=torch.int32, device=dev)
    hip.call('es_point_sample_prefix_fwd_pts', P(coords), P(points), n, P(meta), meta.shape[1], V, P(feats), Hf, Wf, C, P(obuf), ldo, P(pix),
             P(cnt), _st())
    torch.cuda.synchronize()
    _band_ok(obuf, V * n, C, ldo, label)
    assert bool((pix[n * V:] == -77).all()) and bool((cnt[V * n:] == -77).all()), f'{label}: pix / cnt written past their end'
    pix, cnt = pix[:n * V].view(n, V), cnt[:V * n].view(V, n)
    for t in range(V):                                   # (a) the composition: t + 1 views, the sibling kernel
        ft = feats[:, :t + 1].contiguous()
        o_t = torch.full((n, C), SENT, device=dev)
        p_t = torch.empty((n, t + 1), dtype=torch.int32, device=dev)
        c_t = torch.empty(n, dtype=torch.int32, device=dev)
        hip.call('es_point_sample_fwd_pts', P(coords), P(points), n, P(meta), meta.shape[1], t + 1, P(ft), Hf, Wf, C, P(o_t), C, P(p_t), P(c_t),
                 _st())
        torch.cuda.synchronize()
        assert torch.equal(c_t, cnt[t]), f'{label}: cnt of prefix {t} differs from the {t + 1}-view call'
        assert torch.equal(p_t, pix[:, :t + 1]), f'{label}: pix differs from the {t + 1}-view call'
        assert _bits_equal(o_t, out[t * n:(t + 1) * n]), f'{label}: rows of prefix {t} are not bit-equal to the {t + 1}-view call'
    rec = dict(case, coords=coords, feats=feats, out=out, pix=pix, cnt=cnt, obuf=obuf, ldo=ldo)
    S.check_prefix_fwd(rec, dev, stats)                   # (b)
    G.check_geometry(rec, dev, caps=False, label=label)   # pix and cnt themselves, against the f64 geometry
    return rec


def bwd_case(dev, stats, rec, acc, seed, old=True):
    """the prefix backward on a forward record: f64 adjoint bound, two runs, the composition of the existing backward"""
    hip = _hip()
    P = hip.P
    V, C, n, Hf, Wf, B = (rec[k] for k in ('V', 'C', 'n', 'Hf', 'Wf', 'B'))
    label = f'prefix bwd V={V} C={C} n={n} B={B} acc={acc}'
    g = torch.Generator().manual_seed(seed)
    ldo = rec['ldo']
    dbuf, dout = _banded(dev, V * n, C, ldo)
    dout.copy_(torch.randn(V * n, C, generator=g))
    n_img, HW = B * V, Hf * Wf
    prior = torch.randn(n_img * HW, C, generator=g)
    runs = []
    for _ in range(2):
        df = torch.full((n_img * HW * C + 8,), SENT, device=dev)
        df[:n_img * HW * C] = prior.reshape(-1).to(dev)
        head = torch.empty(n_img * HW, dtype=torch.int32, device=dev)
        nxt = torch.empty(n * V, dtype=torch.int32, device=dev)
        hip.call('es_point_sample_prefix_bwd', P(rec['coords']), n, V, P(dbuf), ldo, P(rec['pix']), P(rec['cnt']), Hf, Wf, C, P(df), n_img,
                 P(head), P(nxt), acc, _st())
        torch.cuda.synchronize()
        assert bool((df[n_img * HW * C:] == SENT).all()), f'{label}: written past the end of dfeats'
        runs.append(df[:n_img * HW * C].view(n_img * HW, C))
    assert _bits_equal(runs[0], runs[1]), f'{label}: two runs differ'
    _band_ok(dbuf, V * n, C, ldo, label + ' (dout)')
    brec = dict(rec, dout=dout, acc=acc, dfeats=runs[0], dfeats0=prior)
    S.check_prefix_bwd(brec, dev, stats)
    if old and B == 1:
        # the composition of the existing kernel: call t sees views 0 .. t (pix (n, t + 1), images 0 .. t), rows t n .. of dout
        comp = (prior.clone() if acc else torch.zeros(n_img * HW, C)).to(dev)
        for t in range(V):
            p_t = rec['pix'][:, :t + 1].contiguous()
            c_t = rec['cnt'][t].contiguous()
            head = torch.empty((t + 1) * HW, dtype=torch.int32, device=dev)
            nxt = torch.empty(n * (t + 1), dtype=torch.int32, device=dev)
            hip.call('es_point_sample_bwd', P(rec['coords']), n, t + 1, dbuf.data_ptr() + 4 * t * n * ldo, ldo, P(p_t), P(c_t), Hf, Wf, C, P(comp),
                     t + 1, P(head), P(nxt), 1, _st())
        torch.cuda.synchronize()
        S.check_prefix_bwd(dict(brec, composed=comp), dev, stats, cls='prefix_bwd (V-call composition)', extra_ops=1, key='composed')
        _, b_new, p_new = S.prefix_bwd_bound(brec, dev)
        _, b_old, p_old = S.prefix_bwd_bound(brec, dev, extra_ops=1)
        slack = S.U * (b_new + b_old) + (S.U * (p_new + p_old) if acc else 0)
        diff = (comp.double() - runs[0].double()).abs()
        assert bool((diff <= slack).all()), f'{label}: differs from the V-call composition by more than the sum of the two bounds'
    return brec


def grid(dev):
    """(V, C, n, Hf, Wf, aug, B, blind, cluster, ldo_pad, acc).  Every (V, C) pair occurs; n, the meta kind, the pad, accumulate, the blind
    views and the cluster rotate on counters of their own"""
    small = _small(dev)
    cases, i = [], 0
    for V in (1, 2, 3, 10, 20):
        for C in (32, 40, 256, 512):
            n = ((37, 48, 61, 80) if small else (333, 1024, 1501, 2000))[i % 4]
            if V >= 10 and C >= 256:
                n = 35 if small else 700
            blind = (0, min(2, V - 1), 0, min(1, V - 1), V - 1 if V == 3 else 0)[i % 5]
            cluster = (0, 0, 70)[i % 3] if n > 100 or (small and C <= 40 and V <= 3) else 0
            B = 2 if i % 7 == 3 else 1
            cases.append((V, C, max(n, cluster * 2), (5, 9)[i % 2], (7, 12)[i % 2], int(i % 2 == 1), B, blind, cluster, (8, 0, 3, 40)[i % 4],
                          int(i % 3 == 1)))
            i += 1
    assert {c[5] for c in cases} == {0, 1} and {c[10] for c in cases} == {0, 1} and any(c[9] > 0 for c in cases)
    return cases


def test_prefix_fusion_on_the_shape_grid(dev):
    sf, sb = S.Stats('prefix forward grid'), S.Stats('prefix backward grid')
    cov = dict(late_first=0, never=0, no_pixel_in_live_voxel=0, invalid_with_pixel=0, busiest=0)
    for i, (V, C, n, Hf, Wf, aug, B, blind, cluster, pad, acc) in enumerate(grid(dev)):
        case = S.make_case(V, C, n, Hf, Wf, aug, 1000 + i, B=B, blind=blind, cluster=cluster)
        rec = fwd_case(dev, sf, case, pad)
        bwd_case(dev, sb, rec, acc, 2000 + i)
        c = S.coverage(rec)
        for k in cov:
            cov[k] = max(cov[k], c[k]) if k == 'busiest' else cov[k] + c[k]
    print(sf.report())
    print(sb.report())
    print('coverage:', cov)
    assert cov['late_first'] > 0 and cov['never'] > 0 and cov['no_pixel_in_live_voxel'] > 0 and cov['invalid_with_pixel'] > 0
    assert cov['busiest'] > 64, 'no pixel with more than 64 hits in the grid'


def test_prefix_forward_refusals_write_nothing(dev):
    """C > 512 returns -4 like the sibling, V > 64 a status of its own; nothing is written"""
    hip = _hip()
    P = hip.P
    for V, C, want in ((2, 513, -4), (65, 32, -9)):
        n = 20
        case = S.make_case(min(V, 3), 32, n, 4, 5, 0, 5)
        coords, points = case['coords'].to(dev), case['points'].to(dev)
        meta = torch.zeros(1, S.PROJ + 16 * V, device=dev)
        feats = torch.zeros(V * 20 * C, device=dev)
        out = torch.full((V * n, C), SENT, device=dev)
        pix = torch.full((n, V), -77, dtype=torch.int32, device=dev)
        cnt = torch.full((V, n), -77, dtype=torch.int32, device=dev)
        rc = hip.raw('es_point_sample_prefix_fwd_pts')(P(coords), P(points), n, P(meta), meta.shape[1], V, P(feats), 4, 5, C, P(out), C, P(pix),
                                                       P(cnt), _st())
        rs = hip.raw('es_point_sample_fwd_pts')(P(coords), P(points), n, P(meta), meta.shape[1], V, P(feats), 4, 5, C, P(out), C, P(pix),
                                                P(cnt), _st()) if C > 512 else None
        torch.cuda.synchronize()
        assert rc == want and rc != 0 and (rs is None or rs == rc), (V, C, rc, rs)
        assert bool((out == SENT).all()) and bool((pix == -77).all()) and bool((cnt == -77).all())
    dfe = torch.full((40, 513), SENT, device=dev)
    z = torch.zeros(64, dtype=torch.int32, device=dev)
    assert hip.raw('es_point_sample_prefix_bwd')(P(z), 4, 2, P(dfe), 513, P(z), P(z), 4, 5, 513, P(dfe), 2, P(z), P(z), 0, _st()) == -4
    torch.cuda.synchronize()
    assert bool((dfe == SENT).all())
