"""The view-window fusion kernels (csrc/fusion.hip) held to tests/window_spec.py on the shape grid: V in {1, 3, 10, 64}, C in {1, 40,
256, 512}, n in {1, 15, 16, 17, 150} (a 16-row workgroup that straddles two samples with different windows), window tables all 1 / all
V / ascending (the detector's) / non-monotone, a sample without rows in the middle of the batch, two image sets with the samples
alternating between them, leading views that see nothing (rows valid only beyond their window), meta blocks with and without
reverse-augmentation ops, f32 and bf16 feature maps.

Forward: bit-equal to the per-sample composition of es_point_sample_fwd(_h) (the yardstick) and within the f64 bound; pix beyond the
window is -1 on a buffer handed in full of garbage.  Backward: within the derived bound of the f64 adjoint, two runs bit-equal; with
full windows forward and backward are bit-equal to es_point_sample_fwd / _bwd on the whole batch.

Every body is a function of `dev`: tests/test_emu_window_fusion.py runs the same bodies on the CPU emulator."""
import pytest
import torch

import fusion_geom_spec as G
import window_spec as S

pytestmark = pytest.mark.gpu

SENT = -7.25e5
GARBAGE = 12345


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _hip():
    from embodiedscan_amd import hip
    return hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def yardstick(dev, case, half, V_use=None):
    """per sample b: es_point_sample_fwd(_h) on the sample's row slice, batch column zeroed, V' = w_b (V_use: another view count for
    every sample), meta row b, feature pointer at set s_b -> out (n, C), cnt (n), pix (n, V) with -1 beyond V'"""
    hip = _hip()
    P = hip.P
    V, C, n, Hf, Wf = (case[k] for k in ('V', 'C', 'n', 'Hf', 'Wf'))
    coords, meta, win = case['coords'].to(dev), case['meta'].to(dev), case['win']
    feats = case['feats'].to(dev)
    if half:
        feats = feats.to(torch.bfloat16)
    out = torch.full((n, C), SENT, device=dev)
    cnt = torch.full((n,), -77, dtype=torch.int32, device=dev)
    pix = torch.full((n, V), -1, dtype=torch.int32, device=dev)
    bcol = case['coords'][:, 0]
    for b in range(case['B']):
        rows = torch.nonzero(bcol == b).squeeze(1)
        if rows.numel() == 0:
            continue
        r0, r1 = int(rows[0]), int(rows[-1]) + 1
        assert r1 - r0 == rows.numel(), 'the rows of a sample are contiguous'
        s, w = int(win[b, 0]), (int(win[b, 1]) if V_use is None else V_use)
        cb = coords[r0:r1].clone()
        cb[:, 0] = 0
        ob = torch.full((r1 - r0, C), SENT, device=dev)
        pb = torch.empty((r1 - r0, w), dtype=torch.int32, device=dev)
        kb = torch.empty(r1 - r0, dtype=torch.int32, device=dev)
        hip.call('es_point_sample_fwd_h' if half else 'es_point_sample_fwd', P(cb), r1 - r0, S.VS, meta.data_ptr() + 4 * b * meta.shape[1],
                 meta.shape[1], w, feats.data_ptr() + feats.element_size() * s * V * Hf * Wf * C, Hf, Wf, C, P(ob), C, P(pb), P(kb), _st())
        torch.cuda.synchronize()
        out[r0:r1], cnt[r0:r1], pix[r0:r1, :w] = ob, kb, pb
    return dict(case, coords=coords, feats=feats, out=out, cnt=cnt, pix=pix)


def fwd_case(dev, stats, case, half, ldo_pad=0):
    """the window forward against the yardstick (bits) and the f64 bound; returns (record of the launch, yardstick record)"""
    hip = _hip()
    P = hip.P
    V, C, n, Hf, Wf = (case[k] for k in ('V', 'C', 'n', 'Hf', 'Wf'))
    assert (S.NOPS, S.OPS, S.ROTINV, S.PROJ) == tuple(hip.CONSTS[k] for k in ('ES_FUSE_NOPS', 'ES_FUSE_OPS', 'ES_FUSE_ROTINV', 'ES_FUSE_PROJ'))
    label = f'window fwd V={V} C={C} n={n} B={case["B"]} {case["kind"]} sets={case["n_sets"]} half={half} seed={case["seed"]}'
    yard = yardstick(dev, case, half)
    coords, meta, win, feats = yard['coords'], case['meta'].to(dev), case['win'].to(dev), yard['feats']
    ldo = C + ldo_pad
    obuf = torch.full((n * ldo + 8,), SENT, dtype=torch.float32, device=dev)
    out = obuf[:n * ldo].view(n, ldo)[:, :C]
    pix = torch.full((n * V + 8,), GARBAGE, dtype=torch.int32, device=dev)         # non-negative garbage: every entry must be written
    cnt = torch.full((n + 8,), -77, dtype=torch.int32, device=dev)
    hip.call('es_point_sample_win_fwd_h' if half else 'es_point_sample_win_fwd', P(coords), n, S.VS, P(meta), meta.shape[1], V, P(win), P(feats),
             Hf, Wf, C, P(obuf), ldo, P(pix), P(cnt), _st())
    torch.cuda.synchronize()
    band = obuf.clone()
    band[:n * ldo].view(n, ldo)[:, :C].fill_(SENT)
    assert bool((band == SENT).all()), f'{label}: written outside columns [0, {C}) of the output'
    assert bool((pix[n * V:] == GARBAGE).all()) and bool((cnt[n:] == -77).all()), f'{label}: pix / cnt written past their end'
    pix, cnt = pix[:n * V].view(n, V), cnt[:n]
    assert torch.equal(cnt, yard['cnt']), f'{label}: cnt differs from the yardstick'
    assert torch.equal(pix, yard['pix']), f'{label}: pix differs from the yardstick (in-window columns) or is not -1 beyond the window'
    assert _bits_equal(out, yard['out']), f'{label}: rows are not bit-equal to the yardstick'
    rec = dict(yard, out=out.contiguous(), pix=pix, cnt=cnt, win=win)
    S.check_win_fwd(rec, dev, stats)
    G.check_geometry(rec, dev, vs=S.VS, caps=False, label=label)      # pix and cnt themselves, against the f64 geometry
    return rec, yard


def bwd_case(dev, stats, rec, acc, seed):
    """the window backward on a forward record: f64 adjoint bound, two runs bit-equal"""
    hip = _hip()
    P = hip.P
    V, C, n, Hf, Wf, n_sets = (rec[k] for k in ('V', 'C', 'n', 'Hf', 'Wf', 'n_sets'))
    label = f'window bwd V={V} C={C} n={n} B={rec["B"]} sets={n_sets} acc={acc}'
    g = torch.Generator().manual_seed(seed)
    dout = torch.randn(n, C, generator=g).to(dev)
    n_img, HW = n_sets * V, Hf * Wf
    prior = torch.randn(n_img * HW, C, generator=g)
    runs = []
    for _ in range(2):
        df = torch.full((n_img * HW * C + 8,), SENT, device=dev)
        df[:n_img * HW * C] = prior.reshape(-1).to(dev)
        head = torch.empty(n_img * HW, dtype=torch.int32, device=dev)
        nxt = torch.empty(max(n * V, 1), dtype=torch.int32, device=dev)
        hip.call('es_point_sample_win_bwd', P(rec['coords']), n, V, P(rec['win']), P(dout), C, P(rec['pix']), P(rec['cnt']), Hf, Wf, C, P(df),
                 n_img, P(head), P(nxt), acc, _st())
        torch.cuda.synchronize()
        assert bool((df[n_img * HW * C:] == SENT).all()), f'{label}: written past the end of dfeats'
        runs.append(df[:n_img * HW * C].view(n_img * HW, C))
    assert _bits_equal(runs[0], runs[1]), f'{label}: two runs differ'
    brec = dict(rec, dout=dout, acc=acc, dfeats=runs[0], dfeats0=prior)
    S.check_win_bwd(brec, dev, stats)
    return brec


def grid():
    """(V, C, n, B, kind, n_sets, blind, aug, empty, half).  Every (V, C) pair occurs; n, the window table, the sets, the blind views,
    the meta kind and the feature dtype rotate on counters of their own"""
    cases, i = [], 0
    for V in (1, 3, 10, 64):
        for C in (1, 40, 256, 512):
            n = (150, 17, 16, 15, 1)[i % 5]
            kind = ('asc', 'arb', 'one', 'full')[(i + i // 4) % 4]
            B = 1 if n == 1 else (min(max(V, 2), 10) if n == 150 else (2, 3)[i % 2])
            empty = 1 if B >= 3 else None
            n_sets = 2 if (i % 3 == 1 and B >= 2) else 1
            blind = min((0, 2, 1)[i % 3], V - 1)
            cases.append((V, C, n, B, kind, n_sets, blind, int(i % 2 == 1), empty, int(i % 4 >= 2)))
            i += 1
    # the table kinds every V must meet with a straddled workgroup, blind views under a short window, and both dtypes once more
    cases += [(10, 40, 150, 10, 'asc', 1, 3, 1, None, 0), (10, 40, 150, 10, 'asc', 1, 3, 0, None, 1), (64, 256, 150, 9, 'arb', 2, 2, 1, 4, 1),
              (3, 512, 17, 2, 'asc', 2, 1, 0, None, 0), (64, 1, 16, 3, 'arb', 1, 0, 1, 1, 0), (3, 40, 15, 3, 'asc', 1, 2, 1, 1, 1)]
    assert {c[7] for c in cases} == {0, 1} and {c[9] for c in cases} == {0, 1} and {c[4] for c in cases} == {'asc', 'arb', 'one', 'full'}
    assert {c[2] for c in cases} == {1, 15, 16, 17, 150} and any(c[8] is not None for c in cases) and any(c[5] == 2 for c in cases)
    return cases


def run_grid(dev, do_bwd=True):
    """the grid's forward (and backward) checks; returns the coverage summed over the cases (from the yardstick's outputs)"""
    sf, sb = S.Stats('window forward grid'), S.Stats('window backward grid')
    cov = dict(straddle=0, beyond=0, dead_in_wide_window=0, invalid_with_pixel=0)
    for i, (V, C, n, B, kind, n_sets, blind, aug, empty, half) in enumerate(grid()):
        case = S.make_case(V, C, n, 5, 7, aug, 1000 + i, B=B, kind=kind, n_sets=n_sets, blind=blind, empty=empty)
        rec, yard = fwd_case(dev, sf, case, half, ldo_pad=(0, 8, 3)[i % 3])
        full = yardstick(dev, case, half, V_use=V)['cnt'] if blind else None
        c = S.coverage(yard, full)
        for k in cov:
            cov[k] += c[k]
        if do_bwd:
            bwd_case(dev, sb, dict(rec, feats=None), i % 2, 2000 + i)
    print(sf.report())
    print(sb.report())
    print('coverage:', cov)
    return cov


def test_window_fusion_on_the_shape_grid(dev):
    cov = run_grid(dev)
    assert cov['straddle'] > 0, 'no workgroup straddles two samples with different windows'
    assert cov['beyond'] > 0, 'no row is valid only beyond its window'
    assert cov['dead_in_wide_window'] > 0, 'no row with cnt = 0 inside a window of >= 2 views'
    assert cov['invalid_with_pixel'] > 0, 'no view with a pixel but an invalid flag'


def test_full_windows_are_the_existing_kernels_bit_for_bit(dev):
    """win[b] = (b, V), B = 2: forward and backward equal es_point_sample_fwd / _bwd on the whole batch"""
    hip = _hip()
    P = hip.P
    for V, C, n, acc in ((3, 40, 150, 0), (10, 256, 17, 1), (64, 512, 16, 0), (1, 1, 15, 1)):
        case = S.make_case(V, C, n, 5, 7, 1, 500 + V, B=2, kind='full', n_sets=2, blind=min(1, V - 1), cluster=70 if n == 150 else 0)
        rec, _ = fwd_case(dev, S.Stats('full window'), case, 0)
        coords, meta, feats = rec['coords'], case['meta'].to(dev), rec['feats']
        out = torch.full((n, C), SENT, device=dev)
        pix = torch.empty((n, V), dtype=torch.int32, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        hip.call('es_point_sample_fwd', P(coords), n, S.VS, P(meta), meta.shape[1], V, P(feats), 5, 7, C, P(out), C, P(pix), P(cnt), _st())
        torch.cuda.synchronize()
        assert torch.equal(pix, rec['pix']) and torch.equal(cnt, rec['cnt']) and _bits_equal(out, rec['out'])
        brec = bwd_case(dev, S.Stats('full window'), rec, acc, 600 + V)
        n_img, HW = 2 * V, 35
        df = brec['dfeats0'].clone().to(dev)
        head = torch.empty(n_img * HW, dtype=torch.int32, device=dev)
        nxt = torch.empty(n * V, dtype=torch.int32, device=dev)
        hip.call('es_point_sample_bwd', P(coords), n, V, P(brec['dout']), C, P(pix), P(cnt), 5, 7, C, P(df), n_img, P(head), P(nxt), acc, _st())
        torch.cuda.synchronize()
        assert _bits_equal(df, brec['dfeats']), f'V={V} C={C}: the full-window backward is not bit-equal to es_point_sample_bwd'


def test_window_backward_cluster_two_sets_accumulate(dev):
    """>= 150 rows on one pixel (the more-than-64-hits path of the gather), one and two image sets, accumulate 0 and 1"""
    sf, sb = S.Stats('window forward (cluster)'), S.Stats('window backward (cluster)')
    busiest = 0
    for j, (V, C, n, B, kind, n_sets, acc) in enumerate(((3, 40, 480, 1, 'full', 1, 0), (10, 40, 480, 1, 'arb', 1, 1),
                                                          (3, 256, 500, 4, 'asc', 2, 1), (10, 1, 500, 4, 'arb', 2, 0))):
        case = S.make_case(V, C, n, 5, 7, j % 2, 3000 + j, B=B, kind=kind, n_sets=n_sets, cluster=160)
        rec, _ = fwd_case(dev, sf, case, 0)
        brec = bwd_case(dev, sb, rec, acc, 3100 + j)
        busiest = max(busiest, int(S.win_bwd_bound(brec, dev)[3].max()))
    print(sf.report())
    print(sb.report())
    print('busiest pixel:', busiest, 'hits')
    assert busiest >= 150, 'no pixel with 150 or more linked hits'


def test_window_refusals_write_nothing(dev):
    """C > 512 returns -4, V > 64 returns -9, forward (both dtypes) and backward; nothing is written"""
    hip = _hip()
    P = hip.P
    for V, C, want in ((2, 513, -4), (65, 32, -9)):
        n = 20
        case = S.make_case(min(V, 3), 32, n, 4, 5, 0, 5)
        coords = case['coords'].to(dev)
        meta = torch.zeros(1, S.PROJ + 16 * V, device=dev)
        win = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
        feats = torch.zeros(V * 20 * C, device=dev)
        out = torch.full((n, C), SENT, device=dev)
        pix = torch.full((n, V), GARBAGE, dtype=torch.int32, device=dev)
        cnt = torch.full((n,), -77, dtype=torch.int32, device=dev)
        for name in ('es_point_sample_win_fwd', 'es_point_sample_win_fwd_h'):
            rc = hip.raw(name)(P(coords), n, S.VS, P(meta), meta.shape[1], V, P(win), P(feats), 4, 5, C, P(out), C, P(pix), P(cnt), _st())
            torch.cuda.synchronize()
            assert rc == want, (name, V, C, rc)
            assert bool((out == SENT).all()) and bool((pix == GARBAGE).all()) and bool((cnt == -77).all())
        dfe = torch.full((V * 20, C), SENT, device=dev)
        head = torch.full((V * 20,), GARBAGE, dtype=torch.int32, device=dev)
        nxt = torch.full((n * V,), GARBAGE, dtype=torch.int32, device=dev)
        rc = hip.raw('es_point_sample_win_bwd')(P(coords), n, V, P(win), P(out), C, P(pix), P(cnt), 4, 5, C, P(dfe), V, P(head), P(nxt), 0, _st())
        torch.cuda.synchronize()
        assert rc == want, ('es_point_sample_win_bwd', V, C, rc)
        assert bool((dfe == SENT).all()) and bool((head == GARBAGE).all()) and bool((nxt == GARBAGE).all())
