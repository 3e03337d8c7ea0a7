"""The one-view step of the prefix fusion (csrc/fusion.hip: es_point_sample_step_fwd_pts) held to tests/walk_spec.py: walks of T in
{1, 3, 10} steps, C in {32, 40, 256, 512}, n in {1, 37, 150} with Hf, Wf = 5, 7; two samples in one launch (a workgroup that straddles
the sample boundary reads its meta block from global memory), leading views that see nothing (zero rows, nvalid 0), many voxels on one
pixel, meta blocks with and without reverse-augmentation ops, ldo = C + 8 with a guard band that must keep its bits, sentinel tails
behind pix, nvalid and the sum.

Per step: (a) bit-equal to the prefix kernel's row block, cnt row and pix column, (b) the assembled walk within the f64 bound of
tests/prefix_spec.py, (c) two walks from zero state bit-equal.  Refusals write nothing.

Every body is a function of `dev`: tests/test_emu_walk_step.py runs the same bodies on the CPU emulator (dev.type == 'cpu' selects the
smaller n there; every T and C is kept)."""
import pytest
import torch

import fusion_geom_spec as G
import prefix_spec as S
import walk_spec as W
from test_gpu_prefix_fusion import SENT, _band_ok, _banded, _bits_equal, _hip, _small, _st

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def walk(dev, case, ldo_pad, label):
    """one walk from zero state: T launches -> [dict(out, nvalid, pix)] (copies taken after each step) and the final sum"""
    hip = _hip()
    P = hip.P
    T, C, n, Hf, Wf = (case[k] for k in ('V', 'C', 'n', 'Hf', 'Wf'))
    coords, points = case['coords'].to(dev), case['points'].to(dev)
    ldo = C + ldo_pad
    sbuf = torch.full((n * C + 8,), SENT, dtype=torch.float32, device=dev)
    sbuf[:n * C] = 0.0
    nbuf = torch.full((n + 8,), -77, dtype=torch.int32, device=dev)
    nbuf[:n] = 0
    steps = []
    for t in range(T):
        meta = W.step_meta(case['meta'], t).to(dev)
        feats = W.step_feats(case['feats'], t).to(dev)
        obuf, out = _banded(dev, n, C, ldo)
        pix = torch.full((n + 8,), -77, dtype=torch.int32, device=dev)
        hip.call('es_point_sample_step_fwd_pts', P(coords), P(points), n, P(meta), meta.shape[1], P(feats), Hf, Wf, C, P(sbuf), P(nbuf), P(obuf),
                 ldo, P(pix), _st())
        torch.cuda.synchronize()
        _band_ok(obuf, n, C, ldo, f'{label} step {t}')
        assert bool((pix[n:] == -77).all()) and bool((nbuf[n:] == -77).all()) and bool((sbuf[n * C:] == SENT).all()), \
            f'{label} step {t}: pix / nvalid / sum written past their end'
        steps.append(dict(out=out.clone(), nvalid=nbuf[:n].clone(), pix=pix[:n].clone()))
    return steps, sbuf[:n * C].view(n, C).clone()


def prefix(dev, case):
    """the prefix kernel on the same views: dict(out (T n, C), pix (n, T), cnt (T, n))"""
    hip = _hip()
    P = hip.P
    V, C, n, Hf, Wf = (case[k] for k in ('V', 'C', 'n', 'Hf', 'Wf'))
    coords, points, meta, feats = (case[k].to(dev) for k in ('coords', 'points', 'meta', 'feats'))
    out = torch.full((V * n, C), SENT, device=dev)
    pix = torch.empty((n, V), dtype=torch.int32, device=dev)
    cnt = torch.empty((V, n), dtype=torch.int32, device=dev)
    hip.call('es_point_sample_prefix_fwd_pts', P(coords), P(points), n, P(meta), meta.shape[1], V, P(feats), Hf, Wf, C, P(out), C, P(pix), P(cnt),
             _st())
    torch.cuda.synchronize()
    return dict(out=out, pix=pix, cnt=cnt)


def walk_case(dev, stats, case, ldo_pad):
    """(a), (b), (c) on one case; returns (case with device coords / feats, steps)"""
    label = f'walk T={case["V"]} C={case["C"]} n={case["n"]} B={case["B"]} seed={case["seed"]}'
    steps, state = walk(dev, case, ldo_pad, label)
    W.same_as_prefix(label, steps, prefix(dev, case))                                           # (a)
    dcase = dict(case, coords=case['coords'].to(dev), feats=case['feats'].to(dev))
    W.check_walk(dcase, steps, dev, stats)                                                     # (b)
    G.check_geometry(W.assemble(dcase, steps), dev, caps=False, label=label)                   # pix and nvalid against the f64 geometry
    again, state2 = walk(dev, case, ldo_pad, label)                                            # (c)
    for t, (s, r) in enumerate(zip(steps, again)):
        assert _bits_equal(s['out'], r['out']) and torch.equal(s['nvalid'], r['nvalid']) and torch.equal(s['pix'], r['pix']), \
            f'{label}: step {t} of two walks from zero state differs'
    assert _bits_equal(state, state2), f'{label}: the sums of two walks differ'
    return dcase, steps


def test_walk_step_on_the_shape_grid(dev):
    assert S.PROJ == _hip().CONSTS['ES_FUSE_PROJ']
    st = W.Stats('walk step grid')
    cov = dict(late_first=0, never=0, no_pixel_in_live_voxel=0, invalid_with_pixel=0, busiest=0)
    zero_rows = straddle = 0
    for i, (T, C, n, B, blind, cluster, aug, pad) in enumerate(W.grid(_small(dev))):
        case = S.make_case(T, C, n, 5, 7, aug, 6000 + i, B=B, blind=blind, cluster=cluster)
        dcase, steps = walk_case(dev, st, case, pad)
        c = S.coverage(W.assemble(dcase, steps))
        for k in cov:
            cov[k] = max(cov[k], c[k]) if k == 'busiest' else cov[k] + c[k]
        if blind:
            z = steps[blind - 1]
            assert bool((z['nvalid'] == 0).all()) and bool((z['out'] == 0).all()), 'a step before the first seeing view wrote something'
            zero_rows += n
        if B > 1:
            b = case['coords'][:, 0]
            straddle += sum(int(b[r0] != b[min(r0 + 15, n - 1)]) for r0 in range(0, n, 16))
    print(st.report())
    print('coverage:', cov, 'zero rows before the first seeing view:', zero_rows, 'workgroups across a sample boundary:', straddle)
    assert cov['late_first'] > 0 and cov['never'] > 0 and cov['no_pixel_in_live_voxel'] > 0 and cov['invalid_with_pixel'] > 0
    assert cov['busiest'] > (16 if _small(dev) else 64) and zero_rows > 0 and straddle > 0


def test_walk_step_refusals_write_nothing(dev):
    """C > 512 returns -4 like the siblings with sum, nvalid, out and pix untouched; n = 0 returns 0"""
    hip = _hip()
    P = hip.P
    n, C = 20, 513
    case = S.make_case(1, 32, n, 4, 5, 0, 5)
    coords, points = case['coords'].to(dev), case['points'].to(dev)
    meta = W.step_meta(case['meta'], 0).to(dev)
    feats = torch.zeros(20 * C, device=dev)
    ssum = torch.full((n, C), SENT, device=dev)
    out = torch.full((n, C), SENT, device=dev)
    nval = torch.full((n,), -77, dtype=torch.int32, device=dev)
    pix = torch.full((n,), -77, dtype=torch.int32, device=dev)
    rc = hip.raw('es_point_sample_step_fwd_pts')(P(coords), P(points), n, P(meta), meta.shape[1], P(feats), 4, 5, C, P(ssum), P(nval), P(out), C,
                                                 P(pix), _st())
    r0 = hip.raw('es_point_sample_step_fwd_pts')(P(coords), P(points), 0, P(meta), meta.shape[1], P(feats), 4, 5, 32, P(ssum), P(nval), P(out), C,
                                                 P(pix), _st())
    torch.cuda.synchronize()
    assert rc == -4 and r0 == 0, (rc, r0)
    assert bool((ssum == SENT).all()) and bool((out == SENT).all()) and bool((nval == -77).all()) and bool((pix == -77).all())
