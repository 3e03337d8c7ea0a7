"""Specification of the prefix-fusion kernels (csrc/fusion.hip: es_point_sample_prefix_fwd_pts, es_point_sample_prefix_bwd), the
front of the continuous occupancy detector (embodied_occ.py:165-203 of the reference: one batch_point_sample over views 0..t for
every prefix t).  Used by tests/test_gpu_prefix_fusion.py (MI355X) and tests/test_emu_prefix_fusion.py (the same bodies on the CPU
emulator, plus mutated outputs the checker must reject).  u = 2^-24; every bound is per element and none depends on 1 / |spec|.

Forward.  (a) bit for bit the V-call composition of es_point_sample_fwd_pts with view counts 1 .. V (the test bodies make those
calls).  (b) check_prefix_fwd: on the launch's own pix (n, V) and cnt (V, n), with f(u, i) the feature row view u's pixel of voxel
i holds (nothing where pix = -1; ALL views with a pixel are summed, valid or not: SURVEY Q3),
    out[t n + i] = sum_{u <= t} f(u, i) / cnt[t][i]     (0 where cnt[t][i] = 0),
  |out - spec| <= (k + 1) u sum_{u <= t} |f(u, i)| / cnt[t][i], k the number of summed views: k f32 additions (the first one, into
  0, is exact, so this is one more than needed) and one IEEE division.  cnt must not fall with t and must rise by at most one.

Backward.  check_prefix_bwd: the f64 adjoint of that forward.  Pixel p of view v receives, from every voxel i with pix[i][v] = p,
    g(i, v) = sum_{t = V-1 .. v, cnt[t][i] > 0} dout[t n + i] / cnt[t][i].
  f32 operations a term dout[t n + i][c] / cnt[t][i] passes through in k_ps_prefix_gather before it is part of the element:
    1           inv = 1 / cnt[t][i]                             (one IEEE division)
    V - v       at most: the fused multiply-adds gs = fma(dout, inv, gs) of the suffix chain t = V-1 .. v, one rounding each
                (the product is not rounded on its own); the term enters at its own fma and is re-rounded by the later ones
    H           at most: the additions acc += g(i, v) over the H voxels that hit the pixel and have a valid view in the last prefix
    acc         one more addition into the prior when the launch accumulates (the prior itself is held to u |prior| on top)
  D = 1 + (V - v) + H + acc roundings, each relative u: |got - spec| <= ((1 + u)^D - 1) sum |terms| <= D u / (1 - D u) sum |terms|,
  and D u / (1 - D u) <= (D + 1) u as long as D (D + 1) u <= 1 (D <= 4095, asserted).  So m = D + 1 = V - v + H + acc + 2.
  A pixel nothing hits holds an exact zero (its prior bit for bit when accumulating): its bound is 0.
  The V-call composition of the EXISTING es_point_sample_bwd (call t: views 0 .. t, rows t n .. (t + 1) n of dout, accumulate = 1)
  computes the same adjoint with one more rounding per term when the launch does not itself accumulate (its multiply by inv and
  its addition are separate operations: 2 instead of 1; the V - v accumulating calls stand for the suffix chain, and the first of
  them adds to the prior, which every later one re-rounds: (V - v) u |prior| instead of u |prior|): it is held to m + 1
  (`extra_ops=1`), and the two results then differ by at most the sum of their bounds.

Worst ratios observed, |err| / (bound / G) against G = 8 (MI355X on the full grid / CPU emulator on the reduced grid):
  prefix_fwd 4.83 / 4.51   prefix_bwd 4.10 / 3.87   prefix_bwd (V-call composition) 3.42 / 3.23"""
import math

import torch

from fwd_spec import F64, G, U, Stats, bound_check  # noqa: F401

__all__ = ['Stats', 'U', 'make_case', 'check_prefix_fwd', 'check_prefix_bwd', 'prefix_bwd_bound', 'coverage']

# offsets of the per-sample meta block (include/es_hip.h ES_FUSE_*; the tests assert they equal hip.CONSTS)
NOPS, OPS, ROTINV, ISCALE, NTRANS, SFX, SFY, CROPX, CROPY, FLIP, ORIW, PADW, PADH, PROJ = 0, 1, 9, 18, 19, 22, 23, 24, 25, 26, 27, 28, 29, 32


def _held(label, got, spec, bound_u, prior, cls, stats):
    """|got - spec| <= u bound_u + u |prior|; the printed ratio is |err| / (bound / G): G = 8 means nothing to spare"""
    return bound_check(label, got, spec, U * bound_u / G, prior if prior is not None else torch.zeros_like(spec), False, cls, stats)


def _camera(g, look_away):
    """a 4x4 intrinsic @ extrinsic of a camera 3 m from the origin, looking at it (or away from it: every point is behind it)"""
    d = torch.randn(3, generator=g, dtype=F64)
    d = d / d.norm()
    up = torch.tensor([0.0, 0.0, 1.0], dtype=F64) if abs(float(d[2])) < 0.9 else torch.tensor([1.0, 0.0, 0.0], dtype=F64)
    rx = torch.linalg.cross(up, d)
    rx = rx / rx.norm()
    ry = torch.linalg.cross(d, rx)
    R = torch.stack([rx, ry, d])
    c = -3.0 * d
    if look_away:
        R = torch.stack([rx, -ry, -d])
    E = torch.eye(4, dtype=F64)
    E[:3, :3], E[:3, 3] = R, -R @ c
    return E


def make_case(V, C, n, Hf, Wf, aug, seed, B=1, blind=0, cluster=0, img=(48, 64), focal=40.0):
    """host tensors of one launch: coords (n, 4) int32 (column 0: the sample, ascending), points (n, 3), meta (B, stride), feats
    (B, V, Hf Wf, C), V, C, Hf, Wf.  `blind` leading views look away from the scene (no voxel is valid in them: cnt starts 0 .. 0);
    `cluster` voxels share one location at the origin (one pixel per view then has that many hits); aug: a reverse-augmentation op
    list (T, S, R, HF, VF), image scale factors, crop offset and flip"""
    g = torch.Generator().manual_seed(seed)
    H, W = img
    stride = PROJ + 16 * V + 4
    meta = torch.zeros(B, stride, dtype=torch.float32)
    for b in range(B):
        m = meta[b]
        m[SFX], m[SFY], m[PADW], m[PADH], m[ORIW] = 1.0, 1.0, float(W), float(H), float(W)
        m[ISCALE] = 1.0
        m[ROTINV:ROTINV + 9] = torch.eye(3).reshape(-1)
        if aug:
            a = 0.3 + 0.1 * b
            ops = [1, 2, 3, 4, 5][:5 - b]
            m[NOPS] = len(ops)
            m[OPS:OPS + len(ops)] = torch.tensor(ops, dtype=torch.float32)
            m[ROTINV:ROTINV + 9] = torch.tensor([math.cos(a), -math.sin(a), 0, math.sin(a), math.cos(a), 0, 0, 0, 1], dtype=torch.float32)
            m[ISCALE] = 1 / 1.05
            m[NTRANS:NTRANS + 3] = torch.tensor([0.1, -0.05, 0.02])
            m[SFX], m[SFY], m[CROPX], m[CROPY], m[FLIP] = 0.9, 1.1, 3.0, 2.0, 1.0
        K = torch.tensor([[focal, 0, W / 2, 0], [0, focal, H / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=F64)
        for v in range(V):
            m[PROJ + 16 * v:PROJ + 16 * v + 16] = (K @ _camera(g, v < blind)).reshape(-1).float()
    points = (torch.rand(n, 3, generator=g) * 4 - 2)
    if cluster:
        points[n // 3:n // 3 + cluster] = 0.0
    coords = torch.zeros(n, 4, dtype=torch.int32)
    if B > 1:
        coords[:, 0] = (torch.arange(n) * B // n).int()
    feats = torch.randn(B, V, Hf * Wf, C, generator=g)
    return dict(V=V, C=C, n=n, Hf=Hf, Wf=Wf, B=B, coords=coords, points=points, meta=meta, feats=feats, seed=seed)


def _gathered(rec, dev):
    """f64 feature rows per (voxel, view) (n, V, C), zero where pix = -1, and the (n, V) mask of views with a pixel"""
    V, C, n = rec['V'], rec['C'], rec['n']
    pix = rec['pix'].to(dev).long()
    has = pix >= 0
    b = rec['coords'].to(dev)[:, 0].long()
    feats = rec['feats'].to(dev).to(F64).reshape(-1, rec['Hf'] * rec['Wf'], C)
    img = b[:, None] * V + torch.arange(V, device=dev)[None, :]
    f = feats[img, pix.clamp(min=0)]
    return f * has[:, :, None], has


def check_prefix_fwd(rec, dev, stats, cls='prefix_fwd'):
    """rec: V, C, n, Hf, Wf, coords, feats (as the launch read them), out (V n, C) f32, pix (n, V) int, cnt (V, n) int"""
    V, C, n = rec['V'], rec['C'], rec['n']
    label = f'{stats.label}: prefix fwd V={V} C={C} n={n}'
    cnt = rec['cnt'].to(dev).long().reshape(V, n)
    step = cnt - torch.cat([torch.zeros_like(cnt[:1]), cnt[:-1]])
    if not bool(((step == 0) | (step == 1)).all()):
        raise AssertionError(f'{label}: cnt does not rise by 0 or 1 from one prefix to the next')
    f, has = _gathered(rec, dev)
    S, A = f.cumsum(1), f.abs().cumsum(1)                  # (n, V, C): prefix sums over the views
    k = has.long().cumsum(1)
    c = cnt.t()                                            # (n, V)
    live = (c > 0)[:, :, None]
    den = c.clamp(min=1).to(F64)[:, :, None]
    spec = torch.where(live, S / den, torch.zeros_like(S)).permute(1, 0, 2).reshape(V * n, C)
    bnd = torch.where(live, (k[:, :, None] + 1) * A / den, torch.zeros_like(A)).permute(1, 0, 2).reshape(V * n, C)
    return _held(label, rec['out'].to(dev), spec, bnd, None, cls, stats)


def _adjoint(rec, dev):
    """f64 adjoint (B V HW, C), the same sum on absolute values, hits per pixel (linked ones: a valid view in the last prefix)"""
    V, C, n, B = rec['V'], rec['C'], rec['n'], rec.get('B', 1)
    HW = rec['Hf'] * rec['Wf']
    pix = rec['pix'].to(dev).long()
    cnt = rec['cnt'].to(dev).long().reshape(V, n)
    b = rec['coords'].to(dev)[:, 0].long()
    dout = rec['dout'].to(dev).to(F64).reshape(V, n, C)
    w = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1).to(F64), torch.zeros(1, dtype=F64, device=dev))[:, :, None]
    terms = dout * w
    suf = terms.flip(0).cumsum(0).flip(0)                  # (V, n, C): sum over t >= v
    sufa = terms.abs().flip(0).cumsum(0).flip(0)
    spec = torch.zeros(B * V * HW, C, dtype=F64, device=dev)
    A = torch.zeros_like(spec)
    H = torch.zeros(B * V * HW, dtype=torch.long, device=dev)
    linked = cnt[V - 1] > 0
    for v in range(V):
        m = (pix[:, v] >= 0) & linked
        rows = (b[m] * V + v) * HW + pix[m, v]
        spec.index_add_(0, rows, suf[v][m])
        A.index_add_(0, rows, sufa[v][m])
        H += torch.bincount(rows, minlength=B * V * HW)
    return spec, A, H


def prefix_bwd_bound(rec, dev, extra_ops=0):
    """(spec, bound in units of u, |prior| times the roundings it passes through or None) of check_prefix_bwd"""
    V, B = rec['V'], rec.get('B', 1)
    HW = rec['Hf'] * rec['Wf']
    acc = int(rec['acc'])
    spec, A, H = _adjoint(rec, dev)
    v_of = (torch.arange(B * V * HW, device=dev) // HW) % V
    D = 1 + (V - v_of) + H + acc + extra_ops
    assert int(D.max()) <= 4095, 'the first-order form of the bound needs D (D + 1) u <= 1'
    m = (D + 1).to(F64)[:, None]
    prior = None
    if acc:
        prior = rec['dfeats0'].to(dev).to(F64)
        spec = spec + prior
        prior = prior.abs() * ((V - v_of).to(F64)[:, None] if extra_ops else 1.0)
    return spec, m * A, prior


def check_prefix_bwd(rec, dev, stats, cls='prefix_bwd', extra_ops=0, key='dfeats'):
    """rec: the forward record + dout (V n, C) as read, acc, dfeats (B V HW, C) after, dfeats0 (before; needed for acc = 1)"""
    label = f'{stats.label}: prefix bwd V={rec["V"]} C={rec["C"]} n={rec["n"]} acc={rec["acc"]}'
    spec, bnd, prior = prefix_bwd_bound(rec, dev, extra_ops)
    return _held(label, rec[key].to(dev), spec, bnd, prior, cls, stats)


def coverage(rec):
    """what a case exercises (host): late first-valid view, never-valid voxels, views without a pixel and invalid views with one in
    voxels that have valid views, the busiest pixel's hit count"""
    V, n = rec['V'], rec['n']
    pix, cnt = rec['pix'].cpu().long(), rec['cnt'].cpu().long().reshape(V, n)
    valid = (cnt - torch.cat([torch.zeros_like(cnt[:1]), cnt[:-1]])).t() > 0          # (n, V)
    any_valid = cnt[V - 1] > 0
    first = torch.where(any_valid, valid.long().argmax(1), torch.full((n,), -1))
    HW = rec['Hf'] * rec['Wf']
    b = rec['coords'].cpu()[:, 0].long()
    busiest = 0
    for v in range(V):
        m = (pix[:, v] >= 0) & any_valid
        if bool(m.any()):
            busiest = max(busiest, int(torch.bincount((b[m] * V + v) * HW + pix[m, v]).max()))
    return dict(late_first=int((first > 0).sum()), never=int((~any_valid).sum()),
                no_pixel_in_live_voxel=int(((pix < 0) & any_valid[:, None]).sum()),
                invalid_with_pixel=int(((pix >= 0) & ~valid & any_valid[:, None]).sum()), busiest=busiest)
