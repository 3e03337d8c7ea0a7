"""Specification of the view-window fusion kernels (csrc/fusion.hip: es_point_sample_win_fwd, es_point_sample_win_fwd_h,
es_point_sample_win_bwd), the front of the continuous detector (embodied_det3d.py:90-207 of the reference: the T cumulative clouds are
batch entries 0 .. T-1 and entry t is fused with views 0 .. t of ONE image set).  Used by tests/test_gpu_window_fusion.py (MI355X) and
tests/test_emu_window_fusion.py (the same bodies on the CPU emulator, plus mutated records the checker must reject).
u = 2^-24; every bound is per element and none depends on 1 / |spec|.

A launch carries win (B, 2) int: sample b reads image set s_b = win[b, 0] and its first w_b = win[b, 1] views.

Forward.  (a) bit for bit the per-sample composition of es_point_sample_fwd(_h): sample b's row slice with the batch column zeroed,
V' = w_b, meta row b, the feature pointer at set s_b (the test bodies make those calls); pix[:, w_b:] = -1.  (b) check_win_fwd: on the
launch's own pix and cnt, with f(u, i) the feature row view u's pixel of row i holds (nothing where pix = -1; ALL views of the window
with a pixel are summed, valid or not: SURVEY Q3),
    out[i] = sum_{u < w_b} f(u, i) / cnt[i]      (0 where cnt[i] = 0),
  |out - spec| <= (k + 1) u sum_{u < w_b} |f(u, i)| / cnt[i], k the number of summed views: k f32 additions (the first one, into 0,
  is exact, so this is one more than needed) and one IEEE division.  bf16 feature maps widen exactly, so the bound is the same.

Backward.  check_win_bwd: the f64 adjoint of that forward.  Pixel p of view v of set s receives
    sum over the rows i with s_b = s, v < w_b, cnt[i] > 0, pix[i][v] = p of dout[i] / cnt[i].
  f32 operations a term dout[i][c] / cnt[i] passes through in k_ps_gather before it is part of the element:
    1           inv = 1 / cnt[i]                                (one IEEE division)
    1           at most: the product dout * inv (none when the compiler fuses it with the addition below)
    H           at most: the additions acc += term over the H linked hits of the pixel; the term enters at its own addition and is
                re-rounded by the later ones
    acc         one more addition into the prior when the launch accumulates (the prior itself is held to u |prior| on top)
  D = 2 + H + acc roundings, each relative u: |got - spec| <= ((1 + u)^D - 1) sum |terms| <= D u / (1 - D u) sum |terms|, and
  D u / (1 - D u) <= (D + 1) u as long as D (D + 1) u <= 1 (D <= 4095, asserted).  So m = D + 1 = H + acc + 3.
  A pixel nothing hits holds an exact zero (its prior bit for bit when accumulating): its bound is 0.

Worst ratios observed, |err| / (bound / G) against G = 8 (MI355X and CPU emulator, the same grids; the figures coincide):
  win_fwd 3.66 (grid) / 4.32 (cluster cases)   win_bwd 4.13 (grid) / 3.39 (cluster cases)"""
import torch

import prefix_spec as PS
from fwd_spec import F64, G, U, Stats, bound_check  # noqa: F401

__all__ = ['Stats', 'U', 'VS', 'windows', 'make_case', 'check_win_fwd', 'check_win_bwd', 'win_bwd_bound', 'coverage']

VS = 0.05                       # voxel size of the cases: the points of prefix_spec.make_case (+-2 m) land on +-40 voxels
NOPS, OPS, ROTINV, PROJ = PS.NOPS, PS.OPS, PS.ROTINV, PS.PROJ


def windows(kind, B, V, n_sets=1):
    """(B, 2) int32 table: 'one' (every sample sees view 0), 'full' (all V), 'asc' (sample b sees b + 1 views: the detector's table),
    'arb' (a non-monotone table); sample b reads set b mod n_sets"""
    w = {'one': [1] * B, 'full': [V] * B, 'asc': [min(b + 1, V) for b in range(B)],
         'arb': [((5 * b + 2) * 7) % V + 1 for b in range(B)]}[kind]
    return torch.tensor([[b % n_sets, w[b]] for b in range(B)], dtype=torch.int32)


def make_case(V, C, n, Hf, Wf, aug, seed, B=1, kind='full', n_sets=1, blind=0, cluster=0, empty=None):
    """host tensors of one launch on prefix_spec.make_case's cameras and points: coords (n, 4) int32 (column 0: the sample, ascending;
    sample `empty` owns no row; columns 1..3: the point / VS rounded), meta (B, stride), feats (n_sets, V, Hf Wf, C) f32, win (B, 2)"""
    base = PS.make_case(V, C, n, Hf, Wf, aug, seed, B=B, blind=blind, cluster=cluster)
    g = torch.Generator().manual_seed(seed + 77)
    coords = torch.zeros(n, 4, dtype=torch.int32)
    coords[:, 1:] = torch.round(base['points'] / VS).int()
    live = torch.tensor([b for b in range(B) if b != empty], dtype=torch.int32)
    coords[:, 0] = live[torch.arange(n) * len(live) // n]
    feats = torch.randn(n_sets, V, Hf * Wf, C, generator=g)
    return dict(V=V, C=C, n=n, Hf=Hf, Wf=Wf, B=B, n_sets=n_sets, coords=coords, meta=base['meta'], feats=feats,
                win=windows(kind, B, V, n_sets), seed=seed, kind=kind)


def _held(label, got, spec, bound_u, prior, cls, stats):
    """|got - spec| <= u bound_u + u |prior|; the printed ratio is |err| / (bound / G): G = 8 means nothing to spare"""
    return bound_check(label, got, spec, U * bound_u / G, prior if prior is not None else torch.zeros_like(spec), False, cls, stats)


def _rows(rec, dev):
    """per row: image set, window length; the (n, V) mask `view inside the row's window`"""
    win = rec['win'].to(dev).long()
    b = rec['coords'].to(dev)[:, 0].long()
    s, w = win[b, 0], win[b, 1]
    return s, w, torch.arange(rec['V'], device=dev)[None, :] < w[:, None]


def check_win_fwd(rec, dev, stats, cls='win_fwd'):
    """rec: V, C, n, Hf, Wf, coords, win, feats (as the launch read them, f32 or bf16), out (n, C) f32, pix (n, V) int, cnt (n) int"""
    V, C, n = rec['V'], rec['C'], rec['n']
    label = f'{stats.label}: window fwd V={V} C={C} n={n}'
    s, w, inside = _rows(rec, dev)
    pix = rec['pix'].to(dev).long()
    cnt = rec['cnt'].to(dev).long()
    if not bool((pix[~inside] == -1).all()):
        raise AssertionError(f'{label}: a pix entry beyond its window is not -1')
    has = (pix >= 0) & inside
    if not bool((cnt <= has.sum(1)).all() and (cnt >= 0).all()):
        raise AssertionError(f'{label}: cnt exceeds the number of views with a pixel inside the window')
    feats = rec['feats'].to(dev).to(F64).reshape(-1, rec['Hf'] * rec['Wf'], C)
    img = s[:, None] * V + torch.arange(V, device=dev)[None, :]
    f = feats[img, pix.clamp(min=0)] * has[:, :, None]
    S, A, k = f.sum(1), f.abs().sum(1), has.sum(1)
    live = (cnt > 0)[:, None]
    den = cnt.clamp(min=1).to(F64)[:, None]
    spec = torch.where(live, S / den, torch.zeros_like(S))
    bnd = torch.where(live, (k[:, None] + 1) * A / den, torch.zeros_like(A))
    return _held(label, rec['out'].to(dev), spec, bnd, None, cls, stats)


def _adjoint(rec, dev):
    """f64 adjoint (n_sets V HW, C), the same sum on absolute values, linked hits per pixel"""
    V, C = rec['V'], rec['C']
    HW = rec['Hf'] * rec['Wf']
    n_pix = rec['n_sets'] * V * HW
    s, w, inside = _rows(rec, dev)
    pix = rec['pix'].to(dev).long()
    cnt = rec['cnt'].to(dev).long()
    dout = rec['dout'].to(dev).to(F64)
    terms = torch.where((cnt > 0)[:, None], dout / cnt.clamp(min=1).to(F64)[:, None], torch.zeros_like(dout))
    spec = torch.zeros(n_pix, C, dtype=F64, device=dev)
    A = torch.zeros_like(spec)
    H = torch.zeros(n_pix, dtype=torch.long, device=dev)
    for v in range(V):
        m = (pix[:, v] >= 0) & (cnt > 0) & inside[:, v]
        rows = (s[m] * V + v) * HW + pix[m, v]
        spec.index_add_(0, rows, terms[m])
        A.index_add_(0, rows, terms[m].abs())
        H += torch.bincount(rows, minlength=n_pix)
    return spec, A, H


def win_bwd_bound(rec, dev):
    """(spec, bound in units of u, |prior| or None, hits per pixel) of check_win_bwd"""
    acc = int(rec['acc'])
    spec, A, H = _adjoint(rec, dev)
    D = 2 + H + acc
    assert int(D.max()) <= 4095, 'the first-order form of the bound needs D (D + 1) u <= 1'
    prior = None
    if acc:
        prior = rec['dfeats0'].to(dev).to(F64)
        spec = spec + prior
        prior = prior.abs()
    return spec, (D + 1).to(F64)[:, None] * A, prior, H


def check_win_bwd(rec, dev, stats, cls='win_bwd', key='dfeats'):
    """rec: the forward record + dout (n, C) as read, acc, dfeats (n_sets V HW, C) after, dfeats0 (before; needed for acc = 1)"""
    label = f'{stats.label}: window bwd V={rec["V"]} C={rec["C"]} n={rec["n"]} acc={rec["acc"]}'
    spec, bnd, prior, _ = win_bwd_bound(rec, dev)
    return _held(label, rec[key].to(dev), spec, bnd, prior, cls, stats)


def coverage(rec, cnt_full=None):
    """what a case exercises, from the YARDSTICK's outputs (rec['pix'] (n, V) with -1 beyond the window, rec['cnt'] (n); cnt_full (n):
    the yardstick's count with all V views): workgroups of 16 rows that hold two samples with different windows, rows valid only beyond
    their window, rows with cnt = 0 inside a window of >= 2 views, views inside the window with a pixel but no valid flag"""
    n = rec['n']
    win = rec['win'].cpu().long()
    b = rec['coords'].cpu()[:, 0].long()
    w = win[b, 1]
    pix, cnt = rec['pix'].cpu().long(), rec['cnt'].cpu().long()
    straddle = 0
    for i0 in range(0, n, 16):
        i1 = min(n, i0 + 16) - 1
        straddle += int(b[i0] != b[i1] and not torch.equal(win[b[i0]], win[b[i1]]))
    beyond = 0 if cnt_full is None else int(((cnt == 0) & (cnt_full.cpu().long() > 0)).sum())
    return dict(straddle=straddle, beyond=beyond, dead_in_wide_window=int(((cnt == 0) & (w >= 2)).sum()),
                invalid_with_pixel=int(((pix >= 0).sum(1) > cnt).sum()))
