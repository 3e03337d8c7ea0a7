"""Specifications of the grounding kernels (csrc/transformer.hip, csrc/ground.hip) beyond the forwards tests/fwd_spec.py already holds
(check_attention, check_layernorm, check_contrastive): attention backward, LayerNorm backward, ContrastiveEmbed backward, the two box
coders, the focal loss, the assignment and the sorted top-k, evaluated in f64 on the operands each launch actually received -- the
STORED O / lse / mean / rstd, what an accumulating output held before the launch.  Used by tests/test_gpu_ground_kernels.py (MI355X)
and tests/test_emu_ground_kernels.py (the same bodies on the CPU emulator, plus mutated outputs the checker must reject).
u = 2^-24, G = 8 (fwd_spec); every bound is per element and none depends on 1 / |spec|.

Attention backward (r = RNE to bf16 in bf16 mode, identity in f32 mode; h = 2^-8 / 0; s = 1 / sqrt(32) as f32):
  qs = r(f32(q s))  kr = r(k)  vr = r(v)  gr = r(dO)       S = qs kr^T       P = exp(S - lse_stored) on live keys, 0 elsewhere
  delta = sum_d dO O (stored O)     dP = gr vr^T     dS = P (dP - delta)     dV = P^T gr     dK = dS^T qs     dQ = s dS kr
  eS = G u sqrt(32) |qs| |kr|^T     eP = eS + 4 u (1 + |S - lse|)   (relative error of P: the score GEMM and the fast exponential)
  eDP = G u sqrt(32) |gr| |vr|^T    eDel = G u sqrt(32) sum |dO O|
  E = P [(h + eP) |dP - delta| + eDP + eDel]                        (absolute error of the rounded dS)
  |dV - spec| <= sum_q (h + eP) P |gr| + G u sqrt(Lq) sum_q P |gr| + u |prior|
  |dK - spec| <= sum_q E |qs| + G u sqrt(Lq) sum_q |dS| |qs| + u |prior|
  |dQ - spec| <= s (sum_k E |kr| + G u sqrt(Lk) sum_k |dS| |kr|) + u |dQ| + u |prior|
  Padded keys (k >= klen[b]): exact zeros in dK / dV (accumulate = 0), the prior bit for bit (accumulate = 1).  A sample without a
  valid key (klen[b] <= 0) has O = 0, lse = -inf and zero gradients (the reference yields NaN there: DESIGN.md).
  h stands for the RNE rounding of P and of dS to bf16 as MFMA operands: bf16 carries 8 significant bits, so half an ulp is 2^-8
  relative (with 2^-9 the f32 evaluation of the formula itself, attn_ref, misses the dQ bound where the dS roundings of a row align).
  The printed ratio of these classes is |err| / (bound / G): 8 means the bound is met with nothing to spare.
LayerNorm backward: xh = (z - mean) rstd on the saved statistics, g = dy w, dz = rstd (g - mean_c g - xh mean_c(g xh))
  dz: rstd [8 u (|g| + |mean_c g| + |xh mean_c(g xh)|) + G u sqrt(C) / C (sum |g| + |xh| sum |g xh|)] + u |prior|
  dw: (G sqrt(n) + 3) u sum_rows |dy xh| + u |prior|          db: G u sqrt(n) sum |dy| + u |prior|
ContrastiveEmbed backward (tl = min(tlen[b], T, Tout) live tokens; dlogits is 0 at masked positions by contract):
  dv: (G sqrt(T) + 2) u sum_t |dl| |text| / sqrt(C) + u |prior|     dtext: (G sqrt(L) + 2) u sum_i |dl| |v| / sqrt(C) + u |prior|
  dbias: G u sqrt(B L T) sum |dl| + u |prior|;  text rows t >= tl keep their prior bit for bit.
Box coders (lo = f32(2e-2)): expf is held to 4 u relative; an element whose exp lies within 4 u of lo may take either side of the
  clamp (the kernel decides on its f32 expf).  The two coders differ only where that f32 expf EQUALS lo (baseline: gradient for
  exp > lo, FCAF: for exp >= lo); no output of either coder tells expf == lo from expf < lo, and the f64 exp cannot say which the
  device's expf returned, so that one point is not distinguished here: the nearest rows the tests hold to ONE side sit 2 ulps of the
  argument (8 u of exp) below and above log(lo).
  baseline forward: centre p + point (u (|p| + |point|)), size max(exp p, lo) (4 u), angles exact
  baseline backward: centre / angle gradients exact, size gradient [exp > lo] g exp within 6 u (expf 4 u, the product, u spare)
  FCAF forward: d = max(exp p, lo), shift = ((d1 - d0) / 2, ..), centre = point + R shift, size = d0 + d1 (6 u).  R's entries are
    sums of products of up to three f32 sines / cosines (each within 4 u absolute of the f64 value at |angle| <= 8): the centre is
    held to 32 u (|point| + sum_j Rabs[c, j] (d_2j + d_2j+1) / 2) with Rabs the same sums on absolute values (3 x 4 u for the
    factors, 3 for their products and the sum, 4 for d, 5 for the subtraction, the scaling, the two additions; 8 spare).
  FCAF backward: distances [exp >= lo] (-/+ gs_c / 2 + g_3+c) exp with gs = R^T g_centre: 32 u (Rabs^T |g| / 2 + |g_3+c|) exp;
    angles g_6+k + d<g, R shift>/d angle_k: 64 u sum_c |g_c| sum_j |shift_j| + u |g_6+k| (every entry of dR / d angle is a sum of at
    most two products of sines and cosines: its absolute terms sum to <= 2).  (+ u |prior| when accumulating)
Focal loss: x the logit, y the label, p = sigmoid(x), pt = y ? 1 - p : p, wa = y ? alpha : 1 - alpha, fw = wa pt^gamma,
  bce = max(x, 0) - x y + log1p(exp(-|x|)), dfw = wa gamma pt^(gamma - 1) (y ? -1 : 1) p (1 - p), c = grad_scale / (avg + eps32)
  dlogits = ((p - y) fw + bce dfw) c  within  [16 u (|(p - y) fw| + |bce dfw|) + |p - y| e_fw + [y] fw e + bce e_dfw] c.  The f32
  `1 - p` carries an ABSOLUTE error e = 5 u p (p itself is good to 4 u relative, and p -> 1 cancels), whatever 1 - p is; it moves
  pt and p - y (for y = 1) and p (1 - p) (always): e_pt = [y] e, e_fw = wa (gamma pt^(gamma-1) e_pt + e_pt^2),
  e_dfw = wa gamma ((gamma - 1) pt^(gamma-2) e_pt p (1 - p) + pt^(gamma-1) p e).  The 16 u covers expf / log1pf / powf (4 u each)
  and the products.
  A gradient below the smallest normal f32 is subnormal or flushed, and so is an intermediate product such as (p - y) fw at
  |x| = 30: an absolute 2^-126 (1 + c) on top.
  Exact zero for t >= tlen[b], columns T .. Tout included.  loss_sum: G u sqrt(n) sum |term| (f32 terms, f64 sum).
Assignment: lsa_port() is scipy's shortest-augmenting-path solver (rectangular_lsap.cpp) line by line, its tie rule and column
  order included; lsa_port_np() the same with the column scan vectorised (Q = 1024 in reasonable time).  The kernel is held to the
  port on its OWN f64 cost output; independently the total cost equals scipy's to 1e-9 relative and every box is matched exactly once
  to distinct queries.
Top-k: torch.argsort(vals[:n], descending=True, stable=True)[:k], -1 beyond n.

Worst ratios observed, |err| / (bound / G) against G = 8 (MI355X on the full grid / CPU emulator on the reduced grid):
  attn_bwd bf16  dq 7.47 / 7.20   dk 7.74 / 7.38   dv 7.89 / 7.62      attn_bwd f32  dq 0.48 / 0.31   dk 0.75 / 0.30   dv 2.13 / 1.20
    (bf16: Lq = 1 or Lk = 1 and peaked rows leave ONE product in a sum; a single RNE rounding then uses up to all of h, which is
    a strict bound -- half a bf16 ulp -- so these ratios approach 8 and cannot pass it)
  layernorm_bwd  dz 1.13 / 1.01   dw 1.86 / 1.69   db 1.24 / 1.01      contrastive_bwd  dv 1.11 / 1.01   dtext 0.69 / 1.45   dbias 0.01 / 0.02
  decode_fwd  centre 7.91 / 7.91   size 2.46 / 1.88      decode_bwd  size 2.77 / 2.77   pass-through 7.96 / 7.96
    (centre / pass-through: one IEEE addition held to u (|a| + |b|): again a strict bound that single elements nearly reach)
  fcaf_fwd  centre 0.46 / 0.45   size 2.21 / 2.19      fcaf_bwd  distances 0.66 / 0.68   angles 1.12 / 1.12
  focal  dlogits 3.01 / 3.02   loss_sum 0.00 / 0.00
  forwards (fwd_spec's classes, ratio of their G term only): attention o / lse 0.00, layernorm 0.00, contrastive 0.11 / 0.05
  assignment, top-k: exact; box IoU: 6.0e-8 from the closed form, quarter turns 3.2e-8 from qhull and 2.8e-8 from the oracle on the f32 boxes, 1.8e-8 generic"""
import math

import numpy as np
import torch

from fwd_spec import F64, G, U, Stats, _r, bound_check, check_attention, check_contrastive, check_layernorm  # noqa: F401

__all__ = ['Stats', 'check_attention', 'check_layernorm', 'check_contrastive', 'attn_ref', 'check_attn_bwd', 'ln_bwd_ref',
           'check_layernorm_bwd', 'contrastive_bwd_ref', 'check_contrastive_bwd', 'check_decode_fwd', 'check_decode_bwd',
           'check_decode_fcaf_fwd', 'check_decode_fcaf_bwd', 'check_focal', 'lsa_port', 'lsa_port_np', 'check_assignment', 'check_topk',
           'aligned_iou']

S32 = float(torch.tensor(0.17677669529663687, dtype=torch.float32))     # the kernels' scale, as the f32 they multiply by
H_BF = 2.0 ** -8            # unit roundoff of bf16 (8 significant bits)
LO = float(torch.tensor(2e-2, dtype=torch.float32))
EPS32 = 1.1920929e-07


def _d(t, dev=None):
    return None if t is None else (t.to(dev) if dev is not None else t).to(F64)


def _held(label, got, spec, bound_u, prior, cls, stats, diagnose=None):
    """|got - spec| <= u bound_u + u |prior|, reported like every class of this module: the printed ratio is |err| / (bound / G), so G = 8
    means the bound is met with nothing to spare"""
    return bound_check(label, got, spec, U * bound_u / G, prior if prior is not None else torch.zeros_like(spec), False, cls, stats, diagnose)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _heads(t, B, L, H, dev=None):
    """(B L, H 32) rows -> (B, H, L, 32)"""
    t = t.to(dev) if dev is not None else t
    return t.reshape(B, L, H, 32).permute(0, 2, 1, 3)


def _rows(t, B, L, H):
    """(B, H, L, 32) -> (B L, H 32)"""
    return t.permute(0, 2, 1, 3).reshape(B * L, H * 32)


def _live(klen, B, Lk, dev):
    kl = torch.full((B,), Lk, dtype=torch.long, device=dev) if klen is None else klen.to(dev).long().clamp(min=0, max=Lk)
    return kl, (torch.arange(Lk, device=dev)[None, :] < kl[:, None])[:, None, None, :]


# ------------------------------------------------------------------------------------------------------------------ attention
def attn_ref(q, k, v, do, klen, B, H, Lq, Lk, bf, mutate=None, o=None, lse=None):
    """An f32 torch evaluation of the specification's own formula with the kernels' roundings (operands, P and dS rounded to bf16 in
    bf16 mode), on CPU tensors: forward (o, lse) unless given, then dq, dk, dv.  It must pass check_attention / check_attn_bwd by
    itself (the model is then not tighter than f32 arithmetic) and, with `mutate`, produces the wrong outputs the checker must reject:
      'dk_skip_qstep'  dK without the 32-query step 32 .. 63          'delta_other_o'  delta taken from the O of the next query row
      'dq_no_scale'    dQ without the final scale                     'pad_leak'       the first padded key of sample 0 given probability
    returns dict(o, lse (B, H, Lq), dq, dk, dv) of f32 tensors in the kernels' (B L, H 32) layout"""
    r32 = (lambda t: t.to(torch.bfloat16).float()) if bf else (lambda t: t)
    s = torch.tensor(S32, dtype=torch.float32)
    qs = r32(_heads(q.float(), B, Lq, H) * s)
    kr, vr, gr = r32(_heads(k.float(), B, Lk, H)), r32(_heads(v.float(), B, Lk, H)), r32(_heads(do.float(), B, Lq, H))
    kl, live = _live(klen, B, Lk, q.device)
    S = qs @ kr.transpose(-1, -2)
    Sm = S.masked_fill(~live, -math.inf)
    if o is None:
        m = Sm.amax(-1, keepdim=True)
        m0 = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        p = torch.where(live, torch.exp(S - m0), torch.zeros_like(S))
        l = p.sum(-1, keepdim=True)
        any_key = l > 0
        oh = torch.where(any_key, (r32(p) @ vr) / torch.where(any_key, l, torch.ones_like(l)), torch.zeros(1))
        lse = torch.where(any_key[..., 0], m0[..., 0] + torch.log(torch.where(any_key, l, torch.ones_like(l)))[..., 0],
                          torch.full_like(l[..., 0], -math.inf))
        o = _rows(oh, B, Lq, H).contiguous()
    oh = _heads(o.float(), B, Lq, H)
    lse = lse.reshape(B, H, Lq).float()
    liveP = live.expand(B, H, Lq, Lk).clone()
    if mutate == 'pad_leak':
        assert int(kl[0]) < Lk
        liveP[0, :, :, int(kl[0])] = True
    x = torch.where(liveP, S - lse[..., None], torch.zeros_like(S))
    P = torch.where(liveP, torch.exp(x), torch.zeros_like(S))
    oh_d = oh.roll(1, 2) if mutate == 'delta_other_o' else oh
    delta = (_heads(do.float(), B, Lq, H) * oh_d).sum(-1, keepdim=True)
    dP = gr @ vr.transpose(-1, -2)
    dS = P * (dP - delta)
    dv = r32(P).transpose(-1, -2) @ gr
    dSk = dS.clone()
    if mutate == 'dk_skip_qstep':
        assert Lq > 32
        dSk[:, :, 32:64] = 0
    dk = r32(dSk).transpose(-1, -2) @ qs
    dq = r32(dS) @ kr
    if mutate != 'dq_no_scale':
        dq = dq * s
    return dict(o=o, lse=lse.contiguous(), dq=_rows(dq, B, Lq, H).contiguous(), dk=_rows(dk, B, Lk, H).contiguous(),
                dv=_rows(dv, B, Lk, H).contiguous())


def check_attn_bwd(rec, dev, stats, cls='attn_bwd'):
    """rec: B, H, Lq, Lk, bf, q, k, v, o, do ((B L, H 32) f32 as the launch read them), lse (B H Lq, stored), klen (int tensor or
    None), acc, dq / dk / dv (after), dq0 / dk0 / dv0 (before; needed for acc = 1)"""
    B, H, Lq, Lk, bf, acc = rec['B'], rec['H'], rec['Lq'], rec['Lk'], rec['bf'], rec['acc']
    rr = _r if bf else (lambda t: t.to(F64))
    h = H_BF if bf else 0.0
    s32 = torch.tensor(S32, dtype=torch.float32, device=dev)
    qs = rr(_heads(rec['q'], B, Lq, H, dev).float() * s32)
    kr, vr, gr = rr(_heads(rec['k'], B, Lk, H, dev)), rr(_heads(rec['v'], B, Lk, H, dev)), rr(_heads(rec['do'], B, Lq, H, dev))
    do, o = _d(_heads(rec['do'], B, Lq, H, dev)), _d(_heads(rec['o'], B, Lq, H, dev))
    lse = _d(rec['lse'], dev).reshape(B, H, Lq)
    kl, live = _live(rec['klen'], B, Lk, dev)
    label = f'{stats.label}: attention bwd B={B} H={H} Lq={Lq} Lk={Lk} bf16={bf} klen={kl.tolist()} acc={acc}'
    S = qs @ kr.transpose(-1, -2)
    x = torch.where(live, S - lse[..., None], torch.zeros_like(S))        # (a sample without keys: lse = -inf, nothing live)
    P = torch.where(live, torch.exp(x), torch.zeros_like(S))
    delta = (do * o).sum(-1, keepdim=True)
    dP = gr @ vr.transpose(-1, -2)
    dS = P * (dP - delta)
    dV, dK, dQ = P.transpose(-1, -2) @ gr, dS.transpose(-1, -2) @ qs, S32 * (dS @ kr)
    r32 = math.sqrt(32.0)
    eS = G * U * r32 * (qs.abs() @ kr.abs().transpose(-1, -2))
    eP = eS + 4 * U * (1 + x.abs())
    eDP = G * U * r32 * (gr.abs() @ vr.abs().transpose(-1, -2))
    eDel = G * U * r32 * (do * o).abs().sum(-1, keepdim=True)
    E = P * ((h + eP) * (dP - delta).abs() + eDP + eDel)
    bV = ((h + eP) * P).transpose(-1, -2) @ gr.abs() + G * U * math.sqrt(Lq) * (P.transpose(-1, -2) @ gr.abs())
    bK = E.transpose(-1, -2) @ qs.abs() + G * U * math.sqrt(Lq) * (dS.abs().transpose(-1, -2) @ qs.abs())
    bQ = S32 * (E @ kr.abs() + G * U * math.sqrt(Lk) * (dS.abs() @ kr.abs()))
    padrow = (torch.arange(Lk, device=dev)[None, :] >= kl[:, None]).reshape(B * Lk)          # rows of dK / dV that belong to padded keys
    out = {}
    for name, spec, bnd, L in (('dq', dQ, bQ, Lq), ('dk', dK, bK, Lk), ('dv', dV, bV, Lk)):
        got = rec[name].to(dev)
        spec, bnd = _rows(spec, B, L, H), _rows(bnd, B, L, H)
        extra = spec.abs() if name == 'dq' else torch.zeros_like(spec)
        prior = None
        if acc:
            prior = rec[name + '0'].to(dev)
            spec, extra = spec + prior.to(F64), extra + prior.to(F64).abs()
        if name != 'dq' and bool(padrow.any()):
            want = prior[padrow] if acc else torch.zeros_like(got[padrow])
            if not (_bits_equal(got[padrow], want) if acc else bool((got[padrow] == 0).all())):
                raise AssertionError(f'{label}: {name} of a padded key is not ' + ('its prior bit for bit' if acc else 'an exact zero'))
        if bool((kl == 0).any()):
            dead = (kl == 0).repeat_interleave(L)
            want = prior[dead] if acc else torch.zeros_like(got[dead])
            if not torch.equal(got[dead], want):
                raise AssertionError(f'{label}: {name} of a sample without a valid key is not ' + ('its prior' if acc else 'zero'))
        out[name] = bound_check(f'{label} {name}', got, spec, bnd / G, extra, False, f'{cls} {name} {"bf16" if bf else "f32"}', stats)
    return out


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
def ln_bwd_ref(dy, z, w, mean, rstd, skip_rows=None):
    """f32 torch evaluation (CPU): dz, dw, db; skip_rows = (a, b): dw / db without the rows a .. b (one workgroup's partial)"""
    xh = (z - mean[:, None]) * rstd[:, None]
    g = dy * w[None]
    dz = rstd[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    keep = torch.ones(z.shape[0], dtype=torch.bool)
    if skip_rows is not None:
        keep[skip_rows[0]:skip_rows[1]] = False
    return dz, (dy * xh)[keep].sum(0), dy[keep].sum(0)


def check_layernorm_bwd(rec, dev, stats, cls='layernorm_bwd'):
    """rec: dy, z (n, C), w, mean, rstd (as saved), dz (after), dz0 (prior or None), dw0 / dw1, db0 / db1 (None: not written)"""
    dy, z = _d(rec['dy'], dev), _d(rec['z'], dev)
    n, C = z.shape
    w, mean, rstd = _d(rec['w'], dev)[None], _d(rec['mean'], dev)[:, None], _d(rec['rstd'], dev)[:, None]
    label = f'{stats.label}: layernorm bwd rows {n} C={C}'
    xh = (z - mean) * rstd
    g = dy * w
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    spec = rstd * (g - m1 - xh * m2)
    bnd = G * rstd * math.sqrt(C) / C * (g.abs().sum(1, keepdim=True) + xh.abs() * (g * xh).abs().sum(1, keepdim=True))
    bnd = bnd + 8 * rstd * (g.abs() + m1.abs() + (xh * m2).abs())
    prior = None
    if rec.get('dz0') is not None:
        p = _d(rec['dz0'], dev)
        spec, prior = spec + p, p.abs()
    _held(label + ' dz', rec['dz'].to(dev), spec, bnd, prior, f'{cls} dz', stats,
          [('the xh mean(g xh) term dropped', spec + rstd * xh * m2), ('the mean(g) term dropped', spec + rstd * m1)])
    if rec.get('dw1') is not None:
        A = (dy * xh).abs().sum(0)
        p = _d(rec['dw0'], dev)
        _held(label + ' dw', rec['dw1'].to(dev), p + (dy * xh).sum(0), (G * math.sqrt(n) + 3) * A, p.abs(), f'{cls} dw', stats)
    if rec.get('db1') is not None:
        p = _d(rec['db0'], dev)
        _held(label + ' db', rec['db1'].to(dev), p + dy.sum(0), G * math.sqrt(n) * dy.abs().sum(0), p.abs(), f'{cls} db', stats)


# ------------------------------------------------------------------------------------------------------------------ ContrastiveEmbed
def contrastive_bwd_ref(dl, v, text, tlen, B, L, T, C, Tout, drop_row=None):
    """f32 torch evaluation (CPU): dv (B, L, C), dtext increment (B, T, C), dbias increment; drop_row = (b, i): dtext without that
    visual row"""
    tl = tlen.long().clamp(min=0, max=min(T, Tout))
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(C), dtype=torch.float32))
    d = torch.zeros(B, L, T)
    m = min(T, Tout)
    d[:, :, :m] = dl.view(B, L, Tout)[:, :, :m]
    d = d * (torch.arange(T)[None, None, :] < tl[:, None, None])
    dv = (d * inv) @ text.view(B, T, C)
    d2 = d.clone()
    if drop_row is not None:
        d2[drop_row[0], drop_row[1]] = 0
    return dv, (d2 * inv).transpose(1, 2) @ v.view(B, L, C), d.sum()


def check_contrastive_bwd(rec, dev, stats, cls='contrastive_bwd'):
    """rec: B, L, T, C, Tout, dl (B L Tout), v, text, tlen, dv (after or None), dv0 (prior or None: acc_v = 0), dtext0 / dtext1 (or
    None), dbias0 / dbias1 (or None)"""
    B, L, T, C, Tout = rec['B'], rec['L'], rec['T'], rec['C'], rec['Tout']
    label = f'{stats.label}: contrastive bwd B={B} L={L} T={T} C={C} Tout={Tout}'
    tl = rec['tlen'].to(dev).long().clamp(min=0, max=min(T, Tout))
    m = min(T, Tout)
    d = torch.zeros(B, L, T, dtype=F64, device=dev)
    d[:, :, :m] = _d(rec['dl'], dev).view(B, L, Tout)[:, :, :m]
    tok = torch.arange(T, device=dev)[None, :] < tl[:, None]                 # (B, T)
    d = d * tok[:, None, :]
    v, text = _d(rec['v'], dev).view(B, L, C), _d(rec['text'], dev).view(B, T, C)
    inv = 1.0 / math.sqrt(C)
    if rec.get('dv') is not None:
        spec, A = (d @ text) * inv, (d.abs() @ text.abs()) * inv
        prior = None
        if rec.get('dv0') is not None:
            p = _d(rec['dv0'], dev).view(B, L, C)
            spec, prior = spec + p, p.abs()
        _held(label + ' dv', rec['dv'].to(dev).view(B, L, C), spec, (G * math.sqrt(T) + 2) * A, prior, f'{cls} dv', stats)
    if rec.get('dtext1') is not None:
        p = _d(rec['dtext0'], dev).view(B, T, C)
        spec, A = p + (d.transpose(1, 2) @ v) * inv, (d.abs().transpose(1, 2) @ v.abs()) * inv
        got = rec['dtext1'].to(dev).view(B, T, C)
        if not _bits_equal(got[~tok], rec['dtext0'].to(dev).view(B, T, C)[~tok]):
            raise AssertionError(f'{label}: a text row beyond min(tlen, T, Tout) was written')
        _held(label + ' dtext', got, spec, (G * math.sqrt(L) + 2) * A, p.abs(), f'{cls} dtext', stats)
    if rec.get('dbias1') is not None:
        p = _d(rec['dbias0'], dev).reshape(1)
        _held(label + ' dbias', rec['dbias1'].to(dev).reshape(1), p + d.sum().reshape(1), G * math.sqrt(B * L * T) * d.abs().sum().reshape(1),
              p.abs(), f'{cls} dbias', stats)


# ------------------------------------------------------------------------------------------------------------------ box coders
def _either(label, got, spec_a, spec_b, amb, lin, extra, cls, stats):
    """_held (bound lin, prior extra) against spec_a; where `amb`, spec_b is accepted as well"""
    g = got.to(F64)
    use_b = amb & ((g - spec_b).abs() < (g - spec_a).abs())
    return _held(label, got, torch.where(use_b, spec_b, spec_a), lin, extra, cls, stats)


def _clamp_sides(t):
    """exp(t) in f64, which elements pass the clamp strictly (> lo), inclusively (>= lo), and which lie within 4 u of lo"""
    e = torch.exp(t)
    return e, e > LO, e >= LO, (e / LO - 1).abs() <= 4 * U


def check_decode_fwd(label, pred, pts, box, stats):
    """pred (n, 9) as read, pts (n, 3), box (n, 9)"""
    p, q = pred.to(F64), pts.to(F64)
    _held(label + ' decode centre', box[:, :3], p[:, :3] + q, p[:, :3].abs() + q.abs(), None, 'decode_fwd centre', stats)
    e, _, _, _ = _clamp_sides(p[:, 3:6])
    spec = e.clamp(min=LO)
    _held(label + ' decode size', box[:, 3:6], spec, 4 * spec, None, 'decode_fwd size', stats)
    if not torch.equal(box[:, 6:], pred[:, 6:9]):
        raise AssertionError(f'{label}: decoded angles are not the regression outputs')


def check_decode_bwd(label, pred, dbox, dpred, prior, stats):
    """baseline coder: gradient passes where exp > lo"""
    p, g = pred.to(F64), dbox.to(F64)
    e, gt, _, amb = _clamp_sides(p[:, 3:6])
    on, off = g[:, 3:6] * e, torch.zeros_like(e)
    a, b = torch.where(gt, on, off), torch.where(gt, off, on)
    pr = prior.to(F64) if prior is not None else torch.zeros_like(p)
    _either(label + ' decode bwd size', dpred[:, 3:6], a + pr[:, 3:6], b + pr[:, 3:6], amb, 6 * on.abs(), pr[:, 3:6].abs(), 'decode_bwd size', stats)
    for sl in (slice(0, 3), slice(6, 9)):
        want = g[:, sl] + pr[:, sl]
        _held(label + ' decode bwd centre / angles', dpred[:, sl], want, (g[:, sl].abs() + pr[:, sl].abs()) * (prior is not None), None,
              'decode_bwd pass-through', stats)


def _fcaf_rot(ang):
    """R = Rz(a) Rx(b) Ry(c) in f64 as (n, 3, 3) [row, column], the same sums on absolute values, and dR / d(a, b, c)"""
    a, b, c = ang[:, 0], ang[:, 1], ang[:, 2]
    sa, ca, sb, cb, sc, cc = torch.sin(a), torch.cos(a), torch.sin(b), torch.cos(b), torch.sin(c), torch.cos(c)
    R = torch.stack([torch.stack([ca * cc - sa * sb * sc, -(sa * cb), ca * sc + sa * sb * cc], -1),
                     torch.stack([sa * cc + ca * sb * sc, ca * cb, sa * sc - ca * sb * cc], -1),
                     torch.stack([-(cb * sc), sb, cb * cc], -1)], 1)
    ab = torch.abs
    Rabs = torch.stack([torch.stack([ab(ca * cc) + ab(sa * sb * sc), ab(sa * cb), ab(ca * sc) + ab(sa * sb * cc)], -1),
                        torch.stack([ab(sa * cc) + ab(ca * sb * sc), ab(ca * cb), ab(sa * sc) + ab(ca * sb * cc)], -1),
                        torch.stack([ab(cb * sc), ab(sb), ab(cb * cc)], -1)], 1)
    dRa = torch.stack([-R[:, 1], R[:, 0], torch.zeros_like(R[:, 0])], 1)
    dRb = torch.stack([torch.stack([-(sa * cb * sc), sa * sb, sa * cb * cc], -1),
                       torch.stack([ca * cb * sc, -(ca * sb), -(ca * cb * cc)], -1),
                       torch.stack([sb * sc, cb, -(sb * cc)], -1)], 1)
    dRc = torch.stack([-R[:, :, 2], torch.zeros_like(R[:, :, 0]), R[:, :, 0]], -1)      # d/dc of column 0 = -column 2, of column 2 = column 0
    return R, Rabs, (dRa, dRb, dRc)


def check_decode_fcaf_fwd(label, pred, pts, box, stats):
    p, q = pred.to(F64), pts.to(F64)
    e, _, _, _ = _clamp_sides(p[:, :6])
    d = e.clamp(min=LO)
    sh = torch.stack([(d[:, 1] - d[:, 0]) / 2, (d[:, 3] - d[:, 2]) / 2, (d[:, 5] - d[:, 4]) / 2], -1)
    sha = torch.stack([(d[:, 1] + d[:, 0]) / 2, (d[:, 3] + d[:, 2]) / 2, (d[:, 5] + d[:, 4]) / 2], -1)
    R, Rabs, _ = _fcaf_rot(p[:, 6:9])
    spec = q + (R @ sh[:, :, None])[:, :, 0]
    _held(label + ' fcaf centre', box[:, :3], spec, 32 * (q.abs() + (Rabs @ sha[:, :, None])[:, :, 0]), None, 'fcaf_fwd centre', stats)
    size = torch.stack([d[:, 0] + d[:, 1], d[:, 2] + d[:, 3], d[:, 4] + d[:, 5]], -1)
    _held(label + ' fcaf size', box[:, 3:6], size, 6 * size, None, 'fcaf_fwd size', stats)
    if not torch.equal(box[:, 6:], pred[:, 6:9]):
        raise AssertionError(f'{label}: decoded angles are not the regression outputs')


def check_decode_fcaf_bwd(label, pred, dbox, dpred, prior, stats):
    """FCAF coder: gradient passes where exp >= lo (torch.clamp's rule, the reference's autograd)"""
    p, g = pred.to(F64), dbox.to(F64)
    e, _, ge, amb = _clamp_sides(p[:, :6])
    d = e.clamp(min=LO)
    sh = torch.stack([(d[:, 1] - d[:, 0]) / 2, (d[:, 3] - d[:, 2]) / 2, (d[:, 5] - d[:, 4]) / 2], -1)
    sha = torch.stack([(d[:, 1] + d[:, 0]) / 2, (d[:, 3] + d[:, 2]) / 2, (d[:, 5] + d[:, 4]) / 2], -1)
    R, Rabs, dR = _fcaf_rot(p[:, 6:9])
    gc = g[:, :3]
    gs = (R.transpose(1, 2) @ gc[:, :, None])[:, :, 0]
    gsa = (Rabs.transpose(1, 2) @ gc.abs()[:, :, None])[:, :, 0]
    sgn = torch.tensor([-0.5, 0.5, -0.5, 0.5, -0.5, 0.5], dtype=F64, device=p.device)[None]
    j3 = torch.tensor([0, 0, 1, 1, 2, 2], device=p.device)
    on = (sgn * gs[:, j3] + g[:, 3:6][:, j3]) * e
    mag = (0.5 * gsa[:, j3] + g[:, 3:6][:, j3].abs()) * e
    off = torch.zeros_like(on)
    pr = prior.to(F64) if prior is not None else torch.zeros_like(p)
    _either(label + ' fcaf bwd distances', dpred[:, :6], torch.where(ge, on, off) + pr[:, :6], torch.where(ge, off, on) + pr[:, :6], amb,
            32 * mag, pr[:, :6].abs(), 'fcaf_bwd distances', stats)
    ang = torch.stack([(gc[:, None, :] @ dRk @ sh[:, :, None])[:, 0, 0] for dRk in dR], -1) + g[:, 6:9]
    mag = 64 * gc.abs().sum(1, keepdim=True) * sha.sum(1, keepdim=True) + g[:, 6:9].abs()
    _held(label + ' fcaf bwd angles', dpred[:, 6:9], ang + pr[:, 6:9], mag, pr[:, 6:9].abs(), 'fcaf_bwd angles', stats)


# ------------------------------------------------------------------------------------------------------------------ focal loss
def check_focal(rec, dev, stats, cls='focal'):
    """rec: logits (B, Q, Tout), q2g (B, Q), pos_map (sum G, T) uint8, gt_off (host list), tlen, T, alpha, gamma, avg, grad_scale,
    dlogits (B, Q, Tout), loss0 / loss1 (f64 scalars before / after)"""
    x = _d(rec['logits'], dev)
    B, Q, Tout = x.shape
    T, al, ga = rec['T'], rec['alpha'], rec['gamma']
    label = f'{stats.label}: focal B={B} Q={Q} T={T} Tout={Tout}'
    q2g = rec['q2g'].to(dev).long()
    off = torch.tensor(rec['gt_off'][:-1], dtype=torch.long, device=dev)[:, None]
    pm = rec['pos_map'].to(dev)
    y = torch.zeros(B, Q, Tout, dtype=F64, device=dev)
    if pm.shape[0]:
        rows = (off + q2g.clamp(min=0)).clamp(max=pm.shape[0] - 1)
        y[:, :, :min(T, Tout)] = (pm[rows][:, :, :min(T, Tout)] != 0).to(F64) * (q2g >= 0)[:, :, None]
    tl = rec['tlen'].to(dev).long().clamp(min=0, max=T)
    live = (torch.arange(Tout, device=dev)[None, None, :] < tl[:, None, None]).expand(B, Q, Tout)
    p = torch.sigmoid(x)
    pt = torch.where(y > 0, 1 - p, p)
    wa = torch.where(y > 0, torch.full_like(p, al), torch.full_like(p, 1 - al))
    fw = wa * pt ** ga
    bce = x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))
    fwp = ga * pt ** (ga - 1)
    dfw = wa * fwp * torch.where(y > 0, -1.0, 1.0) * p * (1 - p)
    e1 = 5 * p                                                   # (in units of u) absolute error of the f32 `1 - p`
    ept = e1 * (y > 0)
    e_fw = wa * (fwp * ept + U * ept ** 2)
    e_dfw = wa * ga * ((ga - 1) * pt.clamp(min=1e-300) ** (ga - 2) * ept * p * (1 - p) + pt ** (ga - 1) * p * e1)
    c = rec['grad_scale'] / (float(rec['avg']) + EPS32)
    t1, t2 = (p - y) * fw, bce * dfw
    spec = torch.where(live, (t1 + t2) * c, torch.zeros_like(x))
    extra = (16 * (t1.abs() + t2.abs()) + (p - y).abs() * e_fw + fw * ept + bce * e_dfw) * abs(c) + 2.0 ** -126 * (1 + abs(c)) / U
    got = rec['dlogits'].to(dev)
    if not bool((got[~live] == 0).all()):
        raise AssertionError(f'{label}: dlogits is not an exact zero beyond tlen')
    _held(label + ' dlogits', got, spec, torch.where(live, extra, torch.zeros_like(extra)), None, f'{cls} dlogits', stats)
    term = torch.where(live, bce * fw, torch.zeros_like(x))
    n = max(int(live.sum()), 1)
    l0 = float(rec['loss0'])
    bound_check(label + ' loss_sum', rec['loss1'].to(dev).reshape(1), (l0 + term.sum()).reshape(1), U * math.sqrt(n) * term.abs().sum().reshape(1),
                torch.tensor([abs(l0)], dtype=F64, device=dev), False, f'{cls} loss_sum', stats)


# ------------------------------------------------------------------------------------------------------------------ assignment
def lsa_port(cost):
    """scipy.optimize.linear_sum_assignment's solver (scipy/optimize/rectangular_lsap/rectangular_lsap.cpp, Crouse 2016) for an
    (nr, nc) cost with nr <= nc, statement by statement in plain Python: the column visiting order (`remaining` filled in descending
    order, the removed entry replaced by the last) and the tie rule (the first column of the minimum, replaced by every later tie
    that is unassigned).  Returns col4row (the column of every row)."""
    cost = np.asarray(cost, dtype=np.float64)
    nr, nc = cost.shape
    assert nr <= nc
    C = cost.tolist()
    inf = math.inf
    u, v = [0.0] * nr, [0.0] * nc
    path, col4row, row4col = [-1] * nc, [-1] * nr, [-1] * nc
    for cur in range(nr):
        min_val, i = 0.0, cur
        remaining = [nc - it - 1 for it in range(nc)]
        num_remaining = nc
        SR, SC, sp = [False] * nr, [False] * nc, [inf] * nc
        sink = -1
        while sink == -1:
            index, lowest = -1, inf
            SR[i] = True
            Ci, ui = C[i], u[i]
            for it in range(num_remaining):
                j = remaining[it]
                r = min_val + Ci[j] - ui - v[j]
                if r < sp[j]:
                    path[j] = i
                    sp[j] = r
                if sp[j] < lowest or (sp[j] == lowest and row4col[j] == -1):
                    lowest = sp[j]
                    index = it
            min_val = lowest
            if min_val == inf:
                raise ValueError('cost matrix is infeasible')
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            num_remaining -= 1
            remaining[index] = remaining[num_remaining]
        u[cur] += min_val
        for r in range(nr):
            if SR[r] and r != cur:
                u[r] += min_val - sp[col4row[r]]
        for j in range(nc):
            if SC[j]:
                v[j] -= min_val - sp[j]
        j = sink
        while True:
            r = path[j]
            row4col[j] = r
            col4row[r], j = j, col4row[r]
            if r == cur:
                break
    return col4row


def lsa_port_np(cost):
    """lsa_port with the scan over `remaining` as numpy array operations: the sequential rule `strictly lower, or equal and
    unassigned` ends on the LAST unassigned column among those holding the minimum, else on the FIRST column holding it"""
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    nr, nc = cost.shape
    assert nr <= nc
    u, v = np.zeros(nr), np.zeros(nc)
    path, col4row, row4col = np.full(nc, -1), np.full(nr, -1), np.full(nc, -1)
    for cur in range(nr):
        min_val, i = 0.0, cur
        remaining = np.arange(nc - 1, -1, -1)
        num_remaining = nc
        SR, SC, sp = np.zeros(nr, bool), np.zeros(nc, bool), np.full(nc, np.inf)
        sink = -1
        while sink == -1:
            SR[i] = True
            rem = remaining[:num_remaining]
            r = min_val + cost[i, rem] - u[i] - v[rem]
            better = r < sp[rem]
            path[rem[better]] = i
            sp[rem[better]] = r[better]
            vals = sp[rem]
            lowest = vals.min()
            if lowest == np.inf:
                raise ValueError('cost matrix is infeasible')
            ties = np.nonzero(vals == lowest)[0]
            free = ties[row4col[rem[ties]] == -1]
            index = int(free[-1]) if free.size else int(ties[0])
            min_val = float(lowest)
            j = int(rem[index])
            if row4col[j] == -1:
                sink = j
            else:
                i = int(row4col[j])
            SC[j] = True
            num_remaining -= 1
            remaining[index] = remaining[num_remaining]
        u[cur] += min_val
        rows = np.nonzero(SR)[0]
        rows = rows[rows != cur]
        u[rows] += min_val - sp[col4row[rows]]
        v[SC] -= min_val - sp[SC]
        j = sink
        while True:
            r = int(path[j])
            row4col[j] = r
            col4row[r], j = j, int(col4row[r])
            if r == cur:
                break
    return [int(c) for c in col4row]


def check_assignment(label, cost, Gs, q2g, stats=None, port=lsa_port_np):
    """cost: the kernel's (B, Gmax, Q) f64 output (host); Gs: boxes per sample; q2g (B, Q) int.  Held to the port on that cost, and --
    whatever the tie rule -- to scipy's optimum and to a one-to-one matching"""
    from scipy.optimize import linear_sum_assignment
    cost, q2g = np.asarray(cost, dtype=np.float64), np.asarray(q2g)
    B, _, Q = cost.shape
    for b in range(B):
        g = int(Gs[b])
        got = q2g[b]
        matched = np.nonzero(got >= 0)[0]
        if sorted(got[matched].tolist()) != list(range(g)):
            raise AssertionError(f'{label}: sample {b}: the matched boxes {sorted(got[matched].tolist())} are not each of the {g} boxes exactly once')
        c = cost[b, :g]
        total = float(c[got[matched], matched].sum())
        if g:
            ri, ci = linear_sum_assignment(c)
            best = float(c[ri, ci].sum())
            if abs(total - best) > 1e-9 * max(abs(best), 1e-300):
                raise AssertionError(f'{label}: sample {b}: total cost {total!r} is not the optimum {best!r}')
        want = np.full(Q, -1, dtype=np.int64)
        for r, col in enumerate(port(c) if g else []):
            want[col] = r
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f'{label}: sample {b} (G={g}, Q={Q}): optimal, but {bad.size} queries differ from the tie resolution of '
                                 f'scipy\'s solver (first: query {int(bad[0])} -> box {int(got[bad[0]])}, want {int(want[bad[0]])})')
    if stats is not None:
        stats.note('assignment', None, 0.0)


# ------------------------------------------------------------------------------------------------------------------ top-k
def check_topk(label, vals, vlen, k, idx):
    """vals (B, L) f32, vlen (B,) or None, idx (B, k) int32 (host tensors)"""
    B, L = vals.shape
    for b in range(B):
        n = L if vlen is None else max(min(int(vlen[b]), L), 0)
        want = torch.full((k,), -1, dtype=torch.long)
        order = torch.argsort(vals[b, :n], descending=True, stable=True)[:k]
        want[:order.numel()] = order
        got = idx[b].long()
        if not torch.equal(got, want):
            i = int(torch.nonzero(got != want)[0])
            raise AssertionError(f'{label}: sample {b} (n={n}, k={k}): position {i} holds row {int(got[i])}, the stable descending order '
                                 f'has row {int(want[i])} there ({int((got != want).sum())} positions differ)')


# ------------------------------------------------------------------------------------------------------------------ box IoU
def aligned_iou(a, b):
    """closed-form IoU of two axis-aligned boxes (centre, size): numpy (…, 6)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    lo = np.maximum(a[..., :3] - a[..., 3:6] / 2, b[..., :3] - b[..., 3:6] / 2)
    hi = np.minimum(a[..., :3] + a[..., 3:6] / 2, b[..., :3] + b[..., 3:6] / 2)
    inter = np.prod(np.clip(hi - lo, 0, None), -1)
    return inter / (np.prod(a[..., 3:6], -1) + np.prod(b[..., 3:6], -1) - inter)
