"""Specifications of the kernels that decide what the two dense heads learn and report (csrc/losses.hip, csrc/targets.hip,
csrc/predict.hip, csrc/occ.hip), evaluated in f64 on the operands each launch actually received -- the STORED bbox of
es_reg_decode_bwd, the STORED stats of es_occ_loss, what an accumulating output held before the launch.  Used by
tests/test_gpu_head_kernels.py (MI355X) and tests/test_emu_head_kernels.py (the same bodies on the CPU emulator, plus mutated outputs
the checker must reject and the f32 torch evaluation of each formula, which must pass).
u = 2^-24, G = 8 (fwd_spec); every bound is per element and none depends on 1 / |spec|.  Counts as in ground_spec: expf / logf / powf
4 u relative, one IEEE operation 1 u, a sum of n terms G u sqrt(n) sum |term|.  The printed ratio is |err| / (bound / G).

Focal loss (es_focal_loss; mmcv's sigmoid_focal_loss as the kernel restates it, NOT the grounding form of ground_spec.check_focal):
  p = sigmoid(x), q = 1 - p, FLT_MIN the smallest normal f32, lp = log max(p, FLT_MIN), ln = log max(q, FLT_MIN)
  label == column:  l = -alpha q^gamma lp            g = -alpha q^gamma (q - gamma p lp)
  otherwise:        l = -(1 - alpha) p^gamma ln      g = -(1 - alpha) p^gamma (gamma q ln - p)       (a label outside [0, C) is background)
  dlogits = g c, c = grad_scale / (avg + eps32);  loss_out = prior + sum l / (avg + eps32)
  The f32 `1 - p` carries an ABSOLUTE error 5 u p whatever q is (ground_spec) and, below p = 1 / 2 where the subtraction is not exact, its
  own rounding, at most u 2^floor(log2 q) -- which ln then turns into an ABSOLUTE error, all of ln q at q ~ 1: d = u (5 p + [p < 1/2]
  2^floor(log2 q)).  g is evaluated at q - d (clamped at 0), q and q + d with p fixed; the larger difference e_q to g(q) is the
  propagated error (g is monotone in q: -alpha (q^(gamma+1) + |gamma p lp| q^gamma); q ln q is monotone away from 1 / e, where it is
  flat to second order).  c is the f32 quotient of grad_scale and the f32 sum avg + eps32, reproduced bit for bit.  On top, rounding by
  rounding, in units of u (r_p = 2 + 4 q the relative error of p = 1 / (1 + expf(-x)): expf's 4 u reaches p scaled by q, the addition
  and the division 1 each; pw = 1 for gamma = 2, a product, else 4, powf; T = gamma p |lp|, T2 = gamma q |ln|):
    label column:  |g| (1 [g c] + 1 [times the bracket] + [alpha no power of two] + pw);  inside the bracket, times alpha q^gamma:
      T (r_p + 4 [logf] + 2 [two products]), gamma p r_p (lp moves by r_p ABSOLUTE with p's relative error), q + T (the subtraction)
    other columns: |g| (1 [g c] + 1 [1 - alpha] + 2 [the outer products] + gamma r_p + pw [p^gamma]);  inside the bracket, times
      (1 - alpha) p^gamma: T2 (4 [logf] + 2 [products]), r_p p, T2 + p (the subtraction)
  |dlogits - g c| <= (these terms + e_q) |c| + 2^-126 (1 + |c|)   (a product below the smallest normal f32 is flushed)
  (about 6 u |g| on a label column at x = -10, the best-conditioned element: 4 ulp there is 4 .. 8 u and is rejected.)
  The loss VALUE is not well conditioned: at x ~ 17 the f32 q is 0 and kernel and mmcv return log FLT_MIN.  Every term is held to the
  interval [l_a, l_b] of the formula over q -+ d (the logarithm's argument clamped below at FLT_MIN):
  loss_out in prior + [sum l_a, sum l_b] / (avg + eps32) widened by (G sqrt(ceil(C / 64)) + 16) u sum l_b / (avg + eps32) (a lane adds
  ceil(C / 64) f32 terms, everything above that is an f64 sum; 16 u the relative error of a term) + 3 u |sum| + u |prior|.
Regression decode (es_reg_decode_fwd / _bwd), lo = f32(1e-3), t = the f32 product scale reg (ONE IEEE operation, reproduced bit for bit):
  forward  bbox[:, :6] = max(exp(t), lo) within 6 u (expf 4, 2 spare), bbox[:, 6:] = reg[:, 6:] bit for bit
  backward on the STORED bbox b:  dreg[:, :6] = [b > lo] g b scale within 3 u (two products, 1 spare); |b / lo - 1| <= 4 u may take
  either side (ground_spec explains why > and >= cannot be told apart); dreg[:, 6:] = dbbox[:, 6:] bit for bit;
  dscale = prior + sum [b > lo] g b reg within G u sqrt(6 n) sum |g b reg| + 2 u sum |g b reg| (the two products of a term) + u |prior|
  (+ the terms of the ambiguous elements); two launches on the same operands give the same bits (fixed-order reduction).
Corner-Chamfer losses (es_pos_losses, es_box_cd_pairs): cd_rows() -- per row sum_g w_g sum_{8 source corners} min_{target corners} L1,
  group g takes centre / size / angles / everything from the prediction and the rest from the target; the nearest corner is the first
  minimum, |.|' = sign with sign(0) = 0 (torch.abs) -- as autograd over oracle.geometry evaluated in f64.  The kernels compute in f64
  (forward-mode dual numbers) and round once: |grad - spec| <= u |spec| + 2^-44 K M, M = |inv_mean grad_scale| sum w 8 (1 + sum |size|
  / 2 + sum |shift|) the scale of a row's gradient, K the conditioning of the 6-D rotation chain computed from the row's inputs:
  K = (1 + 1 / |y_raw|) (1 + (1 + |x_raw|) / |x_raw x y|) / (1 - y_z^2)  (normalise, cross product against y, asin / atan2 at the
  gimbal); K = 1 for es_box_cd_pairs, whose angles are inputs.  2^-44 = 512 f64 roundoffs: the chain is ~100 operations long and two
  correct f64 evaluations in different orders differ by that much.  Where two target corners are within 1e-9 of the same L1 distance
  from a source corner the row is held to the first OR the last of the tied corners.
  Centerness: dcenter = (sigmoid(x) - t) c within 8 u (sigmoid(x) + t) |c| (sigmoid 6, the subtraction 1, times c 3, rounded down to
  the issue's 8: c is formed from two roundings that are common to every row); loss_acc[0] = prior + sum bce within
  (G sqrt(P) + 8) u sum (max(x, 0) + |x t| + log1p(exp(-|x|))), loss_acc[1] = prior + sum f32(row inv_mean) within G u sqrt(P) sum |term|.
  max_pos below the number of positives: at most max_pos rows are written, every written row is right, the sums run over the written
  rows, pos_ws[0] is the true count.
Targets (es_get_targets): bit-exact against oracle.geometry.get_targets (pinned to the reference's golden output) for cls, bbox, center
  and n_pos; box_idx is -1 exactly where cls is, otherwise labels[box_idx] == cls and boxes[box_idx] == bbox bit for bit.
Prediction:  scores = sigmoid(cls) sigmoid(ctr) within 10 u relative; max_scores[row] = max of the row the kernel WROTE, bit for bit.
  es_decode_boxes: size b_2k + b_2k+1 within 1 u.  Rotation: R(euler_out) (f64, from the three angles the kernel wrote) against
  M = R(euler(frame)) of the f64 Gram-Schmidt frame [y x z, y, z] of the raw 6-D output, entry by entry -- not angle by angle, which is
  ill-conditioned at the gimbal (the frame itself is no rotation: |y| = 1 - 1e-8 / |y_raw|, 1e-5 at |y_raw| = 1e-3; reference and
  kernel both go through the angles): |R - M| <= 64 u (1 + c) / rho, c = |x_raw| |y| / |x_raw x y| >= 1, rho = sqrt(1 - y_z^2): y = y_raw / (|y_raw| + 1e-8) costs
  8 u relative whatever |y_raw| is (the forward frame is scale-free in y_raw; 1 / |y_raw| only enters the gradients above), the cross
  product 2 u |x_raw| |y| + 8 u of y absolute = 10 u c relative to |x_raw x y|, z and y x z (10 c + 18) u; asinf / atan2f 4 u absolute
  plus their argument's error / rho; every entry of R moves by at most 2 per unit of each angle: 2 (8 / rho + 4) + (8 / rho + 4)
  + 2 ((10 c + 18) / rho + 4) <= (60 + 20 c) / rho + 20 <= 64 (1 + c) / rho with 16 spare at c = rho = 1.
  Centre: point + M shift within 32 u (|point| + Mabs (b_2k + b_2k+1) / 2) (check_decode_fcaf_fwd's count) + 64 u (1 + c) / rho sum |shift|.
  es_nms3d_multiclass: per class the keep list of oracle.predict.nms3d on the candidates (score > thr) in (score descending, index
  ascending) order; keep_idx beyond keep_cnt[c] untouched.  A pair whose f64 IoU is within 1e-9 of the threshold may fall either way:
  nms_margin() returns the smallest |IoU - thr| met and the tests assert it is larger on their random parts.
Occupancy:  es_occ_targets bit-exact against oracle.occ.occupancy_multiscale_supervision on the rows that land inside the grid after the
  truncating division (torch.div(trunc): -1 / ratio = 0), plus the max-pooled visibility mask (255 where a ratio^3 window is hidden).
  es_occ_loss, stage 1 (k_occ_stats): A_c = sum_mask p_c, B_c = sum_mask p_c [t == c], N_c, n_mask, CE = sum (lse - x_t), p the f64
  softmax.  The f32 p is m = max, e = __expf(x - m) (4 u, and the subtraction and the product with log2 e move the argument by
  2 u |x - m|), s = sum e (G u sqrt(C) relative: all terms positive), p = e / s (2 u):
    |A_c - spec| <= u sum_i p_ic (6 + 2 |x_ic - m_i|) + G u sqrt(C) sum_i p_ic  (the f64 sums over voxels add nothing at this scale),
    B_c likewise over its voxels, N_c / n_mask exact, CE: u sum_i (4 |log s| + 2 |lse| + |x_t| + |lse - x_t|) + G u sqrt(C) n_mask.
  stage 2 (k_occ_coeffs, k_occ_grad) on the STORED stats, f64:  pr = B / A, rc = B / N, sp = (rest - (A - B)) / rest, rest = n - N;
    bce1(v) = -max(log v, -100), bce1'(v) = (v - 1) / max((1 - v) v, 1e-12); sem = mean over classes with N > 0 of bce1(pr) [A > 0]
    + bce1(rc) + bce1(sp) [rest > 0]; geo = bce1(inter / D) + bce1(inter / R) + bce1(B_0 / S), inter = (n - N_0) - (A_0 - B_0),
    D = n - A_0 + 1e-6, R = n - N_0 + 1e-6, S = N_0 + 1e-6; ce = CE / n (NaN when everything is ignored, as the reference).
    out = (ce, sem, geo, (ce + sem + geo) weight) within 2 u |spec| (f64 arithmetic, one rounding; 1 spare); total_acc += out[3] (1 u).
    alpha_c = dL / dA_c (applies to p_c of a voxel of another class), gamma_c = dL / dA_c + dL / dB_c (a voxel of class c), the latter
    formed WITHOUT the cancelling pairs: sem gamma_c = (bce1'(pr) (A - B) / A^2 + bce1'(rc) / N) / count, geo gamma_0 = bce1'(P) inter
    / D^2 + bce1'(Sp) / S.  With g_c = [c == t] gamma_c + [c != t] alpha_c, dot = sum_c p_c g_c, ce_scale = weight / n:
    dlogits_c = p_c (g_c - dot) + ce_scale (p_c - [c == t]), zero on ignored voxels.  Error: p_c as above (relative r_c = 6 + 2 |x_c - m|
    apart from the shared s), g_c 1 u (stored as f32), dot: sum p_c' |g_c'| (r_c' + 2) u + its own sum, the subtraction, the two
    products, the final addition:
    |d - spec| <= u [p_c ((r_c + 4) |g_c| + sum_c' p_c' |g_c'| (r_c' + r_c + 6)) + ce_scale ((r_c + 3) p_c + 3 [c == t])]
                  + G u sqrt(C) [p_c (|g_c| + 3 sum_c' p_c' |g_c'|) + ce_scale p_c] + 2^-126
    -- the issue's k u [p_c (|g_c| + sum p |g|) + ce_scale (p_c + [c == t])] with k spelled out.  g is the coefficient that APPLIES to
    the voxel: a bound in |alpha_c| + |beta_c| would have hidden the cancellation defect this specification was written for.

Worst ratios observed, |err| / (bound / G) against G = 8 (MI355X on the full grid / CPU emulator on the reduced grid; n/m: not
measured -- the MI355X column is filled from the output of tests/test_gpu_head_kernels.py, which prints every class):
  focal  dlogits n/m / 7.96   loss_out n/m / 0.00
    (dlogits: on a background column at x ~ -10 the bound is the ONE rounding of 1 - p seen through ln q, a strict half ulp that single
    elements of a 24 591-element grid nearly reach; the f32 torch evaluation of the formula reaches 7.96 as well)
  reg_decode_fwd n/m / 1.33   reg_decode_bwd  dreg n/m / 4.27   dscale n/m / 0.00
  pos_losses  dbbox n/m / 7.80   dcenter n/m / 1.50   loss centre n/m / 0.00   loss box n/m / 0.00
  box_cd_pairs  dpred n/m / 7.56   loss n/m / 0.00
    (dbbox / dpred / decode size: one f32 rounding of an f64 result held to u |spec|, a strict bound that single elements nearly reach)
  predict_scores n/m / 2.31   decode_boxes  size n/m / 7.97   rotation n/m / 0.16   centre n/m / 0.16
  occ_loss  stats A n/m / 0.25   B n/m / 0.63   CE n/m / 0.49   values n/m / 3.57   total_acc n/m / 0.00   dlogits n/m / 2.12
  targets, NMS, occupancy targets: exact.  Smallest |IoU - thr| met by an NMS grid: n/m"""
import math

import numpy as np
import torch

from fwd_spec import F64, G, U, Stats, bound_check  # noqa: F401
from ground_spec import EPS32, _bits_equal, _either, _fcaf_rot, _held

FLT_MIN = float(torch.tensor(1.17549435e-38, dtype=torch.float32))
LO3 = float(torch.tensor(1e-3, dtype=torch.float32))
TINY = 2.0 ** -126


def _d(t, dev=None):
    return None if t is None else (t.to(dev) if dev is not None else t).to(F64)


# ------------------------------------------------------------------------------------------------------------------ focal
def _focal_terms(x, pos, q, al, ga):
    """loss term, gradient factor g and the relative part of g's error (in units of u) at q, with p = sigmoid(x) fixed"""
    p = torch.sigmoid(x)
    lp, ln = torch.log(p.clamp(min=FLT_MIN)), torch.log(q.clamp(min=FLT_MIN))
    wq, wp = q ** ga, p ** ga
    l = torch.where(pos, -al * wq * lp, -(1 - al) * wp * ln)
    g = torch.where(pos, -al * wq * (q - ga * p * lp), -(1 - al) * wp * (ga * q * ln - p))
    rp, pw = 2 + 4 * q, (1 if ga == 2.0 else 4)
    T, T2 = ga * p * lp.abs(), ga * q * ln.abs()
    a2 = 0 if math.frexp(al)[0] == 0.5 else 1                    # alpha a power of two: the product with it is exact
    e_pos = g.abs() * (2 + a2 + pw) + al * wq * (T * (rp + 6) + ga * p * rp + (q + T))
    e_neg = g.abs() * (4 + ga * rp + pw) + (1 - al) * wp * (6 * T2 + rp * p + (T2 + p))
    return l, g, torch.where(pos, e_pos, e_neg)


def focal_ref_f32(x, labels, ga, al, avg, gs):
    """f32 torch evaluation of the formula (CPU): (dlogits, sum l / (avg + eps32))"""
    x = x.float()
    C = x.shape[1]
    pos = labels.long()[:, None] == torch.arange(C)[None]
    one = torch.tensor(1.0)
    p = one / (one + torch.exp(-x))
    q = one - p
    fmin = torch.tensor(FLT_MIN, dtype=torch.float32)
    lp, ln = torch.log(torch.maximum(p, fmin)), torch.log(torch.maximum(q, fmin))
    a, g_ = torch.tensor(al, dtype=torch.float32), torch.tensor(ga, dtype=torch.float32)
    wq, wp = (q * q, p * p) if ga == 2.0 else (torch.pow(q, g_), torch.pow(p, g_))
    l = torch.where(pos, -a * wq * lp, -(one - a) * wp * ln)
    g = torch.where(pos, -a * wq * (one - p - g_ * p * lp), -(one - a) * wp * (g_ * (one - p) * ln - p))
    inv = torch.tensor(gs, dtype=torch.float32) / (torch.tensor(avg, dtype=torch.float32) + torch.tensor(EPS32, dtype=torch.float32))
    return g * inv, (l.double().sum().float() / (torch.tensor(avg, dtype=torch.float32) + torch.tensor(EPS32, dtype=torch.float32)))


def focal_grad_spec(rec, dev):
    """(g c, its bound in units of u, the three evaluations of the loss terms)"""
    x = _d(rec['logits'], dev)
    C = x.shape[1]
    al, ga = rec['alpha'], rec['gamma']
    pos = rec['labels'].to(dev).long()[:, None] == torch.arange(C, device=dev)[None]
    p, q = torch.sigmoid(x), torch.sigmoid(-x)
    d = U * (5 * p + torch.where(p < 0.5, torch.pow(2.0, torch.floor(torch.log2(q))), torch.zeros_like(q)))
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    c = float(f32(rec['grad_scale']) / (f32(rec['avg']) + f32(EPS32)))          # two IEEE operations, reproduced bit for bit
    l, g, rel = _focal_terms(x, pos, q, al, ga)
    l_lo, g_lo, _ = _focal_terms(x, pos, (q - d).clamp(min=0), al, ga)
    l_hi, g_hi, _ = _focal_terms(x, pos, q + d, al, ga)
    eq = torch.maximum((g_lo - g).abs(), (g_hi - g).abs())
    return g * c, (rel + eq / U) * abs(c) + TINY * (1 + abs(c)) / U, (l, l_lo, l_hi)


def check_focal_head(rec, dev, stats, cls='focal'):
    """rec: logits (N, C) as read, labels (N,) int, gamma, alpha, avg (the f32 value), grad_scale, grad (N, C) or None, loss0 / loss1
    (floats: loss_out before / after)"""
    N, C = rec['logits'].shape
    label = f'{stats.label}: focal N={N} C={C} gamma={rec["gamma"]}'
    spec, bound_u, (l, l_lo, l_hi) = focal_grad_spec(rec, dev)
    if rec.get('grad') is not None:
        _held(label + ' dlogits', rec['grad'].to(dev), spec, bound_u, None, f'{cls} dlogits', stats)
    inv = 1.0 / (float(rec['avg']) + EPS32)
    la, lb = torch.minimum(l_lo, l_hi).sum() * inv, torch.maximum(l_lo, l_hi).sum() * inv
    l0 = float(rec['loss0'])
    mid, half = l0 + (la + lb) / 2, (lb - la) / 2
    one = torch.ones(1, dtype=F64, device=dev)
    bound_check(label + ' loss_out', torch.tensor([float(rec['loss1'])], dtype=F64, device=dev), mid * one, U * math.sqrt(math.ceil(C / 64)) * lb * one,
                (half / U + 16 * lb + 3 * (l.sum() * inv).abs() + abs(l0)) * one, False, f'{cls} loss_out', stats)


# ------------------------------------------------------------------------------------------------------------------ regression decode
def reg_decode_ref_f32(reg, scale):
    t = reg[:, :6].float() * scale.float()
    return torch.cat([torch.maximum(torch.exp(t), torch.tensor(LO3, dtype=torch.float32)), reg[:, 6:].float()], 1)


def reg_decode_bwd_ref_f32(reg, bbox, dbbox, scale, skip_row=None):
    live = bbox[:, :6] > LO3
    gb = torch.where(live, dbbox[:, :6] * bbox[:, :6], torch.zeros(1))
    t = gb * reg[:, :6]
    if skip_row is not None:
        t = torch.cat([t[:skip_row], t[skip_row + 1:]])
    return torch.cat([gb * scale, dbbox[:, 6:]], 1), t.double().sum().float()


def check_reg_decode_fwd(label, reg, scale, bbox, stats, cls='reg_decode_fwd'):
    """reg (n, 12) as read (a strided view), scale (1,) f32, bbox (n, 12)"""
    t = (reg[:, :6].float() * scale.float().to(reg.device)).to(F64)
    spec = torch.exp(t).clamp(min=LO3)
    _held(label + ' decode', bbox[:, :6], spec, 6 * spec, None, cls, stats)
    if not _bits_equal(bbox[:, 6:], reg[:, 6:]):
        raise AssertionError(f'{label}: columns 6 .. 11 of bbox are not the regression outputs bit for bit')


def check_reg_decode_bwd(label, reg, bbox, dbbox, scale, dreg, dscale0, dscale1, stats, cls='reg_decode_bwd'):
    """reg (n, 12) as read, bbox / dbbox (n, 12) as stored, dreg (n, 12) view, dscale0 / dscale1 floats"""
    r, b, g, s = _d(reg[:, :6]), _d(bbox[:, :6]), _d(dbbox[:, :6]), float(scale.reshape(-1)[0])
    n = r.shape[0]
    live, amb = b > LO3, (b / LO3 - 1).abs() <= 4 * U
    on, off = g * b * s, torch.zeros_like(b)
    _either(label + ' dreg', dreg[:, :6], torch.where(live, on, off), torch.where(live, off, on), amb, 3 * on.abs(), torch.zeros_like(b), f'{cls} dreg', stats)
    if not _bits_equal(dreg[:, 6:], dbbox[:, 6:]):
        raise AssertionError(f'{label}: columns 6 .. 11 of dreg are not dbbox bit for bit')
    term = g * b * r
    tl = torch.where(live, term, off)
    A = tl.abs().sum().reshape(1)
    bound_check(label + ' dscale', torch.tensor([float(dscale1)], dtype=F64, device=r.device), float(dscale0) + tl.sum().reshape(1), U * math.sqrt(6 * n) * A,
                abs(float(dscale0)) + 2 * A + term.abs()[amb].sum() / U, False, f'{cls} dscale', stats)


# ------------------------------------------------------------------------------------------------------------------ corner Chamfer
def cd_rows(dec, tgt, w, choice='first'):
    """dec, tgt (P, 9) f64 boxes (dec may require grad): (P,) sum_g w_g sum_corners min L1, and which rows hold a tie within 1e-9.
    choice: which of the tied target corners a source corner takes ('first' is the kernels' rule, 'last' the other end of the tie;
    'second' -- for the checker's own test -- the SECOND-nearest corner in row 0)"""
    from oracle import geometry as OG
    tc = OG.bbox_to_corners(tgt)
    tot = torch.zeros(dec.shape[0], dtype=F64, device=dec.device)
    tie = torch.zeros(dec.shape[0], dtype=torch.bool, device=dec.device)
    for grp in range(4):
        v = dec if grp == 3 else torch.cat([dec[:, 3 * k:3 * k + 3] if k == grp else tgt[:, 3 * k:3 * k + 3] for k in range(3)], 1)
        sc = OG.bbox_to_corners(v)
        dist = (sc[:, :, None, :] - tc[:, None, :, :]).abs().sum(-1)
        dd = dist.detach()
        cand = dd <= dd.min(2, keepdim=True).values + 1e-9
        tie |= (cand.sum(2) > 1).any(1)
        idx = cand.int().argmax(2) if choice != 'last' else 7 - cand.flip(2).int().argmax(2)
        if choice == 'second' and grp == 3:
            idx = idx.clone()
            idx[0, 0] = dd[0, 0].argsort()[1]
        tot = tot + w[grp] * dist.gather(2, idx[..., None]).sum((1, 2))
    return tot, tie


def _cd_grads(make_dec, leaf, tgt, w, scale):
    """(loss rows, gradient w.r.t. leaf) x scale for the first and the last tie choice, and the tie rows"""
    out = []
    for ch in ('first', 'last'):
        x = leaf.clone().requires_grad_(True)
        tot, tie = cd_rows(make_dec(x), tgt, w, ch)
        (gr,) = torch.autograd.grad(tot.sum(), x)
        out.append((tot.detach(), gr))
    return out[0], out[1], tie


def _rot_cond(bp):
    xr, yr = bp[:, 6:9], bp[:, 9:12]
    ny = yr.norm(dim=1)
    y = yr / (ny + 1e-8)[:, None]
    cr = torch.linalg.cross(xr, y).norm(dim=1).clamp(min=1e-300)
    rho2 = (1 - y[:, 2] ** 2).clamp(min=1e-300)
    return ny, xr.norm(dim=1), cr, rho2


def check_pos_losses(rec, dev, stats, cls='pos_losses'):
    """rec: pts (n, 3), bbox (n, 12), ctr (n,) centerness logits, cls_t (n,), center_t (n,), bbox_t (n, 9), P (n_pos_dev), avg, grad_scale, w,
    max_pos, dctr (n,), dbbox (n, 12) (both pre-filled with `sent`), sent, acc0 / acc1 (2,) f64, count (pos_ws[0])"""
    from oracle import geometry as OG
    label = f'{stats.label}: es_pos_losses n={rec["pts"].shape[0]} max_pos={rec["max_pos"]}'
    sent = rec['sent']
    posrow = rec['cls_t'].to(dev) >= 0
    npos = int(posrow.sum())
    dbb, dct = rec['dbbox'].to(dev), rec['dctr'].to(dev)
    written = (dbb != sent).any(1)
    if not bool((written == (dct != sent)).all()):
        raise AssertionError(f'{label}: the centerness and the box gradient tables disagree on which rows were written')
    if bool((written & ~posrow).any()):
        raise AssertionError(f'{label}: a row that is not positive was written')
    if int(rec['count']) != npos:
        raise AssertionError(f'{label}: pos_ws[0] = {int(rec["count"])}, the number of positives is {npos}')
    want = min(npos, rec['max_pos'], rec['pts'].shape[0])
    if int(written.sum()) != want:
        raise AssertionError(f'{label}: {int(written.sum())} rows written, expected {want}')
    sel = torch.nonzero(written).squeeze(1)
    acc0, acc1 = _d(rec['acc0'], dev), _d(rec['acc1'], dev)
    if sel.numel() == 0:
        if not torch.equal(acc0, acc1):
            raise AssertionError(f'{label}: loss_acc changed without a positive row')
        return
    Pn = sel.numel()
    pts, bp, tgt = _d(rec['pts'], dev)[sel], _d(rec['bbox'], dev)[sel], _d(rec['bbox_t'], dev)[sel]
    w = [float(torch.tensor(v, dtype=torch.float32)) for v in rec['w']]
    gs = float(torch.tensor(rec['grad_scale'], dtype=torch.float32))
    inv_mean = 1.0 / (float(rec['P']) * 8.0)
    (tot, g1), (_, g2), tie = _cd_grads(lambda x: OG.bbox_pred_to_bbox(pts, x), bp, tgt, w, None)
    sc = inv_mean * gs
    g1, g2 = g1 * sc, g2 * sc
    got = dbb[sel]
    use2 = tie & ((got.to(F64) - g2).abs().sum(1) < (got.to(F64) - g1).abs().sum(1))
    spec = torch.where(use2[:, None], g2, g1)
    ny, nx, cr, rho2 = _rot_cond(bp)
    K = (1 + 1 / ny.clamp(min=1e-300)) * (1 + (1 + nx) / cr) / rho2
    shift = (bp[:, 1:6:2] - bp[:, 0:6:2]).abs().sum(1) / 2
    size = (bp[:, 1:6:2] + bp[:, 0:6:2]).abs().sum(1) / 2
    M = abs(sc) * sum(w) * 8 * (1 + size + shift)
    _held(label + ' dbbox', got, spec, spec.abs() + (2.0 ** -44 / U) * (K * M)[:, None], None, f'{cls} dbbox', stats)
    x, t = _d(rec['ctr'], dev)[sel], _d(rec['center_t'], dev)[sel]
    c = gs / (float(rec['avg']) + EPS32)
    sg = torch.sigmoid(x)
    _held(label + ' dcenter', dct[sel], (sg - t) * c, 8 * (sg + t.abs()) * abs(c) + TINY / U, None, f'{cls} dcenter', stats)
    bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    A = (x.clamp(min=0) + (x * t).abs() + torch.log1p(torch.exp(-x.abs()))).sum().reshape(1)
    bound_check(label + ' loss_acc[0]', acc1[0:1], acc0[0:1] + bce.sum().reshape(1), U * math.sqrt(Pn) * A, 8 * A + acc0[0:1].abs(), False, f'{cls} loss centre', stats)
    rows = tot * inv_mean
    A = rows.abs().sum().reshape(1)
    bound_check(label + ' loss_acc[1]', acc1[1:2], acc0[1:2] + rows.sum().reshape(1), U * math.sqrt(Pn) * A, acc0[1:2].abs() + (2.0 ** -44 / U) * A, False,
                f'{cls} loss box', stats)


def check_box_cd_pairs(rec, dev, stats, cls='box_cd_pairs'):
    """rec: pred (B Q, 9), q2g (B Q,), B, Q, gt (sum G, 9), gt_off (host list), n_pairs, grad_scale, w, dpred (B Q, 9) pre-filled with sent or
    None, sent, acc0 / acc1 (1,) f64"""
    B, Q = rec['B'], rec['Q']
    label = f'{stats.label}: es_box_cd_pairs B={B} Q={Q} n_pairs={rec["n_pairs"]}'
    q2g = rec['q2g'].to(dev).long()
    sel = torch.nonzero(q2g >= 0).squeeze(1)
    acc0, acc1 = _d(rec['acc0'], dev), _d(rec['acc1'], dev)
    dp = None if rec.get('dpred') is None else rec['dpred'].to(dev)
    if dp is not None:
        rest = torch.ones(B * Q, dtype=torch.bool, device=dev)
        rest[sel] = False
        if not bool((dp[rest] == rec['sent']).all()):
            raise AssertionError(f'{label}: a row without a matched box was written')
    if sel.numel() == 0 or rec['n_pairs'] <= 0:
        if not torch.equal(acc0, acc1) or (dp is not None and not bool((dp == rec['sent']).all())):
            raise AssertionError(f'{label}: something was written without a pair')
        return
    off = torch.tensor(rec['gt_off'][:-1], dtype=torch.long, device=dev)
    tgt = _d(rec['gt'], dev)[off[sel // Q] + q2g[sel]]
    pred = _d(rec['pred'], dev)[sel]
    w = [float(torch.tensor(v, dtype=torch.float32)) for v in rec['w']]
    gs = float(torch.tensor(rec['grad_scale'], dtype=torch.float32))
    inv_mean = float(torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(rec['n_pairs']), dtype=torch.float32) * 8.0))
    (tot, g1), (_, g2), tie = _cd_grads(lambda x: x, pred, tgt, w, None)
    if dp is not None:
        sc = inv_mean * gs
        g1, g2 = g1 * sc, g2 * sc
        got = dp[sel]
        use2 = tie & ((got.to(F64) - g2).abs().sum(1) < (got.to(F64) - g1).abs().sum(1))
        spec = torch.where(use2[:, None], g2, g1)
        M = abs(sc) * sum(w) * 8 * (1 + pred[:, 3:6].abs().sum(1) / 2)
        _held(label + ' dpred', got, spec, spec.abs() + (2.0 ** -44 / U) * M[:, None], None, f'{cls} dpred', stats)
    rows = tot * inv_mean
    A = rows.abs().sum().reshape(1)
    bound_check(label + ' loss_acc', acc1[0:1], acc0[0:1] + rows.sum().reshape(1), U * math.sqrt(sel.numel()) * A, acc0[0:1].abs() + 2 * A, False,
                f'{cls} loss', stats)


# ------------------------------------------------------------------------------------------------------------------ targets
def check_targets(label, pts_levels, boxes, labels, assign_thr, center_thr, center_t, bbox_t, cls_t, box_idx, n_pos):
    """host tensors: pts_levels list of (n_l, 3), boxes (G, 9), labels (G,) int; outputs of the kernel"""
    from oracle import geometry as OG
    ct, bt, kt = OG.get_targets(pts_levels, boxes, labels.long(), assign_thr, center_thr)
    if not torch.equal(cls_t.long(), kt.long()):
        i = int(torch.nonzero(cls_t.long() != kt.long())[0])
        raise AssertionError(f'{label}: cls_t differs from the oracle at {int((cls_t.long() != kt.long()).sum())} locations (first {i}: {int(cls_t[i])}, want {int(kt[i])})')
    if not _bits_equal(center_t, ct.float()):
        raise AssertionError(f'{label}: center_t is not the oracle\'s bit for bit ({int((center_t != ct).sum())} locations)')
    if not _bits_equal(bbox_t, bt.float().reshape(bbox_t.shape)):
        raise AssertionError(f'{label}: bbox_t is not the oracle\'s bit for bit')
    if int(n_pos) != int((kt >= 0).sum()):
        raise AssertionError(f'{label}: n_pos = {int(n_pos)}, the oracle has {int((kt >= 0).sum())} positives')
    bi = box_idx.long()
    if not torch.equal(bi < 0, kt < 0) or (boxes.shape[0] and bool((bi >= boxes.shape[0]).any())):
        raise AssertionError(f'{label}: box_idx is not -1 exactly where cls_t is')
    on = bi >= 0
    if bool(on.any()) and not (torch.equal(labels.long()[bi[on]], kt[on].long()) and _bits_equal(boxes[bi[on]], bbox_t[on])):
        raise AssertionError(f'{label}: box_idx does not name the box whose label and parameters were written')
    return kt


# ------------------------------------------------------------------------------------------------------------------ predict
def check_scores(label, ho, C, scores, maxs, stats, cls='predict_scores'):
    """ho (n, ldh) as read, scores (n, C), maxs (n,)"""
    h = _d(ho)
    spec = torch.sigmoid(h[:, 13:13 + C]) * torch.sigmoid(h[:, :1])
    _held(label + ' scores', scores, spec, 10 * spec + TINY / U, None, cls, stats)
    if not _bits_equal(maxs, scores.max(1).values):
        raise AssertionError(f'{label}: max_scores is not the maximum of the row the kernel wrote')


def gram_schmidt(bp):
    """R(euler(M)) in f64, M = [x, y, z] the Gram-Schmidt frame of the raw 6-D output (M itself is no rotation: the 1e-8 under the norm
    leaves |y| = 1 - 1e-8 / |y_raw|; the reference goes through the angles, and so does this), with the conditioning c and rho"""
    xr, yr = bp[:, 6:9], bp[:, 9:12]
    y = yr / (yr.norm(dim=1, keepdim=True) + 1e-8)
    zc = torch.linalg.cross(xr, y)
    z = zc / (zc.norm(dim=1, keepdim=True) + 1e-8)
    x = torch.linalg.cross(y, z)
    c = xr.norm(dim=1) * y.norm(dim=1) / zc.norm(dim=1).clamp(min=1e-300)
    rho = torch.sqrt((1 - y[:, 2] ** 2).clamp(min=1e-300))
    e = torch.stack([torch.atan2(-y[:, 0], y[:, 1]), torch.asin(y[:, 2].clamp(-1, 1)), torch.atan2(-x[:, 2], z[:, 2])], 1)
    return _fcaf_rot(e)[0], c, rho


def check_decode_boxes(label, pts, bbox, idx, out, stats, cls='decode_boxes'):
    """pts (n, 3), bbox (n, 12), idx (m,) long or None, out (m, 9)"""
    sel = torch.arange(out.shape[0], device=out.device) if idx is None else idx.long()
    p, b = _d(pts)[sel], _d(bbox)[sel]
    size = b[:, 0:6:2] + b[:, 1:6:2]
    _held(label + ' size', out[:, 3:6], size, size.abs(), None, f'{cls} size', stats)
    Mf, c, rho = gram_schmidt(b)
    R, _, _ = _fcaf_rot(_d(out[:, 6:9]))
    eR = 64 * (1 + c) / rho
    _held(label + ' rotation', R.reshape(-1, 9), Mf.reshape(-1, 9), eR[:, None].expand(-1, 9), None, f'{cls} rotation', stats)
    sh = (b[:, 1:6:2] - b[:, 0:6:2]) / 2
    spec = p + (Mf @ sh[:, :, None])[:, :, 0]
    bnd = 32 * (p.abs() + (Mf.abs() @ (size.abs() / 2)[:, :, None])[:, :, 0]) + eR[:, None] * sh.abs().sum(1, keepdim=True)
    _held(label + ' centre', out[:, :3], spec, bnd, None, f'{cls} centre', stats)


def nms_margin(boxes, scores, thr):
    """oracle.predict.nms3d's greedy loop on (score descending, index ascending), returning the keep list and the smallest |IoU - thr|
    it met (host tensors)"""
    from oracle import predict as PR
    order = torch.argsort(scores, descending=True, stable=True).tolist()
    b = boxes.double().numpy()
    keep, margin = [], math.inf
    for i in order:
        ok = True
        for j in keep:
            v = PR.iou_bev(b[j], b[i])
            margin = min(margin, abs(v - thr))
            if v > thr:
                ok = False
                break
        if ok:
            keep.append(i)
    return keep, margin


def nms_aligned(boxes, scores, thr):
    """the same greedy loop with the closed-form IoU of axis-aligned footprints (heading 0), vectorised: the M = 4096 case"""
    b = boxes.double().numpy()
    order = torch.argsort(scores, descending=True, stable=True).numpy()
    lo, hi = b[:, :2] - b[:, 3:5] / 2, b[:, :2] + b[:, 3:5] / 2
    area = b[:, 3] * b[:, 4]
    alive = np.ones(len(order), bool)
    keep, margin = [], math.inf
    for k, i in enumerate(order):
        if not alive[k]:
            continue
        keep.append(int(i))
        rest = order[k + 1:]
        inter = np.prod(np.clip(np.minimum(hi[i], hi[rest]) - np.maximum(lo[i], lo[rest]), 0, None), -1)
        iou = inter / np.maximum(area[i] + area[rest] - inter, 1e-8)
        live = alive[k + 1:]
        if live.any():
            margin = min(margin, float(np.abs(iou[live] - thr).min()))
        alive[k + 1:] &= ~(iou > thr)
    return keep, margin


def aligned_iou_bev(a, b):
    """closed-form footprint IoU of two boxes with heading 0 (numpy rows)"""
    w = np.clip(np.minimum(a[:2] + a[3:5] / 2, b[:2] + b[3:5] / 2) - np.maximum(a[:2] - a[3:5] / 2, b[:2] - b[3:5] / 2), 0, None)
    inter = w[0] * w[1]
    return inter / max(a[3] * a[4] + b[3] * b[4] - inter, 1e-8)


def check_nms(label, boxes, scores, score_thr, iou_thr, keep_idx, keep_cnt, sent, aligned=False):
    """host tensors; keep_idx (C, M) pre-filled with `sent`; returns (kept total, smallest margin)"""
    M, C = scores.shape
    thr32 = float(torch.tensor(iou_thr, dtype=torch.float32))
    total, margin = 0, math.inf
    for c in range(C):
        ids = torch.nonzero(scores[:, c] > float(torch.tensor(score_thr, dtype=torch.float32))).squeeze(1)
        keep, mg = (nms_aligned if aligned else nms_margin)(boxes[ids], scores[ids, c], thr32) if ids.numel() else ([], math.inf)
        want = ids[torch.tensor(keep, dtype=torch.long)].tolist() if keep else []
        n = int(keep_cnt[c])
        got = keep_idx[c, :max(n, 0)].tolist()
        if got != want:
            k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            raise AssertionError(f'{label}: class {c}: kept {len(got)} boxes, the oracle {len(want)}; first difference at position {k} '
                                 f'({got[k:k + 3]} vs {want[k:k + 3]})')
        if not bool((keep_idx[c, n:] == sent).all()):
            raise AssertionError(f'{label}: class {c}: keep_idx was written beyond keep_cnt')
        total, margin = total + n, min(margin, mg)
    return total, margin


# ------------------------------------------------------------------------------------------------------------------ occupancy
def check_occ_targets(label, occ, ratio, dims, mask, gt):
    """host tensors: occ (n, 4) int32, dims (X, Y, Z) of the level, mask (X r, Y r, Z r) uint8 / bool or None, gt (X Y Z,) int32"""
    from oracle import occ as OO
    X, Y, Z = dims
    o = occ.long()
    q = torch.div(o[:, :3], ratio, rounding_mode='trunc')
    ok = ((q >= 0) & (q < torch.tensor([X, Y, Z]))).all(1)
    pooled = None
    if mask is not None:
        pooled = [torch.nn.functional.max_pool3d(mask.float()[None], ratio, stride=ratio)[0].bool()]
    want = OO.occ_multiscale_supervision([o[ok]], ratio, (1, 0, X, Y, Z), pooled)[0].reshape(-1)
    if not torch.equal(gt.long(), want):
        bad = torch.nonzero(gt.long() != want).squeeze(1)
        raise AssertionError(f'{label}: {bad.numel()} voxels differ from the reference\'s supervision (first: voxel {int(bad[0])} holds '
                             f'{int(gt[bad[0]])}, want {int(want[bad[0]])})')


def occ_coeffs(stats, C, weight):
    """stage 2 in f64 (numpy) on the stored statistics: dict(out (4,), alpha, beta, gamma (C,), ce_scale); beta = dL / dB_c, the split
    form the kernel used to emit (kept for the checker's own test)"""
    s = np.asarray(stats, np.float64)
    A, B, N, n, CE = s[:C], s[C:2 * C], s[2 * C:3 * C], s[3 * C], s[3 * C + 1]

    def bce1(v):
        with np.errstate(divide='ignore'):
            return -max(math.log(v) if v > 0 else -math.inf, -100.0)

    def dbce1(v):
        return (v - 1.0) / max((1.0 - v) * v, 1e-12)
    alpha, beta, gamma = np.zeros(C), np.zeros(C), np.zeros(C)
    loss, count = 0.0, 0.0
    for c in range(C):
        if N[c] > 0:
            count += 1
            if A[c] > 0:
                pr = B[c] / A[c]
                loss += bce1(pr)
                g = dbce1(pr)
                alpha[c] += -g * B[c] / A[c] ** 2
                beta[c] += g / A[c]
                gamma[c] += g * (A[c] - B[c]) / A[c] ** 2
            rc = B[c] / N[c]
            loss += bce1(rc)
            beta[c] += dbce1(rc) / N[c]
            gamma[c] += dbce1(rc) / N[c]
            rest = n - N[c]
            if rest > 0:
                sp = (rest - (A[c] - B[c])) / rest
                loss += bce1(sp)
                g = dbce1(sp)
                alpha[c] += -g / rest
                beta[c] += g / rest
    sem = loss / count if count else 0.0
    if count:
        alpha, beta, gamma = alpha / count, beta / count, gamma / count
    eps = 1e-6
    inter = (n - N[0]) - (A[0] - B[0])
    D, R, S = n - A[0] + eps, n - N[0] + eps, N[0] + eps
    Pp, Rc, Sp = inter / D, inter / R, B[0] / S
    gP, gR, gS = dbce1(Pp), dbce1(Rc), dbce1(Sp)
    alpha[0] += gP * (inter - D) / D ** 2 - gR / R
    beta[0] += gP / D + gR / R + gS / S
    gamma[0] += gP * inter / D ** 2 + gS / S
    geo = bce1(Pp) + bce1(Rc) + bce1(Sp)
    with np.errstate(divide='ignore', invalid='ignore'):
        ce = CE / n
        ce_scale = np.float64(weight) / n
    w = float(weight)
    return dict(out=np.array([ce, sem, geo, (ce + sem + geo) * w]), alpha=alpha * w, beta=beta * w, gamma=gamma * w, ce_scale=float(ce_scale))


def occ_ref_f32(logits, gt, C, weight, split=False):
    """f32 torch evaluation (CPU) of both stages: (stats f64, out (4,) f32, dlogits); split = the gradient from f32(alpha) + f32(beta),
    the form that loses gamma when the two cancel"""
    x = logits[:, :C].float()
    t = gt.long()
    un = t != 255
    m = x.max(1, keepdim=True).values
    e = torch.exp(x - m)
    s = e.sum(1, keepdim=True)
    p = e * (torch.tensor(1.0) / s)
    lse = (m + torch.log(s))[:, 0]
    oh = (t[:, None] == torch.arange(C)[None]) & un[:, None]
    pd = p.double() * un[:, None]
    stats = torch.zeros(3 * C + 2, dtype=F64)
    stats[:C], stats[C:2 * C], stats[2 * C:3 * C] = pd.sum(0), (pd * oh).sum(0), oh.double().sum(0)
    stats[3 * C] = float(un.sum())
    stats[3 * C + 1] = (lse - x.gather(1, t.clamp(max=C - 1)[:, None])[:, 0]).double()[un].sum()
    k = occ_coeffs(stats.numpy(), C, weight)
    al = torch.from_numpy(k['alpha']).float()
    ga = (al + torch.from_numpy(k['beta']).float()) if split else torch.from_numpy(k['gamma']).float()
    g = torch.where(oh, ga[None], al[None])
    dot = (p * g).sum(1, keepdim=True)
    cs = torch.tensor(k['ce_scale']).float()
    d = p * (g - dot) + cs * (p - oh.float())
    d = torch.where(un[:, None], d, torch.zeros(1))
    out = torch.from_numpy(k['out']).float()
    return stats, out, d


def _softmax_parts(logits, C, dev):
    x = _d(logits, dev)[:, :C]
    m = x.max(1, keepdim=True).values
    p = torch.softmax(x, 1)
    r = 6 + 2 * (x - m).abs()
    return x, m, p, r


def check_occ_stats(label, logits, gt, C, stats_got, dev, st, cls='occ_loss stats'):
    """stage 1: the stored (3 C + 2,) f64 statistics against f64 softmax sums"""
    x, m, p, r = _softmax_parts(logits, C, dev)
    t = gt.to(dev).long()
    un = (t != 255)
    oh = (t[:, None] == torch.arange(C, device=dev)[None]) & un[:, None]
    pu = p * un[:, None]
    got = _d(stats_got, dev)
    sq = math.sqrt(C)
    for name, lo, wgt in (('A', 0, pu), ('B', C, pu * oh)):
        _held(f'{label} {name}', got[lo:lo + C], wgt.sum(0), (wgt * r).sum(0) + G * sq * wgt.sum(0), None, f'{cls} {name}', st)
    if not torch.equal(got[2 * C:3 * C], oh.double().sum(0)) or float(got[3 * C]) != float(un.sum()):
        raise AssertionError(f'{label}: the class counts N_c / n_mask are not exact')
    lse = torch.logsumexp(x, 1)
    tin = un & (t >= 0) & (t < C)
    xt = x.gather(1, t.clamp(min=0, max=C - 1)[:, None])[:, 0]
    ce = torch.where(tin, lse - xt, torch.zeros_like(lse))
    e = torch.where(tin, 4 * (lse - m[:, 0]).abs() + 2 * lse.abs() + xt.abs() + ce.abs() + G * sq, torch.zeros_like(lse))
    _held(f'{label} CE', got[3 * C + 1:], ce.sum().reshape(1), e.sum().reshape(1) + TINY / U, None, f'{cls} CE', st)


def check_occ_stage2(label, logits, gt, C, weight, stats_got, out, total0, total1, dlogits, dev, st, cls='occ_loss'):
    """stage 2 on the stored statistics: out (4,), total_acc before / after (floats or None), dlogits (n, C) view or None"""
    k = occ_coeffs(stats_got.detach().cpu().numpy(), C, weight)
    want = torch.from_numpy(k['out']).to(dev)
    got = _d(out, dev)
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        raise AssertionError(f'{label}: losses {got.tolist()} and specification {want.tolist()} are not NaN in the same places')
    _held(f'{label} losses', torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want),
          2 * torch.where(nan, torch.zeros_like(want), want).abs(), None, f'{cls} values', st)
    if total1 is not None and not bool(nan[3]):
        _held(f'{label} total_acc', torch.tensor([float(total1)], dtype=F64, device=dev), torch.tensor([float(total0)], dtype=F64, device=dev) + got[3:4],
              (got[3:4].abs() + abs(float(total0))), None, f'{cls} total_acc', st)
    if dlogits is None:
        return k
    x, m, p, r = _softmax_parts(logits, C, dev)
    t = gt.to(dev).long()
    un = t != 255
    oh = (t[:, None] == torch.arange(C, device=dev)[None]) & un[:, None]
    got = dlogits.to(dev)
    if not bool((got[~un] == 0).all()):
        raise AssertionError(f'{label}: the gradient of an ignored voxel is not an exact zero')
    if not bool(un.any()):
        return k
    al, ga = torch.from_numpy(k['alpha']).to(dev), torch.from_numpy(k['gamma']).to(dev)
    g = torch.where(oh, ga[None], al[None])
    cs = k['ce_scale']
    dot = (p * g).sum(1, keepdim=True)
    spec = p * (g - dot) + cs * (p - oh.double())
    pg = (p * g.abs())
    S1 = pg.sum(1, keepdim=True)
    bu = p * ((r + 4) * g.abs() + (pg * r).sum(1, keepdim=True) + S1 * (r + 6)) + abs(cs) * ((r + 3) * p + 3 * oh.double())
    bu = bu + G * math.sqrt(C) * (p * (g.abs() + 3 * S1) + abs(cs) * p) + TINY / U
    u2 = un[:, None].expand_as(spec)
    _held(f'{label} dlogits', torch.where(u2, got.to(F64), torch.zeros_like(spec)), torch.where(u2, spec, torch.zeros_like(spec)),
          torch.where(u2, bu, torch.zeros_like(bu)), None, f'{cls} dlogits', st)
    return k
