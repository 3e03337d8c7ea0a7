"""Specifications of the row operators' launches that tests/fwd_spec.py does not cover -- the backward passes of norm / affine_act /
max pooling / FPN upsampling / the head's distance decode, and the exact or bounded forward helpers -- evaluated in f64 (or as an
exact f32 expression) on the operands each launch actually received: the SAVED mean / invstd, the STORED activation y, what an
output held before an accumulating launch.  Used by tests/test_gpu_rowops.py (MI355X) and tests/test_emu_rowops.py (the same bodies
on the CPU emulator).  u = 2^-24, G = 8 (fwd_spec); every bound is per element and none depends on 1 / |spec|.

Norm backward, per segment s of n_s rows (k_norm_bwd_stats / _finalize / _apply(4), k_norm_bwd_cb):
  dz = dy act'(y)   (ReLU: y > 0; ELU: y > 0 ? 1 : y + 1, on the stored y),   xh = (x - mean_s) invstd_s
  Sd = sum dz,  Sq = sum dz xh,  dx (+)= w invstd (dz - Sd / n_s - xh Sq / n_s),  dbias += sum_s Sd,  dweight += sum_s Sq
  The sums are f32 partials (a thread's rows, then a workgroup's) combined in f64: G u sqrt(n_s) sum|.| as in fwd_spec.
  dbias:   G u sum_s sqrt(n_s) sum|dz| + u |prior|
  dweight: sum_s (G sqrt(n_s) + 3) u sum|dz xh| + u |prior|      (+3: the f32 xh and the product dz xh, three roundings a term)
  dx:      |w| invstd [8 u (|dz| + |Sd| / n + |xh Sq| / n) + G u sqrt(n) / n (sum|dz| + |xh| sum|dz xh|)] + u |prior|
           (8 u: the ELU dz (2 u), xh (2 u), 1 / n, the two subtractions, the two scalings and the accumulation, each relative to
           a sum of the absolute terms; the G term carries the error of Sd and Sq into every row)
  dy must hold dz afterwards (the residual's gradient): bit for bit for act 0 / 1, within 2 u (1 + u) |dz| for ELU
  (two roundings: y + 1 and the product).  dx_bf16 is the RNE cast of dx, bit for bit.
affine_act backward: dz = dy act'(y) (the _yh variant reads the mask from the stored bf16 y), dx (+)= dz scale, dres (+)= dz.
  Each written element is held to 2 u (|term| + |prior|) -- one rounding for the product, one for the accumulation -- plus
  2 u |term| on ELU's negative side (the roundings of y + 1 and of dy (y + 1)).
Exact: maxpool backward dx[arg] += dy (disjoint windows: one f32 addition per element), es_row_move, es_relu_*,
  es_upsample_nearest_add_fwd (= fine + F.interpolate(coarse, mode='nearest') in f32), es_row_max, es_row_argmax (lowest index).
Bounded sums:
  es_upsample_nearest_add_bwd: G u sqrt(k) sum|dfine| over the k fine pixels that read the coarse pixel (+ u |prior|), against
                     the adjoint of the f32 nearest rule summed in f64
  es_reg_decode_fwd: (4 + |scale reg|) u relative (the f32 product moves exp's argument by u |t|; expf itself 4 u); cols 6.. exact
  es_reg_decode_bwd: dreg[:, :6] = [b > 1e-3] dbbox b scale (2 u relative), dreg[:, 6:] = dbbox (exact),
                     dscale += sum [b > 1e-3] dbbox b reg: G u sqrt(12 n) sum|.| + u |prior|
  es_interp_scores: 8 u sum|w score| (eight products and seven additions in a fixed order)
  es_bn_fold: scale = w / sqrt(rv + eps) within 4 u |scale|; shift = b - rm scale within u (6 |rm scale| + 2 |b|)"""
import math

import torch

from fwd_spec import F64, G, U, Stats, _check_shadow, bound_check, check_affine_act, check_maxpool, check_norm  # noqa: F401

__all__ = ['Stats', 'check_norm', 'check_affine_act', 'check_maxpool', 'check_norm_bwd', 'check_affine_act_bwd',
           'check_maxpool_first_tap', 'check_maxpool_bwd', 'act_grad', 'exact', 'check_upsample_bwd', 'check_reg_decode_fwd',
           'check_reg_decode_bwd', 'check_interp_scores', 'check_bn_fold']


def _d(t, dev=None):
    return None if t is None else (t.to(dev) if dev is not None else t).to(F64)


def act_grad(dy, y, act):
    """dz = dy act'(y) in f64 on the stored activation y"""
    if act == 1:
        return torch.where(y > 0, dy, torch.zeros_like(dy))
    if act == 2:
        return torch.where(y > 0, dy, dy * (y + 1))
    return dy


def exact(label, got, want, stats=None, cls=None):
    """equal values (torch.equal: -0.0 == 0.0, NaN never equal)"""
    if not torch.equal(got, want):
        bad = (got != want)
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(f'{label}: {int(bad.sum())} elements differ from the exact specification (first at flat index {i}: '
                             f'got {float(got.reshape(-1)[i])!r}, want {float(want.reshape(-1)[i])!r})')
    if stats is not None:
        stats.note(cls or label, None, 0.0)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _seg_index(so, n, dev):
    seg = torch.zeros(n, dtype=torch.long, device=dev)
    for s in range(1, len(so) - 1):
        seg[so[s]:] = s
    return seg


def check_norm_bwd(rec, dev, stats, cls='norm_bwd'):
    """rec: x, seg_off (host list), mean / invstd (nseg, C) as saved, w, act, y (stored), dy0 (dy before), dz (dy after; None for
    an in-place launch, whose dy buffer is dx), dx0 (prior or None), dx, dw0 / dw1, db0 / db1, dxh (bf16 shadow or None)"""
    x = _d(rec['x'], dev)
    n, C = x.shape
    so = [int(v) for v in rec['seg_off']]
    nseg = len(so) - 1
    act = rec['act']
    label = f'{stats.label}: norm bwd rows {n} C={C} segments {nseg} act={act}'
    mean, inv = _d(rec['mean'], dev).view(nseg, C), _d(rec['invstd'], dev).view(nseg, C)
    w = _d(rec['w'], dev).view(1, C)
    dy0 = rec['dy0'].to(dev)
    dz = act_grad(_d(dy0), _d(rec['y'], dev), act)
    if rec.get('dz') is not None:
        got = rec['dz'].to(dev)
        if act in (0, 1):
            if not _bits_equal(got, dz.float()):
                raise AssertionError(f'{label}: dy does not hold dz = dy act\'(y) bit for bit afterwards '
                                     f'({int((got.double() != dz).sum())} elements)')
        else:
            bound_check(label + ' dz (ELU)', got, dz, torch.zeros_like(dz), 2 * (1 + U) * dz.abs(), False, f'{cls} dz', stats)
    seg = _seg_index(so, n, dev)
    cnt = torch.tensor([max(so[s + 1] - so[s], 1) for s in range(nseg)], dtype=F64, device=dev)
    rows = torch.tensor([so[s + 1] - so[s] for s in range(nseg)], dtype=F64, device=dev)
    xh = (x - mean[seg]) * inv[seg]
    dq = dz * xh
    # per-segment column sums (a loop of reductions: index_add_ onto one row is an atomic per element on the GPU)
    Sd, Sq, Ad, Aq = (torch.stack([t[so[s]:so[s + 1]].sum(0) for s in range(nseg)]) for t in (dz, dq, dz.abs(), dq.abs()))
    cn = cnt[seg][:, None]
    wi = w.abs() * inv[seg]
    spec = w * inv[seg] * (dz - Sd[seg] / cn - xh * Sq[seg] / cn)
    lin = U * wi * torch.sqrt(cn) / cn * (Ad[seg] + xh.abs() * Aq[seg])
    extra = 8 * wi * (dz.abs() + Sd[seg].abs() / cn + (xh * Sq[seg]).abs() / cn)
    if rec.get('dx0') is not None:
        p = _d(rec['dx0'], dev)
        spec, extra = spec + p, extra + p.abs()
    dx = rec['dx'].to(dev)
    bound_check(label + ' dx', dx, spec, lin, extra, False, f'{cls} dx', stats,
                [('the xh Sq / n term dropped', spec + w * inv[seg] * xh * Sq[seg] / cn),
                 ('the Sd / n term dropped', spec + w * inv[seg] * Sd[seg] / cn)])
    if rec.get('dxh') is not None:
        _check_shadow(label + ' (dx_bf16)', dx, rec['dxh'].to(dev))
    sq_n = torch.sqrt(rows)[:, None]
    if rec.get('db1') is not None:
        db0 = _d(rec['db0'], dev)
        bound_check(label + ' dbias', rec['db1'].to(dev), db0 + Sd.sum(0), U * (sq_n * Ad).sum(0), db0.abs(), False, f'{cls} dbias',
                    stats)
    if rec.get('dw1') is not None:
        dw0 = _d(rec['dw0'], dev)
        bound_check(label + ' dweight', rec['dw1'].to(dev), dw0 + Sq.sum(0), U * (sq_n * Aq).sum(0), 3 * Aq.sum(0) + dw0.abs(), False,
                    f'{cls} dweight', stats)


def check_affine_act_bwd(rec, dev, stats, cls='affine_act_bwd'):
    """rec: dy, y (f32, or the bf16 y of es_affine_act_bwd_yh), scale, act, dx0 / dx, acc_x, dres0 / dres, acc_r (None: not written)"""
    dy = _d(rec['dy'], dev)
    y = rec['y'].to(dev).to(F64)
    act = rec['act']
    C = dy.shape[1]
    label = f'{stats.label}: affine_act bwd rows {dy.shape[0]} C={C} act={act}'
    dz = act_grad(dy, y, act)
    elu = (2 * dz.abs() * (y <= 0)) if act == 2 else 0
    sc = _d(rec['scale'], dev).view(1, C)
    for name, term, acc in (('dx', dz * sc, rec.get('acc_x')), ('dres', dz, rec.get('acc_r'))):
        if rec.get(name) is None:
            continue
        spec, extra = term, 2 * term.abs() + (elu * sc.abs() if name == 'dx' else elu)
        if acc:
            p = _d(rec[name + '0'], dev)
            spec, extra = spec + p, extra + 2 * p.abs()
        extra = extra * (1 + 8 * U)                    # (the products of the first-order terms)
        bound_check(f'{label} {name}', rec[name].to(dev), spec, torch.zeros_like(spec), extra, False, f'{cls} {name}', stats,
                    [('the ReLU mask', term * (y > 0) + (rec[name + '0'].to(dev).double() if acc else 0))] if act == 2 else None)


def check_maxpool_first_tap(rec, dev, stats):
    """check_maxpool, and the argmax is the FIRST tap (in map order) that holds the maximum (a window without taps: -1)"""
    check_maxpool(rec, dev, stats)
    x, nbr = rec['x'].to(dev).float(), rec['nbr'].to(dev).long()
    arg = rec['arg'].to(dev).long()
    n_out, K = arg.shape[0], nbr.shape[1]
    g = x[nbr[:n_out].clamp(min=0)]                              # (n_out, K, C)
    hit = (nbr[:n_out] >= 0)[:, :, None] & (g == rec['y'].to(dev)[:, None, :])
    kk = torch.arange(K, device=dev).view(1, K, 1).expand_as(hit)
    first = torch.where(hit, kk, torch.full_like(kk, K)).min(1).values   # (n_out, C)
    want = torch.where(first < K, torch.gather(nbr[:n_out], 1, first.clamp(max=K - 1)), torch.full_like(first, -1))
    if not torch.equal(arg, want):
        raise AssertionError(f'{stats.label}: maxpool argmax is not the first tap holding the maximum '
                             f'({int((arg != want).sum())} elements)')


def check_maxpool_bwd(label, dx, dx0, dy, arg, stats):
    """dx[arg[j, c], c] = dx0 + dy[j, c] (one f32 addition per element: the windows are disjoint), every other element untouched"""
    want = dx0.clone()
    live = arg >= 0
    cols = torch.arange(arg.shape[1], device=arg.device).expand_as(arg)
    r, c = arg[live].long(), cols[live]
    if torch.unique(r * arg.shape[1] + c).numel() != r.numel():
        raise AssertionError(f'{label}: two windows share an input element (the race-free precondition of k_maxpool_bwd)')
    want[r, c] = dx0[r, c] + dy[live]
    exact(label + ' maxpool bwd', dx, want, stats, 'maxpool_bwd')


def check_upsample_bwd(label, got, dfine, prior, Hc, Wc, stats):
    """dfine: (n_img, Hf, Wf, C) f32; got / prior: (n_img, Hc, Wc, C).  The adjoint of F.interpolate(mode='nearest') summed in f64,
    with the index rule of the f32 forward (the forward test holds the kernel to it bit for bit; torch's f64 interpolate on the GPU
    takes the scale in f64, which moves a pixel at adversarial widths)"""
    import torch.nn.functional as F
    NI, Hf, Wf, C = dfine.shape
    dev = dfine.device
    ids = torch.arange(Hc * Wc, dtype=torch.float32, device=dev).view(1, 1, Hc, Wc)
    src = F.interpolate(ids, size=(Hf, Wf), mode='nearest').reshape(-1).long()
    g = dfine.to(F64).reshape(NI, Hf * Wf, C)
    spec = torch.zeros((NI, Hc * Wc, C), dtype=F64, device=dev).index_add_(1, src, g).view(NI, Hc, Wc, C)
    absum = torch.zeros((NI, Hc * Wc, C), dtype=F64, device=dev).index_add_(1, src, g.abs()).view(NI, Hc, Wc, C)
    k = torch.zeros(Hc * Wc, dtype=F64, device=dev).index_add_(0, src, torch.ones(Hf * Wf, dtype=F64, device=dev)).view(1, Hc, Wc, 1)
    extra = torch.zeros_like(spec)
    if prior is not None:
        p = prior.to(F64)
        spec, extra = spec + p, p.abs()
    bound_check(label + ' upsample bwd', got, spec, U * torch.sqrt(k.clamp(min=1)) * absum, extra, False, 'upsample_bwd', stats)


def check_reg_decode_fwd(label, reg, scale, bbox, stats):
    """reg: (n, 12) f32 as the kernel read it; bbox (n, 12)"""
    t = reg[:, :6].to(F64) * scale.to(F64)
    lo = float(torch.tensor(1e-3, dtype=torch.float32))
    spec = torch.clamp(torch.exp(t), min=lo)
    bound_check(label + ' reg decode sizes', bbox[:, :6], spec, torch.zeros_like(spec), (4 + t.abs()) * spec, False, 'reg_decode_fwd',
                stats)
    exact(label + ' reg decode offsets', bbox[:, 6:], reg[:, 6:])


def check_reg_decode_bwd(label, reg, bbox, dbbox, scale, dreg, ds0, ds1, stats):
    """reg / bbox / dbbox / dreg: (n, 12) f32; scale, ds0, ds1: one-element f32 tensors"""
    b, g, r = bbox[:, :6].to(F64), dbbox[:, :6].to(F64), reg[:, :6].to(F64)
    live = bbox[:, :6] > torch.tensor(1e-3, dtype=torch.float32, device=bbox.device)
    gb = torch.where(live, g * b, torch.zeros_like(b))
    sc = float(scale.reshape(-1)[0])
    spec = gb * sc
    bound_check(label + ' dreg sizes', dreg[:, :6], spec, torch.zeros_like(spec), 2 * (1 + U) * spec.abs(), False, 'reg_decode_bwd dreg', stats,
                [('gradient through the clamped rows', g * b * sc)])
    exact(label + ' dreg offsets', dreg[:, 6:], dbbox[:, 6:])
    n = reg.shape[0]
    terms = gb * r
    d0 = float(ds0.reshape(-1)[0])
    want = torch.tensor([d0 + float(terms.sum())], dtype=F64, device=bbox.device)
    lin = torch.tensor([U * math.sqrt(12 * n) * float(terms.abs().sum())], dtype=F64, device=bbox.device)
    bound_check(label + ' dscale', ds1.reshape(1), want, lin, torch.tensor([abs(d0)], dtype=F64, device=bbox.device), False,
                'reg_decode_bwd dscale', stats)


def check_interp_scores(label, score, idx, w, out, stats):
    live = idx >= 0
    v = torch.where(live, score.to(F64)[idx.long().clamp(min=0)], torch.zeros_like(w, dtype=F64))
    p = v * torch.where(live, w.to(F64), torch.zeros_like(w, dtype=F64))
    spec = p.sum(1)
    bound_check(label + ' interp scores', out, spec, torch.zeros_like(spec), (8 + 64 * U) * p.abs().sum(1), False, 'interp_scores',
                stats)


def check_bn_fold(label, w, b, rm, rv, eps, scale, shift, stats):
    s = w.to(F64) / torch.sqrt(rv.to(F64) + float(torch.tensor(eps, dtype=torch.float32)))
    bound_check(label + ' bn fold scale', scale, s, torch.zeros_like(s), 4 * s.abs(), False, 'bn_fold scale', stats)
    sh = b.to(F64) - rm.to(F64) * scale.to(F64)                 # on the scale the kernel wrote (its error is held above)
    bound_check(label + ' bn fold shift', shift, sh, torch.zeros_like(sh), 6 * (rm.to(F64) * scale.to(F64)).abs() + 2 * b.to(F64).abs(),
                False, 'bn_fold shift', stats)
