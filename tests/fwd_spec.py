"""Forward specifications of the engine's launches (engine.DEBUG_FWD records), evaluated in f64, and the per-element bound every
matrix-core output is held to.  Used by tests/test_gpu_insitu.py (real bf16 steps) and tests/test_emu_insitu.py (emulated
launches plus mutated records that the checker must reject).

r(.) = round-to-nearest-even to bf16 where the launch rounds (record field `round`: the engine's own >= 16-channel rule).
  convolution / Linear / transposed conv:  y = sum_k r(x[nbr[:, k]]) r(W[k]) (+ bias)
  fused epilogue (conv_affine):            y = act(scale * conv + shift (+ res)), res read as stored
  stem (+ pool):                           exact-f32 7x7 s2 conv -> scale / shift -> ReLU (-> 3x3 s2 max pool) (-> bf16)
Per element, with A = sum_k |r(x)| |r(W)| (the same gather-GEMM on absolute values), n the reduction length and u = 2^-24:
  |y - spec| <= G u sqrt(n) (|scale| A + |bias|) + u (|shift| + |res|) (+ 1 bf16 ulp of spec for bf16 outputs)
(a bias may seed the accumulator: every rounding of the reduction then sees it)
G = 8 (the issue's starting point; `worst ratio` printed per launch class is the smallest G the launches of that class need).
Shadows (bf16 gather copies of rows, bf16 weight copies) must equal the cast of what they stand for, bit for bit.
Norm / LayerNorm / affine / pooling / attention / ContrastiveEmbed: see the check_* docstrings.  No bound depends on 1 / |spec|."""
import math

import torch

U = 2.0 ** -24
G = 8.0
F64 = torch.float64


def _r(t):
    return t.to(torch.bfloat16).to(F64)


def _d(t):
    return None if t is None else t.to(F64)


def ulp_bf16(t):
    """one bf16 ulp of every element of the f64 tensor t (0 where t == 0)"""
    _, e = torch.frexp(t)
    return torch.where(t != 0, torch.pow(2.0, (e - 8).to(F64)), torch.zeros_like(t))


def _act(z, act):
    if act == 1:
        return z.clamp(min=0)
    if act == 2:
        return torch.where(z > 0, z, torch.expm1(z))
    return z


def _act_slack(pre, want, act):
    """what the activation's f32 arithmetic adds, in units of u: ELU is expf(z) - 1.f in the kernels (csrc/rowops.hip act_fwd), so a
    negative z loses the absolute error of expf near 1 (a few u of 1, not of |y|: the subtraction cancels) -- 4 u absolute there,
    4 u |y| elsewhere"""
    if act != 2:
        return 0
    return 4 * want.abs() + 4 * (pre < 0)


def gather_gemm(x, w, nbr, n_out):
    """sum_k x[nbr[:, k]] @ w[k] in f64 (nbr None: the identity map, K = 1)"""
    K, cin, cout = w.shape
    y = torch.zeros((n_out, cout), dtype=F64, device=x.device)
    if nbr is None:
        m = min(n_out, x.shape[0])
        y[:m] = x[:m] @ w[0]
        return y
    nbr = nbr[:n_out].long()
    for k in range(K):
        rows = torch.nonzero(nbr[:, k] >= 0).squeeze(1)
        if rows.numel():
            y.index_add_(0, rows, x[nbr[rows, k]] @ w[k])
    return y


class Stats:
    """per entry point: record count; per launch class: worst bound ratio and worst relative L2"""

    def __init__(self, label):
        self.label = label
        self.count = {}
        self.ratio = {}
        self.rel = {}
        self.n_elems = 0

    def note(self, cls, ratio, rel):
        if ratio is not None and ratio > self.ratio.get(cls, (-1.0,))[0]:
            self.ratio[cls] = (ratio,)
        if rel is not None and rel > self.rel.get(cls, -1.0):
            self.rel[cls] = rel

    def report(self):
        lines = [f'{self.label}: {sum(self.count.values())} forward records: ' +
                 ', '.join(f'{k} {v}' for k, v in sorted(self.count.items()))]
        for cls in sorted(set(self.ratio) | set(self.rel), key=str):
            r = self.ratio.get(cls, (None,))[0]
            lines.append(f'  {cls}: worst |y - spec| / (u sqrt(n) A) = {r if r is None else f"{r:.3f}"} (bound {G:g}), '
                         f'worst rel-L2 {self.rel.get(cls, 0.0):.2e}')
        return '\n'.join(lines)


def _fail_at(label, err, bound, got, spec, extra_msg=''):
    over = (err - bound).reshape(-1)
    i = int(torch.argmax(over))
    C = got.shape[-1] if got.dim() > 1 else 1
    raise AssertionError(f'{label}: per-element bound exceeded at (row {i // C}, col {i % C}): got {float(got.reshape(-1)[i]):.8g}, '
                         f'spec {float(spec.reshape(-1)[i]):.8g}, |err| {float(err.reshape(-1)[i]):.3e} > bound '
                         f'{float(bound.reshape(-1)[i]):.3e} ({int((over > 0).sum())} elements){extra_msg}')


def bound_check(label, got, spec, lin, extra, out_bf16, cls, stats, diagnose=None):
    """assert |got - spec| <= G lin + u extra (+ ulp(spec)) element by element; lin = u sqrt(n) |scale| A.  diagnose: list of
    (name, alternative spec) -- named in the message when the offending element matches the alternative instead"""
    got = got.to(F64)
    err = (got - spec).abs()
    ulp = ulp_bf16(spec) if out_bf16 else 0.0
    slack = U * extra + ulp
    bound = G * lin + slack
    if bool((~(err <= bound)).any()):
        hint = ''
        over = (err - bound).reshape(-1)
        i = int(torch.argmax(over))
        for name, alt in (diagnose or ()):
            a = alt.reshape(-1)[i]
            if abs(float(got.reshape(-1)[i]) - float(a)) <= float(bound.reshape(-1)[i]) + (float(ulp_bf16(a)) if out_bf16 else 0.0):
                hint = f' -- the value matches the specification with {name}'
                break
        _fail_at(label, err, bound, got, spec, hint)
    pos = lin > 0
    ratio = float(((err - slack).clamp(min=0)[pos] / lin[pos]).max()) if bool(pos.any()) else 0.0
    rel = float((got - spec).norm() / (spec.norm() + 1e-300))
    stats.note(cls, ratio, rel)
    return ratio, rel


def _check_shadow(label, rows, shadow):
    """a bf16 gather shadow must be the RNE cast of the rows it stands for, bit for bit"""
    if shadow is None or rows.dtype == torch.bfloat16:
        return
    want = rows.to(torch.bfloat16)
    if not torch.equal(shadow.to(rows.device).view(torch.int16), want.view(torch.int16)):
        bad = int((shadow.to(rows.device).view(torch.int16) != want.view(torch.int16)).sum())
        raise AssertionError(f'{label}: stale shadow -- {bad} bf16 gather values differ from the cast of the rows at launch time')


def _check_weight_copy(label, rec, dev):
    if rec.get('w_h') is None:
        return
    want = rec['w'].to(dev).to(torch.bfloat16).transpose(1, 2)
    if not torch.equal(rec['w_h'].to(dev).view(torch.int16), want.contiguous().view(torch.int16)):
        raise AssertionError(f'{label}: stale bf16 weight copy -- it differs from the cast of the f32 weights')


def check_conv(rec, dev, stats):
    """conv (every dispatch branch, Linear included), conv_affine, gen_transpose, transpose_dense"""
    kind, entry = rec['kind'], rec['entry']
    x, w = rec['x'].to(dev), rec['w'].to(dev)
    K, cin, cout = w.shape
    label = f'{stats.label}: {kind} {entry} K={K} {cin}->{cout} rows {x.shape[0]}'
    _check_shadow(label, x, rec.get('xh'))
    _check_weight_copy(label, rec, dev)
    rnd = rec['round']
    xr, wr = (_r(x), _r(w)) if rnd else (_d(x), _d(w))
    n = K * cin
    y = rec['y'].to(dev)
    if kind == 'gen_transpose':
        spec = torch.stack([xr @ wr[k] for k in range(8)], 1).reshape(-1, cout)
        A = torch.stack([xr.abs() @ wr[k].abs() for k in range(8)], 1).reshape(-1, cout)
        n = cin
    elif kind == 'transpose_dense':
        B, X, Y, Z = rec['dense'][:4]
        spec = torch.zeros((B, X, 2, Y, 2, Z, 2, cout), dtype=F64, device=dev)
        A = torch.zeros_like(spec)
        xv = xr.view(B, X, Y, Z, cin)
        for k in range(8):
            spec[:, :, k >> 2, :, (k >> 1) & 1, :, k & 1] = xv @ wr[k]
            A[:, :, k >> 2, :, (k >> 1) & 1, :, k & 1] = xv.abs() @ wr[k].abs()
        spec, A = spec.reshape(-1, cout), A.reshape(-1, cout)
        n = cin
    else:
        nbr = rec['nbr'].to(dev) if rec['nbr'] is not None else None
        spec = gather_gemm(xr, wr, nbr, rec['n_out'])
        A = gather_gemm(xr.abs(), wr.abs(), nbr, rec['n_out'])
    cls = f'{kind} {entry}' + (' bf16-out' if y.dtype == torch.bfloat16 else '')
    lin = U * math.sqrt(n) * A
    if kind != 'conv_affine':
        extra = torch.zeros_like(spec)
        if rec.get('bias') is not None:
            # the bias may be the accumulator's initial value (the lane-per-output-channel kernels of csrc/spconv.hip): each of the
            # n roundings is then relative to a partial sum that includes it, so it joins A rather than the one-rounding slack
            b = _d(rec['bias'].to(dev)).reshape(1, -1)
            spec = spec + b
            lin = lin + U * math.sqrt(n) * b.abs()
        return bound_check(label, y, spec, lin, extra, False, cls, stats)
    scale, shift = _d(rec['scale'].to(dev)).reshape(1, -1), _d(rec['shift'].to(dev)).reshape(1, -1)
    res = _d(rec['res'].to(dev)) if rec.get('res') is not None else None
    pre = scale * spec + shift + (res if res is not None else 0)
    lin = lin * scale.abs()
    extra = shift.abs() + (res.abs() if res is not None else 0)
    act = rec['act']
    want = _act(pre, act)
    extra = extra + _act_slack(pre, want, act)
    out16 = y.dtype == torch.bfloat16
    diag = []
    if res is not None:
        diag.append(('the residual dropped', _act(scale * spec + shift, act)))
    diag.append(('the shift dropped', _act(scale * spec + (res if res is not None else 0), act)))
    out = bound_check(label, y, want, lin, extra, out16, cls, stats, diag)
    if act == 1:
        neg = pre < -(G * lin + U * extra)
        if bool((y.to(F64)[neg] != 0).any()):
            raise AssertionError(f'{label}: ReLU output not 0 where the specification is clearly negative '
                                 f'({int((y.to(F64)[neg] != 0).sum())} elements)')
    return out


def check_stem(rec, dev, stats):
    """ResNet stem: exact-f32 7x7 / stride 2 / pad 3 conv (f32 FMAs, csrc/data.hip) -> frozen-BN scale / shift -> ReLU, then (pooled)
    the 3x3 / stride 2 / pad 1 max pool and the bf16 rounding (one ulp).  Max pooling is 1-Lipschitz: the pooled bound is the
    window maximum of the stem bound."""
    import torch.nn.functional as F
    n_img, H, W = rec['n_img'], rec['H'], rec['W']
    x = _d(rec['x'].to(dev)).view(n_img, H, W, 3).permute(0, 3, 1, 2)
    Co = rec['scale'].numel()
    w = _d(rec['w'].to(dev)).reshape(7, 7, 3, Co).permute(3, 2, 0, 1)
    scale, shift = _d(rec['scale'].to(dev)).view(1, -1, 1, 1), _d(rec['shift'].to(dev)).view(1, -1, 1, 1)
    acc = F.conv2d(x, w, stride=2, padding=3)
    A = F.conv2d(x.abs(), w.abs(), stride=2, padding=3)
    pre = scale * acc + shift
    spec = pre.clamp(min=0)
    bound = G * U * math.sqrt(147) * scale.abs() * A + U * shift.abs().expand_as(A)
    label = f'{stats.label}: stem {rec["entry"]} {n_img} x {H} x {W} -> {Co}'
    cls = f'stem {rec["entry"]}'
    if rec['pooled']:
        spec = F.max_pool2d(spec, 3, 2, 1)
        bound = F.max_pool2d(bound, 3, 2, 1)
    to_rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, Co)
    spec, bound = to_rows(spec), to_rows(bound)
    lin = bound / G                                       # (the u |shift| term is reported inside the ratio here)
    return bound_check(label, rec['y'].to(dev), spec, lin, torch.zeros_like(spec), rec['y'].dtype == torch.bfloat16, cls, stats)


def check_norm(rec, dev, stats):
    """train-mode batch / instance norm over the segments.  Saved statistics against the f64 mean / biased variance of each segment:
    |mean - spec| <= G u sqrt(n) max(mean|x|, mean|x - x0|),  |invstd - spec| / spec <= G u sqrt(n) M2 / (var + eps) + 4 u with
    M2 = var + max(mean^2, (mean - x0)^2) (the kernels sum about the first row or about 0).  y against act(w (x - mean) invstd + b (+ res)) on the SAVED
    statistics, f32 rounding of five operations: 8 u (|w (x - mean) invstd| + |b| + |res|) (+ _act_slack).  The fused bf16 shadow equals the cast of
    y bit for bit; the running statistics follow F.batch_norm (oracle/sparse.py: unbiased variance, segments of one)."""
    x = _d(rec['x'].to(dev))
    n, C = x.shape
    so = rec['seg_off']
    label = f'{stats.label}: norm rows {n} C={C} segments {len(so) - 1}'
    mean_k, inv_k = _d(rec['mean'].to(dev)), _d(rec['invstd'].to(dev))
    for s in range(len(so) - 1):
        a, b = so[s], so[s + 1]
        if b <= a:
            continue
        xs = x[a:b]
        m = xs.mean(0)
        var = ((xs - m) ** 2).mean(0)
        inv = 1.0 / torch.sqrt(var + rec['eps'])
        cnt = b - a
        # the mean is k + sum(x - k) / n with the sum in f32 about a shift k (0, or the first row): its error is G u sqrt(n) mean|x - k|,
        # so an outlier first row widens it like the invstd bound below
        bm = G * U * math.sqrt(cnt) * torch.maximum(xs.abs().mean(0), (xs - xs[0]).abs().mean(0)) + U * m.abs()
        if bool((~((mean_k[s] - m).abs() <= bm)).any()):
            c = int(torch.argmax((mean_k[s] - m).abs() - bm))
            raise AssertionError(f'{label}: norm mean of segment {s} (rows {a}..{b}) channel {c}: {float(mean_k[s, c]):.8g}, '
                                 f'spec {float(m[c]):.8g}')
        M2 = var + torch.maximum(m ** 2, (m - xs[0]) ** 2)
        bi = G * U * math.sqrt(cnt) * M2 / (var + rec['eps']) + 4 * U
        if bool((~((inv_k[s] - inv).abs() <= bi * inv)).any()):
            c = int(torch.argmax((inv_k[s] - inv).abs() / inv - bi))
            raise AssertionError(f'{label}: norm invstd of segment {s} (rows {a}..{b}) channel {c}: {float(inv_k[s, c]):.8g}, '
                                 f'spec {float(inv[c]):.8g}')
        if rec.get('rm0') is not None and len(so) == 2 and cnt > 1:
            mo = rec['momentum']
            for nm, r0, r1, st, bst in (('running mean', rec['rm0'], rec['rm1'], m, bm),
                                        ('running var', rec['rv0'], rec['rv1'], var * cnt / (cnt - 1), 2 * bi * var * cnt / (cnt - 1))):
                r0, r1 = _d(r0.to(dev)), _d(r1.to(dev))
                want = (1 - mo) * r0 + mo * st
                if bool((~((r1 - want).abs() <= mo * bst + 4 * U * (r0.abs() + st.abs()))).any()):
                    raise AssertionError(f'{label}: {nm} update does not follow (1 - momentum) * old + momentum * batch statistic')
    # y on the saved statistics
    seg = torch.zeros(n, dtype=torch.long, device=dev)
    for s in range(1, len(so) - 1):
        seg[so[s]:] = s
    xh = (x - mean_k[seg]) * inv_k[seg]
    wv, bv = _d(rec['w'].to(dev)).view(1, -1), _d(rec['b'].to(dev)).view(1, -1)
    res = _d(rec['res'].to(dev)) if rec.get('res') is not None else None
    pre = wv * xh + bv + (res if res is not None else 0)
    want = _act(pre, rec['act'])
    extra = 8 * ((wv * xh).abs() + bv.abs() + (res.abs() if res is not None else 0)) + _act_slack(pre, want, rec['act'])
    bound_check(label, rec['y'].to(dev), want, torch.zeros_like(want), extra, False, f'norm act={rec["act"]}', stats)
    if rec.get('yh') is not None:
        _check_shadow(label + ' (fused shadow)', rec['y'].to(dev), rec['yh'])


def check_affine_act(rec, dev, stats):
    """frozen-BN affine: y = act(x scale + shift (+ res)), three f32 roundings"""
    x = _d(rec['x'].to(dev))
    sc, sh = _d(rec['scale'].to(dev)).view(1, -1), _d(rec['shift'].to(dev)).view(1, -1)
    res = _d(rec['res'].to(dev)) if rec.get('res') is not None else None
    pre = x * sc + sh + (res if res is not None else 0)
    want = _act(pre, rec['act'])
    extra = 4 * ((x * sc).abs() + sh.abs() + (res.abs() if res is not None else 0)) + _act_slack(pre, want, rec['act'])
    bound_check(f'{stats.label}: affine_act rows {x.shape[0]}', rec['y'].to(dev), want, torch.zeros_like(want), extra, False,
                'affine_act', stats)


def check_maxpool(rec, dev, stats):
    """bit-exact maximum over the valid taps (f32 rows; es_maxpool_fwd_h: its RNE bf16 cast, 0 for a window without taps); the
    argmax points at a row holding that maximum"""
    x, nbr, y = rec['x'].to(dev).float(), rec['nbr'].to(dev).long(), rec['y'].to(dev)
    n_out = y.shape[0]
    nbr = nbr[:n_out]
    g = x[nbr.clamp(min=0)]                                     # (n_out, K, C)
    g = torch.where((nbr >= 0)[:, :, None], g, torch.full_like(g, -math.inf))
    want = g.max(1).values
    label = f'{stats.label}: maxpool {rec["entry"]} rows {n_out} C={x.shape[1]}'
    if y.dtype == torch.bfloat16:
        want = torch.where(torch.isinf(want), torch.zeros_like(want), want).to(torch.bfloat16)
    if not torch.equal(y, want):
        raise AssertionError(f'{label}: max pool output differs from the maximum over the valid taps '
                             f'({int((y != want).sum())} elements)')
    if rec.get('arg') is not None:
        arg = rec['arg'].to(dev).long()
        live = arg >= 0
        cols = torch.arange(x.shape[1], device=dev).expand_as(arg)
        if not torch.equal(x[arg[live], cols[live]], y[live]) or not bool(torch.isinf(y[~live]).all()):
            raise AssertionError(f'{label}: argmax does not point at a row holding the maximum')
    stats.note(f'maxpool {rec["entry"]}', None, 0.0)


def check_layernorm(rec, dev, stats):
    """z = x (+ res) in f32 (bit-exact); mean / rstd of z against f64 (|dmean| <= G u sqrt(C) mean|z|, relative drstd <= G u sqrt(C)
    + 4 u); y = (z - mean) rstd w + b on the saved statistics, 8 u (|(z - mean) rstd w| + |b|)"""
    x = rec['x'].to(dev)
    n, C = x.shape
    label = f'{stats.label}: layernorm rows {n} C={C}'
    z = x + rec['res'].to(dev) if rec.get('res') is not None else x
    if rec.get('z') is not None and not torch.equal(rec['z'].to(dev), z):
        raise AssertionError(f'{label}: z is not x + res')
    z = _d(z)
    m = z.mean(1)
    rs = 1.0 / torch.sqrt(((z - m[:, None]) ** 2).mean(1) + rec['eps'])
    mk, rk = _d(rec['mean'].to(dev)), _d(rec['rstd'].to(dev))
    if bool((~((mk - m).abs() <= G * U * math.sqrt(C) * z.abs().mean(1) + U * m.abs())).any()):
        raise AssertionError(f'{label}: layernorm mean')
    if bool((~((rk - rs).abs() <= (G * U * math.sqrt(C) + 4 * U) * rs)).any()):
        raise AssertionError(f'{label}: layernorm rstd')
    t = (z - mk[:, None]) * rk[:, None] * _d(rec['w'].to(dev))[None]
    b = _d(rec['b'].to(dev))[None]
    want = t + b
    bound_check(label, rec['y'].to(dev), want, torch.zeros_like(want), 8 * (t.abs() + b.abs()), False, 'layernorm', stats)


def check_attention(rec, dev, stats):
    """S = r(f32(q s)) r(k)^T (s = 1 / sqrt(32)), keys >= klen masked, lse = logsumexp(S), o = softmax(S) r(V).  The kernel runs the
    online softmax: it rounds the UNNORMALISED probabilities exp(S - running max) to bf16 (relative error <= 2^-8 each: bf16 has 8 significant bits, whatever the
    running max), so o is held per element to (2^-8 + G u sqrt(Lk) + 2 dS) (P |r(V)|) with dS = G u sqrt(32) max_j (|r(qs)| |r(k)|^T)
    the error of the score GEMM; lse to dS + G u sqrt(Lk) + 4 u |lse| + 1e-6 (the fast exponential).  A sample with klen <= 0 must
    hold O = 0 and lse = -inf exactly."""
    B, H, Lq, Lk, bf = rec['B'], rec['H'], rec['Lq'], rec['Lk'], rec['bf']
    s = torch.tensor(0.17677669529663687, dtype=torch.float32)
    rr = _r if bf else _d
    hd = lambda t, L: t.to(dev).float().reshape(B, L, H, 32).permute(0, 2, 1, 3)
    qs = rr(hd(rec['q'], Lq) * s.to(dev))
    ks, vs = rr(hd(rec['k'], Lk)), rr(hd(rec['v'], Lk))
    klen = torch.full((B,), Lk, device=dev) if rec['klen'] is None else rec['klen'].to(dev).long().clamp(max=Lk)
    live = (torch.arange(Lk, device=dev)[None, :] < klen[:, None])[:, None, None, :]
    S = qs @ ks.transpose(-1, -2)
    dS = (G * U * math.sqrt(32) * (qs.abs() @ ks.abs().transpose(-1, -2)) * live).amax(-1)
    S = S.masked_fill(~live, -math.inf)
    lse = torch.logsumexp(S, -1)
    # a sample without a valid key (klen <= 0): O = 0 and lse = -inf by definition (the reference's softmax is NaN there)
    dead = (klen <= 0)[:, None, None].expand(B, H, Lq)
    P = torch.where(dead[..., None], torch.zeros_like(S), torch.exp(S - lse.masked_fill(dead, 0.0)[..., None]))
    o = P @ vs
    mag = P @ vs.abs()
    label = f'{stats.label}: attention B={B} H={H} Lq={Lq} Lk={Lk}'
    rel_p = (2.0 ** -8 if bf else 16 * U) + G * U * math.sqrt(Lk) + 2 * dS
    got = rec['o'].to(dev).double().reshape(B, Lq, H, 32).permute(0, 2, 1, 3)
    bound_check(label + ' o', got, o, torch.zeros_like(o), rel_p[..., None] * mag / U, False, 'attention o', stats)
    lk = rec['lse'].to(dev).double().view(B, H, Lq)
    if bool(dead.any()):
        if not (bool(torch.isneginf(lk[dead]).all()) and bool((got[dead] == 0).all())):
            raise AssertionError(f'{label}: a sample without a valid key must get O = 0 and lse = -inf')
        lk, lse = lk.masked_fill(dead, 0.0), lse.masked_fill(dead, 0.0)
    lb = dS + G * U * math.sqrt(Lk) + 4 * U * lse.abs() + 1e-6
    bound_check(label + ' lse', lk, lse, torch.zeros_like(lse), lb / U, False, 'attention lse', stats)


def check_contrastive(rec, dev, stats):
    """logits[b, i, t] = <v[b, i], text[b, t]> / sqrt(C) + bias (t < tlen[b], i < vlen[b]; -inf elsewhere), exact f32 formula:
    G u sqrt(C) (|v| |text|^T) / sqrt(C) + 2 u |dot| / sqrt(C) + u |bias|; rowmax is the maximum of the row's logits"""
    B, L, T = rec['B'], rec['L'], rec['T']
    v, text = _d(rec['v'].to(dev)), _d(rec['text'].to(dev))
    C = v.shape[1]
    v, text = v.view(B, L, C), text.view(B, T, C)
    inv = 1.0 / math.sqrt(C)
    bias = float(rec['bias'].reshape(-1)[0])
    dot = v @ text.transpose(1, 2)
    A = v.abs() @ text.abs().transpose(1, 2)
    tl = rec['tlen'].to(dev).long().clamp(max=T)
    vl = torch.full((B,), L, device=dev) if rec.get('vlen') is None else rec['vlen'].to(dev).long().clamp(max=L)
    live = (torch.arange(T, device=dev)[None, None, :] < tl[:, None, None]) & (torch.arange(L, device=dev)[None, :, None] < vl[:, None, None])
    want = dot * inv + bias
    label = f'{stats.label}: contrastive B={B} L={L} T={T} C={C}'
    if rec.get('logits') is not None:
        got = rec['logits'].to(dev).view(B, L, T)
        if not bool(torch.isneginf(got[~live]).all()):
            raise AssertionError(f'{label}: masked logits are not -inf')
        g = torch.where(live, got.double(), want)
        bound_check(label, g, want, U * math.sqrt(C) * A * inv, 2 * dot.abs() * inv + abs(bias), False, 'contrastive', stats)
    if rec.get('rowmax') is not None:
        wm = torch.where(live, want, torch.full_like(want, -math.inf)).amax(-1)
        am = torch.where(live, G * U * math.sqrt(C) * A * inv + U * (2 * dot.abs() * inv + abs(bias)),
                         torch.zeros_like(A)).amax(-1)
        got = rec['rowmax'].to(dev).double().view(B, L)
        fin = torch.isfinite(wm)
        if not (bool(((got - wm).abs()[fin] <= am[fin]).all()) and bool(torch.isneginf(got[~fin]).all())):
            raise AssertionError(f'{label}: rowmax is not the maximum of the row')


CHECKS = dict(conv=check_conv, conv_affine=check_conv, gen_transpose=check_conv, transpose_dense=check_conv, stem=check_stem,
              norm=check_norm, affine_act=check_affine_act, maxpool=check_maxpool, layernorm=check_layernorm,
              attention=check_attention, contrastive=check_contrastive)


class Checker:
    """engine.DEBUG_FWD = Checker(label, dev): every record checked on the spot (nothing accumulates); .stats, .report()"""

    def __init__(self, label, dev):
        self.stats = Stats(label)
        self.dev = dev

    def __call__(self, rec):
        check(rec, self.dev, self.stats)

    def report(self):
        return self.stats.report()


def check(rec, dev, stats):
    stats.count[rec['entry'] if rec['kind'] != 'norm' else 'norm'] = stats.count.get(rec['entry'] if rec['kind'] != 'norm' else 'norm', 0) + 1
    CHECKS[rec['kind']](rec, dev, stats)


def check_records(recs, label, dev):
    stats = Stats(label)
    for rec in recs:
        check(rec, dev, stats)
    return stats


def check_bias_grad(label, got, want, mag, n_rows):
    """per column: |got - want| <= G u sqrt(n_rows) sum |gy| (a column sum that cancels is held to what an f32 sum can do, not to
    1 / |want|) -> the worst ratio |got - want| / (u sqrt(n_rows) sum |gy|)"""
    err = (got.double() - want).abs()
    lin = U * math.sqrt(max(n_rows, 1)) * mag
    if bool((~(err <= G * lin)).any()):
        c = int(torch.argmax(err - G * lin))
        raise AssertionError(f'{label}: bias gradient column {c}: per-element bound exceeded, got {float(got[c]):.8g}, want '
                             f'{float(want[c]):.8g}, |err| {float(err[c]):.3e} > {float(G * lin[c]):.3e}')
    pos = lin > 0
    return float((err[pos] / lin[pos]).max()) if bool(pos.any()) else 0.0
