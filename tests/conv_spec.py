"""The forward / data-gradient convolution launchers (spconv_fwd_bf16_impl behind es_spconv_fwd_bf16 / _ws / _affine / _io, es_spconv_fwd,
es_gen_transpose_fwd_bf16 / es_gen_transpose_dgrad_bf16, es_spconv_halo_bf16 of csrc/spconv.hip and csrc/halo.hip), specified in f64, the
per-element bound they are held to, and a restatement of the launch plan.  Nothing here imports the product.

Value.   conv[j] = sum_k r(X[nbr[j, k]]) r(W[k]) over the taps with nbr[j, k] >= 0; without a map row j reads row j if j < n_in, else
         nothing.  r = round-to-nearest-even to bf16 (exact on a bf16 shadow), the identity for es_spconv_fwd.
           plain                  prior * accumulate + conv + bias
           affine / io, act 0-2   act(scale conv + shift + res), res read as stored (f32 or bf16)
           act 3 (the gate)       scale conv (+ shift if given) where res > 0, else exactly 0.0
           bf16 Y                 the above, rounded once
Bound.   per element |y - spec| <= G u sqrt(n) (|scale| A + |bias|) + u (|shift| + |res| + |prior|) (+ 1 bf16 ulp of spec for bf16 rows),
         A the same gather-GEMM on absolute values, n the reduction length OF THAT ROW (pairs x Cin), G and u those of fwd_spec.  Nothing
         depends on 1 / |spec| and no element is exempt: where the bound is 0 (a row without a pair, no bias / shift / res) the output
         must be 0.0, or the prior bit for bit.  A tap-split launch adds `split` partial sums in slice order; no slack is granted for it
         (the measured ratios in Stats show that none is needed).
Plan.    plan_fwd restates the branch spconv_fwd_bf16_impl takes from the operand kinds, leading dimensions, pointer alignment, shape,
         epilogue, workspace and the es_set_option values: (tile kernel, split factor, reducer).  split_workspace_floats and is_fast
         restate es_spconv_split_workspace_floats and es_spconv_bf16_is_fast."""
import collections
import math

import torch

from fwd_spec import F64, G, U, _act, _act_slack, gather_gemm, ulp_bf16

Plan = collections.namedtuple('Plan', 'kernel split reducer')

# es_set_option defaults of csrc/spconv.hip: key -> value
DEFAULTS = {1: 1, 3: 1, 8: 384, 10: 2, 11: 768, 12: 0, 13: 1, 16: 0, 19: 0, 20: 0, 21: 1, 23: 1, 24: 256, 25: 65536, 26: 1024}
SPLIT_TICKETS = 1024
MAXK = 27
BM = 128
RG320_MIN_ROWS = 16384


def cdiv(a, b):
    return -(-a // b)


def split_factor(n_out, K, cout, opts=DEFAULTS):
    wgs = cdiv(n_out, BM) * (cout // 128 if cout % 128 == 0 else cout // 64)
    split = 1
    while split < 8 and wgs * split < opts[8] and split * 3 <= K:
        split *= 2
    return split


def split_workspace_floats(n_out, K, cin, cout, opts=DEFAULTS):
    if K <= 1 or cin % 32 or cout % 64 or n_out <= 0:
        return 0
    split = split_factor(n_out, K, cout, opts)
    return SPLIT_TICKETS + split * n_out * cout if split > 1 else 0


def is_fast(n_in, ldx, K, cin, cout):
    return int(cin % 32 == 0 and ldx % 8 == 0 and cout % 64 == 0 and n_in * ldx < (1 << 31) and K * cout * cin < (1 << 31))


def launch(**kw):
    """the attributes of a launch plan_fwd looks at.  *_mod: the pointer modulo 16 bytes; bias / scale / shift / res: operand given"""
    L = dict(xh=0, yh=0, rh=0, ldx=None, ldy=None, ldr=0, x_mod=0, w_mod=0, y_mod=0, r_mod=0, sc_mod=0, b_mod=0, has_map=True, n_out=0,
             n_in=0, K=1, cin=0, cout=0, bias=False, scale=False, shift=False, res=False, act=0, acc=0, ws_floats=0, ws_mod=0)
    assert set(kw) <= set(L), set(kw) - set(L)
    L.update(kw)
    return L


def plan_fwd(L, opts=DEFAULTS):
    """-> Plan(tile kernel, split factor (gridDim.z), reducer: None / 'k_sum_splits' / 'k_sum_splits4' / 'split_tail')"""
    xh, yh, rh, ldx, ldy, ldr = L['xh'], L['yh'], L['rh'] and L['res'], L['ldx'], L['ldy'], L['ldr']
    n_out, n_in, K, cin, cout = L['n_out'], L['n_in'], L['K'], L['cin'], L['cout']
    res, act, acc = L['res'], L['act'], L['acc']
    ax = 8 if xh else 4
    fast = (cin % 32 == 0 and ldx % ax == 0 and L['x_mod'] == 0 and L['w_mod'] == 0 and n_in * ldx < (1 << 31) and
            K * cout * cin < (1 << 31) and cout % 64 == 0)
    if (opts[3] and K == 1 and not L['has_map'] and n_in >= n_out and cin % 8 == 0 and cout % 16 == 0 and ldx % ax == 0 and ldy % 4 == 0 and
            L['x_mod'] == 0 and L['w_mod'] == 0 and L['y_mod'] % (8 if yh else 16) == 0 and
            (not res or (ldr % 4 == 0 and L['r_mod'] % (8 if rh else 16) == 0))):
        wide = cout % 128 == 0 and cin >= opts[12] and cdiv(n_out, BM) * (cout // 128) >= opts[19]
        if (opts[25] and xh and yh and L['scale'] and L['shift'] and not L['bias'] and not acc and act in (0, 1) and (not res or rh) and
                cout == 4 * cin and cin in (16, 32, 64) and n_out >= opts[25] and ldx % 8 == 0 and ldy % 8 == 0 and
                (not res or (ldr % 8 == 0 and L['r_mod'] == 0)) and L['y_mod'] == 0 and L['sc_mod'] == 0 and
                n_out * max(ldy, ldx) < (1 << 31)):
            return Plan(f'k_expand_bf16<{cin}>', 1, None)
        if (opts[24] and not xh and not yh and not L['scale'] and not res and not act and cout % 64 == 0 and cin >= 64 and
                cdiv(n_out, BM) * cdiv(cout, 128) < opts[24] and L['y_mod'] == 0 and (not L['bias'] or L['b_mod'] == 0)):
            return Plan('k_lin_small', 1, None)
        whole = bool(opts[23] and cout == 320 and n_out >= RG320_MIN_ROWS and not res and not acc and not yh and opts[13] and L['y_mod'] == 0)
        nt = 320 if whole else 128 if wide else 64 if cout % 64 == 0 else 32 if cout % 32 == 0 else 16
        g2 = (opts[13] and nt >= 32 and ldy % (8 if yh else 4) == 0 and L['y_mod'] == 0 and
              (not res or (ldr % (8 if rh else 4) == 0 and L['r_mod'] == 0)))
        return Plan(f"k_rowgemm{'2' if (whole or g2) else ''}_bf16<{nt}>", 1, None)
    split = 1
    if fast and not (L['scale'] or res or act) and K > 1 and not yh:
        s = split_factor(n_out, K, cout, opts)
        tiles = cdiv(n_out, BM) * (cout // 128 if cout % 128 == 0 else cout // 64)
        if s > 1 and L['ws_floats'] >= SPLIT_TICKETS + s * n_out * cout and tiles <= SPLIT_TICKETS and L['ws_mod'] == 0:
            split = s
    bnt = 128 if cout % 128 == 0 else 64
    t = ('false', 'true')
    if fast and opts[10] and xh and cin >= opts[11]:
        kernel = f'k_spconv_bf16_dma<{bnt}, 1, 3>' if opts[10] == 3 else f'k_spconv_bf16_dma<{bnt}, {2 if (opts[10] == 2 and cin % 64 == 0) else 1}>'
    elif fast:
        kernel = f'k_spconv_bf16_fast<{bnt}, {t[bool(xh)]}, {t[bool(opts[1])]}>'
    else:
        kernel = f'k_spconv_bf16<{128 if cout >= 128 else 64}>'
    reducer = None
    if split > 1:
        reducer = 'split_tail' if opts[16] else ('k_sum_splits4' if (cout % 4 == 0 and ldy % 4 == 0 and L['y_mod'] == 0) else 'k_sum_splits')
    return Plan(kernel, split, reducer)


def plan_f32(has_map, K, cin, cout, trans_w, opts=DEFAULTS):
    """es_spconv_fwd: the narrow 3 -> 64 kernel or the exact-f32 tile"""
    if not trans_w and opts[21] and has_map and K == 27 and cin == 3 and cout == 64:
        return Plan('k_spconv_narrow_fwd<3>', 1, None)
    return Plan(f"k_spconv<{'true' if trans_w else 'false'}>", 1, None)


def plan_gen_transpose(ncol, kred, ldx, ldy, mods, dgrad, cout):
    """es_gen_transpose_fwd_bf16 (ncol = Cout, kred = Cin, ldy = 8 Cout) / _dgrad_bf16 (ncol = Cin, kred = Cout, ldx = 8 Cout):
    None where the launcher answers 1 (not served).  mods: X | W | Y pointers modulo 16, OR-ed"""
    z_y_bytes, a_tap, w_tap, z_w = (0, cout, kred * ncol, 0) if dgrad else (cout * 4, 0, 0, ncol * kred)
    if ncol % 32 or kred % 8 or ldx % 4 or ldy % 4 or mods or ((z_y_bytes | (a_tap * 4)) & 15) or ((w_tap | z_w) % 8):
        return None
    return Plan(f'k_rowgemm2_bf16<{128 if ncol % 128 == 0 else 64 if ncol % 64 == 0 else 32}, MT>', 1 if dgrad else 8, None)


# ---------------------------------------------------------------------------------------------------------------- value and bound
def operand(t, rounded=True):
    """the f64 values a launch multiplies: f32 rows (rounded to bf16 when `rounded`) or bf16 rows / weights (exact)"""
    if t.dtype == torch.bfloat16 or not rounded:
        return t.to(F64)
    return t.to(torch.bfloat16).to(F64)


def pairs_per_row(nbr, n_out, n_in):
    if nbr is None:
        return (torch.arange(n_out) < n_in).to(F64)
    return (nbr[:n_out] >= 0).sum(1).to(F64)


def conv(x, w, nbr, n_out, n_in):
    """x (>= n_in rows, Cin), w (K, Cin, Cout): f64 operands; nbr (n_out, K) integer tensor or None -> conv, A (n_out, Cout), pairs (n_out,)"""
    x = x[:n_in]                                                      # (rows no pair names may hold NaN: they are never read here)
    assert nbr is None or int(nbr.max()) < n_in
    return gather_gemm(x, w, nbr, n_out), gather_gemm(x.abs(), w.abs(), nbr, n_out), pairs_per_row(nbr, n_out, n_in).to(x.device)


class Stats:
    """per tile kernel (and reducer): case count, worst bound ratio, worst relative L2"""

    def __init__(self, label):
        self.label, self.count, self.ratio, self.rel = label, {}, {}, {}

    def note(self, cls, ratio, rel):
        self.count[cls] = self.count.get(cls, 0) + 1
        self.ratio[cls] = max(self.ratio.get(cls, 0.0), ratio)
        self.rel[cls] = max(self.rel.get(cls, 0.0), rel)

    def worst(self):
        return max(self.ratio.values(), default=0.0)

    def report(self):
        lines = [f'{self.label}: {sum(self.count.values())} launches checked']
        for cls in sorted(self.ratio, key=str):
            lines.append(f'  {cls}: {self.count[cls]} launches, worst (|y - spec| - slack) / (u sqrt(n) A) = {self.ratio[cls]:.3f} '
                         f'(bound {G:g}), worst rel-L2 {self.rel[cls]:.2e}')
        return '\n'.join(lines)


def _row(v, dev):
    return None if v is None else v.to(dev).to(F64).reshape(1, -1)


def specify(cv, A, pairs, cin, bias=None, scale=None, shift=None, res=None, act=0, prior=None, out_bf16=False):
    """-> (spec, lin, slack): the bound is G lin + slack.  cv, A, pairs from conv(); bias / scale / shift per column, res / prior
    (n_out, Cout) as stored, or None"""
    dev = cv.device
    n = (pairs * cin).clamp(min=1).view(-1, 1)
    b, sc, sh = _row(bias, dev), _row(scale, dev), _row(shift, dev)
    r = res.to(dev).to(F64) if res is not None else None
    p = prior.to(dev).to(F64) if prior is not None else None
    lin = U * torch.sqrt(n) * ((sc.abs() if sc is not None else 1.0) * A + (b.abs() if b is not None else 0.0))
    pre = cv + (b if b is not None else 0.0)
    if sc is not None:
        pre = sc * pre + (sh if sh is not None else 0.0)
    extra = (sh.abs() if (sc is not None and sh is not None) else torch.zeros((), dtype=F64, device=dev)).expand_as(cv).clone()
    if act == 3:
        open_ = r > 0
        spec = torch.where(open_, pre, torch.zeros_like(pre))
        lin, extra = lin * open_, extra * open_
    else:
        if r is not None:
            pre = pre + r
            extra = extra + r.abs()
        spec = _act(pre, act)
        extra = extra + _act_slack(pre, spec, act)
    if p is not None:
        spec = spec + p
        extra = extra + p.abs()
    slack = U * extra + (ulp_bf16(spec) if out_bf16 else 0.0)
    return spec, lin, slack


def check(label, got, spec, lin, slack, prior=None, cls=None, stats=None, g=G):
    """got (n_out, Cout) f32 or bf16.  Raises AssertionError on the first violated element; -> the worst (|err| - slack) / lin"""
    got64 = got.to(F64)
    err = (got64 - spec).abs()
    bound = g * lin + slack
    bad = ~(err <= bound)                                              # (a NaN fails)
    dead = bound == 0
    if bool(dead.any()) and prior is not None:                          # nothing may have been added: the prior bit for bit
        bad = bad | (dead & (got.view(torch.int32) != prior.to(got.device).view(torch.int32)))
    if bool(bad.any()):
        over = torch.where(bad, torch.nan_to_num(err - bound, nan=math.inf, posinf=math.inf), torch.full_like(err, -math.inf))
        i = int(torch.argmax(over.reshape(-1)))
        C = got.shape[1]
        what = ('an element without any contribution is not exactly ' + ('the prior' if prior is not None else 'its specified value')
                if bool(dead.reshape(-1)[i]) else 'per-element bound exceeded')
        raise AssertionError(f'{label}: {what} at (row {i // C}, col {i % C}): got {float(got64.reshape(-1)[i]):.9g}, spec '
                             f'{float(spec.reshape(-1)[i]):.9g}, |err| {float(err.reshape(-1)[i]):.3e} > bound '
                             f'{float(bound.reshape(-1)[i]):.3e} ({int(bad.sum())} of {bad.numel()} elements)')
    pos = lin > 0
    ratio = float(((err - slack).clamp(min=0)[pos] / lin[pos]).max()) if bool(pos.any()) else 0.0
    rel = float((got64 - spec).norm() / (spec.norm() + 1e-300))
    if stats is not None:
        stats.note(cls, ratio, rel)
    return ratio


def gen_transpose_fwd(x, w):
    """x (n, Cin), w (8, Cin, Cout) f64 -> y, A (n, 8 Cout): y[i, t Cout : (t + 1) Cout] = x[i] w[t]"""
    return torch.cat([x @ w[t] for t in range(8)], 1), torch.cat([x.abs() @ w[t].abs() for t in range(8)], 1)


def gen_transpose_dgrad(dy, w):
    """dy (n, 8 Cout), w (8, Cin, Cout) f64 -> dX, A (n, Cin): dX[i] = sum_t dy[i, t Cout ...] w[t]^T"""
    cout = w.shape[2]
    dx = sum(dy[:, t * cout:(t + 1) * cout] @ w[t].t() for t in range(8))
    A = sum(dy[:, t * cout:(t + 1) * cout].abs() @ w[t].abs().t() for t in range(8))
    return dx, A
