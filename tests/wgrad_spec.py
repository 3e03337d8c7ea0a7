"""The weight gradient of the map convolutions (es_spconv_wgrad, es_spconv_wgrad_bf16, es_spconv_wgrad_bf16_src of csrc/spconv.hip),
specified in f64, the per-element bound it is held to, and a restatement of the launch plan.  Nothing here imports the product.

Value.   dW[k] = r(X[nbr[rows_k, k]])^T . r(dY[rows_k]),  rows_k = {j < n_out : nbr[j, k] >= 0}; nbr None (the identity map):
         rows = {j < min(n_out, n_in)} for every tap.  r = round-to-nearest-even to bf16 for the bf16 entry points (exact on an operand
         that already is a bf16 shadow), the identity for es_spconv_wgrad.  accumulate: the result is prior + dW.
Bound.   per element |got - want| <= G u sqrt(max(n_k, 1)) A + u (|prior| + |want|), A the same product on absolute values, n_k the
         pair count of the tap, G and u those of fwd_spec.  Nothing depends on 1 / |want|; no element is exempt: where A == 0 (a tap
         without a pair) the output must be 0.0, or the prior bit for bit.
Plan.    plan_f32 / plan_bf16 / cap_splits restate the launchers' choice of tile, row slices and reduction kernel from the operand
         kinds, strides, pointer alignment and shape: (kind, splits, rows_per_split, reducer).  kind 0 exact-f32 64 x 64 tile, 4 the narrow
         3 -> 64 kernel, 5 k_lin_wgrad_small, 1 bf16 64 x 64, 2 bf16 128 x 128 (register-transposing or transposed-read), 3 bf16 256 x 256.
         The plan never looks at the map: without a map a kind-4 plan runs the exact-f32 tile, with a map a kind-5 plan runs the bf16
         64 x 64 tile, each on the plan's own slices (kernel_name)."""
import collections
import math

import torch

from fwd_spec import F64, G, U

Plan = collections.namedtuple('Plan', 'kind splits rows_per_split reducer')

# es_set_option defaults of csrc/spconv.hip: key -> value
DEFAULTS = {2: 1, 4: 2048, 5: 512, 6: 1024, 7: 256, 14: 1, 21: 1, 22: 768, 24: 256}
WS_CAP_BIG = 256 << 20
NW_ROWS, LS_KS, WR, GR = 64, 256, 16, 32


def cdiv(a, b):
    return -(-a // b)


def cap_splits(splits, dw_floats, have_ws, opts=DEFAULTS):
    if not have_ws:
        return 1
    cap = (WS_CAP_BIG if dw_floats > (8 << 20) else (opts[7] << 18)) // (dw_floats if dw_floats > 0 else 1)
    cap = max(cap, 1)
    return max(min(splits, cap), 1)


def reducer_name(splits, nw, aligned16):
    """the kernel that adds the slices' partial tiles (None: one slice, nothing to add); aligned16: workspace and dW both on 16 bytes"""
    if splits <= 1 or nw == 0:
        return None
    if splits >= 512:
        return 'k_wgrad_reduce_ranges<64>'
    if splits >= 64:
        return 'k_wgrad_reduce_ranges<16>'
    return 'k_wgrad_reduce4' if (nw % 4 == 0 and aligned16) else 'k_wgrad_reduce'


def plan_f32(n_out, K, cin, cout, have_ws=True, dw_aligned=True, opts=DEFAULTS):
    nw = K * cin * cout
    if opts[21] and K == 27 and cin == 3 and cout == 64:
        splits = cap_splits(min(cdiv(n_out, NW_ROWS), opts[22]), nw, have_ws, opts)
        rps = cdiv(cdiv(n_out, splits), NW_ROWS) * NW_ROWS
        splits = cdiv(n_out, rps)
        return Plan(4, splits, rps, reducer_name(splits, nw, dw_aligned))
    base = K * cdiv(cin, 64) * cdiv(cout, 64)
    splits = min(cdiv(2048, base), cdiv(n_out, 128))
    splits = cap_splits(splits, nw, have_ws, opts)
    rps = cdiv(cdiv(n_out, splits), WR) * WR
    splits = cdiv(n_out, rps)
    return Plan(0, splits, rps, reducer_name(splits, nw, dw_aligned))


def plan_bf16(xh, yh, x_aligned, y_aligned, ldx, ldy, n_out, n_in, K, cin, cout, have_ws=True, dw_aligned=True, opts=DEFAULTS):
    """x_aligned / y_aligned: the operand's base pointer is a multiple of 16 bytes"""
    nw = K * cin * cout

    def done(kind, splits, unit):
        rps = cdiv(cdiv(n_out, splits), unit) * unit
        splits = cdiv(n_out, rps)
        return Plan(kind, splits, rps, reducer_name(splits, nw, dw_aligned))
    if (opts[24] and K == 1 and not xh and not yh and n_out == n_in and n_out <= 8192 and cin % 64 == 0 and cout % 64 == 0 and
            cin * cout <= 256 * 256 and ldx % 4 == 0 and ldy % 4 == 0 and x_aligned and y_aligned):
        return done(5, cap_splits(cdiv(n_out, LS_KS), nw, have_ws, opts), LS_KS)
    ax, ay = (8 if xh else 4), (8 if yh else 4)
    big = (cin % 128 == 0 and cout % 128 == 0 and ldx % ax == 0 and ldy % ay == 0 and x_aligned and y_aligned and
           n_in * ldx < (1 << 31) and n_out * ldy < (1 << 31) and (n_out >= 512 or cin * cout >= 512 * 512))
    huge = big and xh and yh and opts[2] and cin % 256 == 0 and cout % 256 == 0 and ldx % 8 == 0 and ldy % 8 == 0
    if huge:
        base = K * (cin // 256) * (cout // 256)
        splits = cap_splits(min(cdiv(2048, base), cdiv(n_out, 1024)), nw, have_ws, opts)
        if base * splits >= 960:
            return done(3, splits, GR)
    if big:
        base = K * (cin // 128) * (cout // 128)
        return done(2, cap_splits(min(cdiv(opts[4], base), cdiv(n_out, opts[5])), nw, have_ws, opts), GR)
    base = K * cdiv(cin, 64) * cdiv(cout, 64)
    return done(1, cap_splits(min(cdiv(opts[6], base), cdiv(n_out, 256)), nw, have_ws, opts), GR)


def kernel_name(bf16, kind, xh, yh, ldx, ldy, has_map, opts=DEFAULTS):
    """the tile kernel a launch with this plan runs (the launch log of tests/emu strips nothing but the template arguments XH, YH)"""
    if not bf16:
        return 'k_spconv_narrow_wgrad<3>' if (kind == 4 and has_map) else 'k_spconv_wgrad'
    if kind == 5 and not has_map:
        return 'k_lin_wgrad_small'
    if kind == 3:
        return 'k_spconv_wgrad_bf16_huge'
    if kind == 2 and xh and yh and opts[14] and ldx % 8 == 0 and ldy % 8 == 0:
        return 'k_spconv_wgrad_bf16_tr<64>' if opts[14] == 2 else 'k_spconv_wgrad_bf16_tr<32>'
    return 'k_spconv_wgrad_bf16_big' if kind == 2 else 'k_spconv_wgrad_bf16'


def workspace_floats(plan, K, cin, cout):
    return plan.splits * K * cin * cout if plan.splits > 1 else 0


# ---------------------------------------------------------------------------------------------------------------- value and bound
def operand(t, rounded):
    """the f64 values a launch multiplies: t f32 rows (rounded to bf16 when `rounded`) or a bf16 shadow (exact)"""
    if t.dtype == torch.bfloat16 or not rounded:
        return t.to(F64)
    return t.to(torch.bfloat16).to(F64)


def tap_rows(nbr, k, n_out, n_in):
    """-> (output rows, input rows) of tap k, LongTensors"""
    if nbr is None:
        j = torch.arange(min(n_out, n_in))
        return j, j
    col = nbr[:n_out, k].long()
    j = torch.nonzero(col >= 0).squeeze(1)
    return j, col[j]


def reference(x, dy, nbr, n_out, n_in, K):
    """x (rows, Cin), dy (rows, Cout): f64 operands (operand()); nbr (n_out, K) integer tensor on the CPU or None.
    -> dW (K, Cin, Cout), A (the same product on absolute values), n_k (K,) pair counts"""
    cin, cout = x.shape[1], dy.shape[1]
    want = torch.zeros((K, cin, cout), dtype=F64, device=x.device)
    A = torch.zeros_like(want)
    nk = torch.zeros(K, dtype=F64, device=x.device)
    for k in range(K):
        j, i = tap_rows(nbr, k, n_out, n_in)
        if j.numel() == 0:
            continue
        xs, ys = x[i.to(x.device)], dy[j.to(x.device)]
        want[k] = xs.t() @ ys
        A[k] = xs.abs().t() @ ys.abs()
        nk[k] = j.numel()
    return want, A, nk


class Stats:
    """per (entry point, kind, operand kinds, reducer): case count, worst bound ratio, worst relative L2"""

    def __init__(self, label):
        self.label, self.count, self.ratio, self.rel = label, {}, {}, {}

    def note(self, cls, ratio, rel):
        self.count[cls] = self.count.get(cls, 0) + 1
        self.ratio[cls] = max(self.ratio.get(cls, 0.0), ratio)
        self.rel[cls] = max(self.rel.get(cls, 0.0), rel)

    def worst(self):
        return max(self.ratio.values(), default=0.0)

    def report(self):
        lines = [f'{self.label}: {sum(self.count.values())} weight-gradient launches checked']
        for cls in sorted(self.ratio, key=str):
            lines.append(f'  {cls}: {self.count[cls]} launches, worst (|dW - spec| - slack) / (u sqrt(n) A) = {self.ratio[cls]:.3f} '
                         f'(bound {G:g}), worst rel-L2 {self.rel[cls]:.2e}')
        return '\n'.join(lines)


def bound(want, A, nk, prior, n_acc=1):
    """-> (lin, slack): the bound is G lin + slack.  want: the FINAL value (prior + dW).  n_acc: roundings of the final sum"""
    lin = U * torch.sqrt(nk.clamp(min=1)).view(-1, 1, 1) * A
    slack = U * n_acc * ((prior.abs() if prior is not None else 0) + want.abs())
    return lin, slack


def check(label, got, want, A, nk, prior=None, cls=None, stats=None, g=G):
    """got (K, Cin, Cout) f32; want, A, nk from reference() (want WITHOUT the prior); prior f32 or None.  Raises AssertionError on the
    first violated element; -> the worst ratio (|err| - slack) / (u sqrt(n) A)"""
    got64 = got.to(F64)
    p64 = prior.to(F64) if prior is not None else None
    final = want + p64 if p64 is not None else want
    lin, slack = bound(final, A, nk, p64)
    err = (got64 - final).abs()
    bad = ~(err <= g * lin + slack)                                   # (a NaN fails)
    dead = A == 0
    if bool(dead.any()):
        exact = (got == prior) if prior is not None else (got == 0)
        bad = bad | (dead & ~exact)
    if bool(bad.any()):
        over = torch.where(bad, torch.nan_to_num(err - g * lin - slack, nan=math.inf, posinf=math.inf), torch.full_like(err, -math.inf))
        i = int(torch.argmax(over.reshape(-1)))
        cin, cout = got.shape[1], got.shape[2]
        k, c, n = i // (cin * cout), (i // cout) % cin, i % cout
        what = 'an element without any contribution is not exactly ' + ('the prior' if prior is not None else '0.0') \
            if bool(dead.reshape(-1)[i]) else 'per-element bound exceeded'
        raise AssertionError(f'{label}: {what} at dW[{k}][{c}][{n}] (tap with {int(nk[k])} pairs): got {float(got64.reshape(-1)[i]):.9g}, spec '
                             f'{float(final.reshape(-1)[i]):.9g}, |err| {float(err.reshape(-1)[i]):.3e} > bound '
                             f'{float((g * lin + slack).reshape(-1)[i]):.3e} ({int(bad.sum())} of {bad.numel()} elements)')
    pos = lin > 0
    ratio = float(((err - slack).clamp(min=0)[pos] / lin[pos]).max()) if bool(pos.any()) else 0.0
    rel = float((got64 - final).norm() / (final.norm() + 1e-300))
    if stats is not None:
        stats.note(cls, ratio, rel)
    return ratio


def rel_l2(got, want):
    """the relative L2 the older tests assert on (tests/test_gpu_ops.py: < 5e-3)"""
    return float((got.to(F64) - want).norm() / want.norm())
