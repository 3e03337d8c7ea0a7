"""Specification of the geometry of the projection-fusion kernels (csrc/fusion.hip: undo_aug + project_view, shared by
es_point_sample_fwd, _fwd_h, _fwd_pts, _win_fwd, _win_fwd_h, _prefix_fwd_pts and _step_fwd_pts): which feature-map pixel a
(point, view) pair reads (pix, -1 for none) and whether the view counts (valid; cnt is the number of valid views).  Used by
tests/test_gpu_fusion_geometry.py (MI355X), tests/test_emu_fusion_geometry.py (the same bodies on the CPU emulator, the seed check and
the mutated records the checker must reject) and by the forward bodies of the window, prefix and step tests.  prefix_spec.py and
window_spec.py hold the SUM on the launch's own pix and cnt; this file holds pix and cnt themselves.

The chain, step for step as in fusion.hip (every operation a correctly rounded f32 one; fmaf is ONE operation):
   location   float points as given, or c * voxel_size (one multiplication) for integer voxel coordinates
   undo_aug   the sample's op list: T  p = p + ntrans          (3 additions)
                                    S  p = p * iscale          (3 multiplications)
                                    R  nx = fma(z, r6, fma(y, r3, x * r0)), ny, nz alike
                                    HF x = -x, VF y = -y       (exact)
   project    qx = fma(1, P3, fma(z, P2, fma(y, P1, x * P0))), qy, qz alike (the last fma is an addition)
   clamp      zc = max(qz, float32(1e-3))                      (exact)
   divide     u = qx / zc, v = qy / zc
   image      u = u * sfx - cropx, v = v * sfy - cropy; if flip: u = oriw - u
   valid      u < w and u > 0 and v < h and v > 0 and qz > 0   (w, h: the padded image size)
   grid       gx = u / w * 2 - 1, gy = v / h * 2 - 1
   index      ix = (gx + 1) * ((Wf - 1) / 2), iy = (gy + 1) * ((Hf - 1) / 2)
   round      rx = nearbyint(ix), ry = nearbyint(iy)  (half to even, ATen's grid sampler); pix = ry Wf + rx when 0 <= rx <= Wf - 1
              and 0 <= ry <= Hf - 1 (-0.5 rounds to -0, which is in range), else -1

Error model.  Every quantity is a pair (x, e): x the value of the chain in f64, e a bound on |kernel's f32 value - x|.  u = 2^-24.
An operation with result r, from operands whose errors propagate to p (through |coefficients|: |a| e_b + |b| e_a + e_a e_b for a
product, e_a + e_b for a sum, (e_num + |q| e_den) / (|den| - e_den) for a quotient q), gets e = p + u (|r| + p): the kernel rounds ITS
operands' result, whose magnitude is at most |r| + p.  (2^-50 of the operands' magnitude and 2^-149 are added for the f64 arithmetic
of this file and for a subnormal result; neither is ever visible.)  An operation whose operands are exact (p = 0) and whose f64
result is representable in f32 adds nothing: the kernel's result is that value.  So a chain on dyadic inputs (the edge lattice) is
exact end to end, e = 0, and `exact` says so per pair: every intermediate of that pair was representable.  max, negation and the
constant (size - 1) / 2 are exact.

Decided and undecided.  A comparison x > 0 holds for every value in [x - e, x + e] when x - e > 0 and fails for every one when
x + e <= 0; in between it is undecided (with e = 0 it is always decided: u = 0 exactly is decidedly not valid).  `valid` is decidedly
false when one of its five comparisons decidedly fails, decidedly true when all five decidedly hold, undecided otherwise.  Rounding is
monotone, so the kernel's rx lies in [nearbyint(ix - e), nearbyint(ix + e)] = [lo, hi].  An axis is decidedly out of range when hi <= -1
or lo >= size, decidedly in range when lo >= 0 and hi <= size - 1.  pix is decided -1 when either axis is decidedly out; decided
ry Wf + rx when both axes are decidedly in and lo = hi on both; undecided otherwise, and then the admissible answers are the pixels
(rx, ry) in [lo, hi] x [lo, hi] that are in range, and -1 when an axis is not decidedly in.  (With e < 1 / 2 -- every pair near the
image -- [lo, hi] is the roundings of the interval's two ends.)

check_geometry(rec): every decided pix equals the specification; every undecided one is admissible; cnt lies between the number of
decidedly valid views and that number plus the undecided ones (per prefix for the (V, n) layout, inside the window when the record has
one; pix beyond the window is -1).  No row is left out of the check of `out`: that stays on the launch's own pix and cnt, through the
sum bounds of window_spec / prefix_spec.

Caps (within_caps, asserted per case by check_geometry(caps=True)): undecided pairs are at most 1 / 500 of a case's pairs, rows with
an undecided pair at most 1 / 100 of its rows.  The seeds of the grids were chosen so that the specification alone stays inside the
caps (tests/test_emu_fusion_geometry.py::test_seeds_stay_inside_the_caps: no kernel runs); the edge lattice has no undecided pair on
the rows it declares exact.

spec_out is the f64 mean of the rows the SPECIFICATION's pix names over the specification's count: against
oracle.model.batch_point_sample (one sample, float points, f32 map) it ties this restatement to the reference's semantics rather than
to fusion.hip (test_spec_agrees_with_the_oracle, on the two golden fixtures: every decided row within twice the sum bound).

wrong_rule(case, rule) runs the same chain with ONE rule changed and returns the pix / valid a kernel with that rule would write; the
emulator tests plant those in a correct record and require check_geometry to reject it.

Measured (MI355X on the full grid / CPU emulator on the reduced one): no decided pair differs on any entry point.  Undecided pairs (rows
with one) of the pairs checked: fwd 4 (3) of 71136 / 0 of 13404; fwd_h 1 (1) of 92800 / 0 of 16673; fwd_pts 1 (1) of 71982 / 0 of 15382;
win 0 of 45422 / 0 of 8065; win_h 1 (1) of 22947 / 0 of 3702; prefix 0 of 24007 / 0 of 4763; step 0 of 5400 / 0 of 1155.  Largest
undecided share of one case: 1.34e-4 of its pairs, 6.0e-3 of its rows.  Worst sum ratios |err| / (bound / 8) of the same launches:
fwd 0.87 / 0.75, fwd_h 0.19 / 0.16, fwd_pts 2.65 / 2.65, win 2.67 / 2.66, win_h 1.12 / 1.12, prefix 4.32 / 3.88, step 4.50 / 3.92.
Edge lattice: 0 mismatches of 10200 (integer coordinates) / 10212 (float points) pairs per launch, 0 undecided, on all seven entry points
in both runs.  Golden fixtures: 0 and 1 of 400 rows undecided, no decided row differs from the oracle."""
import torch

import prefix_spec as PS
from fwd_spec import F64, U

__all__ = ['geometry', 'check_geometry', 'within_caps', 'spec_out', 'wrong_rule', 'RULES', 'lattice_case', 'coverage', 'straddles',
           'full_windows']

NOPS, OPS, ROTINV, ISCALE, NTRANS, SFX, SFY, CROPX, CROPY, FLIP, ORIW, PADW, PADH, PROJ = (
    PS.NOPS, PS.OPS, PS.ROTINV, PS.ISCALE, PS.NTRANS, PS.SFX, PS.SFY, PS.CROPX, PS.CROPY, PS.FLIP, PS.ORIW, PS.PADW, PS.PADH, PS.PROJ)
EPS64, TINY = 2.0 ** -50, 2.0 ** -149
CLAMP = float(torch.tensor(1e-3, dtype=torch.float32))

# the single wrong rules of wrong_rule (tests/test_emu_fusion_geometry.py)
RULES = ('u_ge_0', 'u_le_w', 'v_ge_0', 'v_le_h', 'qz_ge_0', 'half_up', 'no_flip', 'flip_before_crop', 'no_clamp', 'size_half',
         'neighbour_meta')


class _Chain:
    """f32 operations on (value, error) pairs; `exact`: every operation so far had exact operands and a representable result"""

    def __init__(self):
        self.exact = None
        self.mask = None

    def _round(self, v, prop, mag):
        ex = (prop == 0) & (v.to(torch.float32).to(F64) == v)
        seen = ex if self.mask is None else (ex | ~self.mask)
        self.exact = seen if self.exact is None else (self.exact & seen)
        e = prop + U * (v.abs() + prop) + EPS64 * mag + TINY
        return v, torch.where(ex, torch.zeros_like(e), e)

    def mul(self, a, b):
        v = a[0] * b[0]
        return self._round(v, a[0].abs() * b[1] + b[0].abs() * a[1] + a[1] * b[1], v.abs())

    def add(self, a, b):
        return self._round(a[0] + b[0], a[1] + b[1], a[0].abs() + b[0].abs())

    def sub(self, a, b):
        return self._round(a[0] - b[0], a[1] + b[1], a[0].abs() + b[0].abs())

    def fma(self, a, b, c):
        p = a[0] * b[0]
        return self._round(p + c[0], a[0].abs() * b[1] + b[0].abs() * a[1] + a[1] * b[1] + c[1], p.abs() + c[0].abs())

    def div(self, a, b):
        q = a[0] / b[0]
        den = b[0].abs() - b[1]
        prop = torch.where(den > 0, (a[1] + q.abs() * b[1]) / den.clamp(min=TINY), torch.full_like(q, float('inf')))
        prop = torch.where((a[1] == 0) & (b[1] == 0), torch.zeros_like(prop), prop)
        return self._round(q, prop, q.abs())


def _where(m, a, b):
    return torch.where(m, a[0], b[0]), torch.where(m, a[1], b[1])


def _axis(x, size, half_up=False):
    """(lo, hi, decidedly in range, decidedly out of range) of the kernel's rounded index"""
    v, e = x
    rnd = (lambda t: torch.floor(t + 0.5)) if half_up else torch.round
    lo, hi = rnd(v - e), rnd(v + e)
    lo = torch.where(torch.isfinite(lo), lo, torch.full_like(lo, -2.0 ** 40))
    hi = torch.where(torch.isfinite(hi), hi, torch.full_like(hi, 2.0 ** 40))
    nan = torch.isnan(v)                                     # (a wrong rule only) the kernel's comparisons fail on a NaN: out of range
    lo, hi = torch.where(nan, torch.full_like(lo, -2.0), lo), torch.where(nan, torch.full_like(hi, -2.0), hi)
    return lo, hi, (lo >= 0) & (hi <= size - 1), (hi <= -1) | (lo >= size)


def _gt0(x):
    """(decidedly holds, decidedly fails) of x > 0"""
    return x[0] - x[1] > 0, ~(x[0] + x[1] > 0)


def geometry(case, dev, vs=None, rule=None):
    """case: V, Hf, Wf, coords (n, 4) int (column 0: the sample), meta (B, stride) f32, and points (n, 3) f32 (vs None) or integer
    coordinates in coords[:, 1:] with voxel size vs.  -> dict of (n, V) tensors on dev:
      pix (long; the expected entry, -1 for none; meaningful where pix_dec), pix_dec, lox / hix / loy / hiy, in_x / in_y (decidedly in
      range), valid, valid_dec, und (pix or valid undecided), exact, and the intermediates qz, u, v, ix, iy as (value, error)
    rule: one of RULES (wrong_rule); None is the specification"""
    V, Hf, Wf = case['V'], case['Hf'], case['Wf']
    coords = case['coords'].to(dev)
    n = coords.shape[0]
    b = coords[:, 0].long()
    if rule == 'neighbour_meta':                             # a straddling workgroup stages the meta row of its FIRST row's sample
        first = b[(torch.arange(n, device=dev) // 16) * 16]
        b = first
    m = case['meta'].to(dev).to(F64)[b]                      # (n, stride)
    k = _Chain()
    zero = torch.zeros(n, 1, dtype=F64, device=dev)

    def M(j):
        return m[:, j:j + 1], zero

    if vs is None:
        p = case['points'].to(dev).to(F64)
        loc = [(p[:, j:j + 1], zero) for j in range(3)]
    else:
        s = (torch.full((n, 1), float(torch.tensor(vs, dtype=torch.float32)), dtype=F64, device=dev), zero)
        loc = [k.mul((coords[:, j + 1:j + 2].to(F64), zero), s) for j in range(3)]
    x, y, z = loc
    nops = m[:, NOPS:NOPS + 1]
    for o in range(8):
        op = torch.where(nops > o, m[:, OPS + o:OPS + o + 1], torch.zeros_like(nops))
        if not bool((op != 0).any()):
            continue
        k.mask = op == 1
        t = [k.add(c, M(NTRANS + j)) for j, c in enumerate((x, y, z))]
        k.mask = op == 2
        s = [k.mul(c, M(ISCALE)) for c in (x, y, z)]
        k.mask = op == 3
        r = [k.fma(z, M(ROTINV + 6 + j), k.fma(y, M(ROTINV + 3 + j), k.mul(x, M(ROTINV + j)))) for j in range(3)]
        k.mask = None
        new = []
        for j, c in enumerate((x, y, z)):
            c = _where(op == 1, t[j], c)
            c = _where(op == 2, s[j], c)
            c = _where(op == 3, r[j], c)
            if j == 0:
                c = _where(op == 4, (-c[0], c[1]), c)
            if j == 1:
                c = _where(op == 5, (-c[0], c[1]), c)
            new.append(c)
        x, y, z = new
    P = m[:, PROJ:PROJ + 16 * V].reshape(n, V, 16)
    zv = torch.zeros(n, V, dtype=F64, device=dev)

    def row(r):
        q = k.mul(x, (P[:, :, 4 * r], zv))
        q = k.fma(y, (P[:, :, 4 * r + 1], zv), q)
        q = k.fma(z, (P[:, :, 4 * r + 2], zv), q)
        return k.add(q, (P[:, :, 4 * r + 3], zv))            # fmaf(1, P3, q)

    qx, qy, qz = row(0), row(1), row(2)
    zc = qz if rule == 'no_clamp' else (qz[0].clamp(min=CLAMP), qz[1])
    u, v = k.div(qx, zc), k.div(qy, zc)
    flip = (m[:, FLIP:FLIP + 1] != 0) & (rule != 'no_flip')
    u = k.mul(u, M(SFX))
    if rule == 'flip_before_crop':
        k.mask = flip
        u = _where(flip, k.sub(M(ORIW), u), u)
        k.mask = None
        u = k.sub(u, M(CROPX))
    else:
        u = k.sub(u, M(CROPX))
        k.mask = flip
        u = _where(flip, k.sub(M(ORIW), u), u)
        k.mask = None
    v = k.sub(k.mul(v, M(SFY)), M(CROPY))
    w, h = M(PADW), M(PADH)
    one, two = (torch.ones_like(zero), zero), (2 * torch.ones_like(zero), zero)
    tests = [_gt0(u), _gt0((w[0] - u[0], u[1])), _gt0(v), _gt0((h[0] - v[0], v[1])), _gt0(qz)]
    if rule in ('u_ge_0', 'u_le_w', 'v_ge_0', 'v_le_h', 'qz_ge_0'):   # x >= 0 in place of x > 0
        j = ('u_ge_0', 'u_le_w', 'v_ge_0', 'v_le_h', 'qz_ge_0').index(rule)
        q = (u, (w[0] - u[0], u[1]), v, (h[0] - v[0], v[1]), qz)[j]
        tests[j] = (q[0] - q[1] >= 0, ~(q[0] + q[1] >= 0))
    vals = [q[0] > 0 for q in (u, (w[0] - u[0],), v, (h[0] - v[0],), qz)]
    if rule in ('u_ge_0', 'u_le_w', 'v_ge_0', 'v_le_h', 'qz_ge_0'):
        vals[j] = q[0] >= 0
    valid_val = torch.stack([t.expand(n, V) for t in vals]).all(0)
    holds = torch.stack([t[0] for t in tests]).all(0)
    fails = torch.stack([t[1] for t in tests]).any(0)
    gx = k.sub(k.mul(k.div(u, w), two), one)
    gy = k.sub(k.mul(k.div(v, h), two), one)
    hw = (Wf / 2.0) if rule == 'size_half' else (Wf - 1) / 2.0
    hh = (Hf / 2.0) if rule == 'size_half' else (Hf - 1) / 2.0
    ix = k.mul(k.add(gx, one), (torch.full_like(zero, hw), zero))
    iy = k.mul(k.add(gy, one), (torch.full_like(zero, hh), zero))
    lox, hix, in_x, out_x = _axis(ix, Wf, rule == 'half_up')
    loy, hiy, in_y, out_y = _axis(iy, Hf, rule == 'half_up')
    none = out_x | out_y
    one_px = in_x & in_y & (lox == hix) & (loy == hiy)
    pix = torch.where(one_px, loy * Wf + lox, torch.full_like(lox, -1.0)).long()
    pix_dec, valid_dec = none | one_px, holds | fails
    return dict(pix=pix, pix_dec=pix_dec, lox=lox, hix=hix, loy=loy, hiy=hiy, in_x=in_x, in_y=in_y, valid=holds, valid_dec=valid_dec,
                und=~(pix_dec & valid_dec), valid_val=valid_val, exact=k.exact.expand(n, V), qz=qz, u=u, v=v, ix=ix, iy=iy, n=n, V=V, Hf=Hf, Wf=Wf)


def wrong_rule(case, dev, rule, vs=None):
    """(pix (n, V) long, valid (n, V) bool) a kernel with ONE wrong rule would write: the chain above with that rule changed, decided on
    its f64 values (a pair whose wrong-rule value sits inside its error interval takes the nearest answer: the tests only use the
    entries that differ from the specification on DECIDED pairs)"""
    g = geometry(case, dev, vs, rule)
    half_up = rule == 'half_up'
    rnd = (lambda t: torch.floor(t + 0.5)) if half_up else torch.round
    rx, ry = rnd(g['ix'][0]), rnd(g['iy'][0])
    ok = (rx >= 0) & (rx <= g['Wf'] - 1) & (ry >= 0) & (ry <= g['Hf'] - 1)           # False on NaN / inf
    pix = torch.where(ok, ry * g['Wf'] + rx, torch.full_like(rx, -1.0)).long()
    return pix, g['valid_val']


def _inside(rec, dev, n, V):
    if rec.get('win') is None:
        return torch.ones(n, V, dtype=torch.bool, device=dev)
    win = rec['win'].to(dev).long()
    w = win[rec['coords'].to(dev)[:, 0].long(), 1].clamp(0, V)
    return torch.arange(V, device=dev)[None, :] < w[:, None]


def within_caps(geo, inside=None):
    """(undecided pairs, rows with one, pairs, rows, inside the caps) from the specification alone"""
    und = geo['und'] if inside is None else (geo['und'] & inside)
    pairs = geo['n'] * geo['V'] if inside is None else int(inside.sum())
    up, ur = int(und.sum()), int(und.any(1).sum())
    return up, ur, pairs, geo['n'], (500 * up <= pairs and 100 * ur <= geo['n'])


def check_geometry(rec, dev, vs=None, caps=True, geo=None, label=None):
    """rec: the case (see geometry) + the launch's pix (n, V) int and cnt -- (n) for the base and window kernels (win (B, 2) int when
    there is a window), (V, n) for the prefix layout.  Returns dict(und_pairs, und_rows, pairs, rows, exact)"""
    geo = geometry(rec, dev, vs) if geo is None else geo
    n, V, Wf = geo['n'], geo['V'], geo['Wf']
    label = label or f'geometry V={V} n={n} {rec["Hf"]}x{Wf} seed={rec.get("seed")}'
    pix = rec['pix'].to(dev).long().reshape(n, V)
    inside = _inside(rec, dev, n, V)
    if not bool((pix[~inside] == -1).all()):
        raise AssertionError(f'{label}: a pix entry beyond its window is not -1')
    dec = geo['pix_dec'] & inside
    bad = dec & (pix != geo['pix'])
    if bool(bad.any()):
        i, v = (int(t) for t in torch.nonzero(bad)[0])
        raise AssertionError(f'{label}: {int(bad.sum())} decided pix entries differ from the specification; first: row {i} view {v} got '
                             f'{int(pix[i, v])} want {int(geo["pix"][i, v])} (ix {float(geo["ix"][0][i, v])!r} +- {float(geo["ix"][1][i, v]):.2e}, '
                             f'iy {float(geo["iy"][0][i, v])!r} +- {float(geo["iy"][1][i, v]):.2e})')
    und = ~geo['pix_dec'] & inside
    rx, ry = (pix % Wf).to(F64), torch.div(pix, Wf, rounding_mode='floor').to(F64)
    a_px = (pix >= 0) & (rx >= geo['lox']) & (rx <= geo['hix']) & (ry >= geo['loy']) & (ry <= geo['hiy'])
    a_none = (pix == -1) & ~(geo['in_x'] & geo['in_y'])
    bad = und & ~(a_px | a_none)
    if bool(bad.any()):
        i, v = (int(t) for t in torch.nonzero(bad)[0])
        raise AssertionError(f'{label}: {int(bad.sum())} undecided pix entries are not admissible; first: row {i} view {v} got {int(pix[i, v])}, '
                             f'columns [{geo["lox"][i, v]:.0f}, {geo["hix"][i, v]:.0f}] rows [{geo["loy"][i, v]:.0f}, {geo["hiy"][i, v]:.0f}]')
    sure = (geo['valid'] & geo['valid_dec'] & inside).long()
    maybe = (~geo['valid_dec'] & inside).long()
    cnt = rec['cnt'].to(dev).long()
    if cnt.dim() == 2:                                       # the prefix layout (V, n): one count per prefix
        cnt = cnt.reshape(V, n).t()
        sure, maybe = sure.cumsum(1), maybe.cumsum(1)
    else:
        cnt = cnt.reshape(n, 1)
        sure, maybe = sure.sum(1, keepdim=True), maybe.sum(1, keepdim=True)
    bad = (cnt < sure) | (cnt > sure + maybe)
    if bool(bad.any()):
        i, t = (int(q) for q in torch.nonzero(bad)[0])
        raise AssertionError(f'{label}: {int(bad.sum())} cnt entries outside [decidedly valid, + undecided]; first: row {i} (prefix {t}) got '
                             f'{int(cnt[i, t])}, want {int(sure[i, t])} .. {int(sure[i, t] + maybe[i, t])}')
    up, ur, pairs, rows, ok = within_caps(geo, inside)
    if caps and not ok:
        raise AssertionError(f'{label}: {up} of {pairs} pairs / {ur} of {rows} rows are undecided: outside the caps 1/500, 1/100')
    return dict(und_pairs=up, und_rows=ur, pairs=pairs, rows=rows, exact=geo['exact'])


def full_windows(B, V):
    """the (B, 2) table under which window_spec.check_win_fwd holds a base-kernel record: sample b reads set b, all V views"""
    return torch.tensor([[b, V] for b in range(B)], dtype=torch.int32)


def spec_out(geo, feats, b, dev):
    """f64 (n, C): the mean of the rows the specification's pix names over the specification's count, and the sum bound's A = sum
    |rows| / count, k = views with a pixel; rows with an undecided pair are flagged in the third result.  feats (B, V, HW, C)"""
    V = geo['V']
    f = feats.to(dev).to(F64).reshape(-1, feats.shape[-2], feats.shape[-1])
    has = geo['pix'] >= 0
    img = b.to(dev).long()[:, None] * V + torch.arange(V, device=dev)[None, :]
    rows = f[img, geo['pix'].clamp(min=0)] * has[:, :, None]
    cnt = geo['valid'].sum(1)
    den = cnt.clamp(min=1).to(F64)[:, None]
    live = (cnt > 0)[:, None]
    out = torch.where(live, rows.sum(1) / den, torch.zeros_like(den))
    bnd = torch.where(live, (has.sum(1)[:, None] + 1) * rows.abs().sum(1) / den, torch.zeros_like(den))
    return out, U * bnd, geo['und'].any(1)


def straddles(coords):
    """16-row workgroups whose first and last row belong to different samples"""
    b = coords[:, 0]
    n = b.shape[0]
    return sum(int(b[i0] != b[min(n, i0 + 16) - 1]) for i0 in range(0, n, 16))


def coverage(case, geo, inside=None):
    """what a case exercises, from the SPECIFICATION (host ints): straddling workgroups, rows with no valid view but a pixel, rows
    valid in some views with an invalid view that has a pixel, views without a pixel, pairs behind the camera, pairs with
    0 < qz < 1e-3 (decided entries only)"""
    inside = torch.ones_like(geo['und']) if inside is None else inside
    dec = geo['pix_dec'] & geo['valid_dec'] & inside
    has, val = dec & (geo['pix'] >= 0), dec & geo['valid']
    alldec = (dec | ~inside).all(1)
    qz, eq = geo['qz']
    return dict(straddle=straddles(case['coords'].cpu()),
                dead_with_pixel=int((alldec & ~val.any(1) & has.any(1)).sum()),
                invalid_with_pixel=int((alldec & val.any(1) & (has & ~val).any(1)).sum()),
                no_pixel=int((dec & (geo['pix'] < 0)).sum()),
                behind=int(((qz + eq < 0) & inside).sum()),
                shallow=int(((qz - eq > 0) & (qz + eq < CLAMP) & inside).sum()))


def lattice_case(C, crop, sf, seed=0, ints=False):
    """the edge lattice: dyadic values only, so every intermediate is exact in f32.  V = 2 views: rows (32, 0, 0, 0), (0, 32, 0, 0),
    (0, 0, 1, 0) and the same shifted by (4, -4) pixels; PADW = ORIW = 64, PADH = 32; Wf = 9, Hf = 5; points (k / 8, j / 8, z), k = -4 .. 20,
    j = -4 .. 12, z in {1, 2, 0, -1}.  Three samples of 1700 (+ 2) rows: 0 flip off, 1 flip on, 2 flip on and all five reverse ops with dyadic
    parameters (T by multiples of 1 / 8, S by 1 / 2, R by 90 degrees, HF, VF) on points placed so that the op list takes them back onto the
    lattice.  At z = 1, crop 0, scale 1 the column index is k / 2 and the row index j / 2.  ints: coords[:, 1:] = points / 0.125 as well;
    without it two more rows per sample, (2^-10, 2^-12, 0) and (2^-10, 2^-12, 2^-11): inside view 0's image under the 1e-3 clamp, so
    that `qz > 0` (not the image borders) decides the first one's flag and the clamp the second one's pixel.
    `exact_rows`: the rows with z in {1, 2}, whose every intermediate must be representable"""
    V, Hf, Wf = 2, 5, 9
    kk, jj, zz = torch.meshgrid(torch.arange(-4, 21), torch.arange(-4, 13), torch.tensor([1, 2, 0, -1]), indexing='ij')
    L = torch.stack([kk.reshape(-1) / 8.0, jj.reshape(-1) / 8.0, zz.reshape(-1).float()], 1).float()       # (1700, 3)
    if not ints:                                             # two more rows in front of view 0's centre: depth exactly 0 and depth 2^-11
        L = torch.cat([L, torch.tensor([[2.0 ** -10, 2.0 ** -12, 0.0], [2.0 ** -10, 2.0 ** -12, 2.0 ** -11]])])
    n1 = L.shape[0]
    meta = torch.zeros(3, PROJ + 16 * V + 4, dtype=torch.float32)
    ntr = torch.tensor([0.375, -0.25, 0.125])
    for b in range(3):
        m = meta[b]
        m[SFX], m[SFY], m[CROPX], m[CROPY] = sf[0], sf[1], crop, crop
        m[PADW], m[ORIW], m[PADH], m[FLIP], m[ISCALE] = 64.0, 64.0, 32.0, float(b > 0), 1.0
        m[ROTINV:ROTINV + 9] = torch.eye(3).reshape(-1)
        m[PROJ:PROJ + 12] = torch.tensor([32.0, 0, 0, 0, 0, 32.0, 0, 0, 0, 0, 1.0, 0])
        m[PROJ + 16:PROJ + 28] = torch.tensor([32.0, 0, 0, 4.0, 0, 32.0, 0, -4.0, 0, 0, 1.0, 0])
        m[PROJ + 15] = m[PROJ + 31] = 1.0
    m = meta[2]
    m[NOPS], m[OPS:OPS + 5], m[ISCALE], m[NTRANS:NTRANS + 3] = 5, torch.tensor([1.0, 2, 3, 4, 5]), 0.5, ntr
    m[ROTINV:ROTINV + 9] = torch.tensor([0.0, -1, 0, 1, 0, 0, 0, 0, 1])                # (x, y, z) -> (y, -x, z)
    # undo: T, S, R, HF, VF.  Backwards from the lattice point (X, Y, Z): before VF (X, -Y, Z); before HF (-X, -Y, Z); before R the q with
    # (q_y, -q_x, q_z) = (-X, -Y, Z), q = (Y, -X, Z); before S 2 q; before T 2 q - ntrans
    q = torch.stack([L[:, 1], -L[:, 0], L[:, 2]], 1)
    P2 = 2 * q - ntr[None, :]
    points = torch.cat([L, L, P2]).contiguous()
    coords = torch.zeros(3 * n1, 4, dtype=torch.int32)
    coords[:, 0] = torch.arange(3).repeat_interleave(n1).int()
    if ints:
        c = points / 0.125
        assert bool((c == c.round()).all())
        coords[:, 1:] = c.int()
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(3, V, Hf * Wf, C, generator=g)
    zrow = torch.cat([L[:, 2]] * 3)
    return dict(V=V, C=C, n=3 * n1, Hf=Hf, Wf=Wf, B=3, coords=coords, points=points, meta=meta, feats=feats, seed=seed,
                exact_rows=(zrow == 1) | (zrow == 2), nonzero_rows=zrow != 0)
