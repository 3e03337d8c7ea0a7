"""The weight-gradient launchers of csrc/spconv.hip (es_spconv_wgrad, es_spconv_wgrad_bf16, es_spconv_wgrad_bf16_src) and es_cast_rows_bf16
held, element by element, to tests/wgrad_spec.py through the C ABI itself: every tile kernel (exact-f32 64 x 64, narrow 3 -> 64,
k_lin_wgrad_small, bf16 64 x 64, 128 x 128 register-transposing and transposed-read in both widths, 256 x 256), all four operand kinds,
all four reduction kernels.  The plan depends on ROWS, the cost on PAIRS: many-slice plans are reached with many rows and few, placed
pairs (place_pairs: per (tap, slice) the counts around the 32 / 64-pair chunk and the 256 / 512-row ring refill, pairs on the first and
last row of a slice, a slice without a pair, a tap without a pair, a short last slice, slice counts that are no multiple of 8).

Every case: dW between sentinel pads, prefilled with NaN (accumulate = 0) or a random prior; a NaN workspace of exactly the queried
size; ld > C with NaN padding; NaN in every X row no pair references and every dY row without a pair.  The 128 x 128 and 256 x 256
register-transposing tiles and the narrow kernel load X row 0 and dY[first row of the slice] unconditionally and mask the result
(a select / a bitwise AND): those rows stay NaN here like every other unreferenced row -- the mask must survive it.  By construction:
no placed pair names X row 0, and every odd slice keeps its first row free of pairs in every tap while the even slices put a pair
there (place_pairs); Problem asserts both on the buffers it hands to the kernel.
es_spconv_wgrad_workspace_floats is compared with the restated plan in every case, and the case's name promises the plan's kind: a
case that would silently test another kernel fails.

Every body is a function of `dev`: tests/test_emu_wgrad_kernels.py runs the same bodies on the CPU emulator, where the launch log
also pins the kernel names."""
import numpy as np
import pytest
import torch

import wgrad_spec as S
from test_gpu_ground_kernels import _hip, _rc, _st

pytestmark = pytest.mark.gpu

PADW = 16
SENT = -777.25
NAN = float('nan')
COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, -1]          # pairs per (tap, slice); -1: every row of the slice
STATS = S.Stats('weight-gradient kernels')


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\n' + STATS.report())


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the case grid
def case(name, entry, kind, K, cin, cout, n_out, **kw):
    c = dict(name=name, entry=entry, kind=kind, K=K, cin=cin, cout=cout, n_out=n_out, n_in=n_out, xh=0, yh=0, map='placed', ldx_pad=None,
             ldy_pad=None, x_off=0, y_off=0, dw_off=0, acc=0, ws=True, opts={}, kernel=None, reducer='any', thin_on_emu=False, seed=0)
    c.update(kw)
    return c


def _grid():
    g = []
    # kind 0: the exact-f32 64 x 64 tile -- channels no multiple of 4 or 64, odd ld, a base 4 bytes off, 1 .. 22 slices
    for n in (1, 15, 16, 17, 129):
        g.append(case(f'f32-3to5-K1-n{n}', 'f32', 0, 1, 3, 5, n, ldx_pad=2, ldy_pad=2, reducer='k_wgrad_reduce' if n == 129 else None))
    g.append(case('f32-24to72-K8-n129-x4bytes', 'f32', 0, 8, 24, 72, 129, n_in=77, x_off=1, reducer='k_wgrad_reduce4'))
    g.append(case('f32-24to72-K8-n129-y4bytes-acc', 'f32', 0, 8, 24, 72, 129, n_in=200, y_off=1, acc=1, reducer='k_wgrad_reduce4'))
    g.append(case('f32-130to67-K27-n17', 'f32', 0, 27, 130, 67, 17, ldx_pad=1, ldy_pad=1, reducer=None))
    g.append(case('f32-130to67-K27-n129-acc', 'f32', 0, 27, 130, 67, 129, ldx_pad=1, ldy_pad=1, acc=1, reducer='k_wgrad_reduce'))
    g.append(case('f32-24to72-K8-22slices-acc', 'f32', 0, 8, 24, 72, 2693, n_in=999, acc=1, reducer='k_wgrad_reduce4'))
    g.append(case('f32-24to72-K1-identity-nout>nin', 'f32', 0, 1, 24, 72, 300, n_in=200, map=None))
    g.append(case('f32-24to72-K1-identity-nout<nin', 'f32', 0, 1, 24, 72, 200, n_in=300, map=None))
    g.append(case('f32-24to72-K8-no-workspace', 'f32', 0, 8, 24, 72, 2693, n_in=999, ws=False, reducer=None))
    # kind 4: the narrow 3 -> 64 kernel; without a map the exact-f32 tile on the narrow plan's slices
    for n in (1, 63, 64, 65):
        g.append(case(f'narrow-n{n}', 'f32', 4, 27, 3, 64, n, kernel='k_spconv_narrow_wgrad<3>'))
    g.append(case('narrow-n65-no-workspace-acc', 'f32', 4, 27, 3, 64, 65, ws=False, acc=1, kernel='k_spconv_narrow_wgrad<3>', reducer=None))
    g.append(case('narrow-385slices-acc', 'f32', 4, 27, 3, 64, 49217, n_in=30000, acc=1, kernel='k_spconv_narrow_wgrad<3>',
                  reducer='k_wgrad_reduce_ranges<16>'))
    g.append(case('narrow-plan-no-map-n65', 'f32', 4, 27, 3, 64, 65, map=None, kernel='k_spconv_wgrad'))
    g.append(case('narrow-plan-no-map-385slices', 'f32', 4, 27, 3, 64, 49217, n_in=700, map=None, kernel='k_spconv_wgrad', reducer='k_wgrad_reduce_ranges<16>'))
    # kind 5: k_lin_wgrad_small (K = 1, f32 rows, identity map); with an explicit identity map the bf16 64 x 64 tile on the kind-5 slices
    for n in (1, 255, 256, 257, 8192):
        g.append(case(f'lin-64to64-n{n}', 'bf16', 5, 1, 64, 64, n, map=None, kernel='k_lin_wgrad_small', acc=n & 1))
    g.append(case('lin-256to256-n257', 'bf16', 5, 1, 256, 256, 257, map=None, kernel='k_lin_wgrad_small'))
    g.append(case('lin-64to256-n255-acc', 'bf16', 5, 1, 64, 256, 255, map=None, kernel='k_lin_wgrad_small', acc=1))
    g.append(case('lin-64to256-n8192', 'bf16', 5, 1, 64, 256, 8192, map=None, kernel='k_lin_wgrad_small', reducer='k_wgrad_reduce4'))
    for n in (1, 257, 8192):
        g.append(case(f'lin-plan-identity-map-64to64-n{n}', 'bf16', 5, 1, 64, 64, n, map='ident', kernel='k_spconv_wgrad_bf16'))
    g.append(case('lin-plan-identity-map-256to256-n257', 'bf16', 5, 1, 256, 256, 257, map='ident', kernel='k_spconv_wgrad_bf16'))
    g.append(case('lin-left-n8193', 'bf16', 1, 1, 64, 64, 8193, map=None, kernel='k_spconv_wgrad_bf16'))
    g.append(case('lin-left-96to64', 'bf16', 1, 1, 96, 64, 256, map=None, kernel='k_spconv_wgrad_bf16'))
    g.append(case('lin-left-base-4bytes-off', 'bf16', 1, 1, 64, 64, 256, map=None, x_off=1, kernel='k_spconv_wgrad_bf16'))
    # kind 1: the bf16 64 x 64 tile, all operand kinds, ragged channels, n_out != n_in both ways
    for xh, yh in ((0, 0), (1, 0), (0, 1), (1, 1)):
        g.append(case(f'bf16-24to40-K8-x{xh}y{yh}', 'bf16', 1, 8, 24, 40, 300, n_in=200, xh=xh, yh=yh, acc=xh ^ yh))
        g.append(case(f'bf16-96to192-K3-x{xh}y{yh}', 'bf16', 1, 3, 96, 192, 200, n_in=300, xh=xh, yh=yh, acc=1 - (xh ^ yh)))
    g.append(case('bf16-24to40-K8-11slices', 'bf16', 1, 8, 24, 40, 2637, n_in=700, reducer='k_wgrad_reduce4'))
    g.append(case('bf16-24to40-K8-11slices-shadows-acc', 'bf16', 1, 8, 24, 40, 2637, n_in=3000, xh=1, yh=1, acc=1, reducer='k_wgrad_reduce4'))
    g.append(case('bf16-24to40-K1-identity-nout>nin', 'bf16', 1, 1, 24, 40, 300, n_in=200, map=None))
    g.append(case('bf16-24to40-K1-identity-nout>nin-shadows', 'bf16', 1, 1, 24, 40, 300, n_in=200, map=None, xh=1, yh=1))
    g.append(case('bf16-24to40-K1-identity-nout<nin', 'bf16', 1, 1, 24, 40, 200, n_in=300, map=None, src=True))
    # kind 2: the 128 x 128 tiles
    g.append(case('big-gate-n511', 'bf16', 1, 3, 128, 128, 511, kernel='k_spconv_wgrad_bf16'))
    g.append(case('big-gate-n512', 'bf16', 2, 3, 128, 128, 512, kernel='k_spconv_wgrad_bf16_big'))
    g.append(case('big-few-rows-512to512', 'bf16', 2, 1, 512, 512, 40, map=None, kernel='k_spconv_wgrad_bf16_big'))
    for xh, yh in ((0, 0), (1, 0), (0, 1), (1, 1)):
        g.append(case(f'big-128to256-K8-6slices-x{xh}y{yh}', 'bf16', 2, 8, 128, 256, 2577, n_in=900, xh=xh, yh=yh, opts={14: 0}, acc=xh ^ yh,
                      kernel='k_spconv_wgrad_bf16_big', reducer='k_wgrad_reduce4'))
    for tr in (1, 2):
        g.append(case(f'tr{32 * tr}-128to256-K8-6slices', 'bf16', 2, 8, 128, 256, 2577, n_in=900, xh=1, yh=1, opts={14: tr}, acc=tr - 1,
                      kernel=f'k_spconv_wgrad_bf16_tr<{32 * tr}>', reducer='k_wgrad_reduce4'))
        g.append(case(f'tr{32 * tr}-128to128-K8-n512', 'bf16', 2, 8, 128, 128, 512, n_in=333, xh=1, yh=1, opts={14: tr}, acc=2 - tr,
                      kernel=f'k_spconv_wgrad_bf16_tr<{32 * tr}>'))
    g.append(case('tr-declined-ldx-no-multiple-of-8', 'bf16', 1, 8, 128, 256, 2577, n_in=900, xh=1, yh=1, ldx_pad=4, kernel='k_spconv_wgrad_bf16'))
    g.append(case('big-left-x-4bytes-off', 'bf16', 1, 8, 128, 256, 2577, n_in=900, xh=1, yh=1, x_off=2, kernel='k_spconv_wgrad_bf16'))
    g.append(case('big-left-y-4bytes-off', 'bf16', 1, 3, 128, 128, 600, y_off=1, kernel='k_spconv_wgrad_bf16'))
    # kind 3: the 256 x 256 tile -- 36 slices x 27 taps = 972 >= 960 workgroups needs 35 841 rows (a 255 MB workspace); one row fewer gives
    # 35 slices and the 128 x 128 tile
    g.append(case('huge-256to256-K27-36slices', 'bf16', 3, 27, 256, 256, 35841, n_in=5000, xh=1, yh=1, kernel='k_spconv_wgrad_bf16_huge',
                  reducer='k_wgrad_reduce4', thin_on_emu=True))
    g.append(case('huge-one-row-fewer', 'bf16', 2, 27, 256, 256, 35840, n_in=5000, xh=1, yh=1, acc=1, kernel='k_spconv_wgrad_bf16_tr<32>',
                  thin_on_emu=True))
    g.append(case('huge-switched-off', 'bf16', 2, 27, 256, 256, 35841, n_in=5000, xh=1, yh=1, opts={2: 0}, kernel='k_spconv_wgrad_bf16_tr<32>',
                  thin_on_emu=True))
    # the reduction kernels: K = 1, 8 -> 8, S slices of 256 rows (the last one short); 65 / 513 leave the last slice ranges empty
    for s, red in ((11, 'k_wgrad_reduce4'), (64, 'k_wgrad_reduce_ranges<16>'), (65, 'k_wgrad_reduce_ranges<16>'),
                   (511, 'k_wgrad_reduce_ranges<16>'), (512, 'k_wgrad_reduce_ranges<64>'), (513, 'k_wgrad_reduce_ranges<64>')):
        g.append(case(f'reduce-{s}slices', 'bf16', 1, 1, 8, 8, s * 256 - 100, n_in=4000, acc=s & 1, reducer=red))
    g.append(case('reduce-11slices-dW-4bytes-off', 'bf16', 1, 1, 8, 8, 11 * 256 - 100, n_in=4000, dw_off=1, acc=1, reducer='k_wgrad_reduce'))
    g.append(case('reduce-lowered-targets-5slices', 'bf16', 1, 1, 8, 8, 70 * 256, n_in=4000, opts={6: 5}, reducer='k_wgrad_reduce4'))
    g.append(case('reduce-lowered-cap', 'bf16', 2, 8, 128, 256, 2577, n_in=900, opts={7: 2, 14: 0}, reducer='k_wgrad_reduce4'))
    for i, c in enumerate(g):
        c['seed'] = 1000 + i
    return g


CASES = _grid()
assert len({c['name'] for c in CASES}) == len(CASES)


def _esize(half):
    return 2 if half else 4


def geometry(c):
    """-> ldx, ldy, the operands' and dW's 16-byte alignment (every flat buffer starts on 16 bytes; offsets are in elements)"""
    ldx = c['cin'] + (c['ldx_pad'] if c['ldx_pad'] is not None else (8 if c['xh'] else 4))
    ldy = c['cout'] + (c['ldy_pad'] if c['ldy_pad'] is not None else (8 if c['yh'] else 4))
    return ldx, ldy, (c['x_off'] * _esize(c['xh'])) % 16 == 0, (c['y_off'] * _esize(c['yh'])) % 16 == 0, (c['dw_off'] * 4) % 16 == 0


def restated_plan(c, have_ws=None):
    ldx, ldy, xa, ya, da = geometry(c)
    opts = dict(S.DEFAULTS)
    opts.update(c['opts'])
    have_ws = c['ws'] if have_ws is None else have_ws
    if c['entry'] == 'f32':
        p = S.plan_f32(c['n_out'], c['K'], c['cin'], c['cout'], have_ws, da, opts)
    else:
        p = S.plan_bf16(c['xh'], c['yh'], xa, ya, ldx, ldy, c['n_out'], c['n_in'], c['K'], c['cin'], c['cout'], have_ws, da, opts)
    return p, S.kernel_name(c['entry'] != 'f32', p.kind, c['xh'], c['yh'], ldx, ldy, c['map'] is not None, opts)


def promised(c, p, kernel):
    """the restated plan must be the one the case's name promises"""
    assert p.kind == c['kind'], f"{c['name']}: the restated plan is kind {p.kind}, the case promises kind {c['kind']}"
    assert c['kernel'] is None or kernel == c['kernel'], f"{c['name']}: the restated plan runs {kernel}, the case promises {c['kernel']}"
    assert c['reducer'] == 'any' or p.reducer == c['reducer'], f"{c['name']}: the restated plan reduces with {p.reducer}, the case promises {c['reducer']}"


def headless(s, m):
    """slices whose FIRST row stays without a pair in any tap (its dY row holds NaN): every odd slice of at least 3 rows"""
    return s % 2 == 1 and m >= 3


def place_pairs(rng, n_out, n_in, K, rps, splits, thin=False):
    """the (n_out, K) map of a case: tap k of slice s holds COUNTS[(k + 5 s) % 12] pairs (at most the slice's rows), among them the
    slice's first and last row (one pair: the first or the last); slice 1 (of >= 3) is empty in every tap, tap K // 2 (of >= 2) in every
    slice; row n_out - 1 and row 0 have a pair in tap 0.  The odd slices (headless) keep their FIRST row free of pairs in every tap --
    their pairs start on the second row -- and no pair names X row 0 (n_in > 1): the rows the masked-load tiles fetch for ring
    entries past the tail hold NaN by construction.  thin: two pairs (first and last row) in ONE tap per slice, nothing else."""
    nbr = np.full((n_out, K), -1, dtype=np.int32)
    empty_slice = 1 if splits >= 3 else -1
    empty_tap = K // 2 if K >= 2 else -1
    live_taps = [k for k in range(K) if k != empty_tap]
    for s in range(splits):
        r0, r1 = s * rps, min(n_out, (s + 1) * rps)
        if s == empty_slice:
            continue
        if headless(s, r1 - r0):
            r0 += 1
        m = r1 - r0
        for k in live_taps:
            if thin:
                cnt = min(2, m) if k == live_taps[s % len(live_taps)] else 0
            else:
                cnt = COUNTS[(k + 5 * s) % len(COUNTS)]
                cnt = m if cnt < 0 else min(cnt, m)
            if (s == 0 or s == splits - 1) and k == 0:
                cnt = max(cnt, min(2, m))
            if cnt == 0:
                continue
            if cnt == 1:
                rows = np.array([r0 if (k + s) % 2 == 0 else r1 - 1])
            else:
                mid = rng.choice(np.arange(r0 + 1, r1 - 1), size=cnt - 2, replace=False) if cnt > 2 else np.zeros(0, dtype=np.int64)
                rows = np.concatenate([[r0, r1 - 1], mid])
            nbr[rows, k] = rng.integers(min(1, n_in - 1), n_in, size=len(rows))
    return nbr


def make_map(c, p, thin):
    rng = np.random.default_rng(c['seed'])
    if c['map'] is None:
        return None
    if c['map'] == 'ident':
        nbr = np.full((c['n_out'], c['K']), -1, dtype=np.int32)
        m = min(c['n_out'], c['n_in'])
        nbr[:m, :] = np.arange(m, dtype=np.int32)[:, None]
        return nbr
    return place_pairs(rng, c['n_out'], c['n_in'], c['K'], p.rows_per_split, p.splits, thin)


def live_rows(c, nbr):
    """-> (X rows some pair references, dY rows with a pair), boolean"""
    lx, ly = np.zeros(c['n_in'], dtype=bool), np.zeros(c['n_out'], dtype=bool)
    if nbr is None:
        m = min(c['n_out'], c['n_in'])
        lx[:m] = ly[:m] = True
    else:
        assert int(nbr.max()) < c['n_in'] and int(nbr.min()) >= -1
        lx[np.unique(nbr[nbr >= 0])] = True
        ly[(nbr >= 0).any(1)] = True
    return lx, ly


def rows_buffer(dev, rng, n, C, ld, off, half, live):
    """-> (flat buffer, (n, C) view): normal values in the live rows, NaN in every other row, in the ld - C padding columns and around"""
    m = np.full((n, ld), np.nan, dtype=np.float32)
    m[live, :C] = (rng.standard_normal((int(live.sum()), C)) * np.exp2(rng.integers(-3, 4, size=(1, C)))).astype(np.float32)
    flat = torch.full((off + n * ld + 16,), NAN, dtype=torch.float32)
    flat[off:off + n * ld] = torch.from_numpy(m).reshape(-1)
    flat = (flat.to(torch.bfloat16) if half else flat).to(dev)
    assert flat.data_ptr() % 16 == 0
    return flat, flat[off:off + n * ld].view(n, ld)[:, :C]


def set_options(opts):
    for k, v in opts.items():
        _hip().call('es_set_option', k, v)


def restore_options(opts):
    for k in opts:
        _hip().call('es_set_option', k, S.DEFAULTS[k])


def launch(c, X, ldx, dY, ldy, nbr_ptr, dW_ptr, acc, ws_ptr, ws_floats, n_out=None, cin=None):
    n_out = c['n_out'] if n_out is None else n_out
    cin = c['cin'] if cin is None else cin
    tail = (nbr_ptr, n_out, c['n_in'], c['K'], cin, c['cout'], dW_ptr, acc, ws_ptr, ws_floats, _st())
    if c['entry'] == 'f32':
        return _rc('es_spconv_wgrad', X, ldx, dY, ldy, *tail)
    if c['xh'] or c['yh'] or c.get('src'):
        return _rc('es_spconv_wgrad_bf16_src', X, c['xh'], ldx, dY, c['yh'], ldy, *tail)
    return _rc('es_spconv_wgrad_bf16', X, ldx, dY, ldy, *tail)


class Problem:
    """the operands, the map, the plan and the f64 specification of a case (built once; run() launches on fresh dW / workspace)"""

    def __init__(self, dev, c, thin=False):
        self.dev, self.c = dev, c
        self.plan, self.kernel = restated_plan(c)
        promised(c, self.plan, self.kernel)
        self.ldx, self.ldy, xa, ya, _ = geometry(c)
        rng = np.random.default_rng(c['seed'] + 7)
        self.nbr = make_map(c, self.plan, thin)
        lx, ly = live_rows(c, self.nbr)
        self.xflat, self.x = rows_buffer(dev, rng, c['n_in'], c['cin'], self.ldx, c['x_off'], c['xh'], lx)
        self.yflat, self.y = rows_buffer(dev, rng, c['n_out'], c['cout'], self.ldy, c['y_off'], c['yh'], ly)
        assert (self.x.data_ptr() % 16 == 0) == xa and (self.y.data_ptr() % 16 == 0) == ya
        if c['map'] == 'placed':
            # the rows the masked-load tiles fetch unconditionally hold NaN: X row 0, and dY's first row of every headless slice --
            # beside slices whose first row does carry a pair
            p, heads = self.plan, [s * self.plan.rows_per_split for s in range(self.plan.splits)]
            dead = [r for s, r in enumerate(heads) if s != (1 if p.splits >= 3 else -1) and headless(s, min(c['n_out'], r + p.rows_per_split) - r)]
            assert c['n_in'] == 1 or bool(torch.isnan(self.x[0]).all()), f"{c['name']}: X row 0 is referenced"
            assert all(bool(torch.isnan(self.y[r]).all()) for r in dead), f"{c['name']}: a headless slice's first dY row is live"
            busy = [r for r in dead if bool((self.nbr[r:r + p.rows_per_split] >= 0).any())]
            assert (len(busy) > 0 or p.splits < 4) and bool(torch.isfinite(self.y[0]).all()), f"{c['name']}: no slice with pairs leaves its first dY row NaN"
        self.nbr_t = torch.from_numpy(self.nbr) if self.nbr is not None else None
        self.nbr_d = self.nbr_t.to(dev) if self.nbr is not None else None
        rounded = c['entry'] != 'f32'
        self.want, self.A, self.nk = S.reference(S.operand(self.x, rounded), S.operand(self.y, rounded), self.nbr_t, c['n_out'], c['n_in'], c['K'])
        # the inputs alone, before any kernel runs: finite, and a contribution wherever one is intended
        assert bool(torch.isfinite(self.want).all()) and bool((self.A[self.nk > 0] > 0).all()), f"{c['name']}: the case's inputs leave a tap dead"
        self.nw = c['K'] * c['cin'] * c['cout']
        self.prior = torch.from_numpy(np.random.default_rng(c['seed'] + 11).standard_normal(self.nw).astype(np.float32)).to(dev)

    def query(self):
        c = self.c
        return int(_hip().raw('es_spconv_wgrad_workspace_floats')(int(c['entry'] != 'f32'), self.x.data_ptr(), c['xh'], self.ldx, self.y.data_ptr(),
                                                                  c['yh'], self.ldy, c['n_out'], c['n_in'], c['K'], c['cin'], c['cout']))

    def dw_buffer(self, acc, prior=None):
        c = self.c
        flat = torch.full((PADW + c['dw_off'] + self.nw + PADW,), SENT, dtype=torch.float32, device=self.dev)
        dW = flat[PADW + c['dw_off']:PADW + c['dw_off'] + self.nw]
        dW.copy_(self.prior if prior is None else prior) if acc else dW.fill_(NAN)
        return flat, dW

    def pads_intact(self, flat, label):
        lo = PADW + self.c['dw_off']
        assert bool((flat[:lo] == SENT).all()) and bool((flat[lo + self.nw:] == SENT).all()), f'{label}: a launch wrote outside dW'

    def run(self, acc=None, use_ws=None, short=0, prior=None, launches=None):
        """one launch -> (status, dW pad buffer, dW view); the launch's workspace stays in self.ws"""
        c = self.c
        acc = c['acc'] if acc is None else acc
        use_ws = c['ws'] if use_ws is None else use_ws
        need = self.query()
        assert need == S.workspace_floats(restated_plan(c, True)[0], c['K'], c['cin'], c['cout']), \
            f"{c['name']}: es_spconv_wgrad_workspace_floats = {need}, the restated plan needs {S.workspace_floats(restated_plan(c, True)[0], c['K'], c['cin'], c['cout'])}"
        ws = torch.full((max(need - short, 1),), NAN, dtype=torch.float32, device=self.dev) if use_ws and need else None
        self.ws = ws
        flat, dW = self.dw_buffer(acc, prior)
        if launches is not None:
            launches()
        rc = launch(c, self.x.data_ptr(), self.ldx, self.y.data_ptr(), self.ldy, self.nbr_d.data_ptr() if self.nbr_d is not None else 0,
                    dW.data_ptr(), acc, ws.data_ptr() if ws is not None else 0, need - short if ws is not None else 0)
        _sync()
        if launches is not None and rc == 0:
            p, kernel = restated_plan(c, ws is not None)
            ran = [k.strip('()').replace('<XH, YH>', '') for k in launches()]
            assert ran == [kernel] + ([p.reducer] if p.reducer else []), f"{c['name']}: launched {ran}, the restated plan says {kernel} + {p.reducer}"
        return rc, flat, dW

    def check(self, dW, acc, prior=None, times=1, use_ws=True):
        c = self.c
        p, _ = restated_plan(c, use_ws and c['ws'])
        cls = (f"{'es_spconv_wgrad' if c['entry'] == 'f32' else 'es_spconv_wgrad_bf16'} kind {p.kind} {self.kernel} "
               f"x{'h' if c['xh'] else 'f'} y{'h' if c['yh'] else 'f'} {p.reducer or 'one slice'}")
        pr = (self.prior if prior is None else prior) if acc else None
        got = dW.view(c['K'], c['cin'], c['cout'])
        pr = pr.view_as(got) if pr is not None else None
        if times == 1:
            return S.check(c['name'], got, self.want, self.A, self.nk, pr, cls, STATS)
        # `times` accumulating launches: the sum of the launches' bounds, and one rounding of the running sum per launch
        final = times * self.want + pr.to(S.F64)
        lin, slack = S.bound(final, times * self.A, self.nk, pr.to(S.F64), n_acc=times)
        err = (got.to(S.F64) - final).abs()
        assert bool((err <= S.G * lin + slack).all()), f"{c['name']}: {times} accumulating launches leave the bound"
        return 0.0


def wgrad_case(dev, c, launches=None):
    thin = c['thin_on_emu'] and dev.type == 'cpu'
    set_options(c['opts'])
    try:
        pb = Problem(dev, c, thin)
        rc, flat, dW = pb.run(launches=launches)
        assert rc == 0, (c['name'], rc)
        pb.pads_intact(flat, c['name'])
        ratio = pb.check(dW, c['acc'])
        print(f"{c['name']}: kind {pb.plan.kind} {pb.kernel}, {pb.plan.splits} slices of {pb.plan.rows_per_split} rows, {pb.plan.reducer}, "
              f"{int(pb.nk.sum())} pairs, worst ratio {ratio:.3f}")
    finally:
        restore_options(c['opts'])


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_weight_gradient_per_element(dev, name):
    wgrad_case(dev, next(c for c in CASES if c['name'] == name))


# ------------------------------------------------------------------------------------------------------------------ contracts
CONTRACT_CASES = ['f32-24to72-K8-22slices-acc', 'narrow-385slices-acc', 'lin-64to256-n8192', 'bf16-24to40-K8-11slices',
                  'big-128to256-K8-6slices-x0y1', 'tr32-128to256-K8-6slices', 'tr64-128to256-K8-6slices', 'reduce-513slices']


def contracts_case(dev, c):
    """a workspace one float short: -5 before any launch (dW, its pads and the workspace untouched); no workspace: one slice, the same
    value within the bound; n_out = 0 and Cin = 0: nothing written; two runs: the same bits; accumulate twice: prior + 2 dW"""
    set_options(c['opts'])
    try:
        pb = Problem(dev, c, thin=dev.type == 'cpu')                                 # the contracts do not depend on the pair counts
        assert pb.query() > 0
        for acc in (0, 1):
            rc, flat, dW = pb.run(acc=acc, short=1)
            assert rc == -5, (c['name'], rc)
            pb.pads_intact(flat, c['name'])
            assert bool(torch.isnan(dW).all()) if not acc else torch.equal(dW, pb.prior), f"{c['name']}: dW written by a refused launch"
            assert pb.ws.numel() == pb.query() - 1 and bool(torch.isnan(pb.ws).all()), f"{c['name']}: workspace written by a refused launch"
        rc, flat, dW = pb.run(acc=0, use_ws=False)
        assert rc == 0
        pb.pads_intact(flat, c['name'])
        pb.check(dW, 0, use_ws=False)
        for n_out, cin in ((0, c['cin']), (c['n_out'], 0)):
            flat, dW = pb.dw_buffer(0)
            ws = torch.full((pb.query(),), NAN, device=dev)
            rc = launch(c, pb.x.data_ptr(), pb.ldx, pb.y.data_ptr(), pb.ldy, pb.nbr_d.data_ptr() if pb.nbr_d is not None else 0, dW.data_ptr(), 0,
                        ws.data_ptr(), ws.numel(), n_out=n_out, cin=cin)
            _sync()
            assert rc == 0 and bool(torch.isnan(dW).all()) and bool(torch.isnan(ws).all()), f"{c['name']}: an empty launch wrote"
            pb.pads_intact(flat, c['name'])
        _, _, a = pb.run(acc=1)
        _, _, b = pb.run(acc=1)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{c['name']}: two runs differ"
        pb.check(a, 1)
        rc, flat, twice = pb.run(acc=1, prior=a)
        assert rc == 0
        pb.pads_intact(flat, c['name'])
        pb.check(twice, 1, times=2)
    finally:
        restore_options(c['opts'])


@pytest.mark.parametrize('name', CONTRACT_CASES)
def test_weight_gradient_contracts(dev, name):
    contracts_case(dev, next(c for c in CASES if c['name'] == name))


# ------------------------------------------------------------------------------------------------------------------ es_cast_rows_bf16
def special_floats():
    """ties (both ways), a carry into the exponent, denormals, +-0, +-inf, NaNs with payloads, the largest finite f32 and bf16"""
    bits = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3FFF8000, 0x3FFFFFFF, 0x00000001, 0x00007FFF, 0x00008000, 0x00018000,
            0x007FFFFF, 0x00800000, 0x80000001, 0x80018000, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FC12345,
            0x7F800001, 0xFFC00001, 0x7FFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F7FFF, 0x7F7F8000, 0x477FE000, 0xC77FF000]
    return np.array(bits, dtype=np.uint32).view(np.float32)


def cast_rows_case(dev, n, C, ld, x_off, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, ld)) * np.exp2(rng.integers(-20, 20, size=(n, 1)))).astype(np.float32)
    sp = special_floats()
    xf = x.reshape(-1)
    pos = rng.integers(0, xf.size, size=8 * sp.size)
    xf[pos] = np.tile(sp, 8)
    xf[:min(sp.size, xf.size)] = sp[:xf.size]
    x[:, C:] = np.nan                                                                # the padding columns are never read as values
    flat = torch.zeros(x_off + n * ld + 4, dtype=torch.float32)
    flat[x_off:x_off + n * ld] = torch.from_numpy(x).reshape(-1)
    flat = flat.to(dev)
    xv = flat[x_off:x_off + n * ld].view(n, ld)
    hbuf = torch.full((PADW + n * C + PADW,), -3.0, dtype=torch.bfloat16, device=dev)
    h = hbuf[PADW:PADW + n * C]
    rc = _rc('es_cast_rows_bf16', xv.data_ptr(), ld, n, C, h.data_ptr(), _st())
    _sync()
    label = f'es_cast_rows_bf16 n={n} C={C} ld={ld} base+{4 * x_off}'
    assert bool((hbuf[:PADW] == -3.0).all()) and bool((hbuf[PADW + n * C:] == -3.0).all()), f'{label}: wrote outside its output'
    if C & 1:
        assert rc == -8 and bool((h == -3.0).all()), f'{label}: an odd channel count must be refused before anything is written'
        return
    assert rc == 0, (label, rc)
    want = xv[:, :C].to(torch.bfloat16).reshape(-1)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(h), nan), f'{label}: a NaN is not kept as NaN'
    gi, wi = h.view(torch.int16)[~nan], want.view(torch.int16)[~nan]
    assert torch.equal(gi, wi), f'{label}: {int((gi != wi).sum())} values differ from round-to-nearest-even'


CAST_CASES = [(37, 8, 12, 0), (300, 16, 16, 0), (129, 64, 68, 0), (37, 2, 3, 0), (41, 6, 9, 0), (300, 10, 12, 0), (37, 8, 12, 1), (64, 16, 18, 0),
              (5, 7, 8, 0), (8192 * 256 + 77, 8, 8, 0), (8192 * 256 + 77, 2, 2, 0)]


@pytest.mark.parametrize('n,C,ld,x_off', CAST_CASES)
def test_cast_rows_bf16_bit_exact(dev, n, C, ld, x_off):
    """k_cast_rows8 (C % 8 == 0, ld % 4 == 0, aligned) and k_cast_rows (everything else); the last two cases need a second pass of the
    8192 x 256 grid threads"""
    cast_rows_case(dev, n, C, ld, x_off, n + C)
