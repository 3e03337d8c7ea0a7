"""The row operators held to f64 specifications (tests/rowops_spec.py, tests/fwd_spec.py) on every dispatch branch, with operands
chosen to force what a train step never reaches: the scalar paths (C % 4 != 0, leading dimensions > C, views offset by one float),
the statistics chunk rules at 2^17 / 2^18 rows, empty and one-row segments, nseg = ES_MAX_SEG, the in-place backward, the one-launch
norm cut-off under options 15 / 17 / 9, tied maxima, missing pooling taps, non-integer upsampling ratios, clamped box distances.
Every launch writes into buffers that hold a sentinel outside the view it is given; the sentinel must survive.

Every body is a function of `dev` and of an optional `launched` hook: tests/test_emu_rowops.py runs the same bodies on the CPU
emulator and passes its launch log there, so that each case asserts the kernels its branch label names (the GPU has no launch
log).  Cases of 2^17 rows or more run on the GPU only.  Each body prints the worst bound ratio per launch class."""
import os

import pytest
import torch

import rowops_spec as S

pytestmark = pytest.mark.gpu

BIG = 1 << 17                   # cases with this many rows or more: GPU only
SENT = -7.25e5                  # what a buffer holds outside the view a launch is given
NAN = float('nan')
EPS = float(torch.tensor(1e-5, dtype=torch.float32))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _hip():
    from embodiedscan_amd import hip
    return hip


def _rc(name, *args):
    """the status an entry point returns (hip.call raises on anything but 0)"""
    return _hip().raw(name)(*args)


def _expect(launched, want, label):
    if launched is not None:
        got = launched()
        assert got == want, f'{label}: launched {got}, its branch label names {want}'


class Buf:
    """an (rows, C) f32 view with leading dimension ld, `off` floats into a buffer that holds SENT everywhere else"""

    def __init__(self, dev, rows, C, ld=None, off=0, init=None):
        self.rows, self.C, self.ld, self.off = rows, C, C if ld is None else ld, off
        self.buf = torch.full((rows * self.ld + off + 8,), SENT, dtype=torch.float32, device=dev)
        self.v = self._view(self.buf)
        if isinstance(init, float):
            self.v.fill_(init)
        elif init is not None:
            self.v.copy_(init)

    def _view(self, b):
        return b[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)[:, :self.C]

    def ptr(self):
        return self.v.data_ptr()

    def outside_untouched(self, label):
        b = self.buf.clone()
        self._view(b).fill_(SENT)
        if not bool((b == SENT).all()):
            raise AssertionError(f'{label}: a launch wrote outside the ({self.rows}, {self.C}) view (ld {self.ld}, offset {self.off})')


def _gen(seed, dev=None):
    """a generator on the host, or on `dev` (the norm cases: 10^6-row operands are drawn where they are used)"""
    return torch.Generator(device=dev if dev is not None else 'cpu').manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(shape, generator=g, device=g.device)


# ------------------------------------------------------------------------------------------------------------------ norm
# branch labels: the kernels es_norm_fwd / es_norm_bwd launch on each
FWD_K = {'one-launch': ['k_norm_fwd_cb'], 'chunked': ['k_norm_stats', 'k_norm_finalize', 'k_norm_apply4'],
         'scalar': ['k_norm_stats', 'k_norm_finalize', 'k_norm_apply']}


def _bwd_kernels(path, inplace):
    if path == 'one-launch' and not inplace:
        return ['k_norm_bwd_cb']
    apply = 'k_norm_bwd_apply4' if path != 'scalar' and not inplace else 'k_norm_bwd_apply'     # (dx == dy: the scalar apply)
    return ['k_norm_bwd_stats', 'k_norm_bwd_finalize', apply]


# (act, residual, accumulate, bf16 shadows, in-place dx == dy, running statistics): every act with and without a residual, both
# accumulate values and a shadow for every act, the in-place backward once
VARIANTS = ((0, 0, 0, 1, 0, 1), (0, 1, 1, 0, 0, 0), (1, 0, 1, 0, 0, 1), (1, 1, 0, 1, 0, 0), (2, 0, 0, 0, 1, 0), (2, 1, 1, 1, 0, 0))


def _norm_x(g, n, C):
    """random rows and the statistics edges: channel 0 constant (var = 0), channel 1 at |mean| / std = 1e4, channel 2 with row 0 an
    outlier at 1e3 std (the kernels sum about the first row), channel 3 all zero"""
    x = _randn(g, n, C) * 2 + 1
    if n:
        x[:, 0] = 0.1
        if C > 1:
            x[:, 1] = 1e4 + _randn(g, n)
        if C > 2:
            x[0, 2] = 1 + 2e3
        if C > 3:
            x[:, 3] = 0
    return x


def _norm_run(dev, st, g, label, sizes, C, path, ld, off, var, launched, cast='k_cast_rows'):
    """one forward + backward pair on one variant; path: the branch label, or (forward label, backward label)"""
    hip = _hip()
    P = hip.P
    act, use_res, acc, shadow, inplace, running = var
    fpath, bpath = path if isinstance(path, tuple) else (path, path)
    so = [0]
    for s in sizes:
        so.append(so[-1] + s)
    n, nseg = so[-1], len(sizes)
    shadow = bool(shadow) and C % 2 == 0
    running = bool(running) and nseg == 1
    name = f'{label} [act={act} res={use_res} acc={acc}{" shadows" if shadow else ""}{" in-place" if inplace else ""}]'
    x = Buf(dev, n, C, ld, off, _norm_x(g, n, C))
    res = Buf(dev, n, C, ld, off, _randn(g, n, C)) if use_res else None
    w = ((torch.rand(C, generator=g, device=g.device) + 0.5) * torch.where(torch.rand(C, generator=g, device=g.device) < 0.25, -1.0, 1.0)).to(dev)
    b = (_randn(g, C) * 0.3).to(dev)
    rm0, rv0 = _randn(g, C).to(dev), (torch.rand(C, generator=g, device=g.device) + 0.5).to(dev)
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd = torch.full((nseg, C), NAN, device=dev), torch.full((nseg, C), NAN, device=dev)
    segs = hip.iarr(so)
    ws = torch.zeros(int(_rc('es_norm_workspace_floats', n, C, segs, nseg)) + 2 * nseg * C, device=dev)
    y = Buf(dev, n, C, ld, off, NAN)
    yh = torch.full((n, C), NAN, dtype=torch.bfloat16, device=dev) if shadow else None
    hip.call('es_norm_fwd', x.ptr(), ld, n, C, segs, nseg, EPS, P(w), P(b), res.ptr() if res else 0, ld, act, P(rm) if running else 0,
             P(rv) if running else 0, 0.1, P(mean), P(invstd), P(ws), y.ptr(), ld, P(yh), hip.stream())
    _expect(launched, FWD_K[fpath] + ([cast] if shadow and fpath == 'scalar' else []), name + ' forward')
    S.check_norm(dict(x=x.v, seg_off=so, mean=mean, invstd=invstd, eps=EPS, w=w, b=b, res=res.v if res else None, act=act, y=y.v,
                      yh=yh, rm0=rm0 if running else None, rm1=rm, rv0=rv0, rv1=rv, momentum=0.1), dev, st)
    y.outside_untouched(name + ' forward y')
    dy = Buf(dev, n, C, ld, off, _randn(g, n, C))
    dy0 = dy.v.clone()
    dx = dy if inplace else Buf(dev, n, C, ld, off, _randn(g, n, C) if acc else NAN)
    dx0 = dx.v.clone() if acc else None
    dxh = torch.full((n, C), NAN, dtype=torch.bfloat16, device=dev) if shadow else None
    dw0, db0 = _randn(g, C).to(dev), _randn(g, C).to(dev)
    dw, db = dw0.clone(), db0.clone()
    hip.call('es_norm_bwd', dy.ptr(), ld, y.ptr(), ld, x.ptr(), ld, n, C, segs, nseg, P(mean), P(invstd), P(w), act, P(dw), P(db), P(ws),
             dx.ptr(), ld, acc, P(dxh), hip.stream())
    _expect(launched, _bwd_kernels(bpath, inplace) + ([cast] if shadow and (bpath == 'scalar' or inplace) else []), name + ' backward')
    S.check_norm_bwd(dict(x=x.v, seg_off=so, mean=mean, invstd=invstd, w=w, act=act, y=y.v, dy0=dy0, dz=None if inplace else dy.v,
                          dx0=dx0, dx=dx.v, dw0=dw0, dw1=dw, db0=db0, db1=db, dxh=dxh), dev, st,
                     f'norm_bwd {bpath}{" in-place" if inplace else ""}')
    dx.outside_untouched(name + ' backward dx')
    dy.outside_untouched(name + ' backward dy')


def _norm_cases(dev, st, cases, launched):
    for label, sizes, C, pad, off, path in cases:
        if dev.type == 'cpu' and sum(sizes) >= BIG:
            continue
        g = _gen(sum(sizes) * 131 + C, dev)
        for var in VARIANTS:
            _norm_run(dev, st, g, label, sizes, C, path, C + pad, off, var, launched)


NORM_BRANCHES = [
    # (label, segment sizes, C, ld - C, view offset in floats, branch)
    *[(f'one-launch: {n} rows, C = {C}', (n,), C, 0, 0, 'one-launch') for n in (1, 2, 17, 4096) for C in (16, 64, 512)],
    ('chunked float4: 4097 rows, one past the one-launch cut-off', (4097,), 64, 0, 0, 'chunked'),
    ('chunked float4: C = 20 is no multiple of 16', (300,), 20, 0, 0, 'chunked'),
    ('chunked float4: C = 20, ld = 28, 4097 rows', (4097,), 20, 8, 0, 'chunked'),
    ('scalar: C = 3, ld = 5', (500,), 3, 2, 0, 'scalar'),
    ('scalar: C = 7, ld = 10', (1000,), 7, 3, 0, 'scalar'),
    ('scalar: C = 24, ld = 29', (700,), 24, 5, 0, 'scalar'),
    ('scalar: C = 24, view offset by one float', (700,), 24, 0, 1, 'scalar'),
    ('scalar: C = 64, 300 rows, view offset by one float', (300,), 64, 0, 1, 'scalar'),
]
NORM_SEGMENTS = [
    ('segments: 2, one of them empty', (0, 777), 64, 0, 0, 'chunked'),
    ('segments: 7, sizes 0 / 1 / odd', (1, 0, 5, 300, 1, 129, 64), 64, 0, 0, 'chunked'),
    ('segments: 32 = ES_MAX_SEG, sizes 0 .. 97', tuple((i * 37) % 98 if i % 5 else i % 2 for i in range(32)), 16, 0, 0, 'chunked'),
    ('segments, scalar: 5, C = 24, ld = 29', (3, 0, 1, 200, 40), 24, 5, 0, 'scalar'),
    ('segments: 2^17 + 1 rows beside tiny ones', (3, 131073, 0, 1), 64, 0, 0, 'chunked'),
]
# the statistics chunk rule (norm_chunk_rows): 128 rows up to 2^17 rows, 256 up to 2^18, 512 beyond -> chunks per segment
NORM_CHUNK_RULE = [((131072,), 1024), ((131073,), 513), ((262145,), 513), ((1200000,), 2344)]


def test_norm_every_branch(dev, launched=None):
    st = S.Stats('norm branches')
    _norm_cases(dev, st, NORM_BRANCHES, launched)
    print(st.report())


def test_norm_segments(dev, launched=None):
    st = S.Stats('norm segments')
    _norm_cases(dev, st, NORM_SEGMENTS, launched)
    print(st.report())


def test_norm_chunk_rules_and_production_size(dev):
    """2^17 / 2^17 + 1 / 2^18 + 1 rows (128 / 256 / 512-row statistics chunks, read back through the workspace size) and one
    production-size matrix (1.2 M x 64, the finest level of an mv-3ddet step)"""
    hip = _hip()
    st = S.Stats('norm chunk rules')
    for sizes, chunks in NORM_CHUNK_RULE:
        n = sum(sizes)
        assert int(_rc('es_norm_workspace_floats', n, 64, hip.iarr([0, n]), 1)) == chunks * 2 * 64, (sizes, chunks)
    cases = [(f'chunk rule: {sizes[0]} rows', sizes, 64, 0, 0, 'chunked') for sizes, _ in NORM_CHUNK_RULE]
    _norm_cases(dev, st, cases, None)
    print(st.report())


def test_norm_refuses_33_segments(dev, launched=None):
    """nseg = ES_MAX_SEG + 1: -3 from both entry points, and no output touched"""
    hip = _hip()
    P = hip.P
    assert hip.CONSTS['ES_MAX_SEG'] == 32
    n, C = 33, 16
    so = hip.iarr(range(34))
    g = _gen(33)
    x, dy = _randn(g, n, C).to(dev), _randn(g, n, C).to(dev)
    dy0 = dy.clone()
    w, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    rm, rv, dw, db = (_randn(g, C).to(dev) for _ in range(4))
    keep = [t.clone() for t in (rm, rv, dw, db)]
    mean, invstd = torch.full((33, C), NAN, device=dev), torch.full((33, C), NAN, device=dev)
    y, dx = torch.full((n, C), NAN, device=dev), torch.full((n, C), NAN, device=dev)
    ws = torch.zeros(33 * 2 * C * 2, device=dev)
    assert _rc('es_norm_fwd', P(x), C, n, C, so, 33, EPS, P(w), P(b), 0, C, 1, P(rm), P(rv), 0.1, P(mean), P(invstd), P(ws), P(y), C, 0,
               hip.stream()) == -3
    assert _rc('es_norm_bwd', P(dy), C, P(x), C, P(x), C, n, C, so, 33, P(x), P(x), P(w), 1, P(dw), P(db), P(ws), P(dx), C, 0, 0,
               hip.stream()) == -3
    _expect(launched, [], 'nseg = 33')
    assert bool(mean.isnan().all() and invstd.isnan().all() and y.isnan().all() and dx.isnan().all())
    assert torch.equal(dy, dy0) and all(torch.equal(a, k) for a, k in zip((rm, rv, dw, db), keep))


def test_norm_options_select_paths_that_all_meet_the_specification(dev, launched=None):
    """the same inputs under es_set_option 15 (one-launch row cut-off), 17 (one-launch backward) and 9 (rows per statistics chunk,
    1 included): every path meets the specification; the options are restored whatever happens"""
    hip = _hip()
    d15 = int(os.environ.get('ES_NORM_CB_ROWS', 4096))

    def defaults():
        hip.call('es_set_option', 15, d15)
        hip.call('es_set_option', 17, 1)
        hip.call('es_set_option', 9, 0)
    st = S.Stats('norm options')
    states = (({}, 'one-launch', (1000,)), ({17: 0}, ('one-launch', 'chunked'), (1000,)), ({15: 0}, 'chunked', (1000,)),
              ({15: 0, 9: 1}, 'chunked', (1000,)), ({15: 6000}, 'one-launch', (5000,)), ({9: 1}, 'chunked', (3, 0, 1, 200, 40)),
              ({9: 7}, 'chunked', (3, 0, 1, 200, 40)))
    try:
        for opts, path, sizes in states:
            defaults()
            for k, v in opts.items():
                hip.call('es_set_option', k, v)
            label = f'options {opts or "default"}: {sizes} rows, C = 64'
            g = _gen(sum(sizes), dev)                     # the same inputs under every option state
            for var in VARIANTS:
                _norm_run(dev, st, g, label, sizes, 64, path, 64, 0, var, launched)
    finally:
        defaults()
    print(st.report())


# ------------------------------------------------------------------------------------------------------------------ affine_act
def test_affine_act_every_branch(dev, launched=None):
    """es_affine_act_fwd / _bwd / _bwd_yh: the float4 and the scalar backward (C in {3, 6, 64}, pointers offset by one float), act 0 / 1
    / 2, every combination of dx / dres being NULL, overwritten or accumulated; the _yh refusals (-7: C % 4 != 0 or misaligned; -2:
    act = 2) write nothing"""
    hip = _hip()
    P = hip.P
    st = S.Stats('affine_act')
    g = _gen(17)
    for C, off, n in ((64, 0, 64), (64, 1, 64), (6, 0, 67), (3, 0, 257), (3, 1, 257)):
        v4 = C % 4 == 0 and off == 0
        label = f'affine_act {"float4" if v4 else "scalar"}: C = {C}, offset {off}'
        x, res = Buf(dev, n, C, C, off, _randn(g, n, C) * 2), Buf(dev, n, C, C, off, _randn(g, n, C))
        sc, sh = Buf(dev, 1, C, C, off, torch.rand(1, C, generator=g) + 0.5), Buf(dev, 1, C, C, off, _randn(g, 1, C))
        for act in (0, 1, 2):
            y = Buf(dev, n, C, C, off, torch.full((n, C), NAN))
            hip.call('es_affine_act_fwd', x.ptr(), sc.ptr(), sh.ptr(), res.ptr(), n, C, act, y.ptr(), hip.stream())
            _expect(launched, ['k_affine_act'], label + ' forward')
            S.check_affine_act(dict(x=x.v, scale=sc.v, shift=sh.v, res=res.v, act=act, y=y.v), dev, st)
            y.outside_untouched(label + ' forward')
            yv = y.v.clone()
            yv[::13] = 0.0                                  # the activation's boundary: y = 0 passes no gradient under ReLU
            y.v.copy_(yv)
            yh = y.v.to(torch.bfloat16).contiguous()        # the image backbone's bf16 copy of y
            dy = Buf(dev, n, C, C, off, _randn(g, n, C))
            for mx in (None, 0, 1):                         # dx: NULL / overwritten / accumulated
                for mr in (None, 0, 1):                     # dres likewise
                    outs = {}
                    for yy, entry in ((y, 'es_affine_act_bwd'), (yh, 'es_affine_act_bwd_yh')):
                        dx = Buf(dev, n, C, C, off, _randn(g, n, C) if mx else torch.full((n, C), NAN)) if mx is not None else None
                        dr = Buf(dev, n, C, C, off, _randn(g, n, C) if mr else torch.full((n, C), NAN)) if mr is not None else None
                        dx0, dr0 = (dx.v.clone() if dx else None), (dr.v.clone() if dr else None)
                        yp = yy.ptr() if entry == 'es_affine_act_bwd' else P(yy)
                        rc = _rc(entry, dy.ptr(), yp, sc.ptr(), n, C, act, dx.ptr() if dx else 0, mx or 0, dr.ptr() if dr else 0,
                                 mr or 0, hip.stream())
                        tag = f'{label} {entry} act {act} dx {mx} dres {mr}'
                        if entry == 'es_affine_act_bwd_yh' and (act == 2 or not v4):
                            assert rc == (-2 if act == 2 else -7), (tag, rc)
                            _expect(launched, [], tag + ' (refused)')
                            for bb, b0 in ((dx, dx0), (dr, dr0)):
                                if bb is not None:
                                    assert torch.equal(bb.v.nan_to_num(1.5), b0.nan_to_num(1.5)), f'{tag}: a refused launch wrote'
                            continue
                        assert rc == 0, (tag, rc)
                        kern = 'k_affine_act_bwd4_yh' if entry == 'es_affine_act_bwd_yh' else ('k_affine_act_bwd4' if v4 else 'k_affine_act_bwd')
                        _expect(launched, [kern], tag)
                        S.check_affine_act_bwd(dict(dy=dy.v, y=yy.v if entry == 'es_affine_act_bwd' else yy, scale=sc.v, act=act,
                                                    dx0=dx0 if mx else None, dx=dx.v if dx else None, acc_x=mx,
                                                    dres0=dr0 if mr else None, dres=dr.v if dr else None, acc_r=mr), dev, st, kern)
                        for bb in (dx, dr):
                            if bb is not None:
                                bb.outside_untouched(tag)
    print(st.report())


# ------------------------------------------------------------------------------------------------------------------ max pooling
def test_maxpool_ties_missing_taps_empty_windows(dev, launched=None):
    """disjoint windows of 0 .. 8 taps in random tap slots (-1 elsewhere), three windows without a tap (y = -inf, arg = -1, no
    gradient), values from seven levels (ties between taps in most windows: the first tap wins), ldx = 24 and ldo = 28 > C = 20; the
    backward adds onto a non-zero prior"""
    hip = _hip()
    P = hip.P
    st = S.Stats('maxpool')
    g = _gen(21)
    n_in, K, C, ldx, ldo = 3000, 8, 20, 24, 28
    perm = torch.randperm(n_in, generator=g).tolist()
    rows, i = [], 0
    while i < n_in:
        row = [-1] * K
        for p in torch.randperm(K, generator=g)[:int(torch.randint(0, K + 1, (1,), generator=g))].tolist():
            if i < n_in:
                row[p], i = perm[i], i + 1
        rows.append(row)
    rows[3:3] = [[-1] * K] * 3
    nbr = torch.tensor(rows, dtype=torch.int32, device=dev)
    n_out = nbr.shape[0]
    x = Buf(dev, n_in, C, ldx, 0, torch.randint(-3, 4, (n_in, C), generator=g).float())
    y = torch.full((n_out, C), NAN, device=dev)
    arg = torch.full((n_out, C), -7, dtype=torch.int32, device=dev)
    hip.call('es_maxpool_fwd', x.ptr(), ldx, P(nbr), n_out, K, C, P(y), P(arg), hip.stream())
    _expect(launched, ['k_maxpool_fwd'], 'maxpool forward')
    S.check_maxpool_first_tap(dict(entry='es_maxpool_fwd', x=x.v, nbr=nbr, y=y, arg=arg), dev, st)
    assert bool(torch.isneginf(y[3:6]).all()) and bool((arg[3:6] == -1).all())
    dy = _randn(g, n_out, C).to(dev)
    dx = Buf(dev, n_in, C, ldo, 0, _randn(g, n_in, C))
    dx0 = dx.v.clone()
    hip.call('es_maxpool_bwd', P(dy), P(arg), n_out, C, dx.ptr(), ldo, hip.stream())
    _expect(launched, ['k_maxpool_bwd'], 'maxpool backward')
    S.check_maxpool_bwd('maxpool', dx.v, dx0, dy, arg, st)
    dx.outside_untouched('maxpool backward')
    print(st.report())


def test_minkresnet_pool_map_has_disjoint_windows(dev):
    """k_maxpool_bwd adds without atomics: race-free only because no input row lies in two windows.  The map MinkResNet pools
    through, CoordSet.kernel_map(strided, 2), on a synthetic two-sample scan, three levels down: every row of the finer set in
    exactly one window"""
    from test_gpu_ops import _sparse_case
    cs, _ = _sparse_case(dev, 6000, 9)
    for level in range(3):
        out = cs.strided(2)
        nbr = cs.kernel_map(out, 2)
        v = nbr[nbr >= 0].long()
        assert v.numel() == cs.n and torch.unique(v).numel() == cs.n, (level, v.numel(), cs.n)
        cs = out


# ------------------------------------------------------------------------------------------------------------------ row moves
def test_row_move_axpy_relu(dev, launched=None):
    """es_row_move modes 0 / 1 / 2 on the float4 and the scalar path, idx NULL or holding -1; es_axpy2d op 0 / 1 with alpha != 1 on
    strided operands; es_relu_fwd / _bwd with y = 0 and -0.0.  All exact."""
    hip = _hip()
    P = hip.P
    st = S.Stats('row moves')
    g = _gen(31)
    n, m = 300, 420
    for C, ldd, lds, off, kern in ((8, 12, 16, 0, 'k_row_move4'), (5, 7, 9, 0, 'k_row_move'), (8, 8, 8, 1, 'k_row_move')):
        for mode in (0, 1, 2):
            for with_idx in (False, True):
                label = f'row_move mode {mode} {kern} C = {C} ld {ldd} / {lds} offset {off} idx {"with -1" if with_idx else "NULL"}'
                src_rows, dst_rows = (m, n) if mode == 0 else (n, m)
                idx = None
                if with_idx:
                    idx = (torch.randint(0, src_rows, (n,), generator=g) if mode == 0 else torch.randperm(m, generator=g)[:n]).int()
                    idx[::7] = -1
                    idx = idx.to(dev)
                src = Buf(dev, src_rows, C, lds, off, _randn(g, src_rows, C))
                dst = Buf(dev, dst_rows, C, ldd, off, _randn(g, dst_rows, C))
                d0 = dst.v.clone()
                hip.call('es_row_move', dst.ptr(), ldd, src.ptr(), lds, P(idx), n, C, mode, hip.stream())
                _expect(launched, [kern], label)
                want = d0.clone()
                ii = torch.arange(n, device=dev) if idx is None else idx.long()
                live = ii >= 0
                rows, r = torch.arange(n, device=dev)[live], ii[live]
                if mode == 0:
                    want[rows] = src.v[r]
                elif mode == 1:
                    want[r] = d0[r] + src.v[rows]
                else:
                    want[r] = src.v[rows]
                S.exact(label, dst.v, want, st, f'row_move mode {mode}')
                dst.outside_untouched(label)
    for op in (0, 1):
        label = f'axpy2d op {op}'
        src, dst = Buf(dev, 77, 13, 19, 1, _randn(g, 77, 13)), Buf(dev, 77, 13, 17, 0, _randn(g, 77, 13))
        d0 = dst.v.clone()
        alpha = float(torch.tensor(0.37, dtype=torch.float32))
        hip.call('es_axpy2d', dst.ptr(), 17, src.ptr(), 19, 77, 13, alpha, op, hip.stream())
        _expect(launched, ['k_axpy2d'], label)
        want = torch.tensor(alpha, dtype=torch.float32, device=dev) * src.v
        S.exact(label, dst.v, want + d0 if op else want, st, label)
        dst.outside_untouched(label)
    xr = _randn(g, 1003)
    xr[::9], xr[4::9] = 0.0, -0.0
    x = xr.to(dev)
    hip.call('es_relu_fwd', P(x), x.numel(), hip.stream())
    _expect(launched, ['k_relu_fwd'], 'relu forward')
    S.exact('relu forward', x, torch.where(xr > 0, xr, torch.zeros_like(xr)).to(dev), st, 'relu')
    yb = xr.clone()
    yb[5::9] = -0.0
    y, dy0 = yb.to(dev), _randn(g, 1003).to(dev)
    dy = dy0.clone()
    hip.call('es_relu_bwd', P(dy), P(y), y.numel(), hip.stream())
    _expect(launched, ['k_relu_bwd'], 'relu backward')
    S.exact('relu backward', dy, torch.where(y > 0, dy0, torch.zeros_like(dy0)), st, 'relu')
    print(st.report())


# ------------------------------------------------------------------------------------------------------------------ FPN upsampling
# (Hf, Wf, Hc, Wc).  The last: one row of 11819 fine pixels over 7879 coarse ones, where the f32 scale of the nearest rule sends a
# fine pixel outside [floor(wc Wf / Wc), floor((wc + 1) Wf / Wc)] (asserted below): what the -1 / +1 margins of
# k_upsample_add_bwd's candidate window are for
UPSAMPLE = [(120, 160, 60, 80), (30, 40, 15, 20), (15, 20, 8, 10), (7, 9, 3, 4), (5, 5, 5, 5), (4, 6, 7, 9), (1, 11819, 1, 7879)]


def _outside_window(Wf, Wc, margin):
    """fine pixels the candidate window of their own coarse pixel (the f32 nearest rule) misses"""
    s = torch.tensor(Wc, dtype=torch.float32) / torch.tensor(Wf, dtype=torch.float32)
    d = torch.arange(Wf)
    src = torch.floor(d.float() * s).long().clamp(max=Wc - 1)
    return int(((d < src * Wf // Wc - margin) | (d > (src + 1) * Wf // Wc + margin)).sum())


def test_upsample_nearest_add(dev, launched=None):
    """fwd exact against fine + F.interpolate(coarse, size, mode='nearest') in f32; bwd against f64 autograd of F.interpolate, with
    accumulate 0 / 1, integer and non-integer ratios, Hf < Hc; C % 4 != 0 returns -4 and writes nothing"""
    import torch.nn.functional as F
    hip = _hip()
    P = hip.P
    st = S.Stats('upsample')
    g = _gen(41)
    assert _outside_window(UPSAMPLE[-1][1], UPSAMPLE[-1][3], 0) > 0 and _outside_window(UPSAMPLE[-1][1], UPSAMPLE[-1][3], 1) == 0
    NI, C = 2, 8
    for Hf, Wf, Hc, Wc in UPSAMPLE:
        for acc in (0, 1):
            label = f'upsample {Hf}x{Wf} <- {Hc}x{Wc} acc {acc}'
            fine0, coarse = _randn(g, NI, Hf, Wf, C).to(dev), _randn(g, NI, Hc, Wc, C).to(dev)
            fine = fine0.clone()
            hip.call('es_upsample_nearest_add_fwd', P(fine), P(coarse), NI, Hf, Wf, Hc, Wc, C, hip.stream())
            _expect(launched, ['k_upsample_add_fwd'], label + ' forward')
            up = F.interpolate(coarse.permute(0, 3, 1, 2), size=(Hf, Wf), mode='nearest').permute(0, 2, 3, 1)
            S.exact(label + ' forward', fine, fine0 + up, st, 'upsample_fwd')
            dfine = _randn(g, NI, Hf, Wf, C).to(dev)
            dco = _randn(g, NI, Hc, Wc, C).to(dev) if acc else torch.full((NI, Hc, Wc, C), NAN, device=dev)
            d0 = dco.clone()
            hip.call('es_upsample_nearest_add_bwd', P(dfine), P(dco), NI, Hf, Wf, Hc, Wc, C, acc, hip.stream())
            _expect(launched, ['k_upsample_add_bwd'], label + ' backward')
            S.check_upsample_bwd(label, dco, dfine, d0 if acc else None, Hc, Wc, st)
    f6, c6 = torch.zeros(1, 4, 4, 6, device=dev), torch.ones(1, 2, 2, 6, device=dev)
    assert _rc('es_upsample_nearest_add_fwd', P(f6), P(c6), 1, 4, 4, 2, 2, 6, hip.stream()) == -4
    assert _rc('es_upsample_nearest_add_bwd', P(f6), P(c6), 1, 4, 4, 2, 2, 6, 0, hip.stream()) == -4
    _expect(launched, [], 'upsample C = 6')
    assert bool((f6 == 0).all()) and bool((c6 == 1).all())
    print(st.report())


# ------------------------------------------------------------------------------------------------------------------ head kernels
def test_reg_decode_on_the_head_layout(dev, launched=None):
    """es_reg_decode_fwd / _bwd on the head's real layout: reg = columns 1 .. 12 of an (n, 13 + C) matrix (4-byte offset, strided);
    rows clamped at 1e-3, scale != 1, dscale accumulating onto a non-zero value, n past the 512-block cap of k_reg_decode_bwd; two
    runs bit-identical; the other columns of the gradient matrix untouched"""
    hip = _hip()
    P = hip.P
    st = S.Stats('reg_decode')
    g = _gen(51)
    n, ncls = 20000, 18
    ld = 13 + ncls
    assert n * 12 > 512 * 256                               # more elements than the 512 capped blocks have threads
    mat = _randn(g, n, ld) * 0.6
    mat[::7, 1:7] = -20.0                                   # exp(-14) < 1e-3: whole rows clamped
    mat[3::11, 2] = -12.0                                   # single clamped distances
    ho = mat.to(dev)
    reg = ho[:, 1:13]
    scale = torch.tensor([0.7], device=dev)
    bbox = torch.full((n, 12), NAN, device=dev)
    hip.call('es_reg_decode_fwd', ho.data_ptr() + 4, ld, n, P(scale), P(bbox), hip.stream())
    _expect(launched, ['k_reg_decode'], 'reg decode forward')
    S.check_reg_decode_fwd('reg decode', reg, scale, bbox, st)
    assert int((bbox[:, :6] == float(torch.tensor(1e-3, dtype=torch.float32))).sum()) > n // 7 * 6
    dbbox = _randn(g, n, 12).to(dev)
    gm0 = _randn(g, n, ld).to(dev)
    runs = []
    for _ in range(2):
        gm, dscale = gm0.clone(), torch.tensor([0.25], device=dev)
        partial = torch.full((512,), NAN, device=dev)
        hip.call('es_reg_decode_bwd', ho.data_ptr() + 4, ld, P(bbox), P(dbbox), n, P(scale), gm.data_ptr() + 4, ld, P(dscale),
                 P(partial), hip.stream())
        _expect(launched, ['k_reg_decode_bwd', 'k_sum_partials_add'], 'reg decode backward')
        S.check_reg_decode_bwd('reg decode', reg, bbox, dbbox, scale, gm[:, 1:13], torch.tensor([0.25]), dscale, st)
        assert torch.equal(gm[:, 0], gm0[:, 0]) and torch.equal(gm[:, 13:], gm0[:, 13:]), 'reg decode backward wrote outside dreg'
        runs.append((gm, dscale))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), 'dscale differs between two identical runs'
    print(st.report())


def test_interp_scores_row_max_argmax_bn_fold(dev, launched=None):
    """es_interp_scores with absent corners (8 u sum|w score|); es_row_max / es_row_argmax with ldx > C, C no multiple of 64 and ties
    (exact; argmax: the lowest index); es_bn_fold (a few u)"""
    hip = _hip()
    P = hip.P
    st = S.Stats('head helpers')
    g = _gen(61)
    n, m = 1000, 500
    idx = torch.randint(-1, m, (n, 8), generator=g).int()
    idx[::5, :3] = -1
    idx[7] = -1
    w, score = torch.rand(n, 8, generator=g), _randn(g, m)
    out = torch.full((n,), NAN, device=dev)
    idd, wd, sd = idx.to(dev), w.to(dev), score.to(dev)
    hip.call('es_interp_scores', P(sd), P(idd), P(wd), n, P(out), hip.stream())
    _expect(launched, ['k_interp_scores'], 'interp scores')
    S.check_interp_scores('interp scores', sd, idd, wd, out, st)
    assert float(out[7]) == 0.0
    for C, ldx in ((100, 104), (37, 40), (64, 64), (130, 131)):
        label = f'row max / argmax C = {C} ldx = {ldx}'
        x = Buf(dev, n, C, ldx, 0, torch.randint(-4, 5, (n, C), generator=g).float())
        mx = torch.full((n,), NAN, device=dev)
        hip.call('es_row_max', x.ptr(), ldx, n, C, P(mx), hip.stream())
        _expect(launched, ['k_row_max'], label)
        S.exact(label + ' max', mx, x.v.max(1).values, st, 'row_max')
        am = torch.full((n,), -5, dtype=torch.int32, device=dev)
        hip.call('es_row_argmax', x.ptr(), ldx, n, C, P(am), hip.stream())
        _expect(launched, ['k_row_argmax'], label)
        cols = torch.arange(C, device=dev).expand(n, C)
        want = torch.where(x.v == x.v.max(1, keepdim=True).values, cols, torch.full_like(cols, C)).min(1).values.int()
        S.exact(label + ' argmax (ties: the lowest index)', am, want, st, 'row_argmax')
    C = 100
    wv, bv, rm, rv = _randn(g, C), _randn(g, C), _randn(g, C) * 3, torch.rand(C, generator=g) * 2 + 1e-3
    wv, bv, rm, rv = (t.to(dev) for t in (wv, bv, rm, rv))
    sc, sh = torch.full((C,), NAN, device=dev), torch.full((C,), NAN, device=dev)
    hip.call('es_bn_fold', P(wv), P(bv), P(rm), P(rv), C, EPS, P(sc), P(sh), hip.stream())
    _expect(launched, ['k_bn_fold'], 'bn fold')
    S.check_bn_fold('bn fold', wv, bv, rm, rv, EPS, sc, sh, st)
    print(st.report())
