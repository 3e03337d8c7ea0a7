"""es_norm_bwd with dx = NULL (the bf16 rows are the gradient's only copy: engine.GRAD_ROWS_BF16) against the same call with dx given:
dx_bf16, dweight, dbias and the in-place dz are bit-equal, on the one-launch path (one segment, at most 4096 rows, C % 16 == 0), the
chunked path (4097 rows, or three segments) and the scalar path (C % 4 != 0, where the call with dx makes its shadow with a cast
launch and the call without writes it from the apply kernel).  Rows {1, 130, 4096, 4097} x C {16, 64, 256} x {1, 3} segments x act
{0, 1, 2} x {no residual, residual}.  The residual enters through the forward pass only (the stored y decides act'(y)).

Every body is a function of `dev` and an optional `launched` hook: tests/test_emu_norm_bwd_null_dx.py runs the same bodies on the CPU
emulator and asserts the kernels each call launches."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = float(torch.tensor(1e-5, dtype=torch.float32))
ROWS = (1, 130, 4096, 4097)
CHANNELS = (16, 64, 256)
LONG = ['k_norm_bwd_stats', 'k_norm_bwd_finalize', 'k_norm_bwd_apply4']
SCALAR = ['k_norm_bwd_stats', 'k_norm_bwd_finalize', 'k_norm_bwd_apply']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _hip():
    from embodiedscan_amd import hip
    return hip


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _sizes(rows, nseg):
    if nseg == 1:
        return [rows]
    a, b = rows // 3, rows // 4                 # (one row: an empty, a one-row and an empty segment)
    return [a, rows - a - b, b]


def _setup(dev, rows, C, nseg, act, use_res, seed):
    """one forward pass -> everything es_norm_bwd reads"""
    hip = _hip()
    P = hip.P
    g = torch.Generator().manual_seed(seed)
    so = [0]
    for s in _sizes(rows, nseg):
        so.append(so[-1] + s)
    x = (torch.randn(rows, C, generator=g) * 2 + 1).to(dev)
    res = torch.randn(rows, C, generator=g).to(dev) if use_res else None
    w = ((torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)).to(dev)
    b = (torch.randn(C, generator=g) * 0.3).to(dev)
    mean, invstd = torch.zeros((nseg, C), device=dev), torch.zeros((nseg, C), device=dev)
    segs = hip.iarr(so)
    ws = torch.zeros(int(hip.raw('es_norm_workspace_floats')(rows, C, segs, nseg)) + 2 * nseg * C, device=dev)
    y = torch.zeros((rows, C), device=dev)
    hip.call('es_norm_fwd', P(x), C, rows, C, segs, nseg, EPS, P(w), P(b), P(res), C, act, 0, 0, 0.1, P(mean), P(invstd), P(ws), P(y), C, 0,
             hip.stream())
    dy = torch.randn(rows, C, generator=g).to(dev)
    dw, db = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    return dict(x=x, y=y, w=w, mean=mean, invstd=invstd, segs=segs, nseg=nseg, ws=ws, dy=dy, dw=dw, db=db, n=rows, C=C, act=act)


def _bwd(dev, c, with_dx, launched):
    hip = _hip()
    P = hip.P
    n, C = c['n'], c['C']
    dy, dw, db = c['dy'].clone(), c['dw'].clone(), c['db'].clone()
    dx = torch.full((n, C), float('nan'), device=dev) if with_dx else None
    dxh = torch.full((n, C), float('nan'), dtype=torch.bfloat16, device=dev)
    ws = torch.zeros_like(c['ws'])
    if launched is not None:
        launched()
    hip.call('es_norm_bwd', P(dy), C, P(c['y']), C, P(c['x']), C, n, C, c['segs'], c['nseg'], P(c['mean']), P(c['invstd']), P(c['w']),
             c['act'], P(dw), P(db), P(ws), P(dx), C if with_dx else 0, 0, P(dxh), hip.stream())
    return dict(dz=dy, dw=dw, db=db, dxh=dxh, dx=dx, kernels=launched() if launched is not None else None)


def _pair(dev, rows, C, nseg, act, use_res, launched, want, want_with_dx=None):
    label = f'rows {rows} C {C} segments {nseg} act {act} res {use_res}'
    c = _setup(dev, rows, C, nseg, act, use_res, seed=rows * 131 + C * 7 + nseg * 3 + act + 5 * use_res)
    a, b = _bwd(dev, c, True, launched), _bwd(dev, c, False, launched)
    assert not bool(torch.isnan(a['dx']).any()), label
    for k in ('dxh', 'dz', 'dw', 'db'):
        assert torch.equal(_bits(a[k]), _bits(b[k])), f'{label}: {k} differs between dx given and dx = NULL'
    if launched is not None:
        assert a['kernels'] == (want_with_dx or want), (label, a['kernels'])
        assert b['kernels'] == want, (label, b['kernels'])


def run_rows(dev, rows, launched=None, channels=CHANNELS):
    for C in channels:
        for nseg in (1, 3):
            want = ['k_norm_bwd_cb'] if (nseg == 1 and rows <= 4096) else LONG
            for act in (0, 1, 2):
                for use_res in (0, 1):
                    _pair(dev, rows, C, nseg, act, use_res, launched, want)


def run_scalar(dev, launched=None):
    """C % 4 != 0: k_norm_bwd_apply writes the bf16 rows itself where the call with dx runs the cast launch on them"""
    for rows, nseg in ((5, 1), (130, 3)):
        for act in (0, 1, 2):
            _pair(dev, rows, 18, nseg, act, 1, launched, SCALAR, SCALAR + ['k_cast_rows'])


def run_refusals(dev):
    """dx = NULL needs the bf16 rows and has nothing to accumulate onto: -2 before anything is written"""
    hip = _hip()
    P = hip.P
    c = _setup(dev, 130, 16, 1, 1, 0, seed=3)
    dy, dw, db = c['dy'].clone(), c['dw'].clone(), c['db'].clone()
    dxh = torch.zeros((130, 16), dtype=torch.bfloat16, device=dev)
    for acc, h in ((0, 0), (1, P(dxh))):
        rc = hip.raw('es_norm_bwd')(P(dy), 16, P(c['y']), 16, P(c['x']), 16, 130, 16, c['segs'], 1, P(c['mean']), P(c['invstd']), P(c['w']),
                                    1, P(dw), P(db), P(c['ws']), 0, 0, acc, h, hip.stream())
        assert rc == -2, (acc, h, rc)
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert torch.equal(dy, c['dy']) and torch.equal(dw, c['dw']) and torch.equal(db, c['db']) and not bool(dxh.any())


@pytest.mark.parametrize('rows', ROWS)
def test_null_dx_keeps_every_other_output_bit_for_bit(dev, rows):
    run_rows(dev, rows)


def test_null_dx_on_the_scalar_path(dev):
    run_scalar(dev)


def test_null_dx_refused_without_bf16_rows_or_with_accumulate(dev):
    run_refusals(dev)
