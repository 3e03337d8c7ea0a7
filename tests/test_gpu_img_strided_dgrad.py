"""Stride-2 data gradients of the image backbone by address arithmetic (csrc/imgconv.hip: es_img_dgrad3_s2_bf16, es_img_dgrad1_s2_bf16) on
the GPU through the C ABI.  Per case: bit-identical to the map-kernel launch it replaces on the same operands (es_image_map ->
es_inverse_map -> es_spconv_fwd_bf16_io gated / es_spconv_fwd_bf16); element by element against f64 conv_transpose2d on the bf16-rounded
operands to the bound of tests/fwd_spec.py (reduction length: the 4 taps x C (3x3) / the C products (1x1) an element can receive);
NaN-prefilled output fully defined (accumulate 0), odd pixels bit-unchanged (accumulate 1); a second run bit-identical; refusals return -4
with the output untouched.  One engine-level case: a two-block ResNet stage with the switch on against the switch off."""
import math

import pytest
import torch

import fwd_spec as FS

pytestmark = pytest.mark.gpu

CASES3 = [(2, 10, 22, 32), (2, 8, 12, 64), (1, 2, 2, 32), (3, 6, 34, 32)]        # (2, 30, 30, 128): not taken (the plan refuses 128 channels)
CASES1 = [(2, 10, 22, 64, 32), (1, 4, 6, 256, 128)]


def _nchw(rows, n_img, H, W):
    return rows.double().view(n_img, H, W, -1).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _wk(w, k):
    """(k*k, Cin, Cout) taps in (ky, kx) order -> conv2d weight (Cout, Cin, k, k)"""
    return w.double().view(k, k, w.shape[1], w.shape[2]).permute(3, 2, 0, 1)


def _inverse_map(n_img, H, W, k, pad, dev, st):
    from embodiedscan_amd.hip import P, call
    n, n_o = n_img * H * W, n_img * (H // 2) * (W // 2)
    nbr = torch.empty((n_o, k * k), dtype=torch.int32, device=dev)
    inv = torch.empty((n, k * k), dtype=torch.int32, device=dev)
    call('es_image_map', n_img, H, W, H // 2, W // 2, k, k, 2, pad, P(nbr), st)
    call('es_inverse_map', P(nbr), n_o, k * k, n, P(inv), st)
    return inv


@pytest.mark.parametrize('case', CASES3)
def test_gated_3x3_stride2_data_gradient(case):
    from embodiedscan_amd.hip import P, call, raw
    import torch.nn.functional as F
    n_img, H, W, C = case
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(31)
    n, n_o = n_img * H * W, n_img * (H // 2) * (W // 2)
    gy = torch.randn(n_o, C, generator=g).to(dev)
    act = torch.randn(n, C, generator=g).to(dev).to(torch.bfloat16)
    w = (torch.randn(9, C, C, generator=g) / (9 * C) ** 0.5).to(dev)
    scale = (0.5 + torch.rand(C, generator=g)).to(dev)
    wn, wt = torch.empty((9, C, C), dtype=torch.bfloat16, device=dev), torch.empty((9, C, C), dtype=torch.bfloat16, device=dev)
    call('es_cast_weight_bf16', P(w), 9, C, C, P(wn), P(wt), st)
    inv = _inverse_map(n_img, H, W, 3, 1, dev, st)
    assert raw('es_img_dgrad3_s2_supported')(n_img, H, W, C) == 1
    d1 = torch.zeros((n, C), device=dev)
    call('es_spconv_fwd_bf16_io', P(gy), 0, C, P(wn), P(inv), n, n_o, 9, C, C, P(scale), 0, P(act), 1, C, 3, P(d1), 0, C, st)
    d2 = torch.full((n, C), float('nan'), device=dev)
    call('es_img_dgrad3_s2_bf16', P(gy), C, P(wn), n_img, H, W, C, P(scale), P(act), C, P(d2), C, st)
    d3 = torch.full((n, C), float('nan'), device=dev)
    call('es_img_dgrad3_s2_bf16', P(gy), C, P(wn), n_img, H, W, C, P(scale), P(act), C, P(d3), C, st)
    torch.cuda.synchronize()
    nd = int((d1.view(torch.int32) != d2.view(torch.int32)).sum())
    print(f'{case}: elements differing from the map kernel {nd}; defined {bool(torch.isfinite(d2).all())}')
    assert bool(torch.isfinite(d2).all())
    assert torch.equal(d2.view(torch.int32), d3.view(torch.int32)), 'two runs differ'
    assert nd == 0
    gr = _nchw(gy.to(torch.bfloat16), n_img, H // 2, W // 2)
    mask = (act.double() > 0) * scale.double()[None]
    want = _rows(F.conv_transpose2d(gr, _wk(wn, 3), stride=2, padding=1, output_padding=1)) * mask
    A = _rows(F.conv_transpose2d(gr.abs(), _wk(wn, 3).abs(), stride=2, padding=1, output_padding=1)) * mask.abs()
    r = FS.bound_check(f'{case} gated stride-2 data gradient', d2, want, FS.U * math.sqrt(4 * C) * A, torch.zeros_like(want), False, 'dgrad',
                       FS.Stats('strided dgrad'))[0]
    print(f'   vs f64 conv_transpose2d: worst |d - spec| / (u sqrt(4C) A) {r:.3f} (bound {FS.G:g})')


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('case', CASES1)
def test_1x1_stride2_data_gradient(case, accumulate):
    from embodiedscan_amd.hip import P, call, raw
    import torch.nn.functional as F
    n_img, H, W, cg, cx = case
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(32)
    n, n_o = n_img * H * W, n_img * (H // 2) * (W // 2)
    gy = torch.randn(n_o, cg, generator=g).to(dev)
    w = (torch.randn(1, cx, cg, generator=g) / cg ** 0.5).to(dev)                  # the layer's (1, Cin, Cout)
    pat = torch.randn(n, cx, generator=g).to(dev)
    wn, wt = torch.empty((1, cx, cg), dtype=torch.bfloat16, device=dev), torch.empty((1, cg, cx), dtype=torch.bfloat16, device=dev)
    call('es_cast_weight_bf16', P(w), 1, cx, cg, P(wn), P(wt), st)
    inv = _inverse_map(n_img, H, W, 1, 0, dev, st)
    assert raw('es_img_dgrad1_s2_supported')(n_img, H, W, cg, cx) == 1

    def fresh():
        return pat.clone() if accumulate else torch.full((n, cx), float('nan'), device=dev)
    d1 = pat.clone() if accumulate else torch.zeros((n, cx), device=dev)
    call('es_spconv_fwd_bf16', P(gy), 0, cg, P(wn), P(inv), n, n_o, 1, cg, cx, 0, P(d1), cx, accumulate, st)
    d2, d3 = fresh(), fresh()
    call('es_img_dgrad1_s2_bf16', P(gy), cg, P(wn), n_img, H, W, cg, cx, P(d2), cx, accumulate, st)
    call('es_img_dgrad1_s2_bf16', P(gy), cg, P(wn), n_img, H, W, cg, cx, P(d3), cx, accumulate, st)
    torch.cuda.synchronize()
    nd = int((d1.view(torch.int32) != d2.view(torch.int32)).sum())
    print(f'{case} accumulate {accumulate}: elements differing from the map kernel {nd}; defined {bool(torch.isfinite(d2).all())}')
    assert bool(torch.isfinite(d2).all())
    assert torch.equal(d2.view(torch.int32), d3.view(torch.int32)), 'two runs differ'
    assert nd == 0
    odd = torch.ones((n_img, H, W), dtype=torch.bool, device=dev)
    odd[:, ::2, ::2] = False
    odd = odd.view(n)
    if accumulate:
        assert torch.equal(d2[odd].view(torch.int32), pat[odd].view(torch.int32)), 'accumulate = 1 touched a pixel without a source'
    else:
        assert bool((d2[odd] == 0).all())
    gr = _nchw(gy.to(torch.bfloat16), n_img, H // 2, W // 2)
    base = pat.double() if accumulate else torch.zeros((n, cx), dtype=torch.float64, device=dev)
    conv = _rows(F.conv_transpose2d(gr, _wk(wn, 1), stride=2, output_padding=1))
    A = _rows(F.conv_transpose2d(gr.abs(), _wk(wn, 1).abs(), stride=2, output_padding=1))
    want = conv + base
    r = FS.bound_check(f'{case} 1x1 stride-2 data gradient', d2, want, FS.U * math.sqrt(cg) * A, want.abs(), False, 'dgrad',
                       FS.Stats('strided dgrad'))[0]                             # (+ u |want|: the f32 add onto the buffer)
    print(f'   vs f64 conv_transpose2d: worst |d - spec| / (u sqrt(C) A) {r:.3f} (bound {FS.G:g})')


def test_refusals_leave_the_output_untouched():
    from embodiedscan_amd.hip import P, raw
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.full((1 << 16,), 7.0, device=dev)
    a = P(buf)
    assert a % 16 == 0
    d3, d1 = raw('es_img_dgrad3_s2_bf16'), raw('es_img_dgrad1_s2_bf16')
    s3 = raw('es_img_dgrad3_s2_supported')
    assert s3(80, 120, 120, 32) == 1 and s3(80, 60, 60, 64) == 1 and s3(80, 30, 30, 128) == 0 and s3(2, 9, 10, 32) == 0
    for args in ((a, 32, a, 2, 9, 10, 32, a, a, 32, a, 32), (a, 32, a, 2, 10, 9, 32, a, a, 32, a, 32), (a, 34, a, 2, 10, 10, 32, a, a, 32, a, 32),
                 (a, 32, a, 2, 10, 10, 32, a, a, 32, a, 34), (a + 8, 32, a, 2, 10, 10, 32, a, a, 32, a, 32),
                 (a, 32, a, 2, 10, 10, 32, a, a, 32, a + 8, 32), (a, 32, a, 1 << 13, 64, 128, 32, a, a, 32, a, 32)):
        assert d3(*args, st) == -4, args
    for args in ((a, 64, a, 2, 9, 10, 64, 32, a, 32), (a, 66, a, 2, 10, 10, 64, 32, a, 32), (a, 64, a, 2, 10, 10, 64, 32, a, 34),
                 (a + 8, 64, a, 2, 10, 10, 64, 32, a, 32), (a, 64, a, 2, 10, 10, 64, 32, a + 8, 32), (a, 64, a, 1 << 13, 64, 128, 64, 32, a, 32)):
        for accumulate in (0, 1):
            assert d1(*args, accumulate, st) == -4, args
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())


def _stage(E, n_img, H, W, x, par, fold, dev):
    """two Bottleneck blocks (the first with stride 2 and a 1x1 / stride-2 downsample), wired as models/backbones/resnet2d.py does"""
    from embodiedscan_amd.models.backbones.resnet2d import _Grid
    grids = (_Grid(n_img, H, W, dev), _Grid(n_img, H // 2, W // 2, dev))
    cur = x
    for bi in range(2):
        stride, g_in = (2, grids[0]) if bi == 0 else (1, grids[1])
        o = E.conv_affine(cur, par[f'{bi}.conv1'], None, None, cur.d.shape[0], *fold[f'{bi}.bn1'], act=1, out_bf16=True)
        nbr, inv, n_out, _, _ = g_in.conv_map(3, stride, 1)
        o = E.conv_affine(o, par[f'{bi}.conv2'], nbr, inv, n_out, *fold[f'{bi}.bn2'], act=1, sole_consumer=True, out_bf16=True,
                          img=(n_img, g_in.H, g_in.W, stride))
        if bi == 0:
            dn, di, _, _, _ = g_in.conv_map(1, 2, 0)
            idt = E.conv_affine(cur, par['0.down'], dn, di, n_out, *fold['0.down'], act=0, out_bf16=True, img=(n_img, g_in.H, g_in.W, 2))
        else:
            idt = cur
        cur = E.conv_affine(o, par[f'{bi}.conv3'], None, None, n_out, *fold[f'{bi}.bn3'], act=1, res=idt, sole_consumer=True, out_bf16=True)
    return cur


def test_two_block_stage_switch_on_equals_switch_off(monkeypatch):
    """a two-block ResNet stage (64 -> 32 -> 128 channels, stride 2) on a (2, 16, 16) grid in bf16 mode with bf16 activation rows: every
    parameter gradient and the input gradient with IMG_STRIDED_DGRAD on are the bits of the map-kernel path"""
    from embodiedscan_amd import engine as E
    dev = torch.device('cuda:0')
    n_img, H, W, cin, mid, cout = 2, 16, 16, 64, 32, 128
    taken, try_call = [], E.hip.try_call

    def spy(name, *args):
        ok = try_call(name, *args)
        if ok:
            taken.append(name)
        return ok
    monkeypatch.setattr(E.hip, 'try_call', spy)
    g = torch.Generator().manual_seed(33)
    shapes = {'0.conv1': (1, cin, mid), '0.conv2': (9, mid, mid), '0.conv3': (1, mid, cout), '0.down': (1, cin, cout),
              '1.conv1': (1, cout, mid), '1.conv2': (9, mid, mid), '1.conv3': (1, mid, cout)}
    owner = object()
    E.begin_bind(id(owner))
    try:
        par = {k: E.Param((torch.randn(s, generator=g) / (s[0] * s[1]) ** 0.5).to(dev), torch.zeros(s, device=dev)) for k, s in shapes.items()}
    finally:
        E.end_bind()
    fold = {}
    for k, s in shapes.items():
        name = k.replace('conv', 'bn') if 'conv' in k else k
        fold[name] = ((0.5 + torch.rand(s[2], generator=g)).to(dev), (0.1 * torch.randn(s[2], generator=g)).to(dev))
    x0 = torch.randn(n_img * H * W, cin, generator=g).to(dev).to(torch.bfloat16)
    gout = torch.randn(n_img * (H // 2) * (W // 2), cout, generator=g).to(dev)
    launched = []
    res = {}
    prev_mode, prev_sw, prev_tape = E.PRECISION[0], E.IMG_STRIDED_DGRAD[0], E.TAPE.enabled
    E.PRECISION[0] = 'bf16'
    E.TAPE.enabled = True
    try:
        for sw in (False, True):
            E.IMG_STRIDED_DGRAD[0] = sw
            E.WEIGHT_VERSION[0] += 1
            E.TAPE.clear()
            for p in par.values():
                p.g.zero_()
            x = E.Var(x0.clone(), rg=True)
            x.dh = x.d
            del taken[:]
            y = _stage(E, n_img, H, W, x, par, fold, dev)
            y.g = gout.clone()
            E.TAPE.backward()
            torch.cuda.synchronize()
            launched.append(set(taken))
            res[sw] = ({k: p.g.clone() for k, p in par.items()}, x.g.clone(), y.d.clone())
    finally:
        E.PRECISION[0], E.IMG_STRIDED_DGRAD[0], E.TAPE.enabled = prev_mode, prev_sw, prev_tape
        E.TAPE.clear()
        E.release(id(owner))
    new = {'es_img_dgrad3_s2_bf16', 'es_img_dgrad1_s2_bf16'}
    assert not (launched[0] & new) and new <= launched[1], (sorted(launched[0] & new), sorted(launched[1] & new))
    assert torch.equal(res[False][2].view(torch.int16), res[True][2].view(torch.int16))
    assert bool(torch.isfinite(res[True][1]).all()) and float(res[True][1].abs().max()) > 0
    assert torch.equal(res[False][1].view(torch.int32), res[True][1].view(torch.int32)), 'input gradient differs'
    for k in shapes:
        assert float(res[True][0][k].abs().max()) > 0, k
        assert torch.equal(res[False][0][k].view(torch.int32), res[True][0][k].view(torch.int32)), k
