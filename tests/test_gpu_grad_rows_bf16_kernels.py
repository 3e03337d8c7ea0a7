"""The kernels behind engine.GRAD_ROWS_BF16 on the image backbone's residual joins, each held bit for bit to the launch it replaces.

Join (es_affine_act_bwd_yh_xh): the bf16 rows are es_cast_rows_bf16 of the f32 dx es_affine_act_bwd_yh stores, dres is bit-equal; rows
{1, 5, 257, 4099} x C {64, 128, 512} x acc_r {0, 1} x act {0, 1}, with y holding +0, -0, the smallest positive bf16 and negative values.
With two scales (es_affine_act_bwd_yh_xh2, the join of a downsample block): the first matrix as above, the second bit-equal to the rounded
output of the two launches it replaces -- the one-scale join's f32 dres fed to the act = 0 es_affine_act_bwd_yh with the second scale.

Readers on r(G) (the join's bf16 rows) against the f32 form on G, channel pairs 32 -> 128, 64 -> 256, 128 -> 512:
  - es_rows_wgrad1_bf16 with bit 1 of `accumulate`: 4096 rows (whole 64-row steps) and 4161 (a ragged last step).  The launcher slices when
    n (2 Cin + 4 Cout) >= 32 Cin Cout (rows_wgrad_plan) and takes nothing below 4096 rows or above 512 channels: at 4096 rows even 512 -> 512
    gives 3 slices, so the unsliced store (straight into dW) is unreachable for every shape it takes, with f32 and with bf16 rows alike --
    there is no case on that side of the threshold; the slice count of each case is printed and asserted > 1;
  - es_spconv_wgrad_bf16_src with dy_half = 3 on the identity map: 300 rows (one slice) and 5000 (several), first write and accumulate;
  - es_spconv_fwd_bf16_io with x_half = 1 in the gated mode act = 3 (the transposed pairs): 257 and 4099 rows;
  - es_img_dgrad1_s2_bf16 with bit 1 of `accumulate` (the transposed pairs and the downsample's 256 -> 128): a 2 x 10 x 6 grid (30 gradient
    rows) and a 2 x 18 x 16 one (144: a second 128-row tile), first write and accumulate; a grid with odd H and W (9 x 7) is outside what
    the launcher takes (es_img_dgrad1_s2_supported = 0): both forms return -4 and write nothing, and the engine keeps f32 rows there.

Every body is a function of `dev`: tests/test_emu_grad_rows_bf16_kernels.py runs them on the CPU emulator."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PAIRS = ((32, 128), (64, 256), (128, 512))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _hip():
    from embodiedscan_amd import hip
    return hip


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _round(hip, g):
    """r(G): es_cast_rows_bf16, the conversion every bf16 row uses"""
    n, C = g.shape
    h = torch.empty((n, C), dtype=torch.bfloat16, device=g.device)
    hip.call('es_cast_rows_bf16', hip.P(g), C, n, C, hip.P(h), hip.stream())
    return h


def _sync(dev):
    if dev.type == 'cuda':
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the join
def run_join(dev, rows, channels=(64, 128, 512)):
    hip = _hip()
    P = hip.P
    tiny = float(torch.tensor([1], dtype=torch.int16).view(torch.bfloat16))        # smallest positive (subnormal) bf16
    for C in channels:
        g = torch.Generator().manual_seed(rows * 17 + C)
        y = torch.randn(rows, C, generator=g)
        edge = torch.tensor([0.0, -0.0, tiny, -tiny, -1.5, 2.0])
        y.view(-1)[:min(6, y.numel())] = edge[:min(6, y.numel())]
        y.view(-1)[-1] = -0.0
        yh = y.to(torch.bfloat16).to(dev)
        dy = (torch.randn(rows, C, generator=g) * 3).to(dev)
        scale = ((torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)).to(dev)
        r0 = torch.randn(rows, C, generator=g).to(dev)
        for act in (0, 1):
            for acc_r in (0, 1):
                dx = torch.full((rows, C), float('nan'), device=dev)
                ra, rb = r0.clone(), r0.clone()
                hip.call('es_affine_act_bwd_yh', P(dy), P(yh), P(scale), rows, C, act, P(dx), 0, P(ra), acc_r, hip.stream())
                dxh = torch.full((rows, C), float('nan'), dtype=torch.bfloat16, device=dev)
                hip.call('es_affine_act_bwd_yh_xh', P(dy), P(yh), P(scale), rows, C, act, P(dxh), P(rb), acc_r, hip.stream())
                _sync(dev)
                label = f'rows {rows} C {C} act {act} acc_r {acc_r}'
                assert torch.equal(_bits(dxh), _bits(_round(hip, dx))), label + ': bf16 rows'
                assert torch.equal(_bits(ra), _bits(rb)), label + ': dres'
                if act:                                         # +0, -0 and negative activations pass nothing (the subnormal positive one:
                    flat, src = dxh.float().view(-1).cpu(), (dy * scale).view(-1).cpu()      # whatever the f32-rows launch decides)
                    for i in (0, 1, 3, 4, 5):
                        want = float(src[i].to(torch.bfloat16)) if float(edge[i]) > 0 else 0.0
                        assert float(flat[i]) == want, (label, i, float(flat[i]), want)
        # two scales: what the one-scale join's dres, read back by the act = 0 launch of the downsample's BN, would give
        scale2 = ((torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)).to(dev)
        for act in (0, 1):
            dx, dres = torch.full((rows, C), float('nan'), device=dev), torch.full((rows, C), float('nan'), device=dev)
            hip.call('es_affine_act_bwd_yh', P(dy), P(yh), P(scale), rows, C, act, P(dx), 0, P(dres), 0, hip.stream())
            dx2 = torch.full((rows, C), float('nan'), device=dev)
            hip.call('es_affine_act_bwd_yh', P(dres), P(yh), P(scale2), rows, C, 0, P(dx2), 0, 0, 0, hip.stream())
            a = torch.full((rows, C), float('nan'), dtype=torch.bfloat16, device=dev)
            b = torch.full((rows, C), float('nan'), dtype=torch.bfloat16, device=dev)
            hip.call('es_affine_act_bwd_yh_xh2', P(dy), P(yh), P(scale), P(scale2), rows, C, act, P(a), P(b), hip.stream())
            _sync(dev)
            assert torch.equal(_bits(a), _bits(_round(hip, dx))), f'rows {rows} C {C} act {act}: first matrix'
            assert torch.equal(_bits(b), _bits(_round(hip, dx2))), f'rows {rows} C {C} act {act}: second matrix'
        assert hip.raw('es_affine_act_bwd_yh_xh2')(P(dy), P(yh), P(scale), 0, rows, C, 1, P(a), P(b), hip.stream()) == -2
        assert hip.raw('es_affine_act_bwd_yh_xh2')(P(dy), P(yh), P(scale), P(scale2), rows, C, 1, P(a), 0, hip.stream()) == -2
        # without a residual gradient; refusals write nothing
        dxh = torch.zeros((rows, C), dtype=torch.bfloat16, device=dev)
        hip.call('es_affine_act_bwd_yh_xh', P(dy), P(yh), P(scale), rows, C, 1, P(dxh), 0, 0, hip.stream())
        dx = torch.zeros((rows, C), device=dev)
        hip.call('es_affine_act_bwd_yh', P(dy), P(yh), P(scale), rows, C, 1, P(dx), 0, 0, 0, hip.stream())
        assert torch.equal(_bits(dxh), _bits(_round(hip, dx)))
        assert hip.raw('es_affine_act_bwd_yh_xh')(P(dy), P(yh), P(scale), rows, C, 2, P(dxh), 0, 0, hip.stream()) == -2
        assert hip.raw('es_affine_act_bwd_yh_xh')(P(dy), P(yh), P(scale), rows, C, 1, 0, 0, 0, hip.stream()) == -2


# ------------------------------------------------------------------------------------------------------------------ the readers
def _operands(dev, n, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    xh = torch.randn(n, cin, generator=g).to(torch.bfloat16).to(dev)
    G = (torch.randn(n, cout, generator=g) * 2).to(dev)
    return xh, G


def run_rows_wgrad(dev, n):
    hip = _hip()
    P = hip.P
    hip.raw('es_img_wgrad_set_option')(43, 0)              # every width from 4 096 rows (the shipped rule: < 256 input channels from 500 000)
    try:
        for cin, cout in PAIRS:
            xh, G = _operands(dev, n, cin, cout, n + cin)
            Gh = _round(hip, G)
            nf = int(hip.raw('es_rows_wgrad1_workspace_floats')(n, cin, cout))
            slices = nf // (cin * cout)
            print(f'es_rows_wgrad1_bf16 {cin} -> {cout}, {n} rows: {slices} slices')
            assert slices > 1
            ws = torch.zeros(nf, device=dev)
            prior = torch.randn(cin, cout, generator=torch.Generator().manual_seed(3)).to(dev)
            for acc in (0, 1):
                a, b = prior.clone(), prior.clone()
                hip.call('es_rows_wgrad1_bf16', P(xh), cin, P(G), cout, n, cin, cout, P(a), acc, P(ws), nf, hip.stream())
                hip.call('es_rows_wgrad1_bf16', P(xh), cin, P(Gh), cout, n, cin, cout, P(b), acc | 2, P(ws), nf, hip.stream())
                _sync(dev)
                assert float(a.abs().max()) > 0 and torch.equal(_bits(a), _bits(b)), (cin, cout, n, acc)
    finally:
        hip.raw('es_img_wgrad_set_option')(43, 500000)


def run_map_wgrad(dev, n):
    hip = _hip()
    P = hip.P
    for cin, cout in PAIRS:
        xh, G = _operands(dev, n, cin, cout, n + cout)
        Gh = _round(hip, G)
        need = [int(hip.raw('es_spconv_wgrad_workspace_floats')(1, P(xh), 1, cin, P(d), h, cout, n, n, 1, cin, cout)) for d, h in ((G, 0), (Gh, 3))]
        assert need[0] == need[1], need                     # the plan of the f32 matrix
        print(f'es_spconv_wgrad_bf16_src {cin} -> {cout}, {n} rows: {need[0] // (cin * cout)} slices')
        ws = torch.zeros(max(need[0], 1), device=dev)
        prior = torch.randn(cin, cout, generator=torch.Generator().manual_seed(4)).to(dev)
        for acc in (0, 1):
            a, b = prior.clone(), prior.clone()
            hip.call('es_spconv_wgrad_bf16_src', P(xh), 1, cin, P(G), 0, cout, 0, n, n, 1, cin, cout, P(a), acc, P(ws), need[0], hip.stream())
            hip.call('es_spconv_wgrad_bf16_src', P(xh), 1, cin, P(Gh), 3, cout, 0, n, n, 1, cin, cout, P(b), acc, P(ws), need[0], hip.stream())
            _sync(dev)
            assert float(a.abs().max()) > 0 and torch.equal(_bits(a), _bits(b)), (cin, cout, n, acc)


def run_gated_dgrad(dev, n):
    """conv3's data gradient: dX = (G @ W^T) * gate where the stored activation is positive; reduction over conv3's output channels"""
    hip = _hip()
    P = hip.P
    for cin, cout in PAIRS:
        g = torch.Generator().manual_seed(n + cin * 3)
        G = (torch.randn(n, cout, generator=g) * 2).to(dev)
        Gh = _round(hip, G)
        wn = (torch.randn(1, cin, cout, generator=g) / cout ** 0.5).to(torch.bfloat16).to(dev)      # natural copy [K][Cin][Cout]: reduction contiguous
        gate = (torch.rand(cin, generator=g) + 0.5).to(dev)
        act = torch.randn(n, cin, generator=g).to(torch.bfloat16).to(dev)
        a = torch.full((n, cin), float('nan'), device=dev)
        b = torch.full((n, cin), float('nan'), device=dev)
        hip.call('es_spconv_fwd_bf16_io', P(G), 0, cout, P(wn), 0, n, n, 1, cout, cin, P(gate), 0, P(act), 1, cin, 3, P(a), 0, cin, hip.stream())
        hip.call('es_spconv_fwd_bf16_io', P(Gh), 1, cout, P(wn), 0, n, n, 1, cout, cin, P(gate), 0, P(act), 1, cin, 3, P(b), 0, cin, hip.stream())
        _sync(dev)
        assert not bool(torch.isnan(a).any()) and float(a.abs().max()) > 0
        assert bool(((a == 0) | (act.float() > 0)).all())                                      # the gate closed where the activation is not positive
        assert torch.equal(_bits(a), _bits(b)), (cin, cout, n)


def run_s2_dgrad(dev, H, W):
    """the downsample's data gradient: dX[(im, 2 oy, 2 ox)] (+)= G[(im, oy, ox)] . W^T, reduction over the downsample's output channels"""
    hip = _hip()
    P = hip.P
    n_img = 2
    n_g, n_x = n_img * (H // 2) * (W // 2), n_img * H * W
    for cx, cg in PAIRS + ((128, 256),):
        g = torch.Generator().manual_seed(H * 31 + W + cg)
        G = (torch.randn(n_g, cg, generator=g) * 2).to(dev)
        Gh = _round(hip, G)
        wn = (torch.randn(1, cx, cg, generator=g) / cg ** 0.5).to(torch.bfloat16).to(dev)        # natural copy [Cx][Cg]
        prior = torch.randn(n_x, cx, generator=g).to(dev)
        ok = hip.raw('es_img_dgrad1_s2_supported')(n_img, H, W, cg, cx) == 1
        assert ok == (H % 2 == 0 and W % 2 == 0)
        for acc in (0, 1):
            a, b = prior.clone(), prior.clone()
            ra = hip.raw('es_img_dgrad1_s2_bf16')(P(G), cg, P(wn), n_img, H, W, cg, cx, P(a), cx, acc, hip.stream())
            rb = hip.raw('es_img_dgrad1_s2_bf16')(P(Gh), cg, P(wn), n_img, H, W, cg, cx, P(b), cx, acc | 2, hip.stream())
            _sync(dev)
            assert ra == rb == (0 if ok else -4), (ra, rb)
            if ok:
                assert not torch.equal(a, prior) and torch.equal(_bits(a), _bits(b)), (cg, cx, H, W, acc)
            else:
                assert torch.equal(a, prior) and torch.equal(b, prior)


@pytest.mark.parametrize('rows', [1, 5, 257, 4099])
def test_join_bf16_rows_are_the_rounded_f32_rows(dev, rows):
    run_join(dev, rows)


@pytest.mark.parametrize('n', [4096, 4161])
def test_rows_wgrad1_on_bf16_rows(dev, n):
    run_rows_wgrad(dev, n)


@pytest.mark.parametrize('n', [300, 5000])
def test_map_wgrad_on_pre_rounded_rows(dev, n):
    run_map_wgrad(dev, n)


@pytest.mark.parametrize('n', [257, 4099])
def test_gated_data_gradient_on_bf16_rows(dev, n):
    run_gated_dgrad(dev, n)


@pytest.mark.parametrize('H,W', [(10, 6), (18, 16), (9, 7)])
def test_stride2_data_gradient_on_bf16_rows(dev, H, W):
    run_s2_dgrad(dev, H, W)
