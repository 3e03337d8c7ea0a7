"""tests/test_gpu_conv_kernels.py on the CPU emulator (tests/emu): the same bodies on the same shapes under the `emulated` fixture of
tests/test_emu_product.py (random thread schedule, late LDS-DMA delivery), with the launch log compared against the restated plan: the
kernel name, the split factor (gridDim.z) and the reducer of every case.  Then the specification alone: it rejects a correct output with
ONE thing wrong, and the restated plan sends every case of the grid to the kernel its name promises -- every tile kernel of the family.
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import numpy as np
import pytest
import torch

import conv_spec as S
import test_gpu_conv_kernels as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)

SEEN = set()          # the kernels (and reducers) the launch log showed, over the whole module


def _lib():
    import build as emu_build
    return ctypes.CDLL(emu_build.build())


def _launches():
    """the launches since the last call: '<kernel expression> grid=(x,y,z) block=n' lines"""
    buf = ctypes.create_string_buffer(1 << 16)
    _lib().es_emu_take_launch_log(buf, len(buf))
    lines = buf.value.decode().splitlines()
    SEEN.update(T.normalise(ln.split(' grid=')[0]) for ln in lines)
    return lines


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\n' + T.STATS.report())


def _case(name):
    return next(c for c in T.CASES if c['name'] == name)


# ------------------------------------------------------------------------------------------------------------ the GPU bodies
@pytest.mark.parametrize('name', [c['name'] for c in T.CASES])
def test_convolution_per_element(emulated, name):  # noqa: F811
    c = _case(name)
    T.conv_case(emulated, c, _launches)
    if c['reducer'] == 'split_tail':
        SEEN.add('split_tail')                    # (a device function: the case passed with gridDim.z = split and no second launch)


@pytest.mark.parametrize('args', T.F32_CASES, ids=[a[0] for a in T.F32_CASES])
def test_exact_f32_convolution_per_element(emulated, args):  # noqa: F811
    T.f32_case(emulated, *args, launches=_launches)


@pytest.mark.parametrize('cin,cout,n', T.GT_CASES)
def test_fused_transposed_taps_per_element(emulated, cin, cout, n):  # noqa: F811
    T.gen_transpose_case(emulated, cin, cout, n, _launches)


def test_fused_transposed_taps_not_served(emulated):  # noqa: F811
    T.gen_transpose_not_served_case(emulated)


def test_refusal_codes_leave_everything_untouched(emulated):  # noqa: F811
    _launches()
    T.refusals_case(emulated)
    assert _launches() == [], 'a refused launch started a kernel'


KERNELS = {'k_expand_bf16<16>', 'k_expand_bf16<32>', 'k_expand_bf16<64>', 'k_lin_small', 'k_rowgemm2_bf16<320>', 'k_rowgemm2_bf16<128>',
           'k_rowgemm2_bf16<64>', 'k_rowgemm2_bf16<32>', 'k_rowgemm_bf16<128>', 'k_rowgemm_bf16<64>', 'k_rowgemm_bf16<32>', 'k_rowgemm_bf16<16>',
           'k_spconv_bf16_dma<128, 1>', 'k_spconv_bf16_dma<128, 2>', 'k_spconv_bf16_dma<64, 1>', 'k_spconv_bf16_dma<64, 2>',
           'k_spconv_bf16_dma<128, 1, 3>', 'k_spconv_bf16_dma<64, 1, 3>',
           'k_spconv_bf16_fast<128, true, true>', 'k_spconv_bf16_fast<128, true, false>', 'k_spconv_bf16_fast<128, false, true>',
           'k_spconv_bf16_fast<128, false, false>', 'k_spconv_bf16_fast<64, true, true>', 'k_spconv_bf16_fast<64, true, false>',
           'k_spconv_bf16_fast<64, false, true>', 'k_spconv_bf16_fast<64, false, false>', 'k_spconv_bf16<128>', 'k_spconv_bf16<64>'}
REDUCERS = {'k_sum_splits', 'k_sum_splits4', 'split_tail'}
OTHERS = {'k_spconv<false>', 'k_spconv<true>', 'k_spconv_narrow_fwd<3>', 'k_rowgemm2_bf16<128, MT>', 'k_rowgemm2_bf16<64, MT>', 'k_rowgemm2_bf16<32, MT>'}


def test_zz_every_kernel_of_the_family_was_launched(emulated):  # noqa: F811
    """the launch logs of this module hold every tile kernel, every reducer and the other launchers' kernels (a kernel whose cases were
    deselected runs its first case here)"""
    for k in sorted((KERNELS | REDUCERS) - SEEN):
        c = next(c for c in T.CASES if k in (c['kernel'], c['reducer']))
        test_convolution_per_element(emulated, c['name'])
    for a in T.F32_CASES:
        if a[1] not in SEEN:
            T.f32_case(emulated, *a, launches=_launches)
    for cin, cout, n in T.GT_CASES[::3]:
        if OTHERS - SEEN:
            T.gen_transpose_case(emulated, cin, cout, n, _launches)
    missing = (KERNELS | REDUCERS | OTHERS) - SEEN
    assert not missing, f'never launched on the emulator: {sorted(missing)}'


# ------------------------------------------------------------------------------------------------------------ the specification alone
def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the specification accepted {what}')


def test_restated_plan_sends_every_case_to_the_kernel_it_names():
    """no device, no emulator: every tile kernel, every split factor and every reducer is promised by some case"""
    kernels, reducers, splits = set(), set(), set()
    for c in T.CASES:
        p = T.restated_plan(c)
        T.promised(c, p)
        kernels.add(p.kernel), reducers.add(p.reducer), splits.add(p.split)
    assert kernels == KERNELS, kernels ^ KERNELS
    assert reducers == REDUCERS | {None} and splits == {1, 2, 4, 8}
    assert {S.plan_f32(a[7] is not None, a[2], a[3], a[4], a[8], {**S.DEFAULTS, **a[13]}).kernel for a in T.F32_CASES} == \
        {'k_spconv<false>', 'k_spconv<true>', 'k_spconv_narrow_fwd<3>'}
    # the placed map holds what its docstring says
    nbr = T.place_map(np.random.default_rng(1), 257, 300, 27)
    assert (nbr[128:256] < 0).all() and (nbr[128] < 0).all() and (nbr[:, 13] < 0).all() and (nbr[:256, 26] < 0).all() and nbr[256, 26] == 299
    assert nbr[0, 0] == 299 and nbr[256, 0] == 299 and (nbr != 0).all() and (nbr[:128] >= 0).any(1).sum() > 100
    assert S.split_factor(300, 27, 64) == 8 and S.split_factor(300, 8, 64) == 4 and S.split_factor(300, 8, 64, {**S.DEFAULTS, 8: 6}) == 2
    assert S.split_workspace_floats(300, 27, 64, 64) == 1024 + 8 * 300 * 64 and S.split_workspace_floats(300, 1, 64, 64) == 0


def _affine_problem(seed=3, n_out=300, n_in=200, K=8, cin=32, cout=24, ldr=28):
    rng = np.random.default_rng(seed)
    nbr = torch.from_numpy(T.place_map(rng, n_out, n_in, K))
    x = torch.from_numpy(rng.standard_normal((n_in, cin)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32))
    col = lambda: torch.from_numpy(rng.standard_normal(cout).astype(np.float32))
    resbuf = torch.from_numpy(rng.standard_normal((n_out + 1, ldr)).astype(np.float32))
    return nbr, x, w, col(), col(), col(), resbuf


def test_specification_rejects_one_thing_wrong():
    """each mutation is an output a plausible kernel defect would produce, constructed on the host; every one fails the per-element check
    (the first passes the relative-L2 gate of the older tests by four orders of magnitude)"""
    n_out, n_in, K, cin, cout, ldr = 300, 200, 8, 32, 24, 28
    nbr, x, w, bias, scale, shift, resbuf = _affine_problem()
    res = resbuf[:n_out, :cout]
    xr, wr = S.operand(x), S.operand(w)
    cv, A, pairs = S.conv(xr, wr, nbr, n_out, n_in)
    # plain with bias
    spec, lin, slack = S.specify(cv, A, pairs, cin, bias=bias)
    good = spec.float()
    S.check('good', good, spec, lin, slack)
    # 1. one element two bound-widths off
    i, j = 17, 5
    assert float(lin[i, j]) > 0
    off = good.clone()
    off[i, j] = float(spec[i, j] + 2 * (S.G * lin[i, j] + slack[i, j]))
    assert float((off.double() - spec).norm() / spec.norm()) < 1e-6                    # (the relative-L2 gate of tests/test_gpu_ops.py: 1e-2)
    _rejected(lambda: S.check('off', off, spec, lin, slack), 'one element two bound-widths off')
    # 2. a dropped bias column
    dropped = good.clone()
    dropped[:, cout - 1] = cv[:, cout - 1].float()
    _rejected(lambda: S.check('bias', dropped, spec, lin, slack), 'a dropped bias column')
    # 3. one missing pair
    j0 = int(torch.nonzero(nbr[:, 0] >= 0)[3])
    short = nbr.clone()
    short[j0, 0] = -1
    one_short = (S.conv(xr, wr, short, n_out, n_in)[0] + bias.double()).float()
    _rejected(lambda: S.check('pair', one_short, spec, lin, slack), 'one missing pair')
    # ... and a row without any pair must hold the bias exactly / the prior bit for bit
    dead = n_out // 2
    assert float(pairs[dead]) == 0
    s0, l0, k0 = S.specify(cv, A, pairs, cin)
    z = s0.float()
    S.check('good', z, s0, l0, k0)
    z[dead, 3] = 1e-30
    _rejected(lambda: S.check('dead', z, s0, l0, k0), 'a value other than 0.0 in a row without a pair')
    prior = torch.from_numpy(np.random.default_rng(4).standard_normal((n_out, cout)).astype(np.float32))
    sp, lp, kp = S.specify(cv, A, pairs, cin, prior=prior)
    acc = sp.float()
    S.check('good', acc, sp, lp, kp, prior)
    acc[dead, 3] = float(np.nextafter(np.float32(acc[dead, 3]), np.float32(9)))
    _rejected(lambda: S.check('prior', acc, sp, lp, kp, prior), 'a prior one ulp off in a row without a pair')
    # 4. a residual read at the wrong stride (ld = Cout instead of ldr), affine + ReLU; 5. the shift skipped for one column
    sa, la, ka = S.specify(cv, A, pairs, cin, scale=scale, shift=shift, res=res, act=1)
    S.check('good', sa.float(), sa, la, ka)
    wrong = resbuf.reshape(-1)[:n_out * cout].view(n_out, cout)
    _rejected(lambda: S.check('stride', S.specify(cv, A, pairs, cin, scale=scale, shift=shift, res=wrong, act=1)[0].float(), sa, la, ka),
              'a residual read at the wrong stride')
    noshift = shift.clone()
    noshift[cout - 1] = 0
    _rejected(lambda: S.check('shift', S.specify(cv, A, pairs, cin, scale=scale, shift=noshift, res=res, act=1)[0].float(), sa, la, ka), 'a dropped shift column')
    # 6. the gate: a closed element that is not exactly 0.0; the gate read as >= 0
    r0 = res.clone()
    r0[0, 0], r0[1, 1] = 0.0, -0.0
    sg, lg, kg = S.specify(cv, A, pairs, cin, scale=scale, res=r0, act=3)
    g = sg.float()
    S.check('good', g, sg, lg, kg)
    assert float(sg[0, 0]) == 0 and float(sg[1, 1]) == 0
    g[0, 0] = float(scale[0] * cv[0, 0])
    _rejected(lambda: S.check('gate', g, sg, lg, kg), 'a gate that opens at res == 0')
    # 7. bf16 rows: one ulp is allowed, two are not
    sh, lh, kh = S.specify(cv, A, pairs, cin, scale=scale, shift=shift, out_bf16=True)
    h = sh.to(torch.bfloat16)
    S.check('good', h, sh, lh, kh)
    two = h.clone()
    two[i, j] = (sh[i, j] + 2.5 * S.ulp_bf16(sh[i, j])).to(torch.bfloat16)
    _rejected(lambda: S.check('bf16', two, sh, lh, kh), 'a bf16 output two ulps off')
    # 8. operands not rounded to bf16
    exact = (S.conv(S.operand(x, False), S.operand(w, False), nbr, n_out, n_in)[0] + bias.double()).float()
    _rejected(lambda: S.check('unrounded', exact, spec, lin, slack), 'operands not rounded')


def test_the_window_check_rejects_a_value_written_into_the_padding():
    """outside_intact: a value in the ld padding, in the pads or before a shifted base fails; the window itself is free"""
    dev = torch.device('cpu')
    for half in (0, 1):
        flat, y = T.window_buffer(dev, 5, 6, 8, 2, half, None)
        before = flat.clone()
        y.fill_(1.0)
        T.outside_intact('ok', flat, before, 5, 6, 8, 2)
        for pos in (T.PAD + 2 + 6, T.PAD + 2 + 4 * 8 + 7, T.PAD + 1, 0, flat.numel() - 1):
            bad = flat.clone()
            bad[pos] = 1.0
            _rejected(lambda: T.outside_intact('bad', bad, before, 5, 6, 8, 2), f'a value written at flat element {pos}')
        nan_to_other_nan = flat.clone()
        T.bits(nan_to_other_nan)[T.PAD + 2 + 7] += 1                      # another NaN payload in the padding is a write too
        _rejected(lambda: T.outside_intact('bad', nan_to_other_nan, before, 5, 6, 8, 2), 'a rewritten NaN in the padding')


# ------------------------------------------------------------------------------------------------------------ the launchers around it
@pytest.mark.parametrize('args', T.HALO_CASES, ids=[f'n{a[0]}-{a[2]}to{a[3]}-mirror{a[4]}' for a in T.HALO_CASES])
def test_halo_convolution_per_element(emulated, args):  # noqa: F811
    T.halo_case(emulated, *args, launches=_launches)


@pytest.mark.parametrize('args', T.DCONV_CASES, ids=[f'mode{a[5]}-stride{a[4]}-{a[6]}to{a[7]}' for a in T.DCONV_CASES])
def test_dense_convolution_per_element(emulated, args):  # noqa: F811
    T.dconv_case(emulated, *args, launches=_launches)


@pytest.mark.parametrize('args', T.IMG_CASES, ids=[f'C{a[0]}-W{a[1]}-stride{a[2]}-mode{a[3]}' for a in T.IMG_CASES])
def test_image_convolution_per_element(emulated, args):  # noqa: F811
    T.img_conv_case(emulated, *args, launches=_launches)


def test_halo_and_image_launchers_answer_minus_4_for_operands_the_query_cannot_see(emulated):  # noqa: F811
    T.not_taken_case(emulated)


def test_implied_maps_against_a_dense_reference():
    """grid_map against torch's own conv2d / conv3d on a one-channel impulse response: tap order, stride, padding, batch"""
    import torch.nn.functional as F
    for B, dims, st in ((2, (5, 4, 3), 1), (1, (6, 4, 4), 2), (2, (5, 7), 1), (2, (10, 6), 2)):
        nbr, odims = T.grid_map(B, dims, 3, st, 1)
        K = 3 ** len(dims)
        rng = np.random.default_rng(len(dims) + st)
        x = torch.from_numpy(rng.standard_normal((B,) + dims))
        w = torch.from_numpy(rng.standard_normal((K,)))
        conv = F.conv3d if len(dims) == 3 else F.conv2d
        want = conv(x[:, None], w.view((1, 1) + (3,) * len(dims)), stride=st, padding=1).reshape(-1)
        xf = torch.cat([x.reshape(-1), torch.zeros(1, dtype=x.dtype)])
        got = (xf[torch.from_numpy(nbr).long()] * w).sum(1)                   # (-1 reads the appended zero)
        assert list(want.shape) == [B * int(np.prod(odims))] and torch.allclose(got, want, atol=1e-12)
