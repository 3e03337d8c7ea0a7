"""The forward / data-gradient convolution launchers of csrc/spconv.hip held, element by element, to tests/conv_spec.py through the C ABI
itself: every tile kernel behind es_spconv_fwd_bf16 / _ws / _affine / _io (k_expand_bf16, k_lin_small, the 320-column row GEMM, both row-GEMM
generations in every width, the LDS-DMA kernel with 32- and 64-channel chunks and its three-buffer ring, the register-staged fast kernels with
and without ping-pong, the generic kernels, the tap split with each of its reducers), es_spconv_fwd (exact f32 and the narrow 3 -> 64 kernel),
es_gen_transpose_fwd_bf16 / es_gen_transpose_dgrad_bf16, and es_spconv_halo_bf16 (both mirror values), es_dconv_fwd_bf16 (forward and data gradient)
and es_img_conv3_bf16 (every reachable instantiation of its launch table; 64 channels at stride 2 is refused by its own plan) on the maps these
launchers imply, built on the host (grid_map) -- and the refusal codes of these entry points.

Every case: Y between sentinel pads, prefilled with NaN (accumulate = 0) or a random prior; ldy > Cout where the branch allows it, with NaN
padding that must survive (everything outside the (n_out, Cout) window is compared bit for bit with its prefill); ldx > Cin with NaN
padding; NaN in every X row no pair references and in the rows >= n_in; a workspace of exactly the queried size between sentinels whose
tile tickets are zero on exit; a second run with the same bits.  The maps are placed (place_map): an all -1 row, an all -1 128-row tile, a
tap no row uses, a tap only the last row uses, pairs that name row n_in - 1, X row 0 unreferenced (the fast kernels fetch it for every
absent neighbour and must mask it).  es_spconv_split_workspace_floats and es_spconv_bf16_is_fast are compared with the restated plan in
every case, and the case's name promises the kernel: a case that would silently test another kernel fails.

Every body is a function of `dev`: tests/test_emu_conv_kernels.py runs the same bodies on the CPU emulator, where the launch log also pins
the kernel name, the split factor and the reducer."""
import re

import numpy as np
import pytest
import torch

import conv_spec as S
from test_gpu_ground_kernels import _hip, _rc, _st

pytestmark = pytest.mark.gpu

PAD = 16
SENT = -777.25
NAN = float('nan')
STATS = S.Stats('convolution forward / data-gradient kernels')
F32, B16 = torch.float32, torch.bfloat16


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
def case(name, kernel, K, cin, cout, n_out, **kw):
    c = dict(name=name, kernel=kernel, K=K, cin=cin, cout=cout, n_out=n_out, n_in=n_out, mode='plain', map='placed', xh=0, yh=0, rh=0,
             ldx_pad=None, ldy_pad=None, ldr_pad=None, x_off=0, y_off=0, r_off=0, bias=0, acc=0, shift=1, res=0, act=0, ws=True, opts={},
             split=1, reducer=None, seed=0)
    c.update(kw)
    if c['mode'] == 'plain':
        c['shift'] = 0
    return c


RG_MODES = [
    dict(tag='bias', bias=1),
    dict(tag='acc-strided', acc=1, ldy_pad=8),
    dict(tag='affine-act0', mode='affine', ldy_pad=8),
    dict(tag='affine-res-act1', mode='affine', res=1, act=1, ldr_pad=8),
    dict(tag='affine-res-act2', mode='affine', res=1, act=2),
    dict(tag='gate-noshift', mode='affine', res=1, act=3, shift=0, ldr_pad=8),
    dict(tag='io-r16-act1', mode='io', res=1, rh=1, act=1, ldr_pad=8),
    dict(tag='io-y16-act0', mode='io', yh=1, ldy_pad=8),
    dict(tag='io-gate-r16', mode='io', res=1, rh=1, act=3),
    dict(tag='io-x16-r16-y16-act1', mode='io', xh=1, res=1, rh=1, yh=1, act=1, ldr_pad=8, ldy_pad=8),
]
ROWS = (1, 127, 128, 129, 257)


def _grid():
    g = []
    # the generic kernels: channels no multiple of the tile, odd ldx, an X base 4 bytes off
    g.append(case('generic64-24to40-K8-n129-odd-ldx-bias', 'k_spconv_bf16<64>', 8, 24, 40, 129, n_in=77, ldx_pad=1, ldy_pad=3, bias=1))
    g.append(case('generic128-96to192-K27-n257-x4bytes-acc', 'k_spconv_bf16<128>', 27, 96, 192, 257, n_in=300, x_off=1, acc=1))
    g.append(case('generic128-40to130-K2-n127', 'k_spconv_bf16<128>', 2, 40, 130, 127, n_in=200, ldy_pad=1))
    g.append(case('generic64-24to40-K1-n1', 'k_spconv_bf16<64>', 1, 24, 40, 1, n_in=5, bias=1))
    g.append(case('generic64-24to40-identity-nin<nout', 'k_spconv_bf16<64>', 1, 24, 40, 129, n_in=77, map=None, acc=1))
    g.append(case('generic64-24to40-identity-nin>nout', 'k_spconv_bf16<64>', 1, 24, 40, 129, n_in=200, map=None, bias=1))
    g.append(case('generic64-24to40-K8-affine-res-act1', 'k_spconv_bf16<64>', 8, 24, 40, 129, n_in=77, mode='affine', res=1, act=1, ldr_pad=3))
    g.append(case('generic64-24to40-K8-affine-act2', 'k_spconv_bf16<64>', 8, 24, 40, 129, n_in=77, mode='affine', act=2))
    g.append(case('generic64-24to40-K8-gate-noshift', 'k_spconv_bf16<64>', 8, 24, 40, 128, n_in=77, mode='affine', res=1, act=3, shift=0))
    g.append(case('generic128-40to132-K2-io-r16-y16', 'k_spconv_bf16<128>', 2, 40, 132, 127, n_in=200, mode='io', res=1, rh=1, yh=1, act=1))
    # the register-staged fast kernels: f32 rows and bf16 shadows, ping-pong on and off
    for pp in (1, 0):
        o = {} if pp else {1: 0}
        t = 'true' if pp else 'false'
        g.append(case(f'fast64-f32rows-64to64-K27-n257-pp{pp}', f'k_spconv_bf16_fast<64, false, {t}>', 27, 64, 64, 257, n_in=200, ws=False, bias=1, opts=o))
        g.append(case(f'fast128-f32rows-32to128-K8-n129-pp{pp}-acc', f'k_spconv_bf16_fast<128, false, {t}>', 8, 32, 128, 129, n_in=300, ws=False, acc=1, opts=o))
        g.append(case(f'fast64-shadow-64to64-K2-n127-pp{pp}-acc', f'k_spconv_bf16_fast<64, true, {t}>', 2, 64, 64, 127, n_in=129, xh=1, acc=1, opts=o))
        g.append(case(f'fast128-shadow-32to128-K27-n257-pp{pp}', f'k_spconv_bf16_fast<128, true, {t}>', 27, 32, 128, 257, n_in=300, ws=False, xh=1, bias=1, opts=o))
        g.append(case(f'fast64-64to64-K8-n129-affine-res-act1-pp{pp}', f'k_spconv_bf16_fast<64, false, {t}>', 8, 64, 64, 129, n_in=77, mode='affine',
                      res=1, act=1, ldr_pad=4, opts=o))
        g.append(case(f'fast128-32to128-K8-n128-io-x16-r16-y16-pp{pp}', f'k_spconv_bf16_fast<128, true, {t}>', 8, 32, 128, 128, n_in=77, mode='io', xh=1,
                      res=1, rh=1, yh=1, act=1, opts=o))
    g.append(case('fast64-64to64-K8-n129-gate', 'k_spconv_bf16_fast<64, false, true>', 8, 64, 64, 129, n_in=77, mode='affine', res=1, act=3, shift=0, ldy_pad=0, ldr_pad=0))
    g.append(case('fast64-64to64-K8-n129-io-gate-r16-shift', 'k_spconv_bf16_fast<64, false, true>', 8, 64, 64, 129, n_in=77, mode='io', res=1, rh=1, act=3))
    g.append(case('fast64-64to64-K8-n129-affine-act2', 'k_spconv_bf16_fast<64, false, true>', 8, 64, 64, 129, n_in=77, mode='affine', res=1, act=2))
    g.append(case('fast64-64to64-identity-nin<nout', 'k_spconv_bf16_fast<64, false, true>', 1, 64, 64, 129, n_in=77, map=None, bias=1))
    g.append(case('fast64-shadow-64to64-identity-nin<nout-acc', 'k_spconv_bf16_fast<64, true, true>', 1, 64, 64, 257, n_in=129, map=None, xh=1, acc=1))
    # the LDS-DMA kernel (option 11 lowered to 64): 64- and 32-channel chunks, the three-buffer ring
    g.append(case('dma128-kb2-64to128-K27-n257', 'k_spconv_bf16_dma<128, 2>', 27, 64, 128, 257, n_in=200, xh=1, ws=False, bias=1, opts={11: 64}))
    g.append(case('dma64-kb1-96to64-K8-n129-acc', 'k_spconv_bf16_dma<64, 1>', 8, 96, 64, 129, n_in=300, xh=1, ws=False, acc=1, opts={11: 64}))
    g.append(case('dma64-kb2-64to64-K2-n127', 'k_spconv_bf16_dma<64, 2>', 2, 64, 64, 127, n_in=129, xh=1, opts={11: 64}))
    g.append(case('dma128-kb1-64to128-K8-n128-option10-1', 'k_spconv_bf16_dma<128, 1>', 8, 64, 128, 128, n_in=77, xh=1, ws=False, opts={10: 1, 11: 64}))
    g.append(case('dma64-ring-64to64-K27-n257', 'k_spconv_bf16_dma<64, 1, 3>', 27, 64, 64, 257, n_in=200, xh=1, ws=False, bias=1, opts={10: 3, 11: 64}))
    g.append(case('dma128-ring-64to128-K8-n129-acc', 'k_spconv_bf16_dma<128, 1, 3>', 8, 64, 128, 129, n_in=300, xh=1, ws=False, acc=1, opts={10: 3, 11: 64}))
    g.append(case('dma64-kb2-64to64-K8-n129-io-r16-y16-act1', 'k_spconv_bf16_dma<64, 2>', 8, 64, 64, 129, n_in=77, mode='io', xh=1, res=1, rh=1, yh=1,
                  act=1, opts={11: 64}))
    g.append(case('dma64-kb2-64to64-K8-n129-io-res-act2', 'k_spconv_bf16_dma<64, 2>', 8, 64, 64, 129, n_in=77, mode='io', xh=1, res=1, act=2, opts={11: 64}))
    g.append(case('dma128-kb1-96to128-K8-n257-io-y16-act2', 'k_spconv_bf16_dma<128, 1>', 8, 96, 128, 257, n_in=200, mode='io', xh=1, yh=1, act=2, opts={11: 64}))
    g.append(case('dma64-ring-64to64-K8-n128-io-gate-r16', 'k_spconv_bf16_dma<64, 1, 3>', 8, 64, 64, 128, n_in=77, mode='io', xh=1, res=1, rh=1, act=3, shift=0,
                  opts={10: 3, 11: 64}))
    g.append(case('dma64-kb2-64to64-identity-nin<nout', 'k_spconv_bf16_dma<64, 2>', 1, 64, 64, 129, n_in=77, map=None, xh=1, opts={11: 64}))
    g.append(case('dma128-kb2-64to128-K27-n257-split8', 'k_spconv_bf16_dma<128, 2>', 27, 64, 128, 257, n_in=200, xh=1, bias=1, opts={11: 64}, split=8,
                  reducer='k_sum_splits4'))
    # the tap split: 8 slices (K = 27), 4 (K = 8), 2 (K = 8 with option 8 lowered), each reducer, no workspace, the weight-sharing order
    for acc in (0, 1):
        g.append(case(f'split8-64to64-K27-n300-acc{acc}', 'k_spconv_bf16_fast<64, false, true>', 27, 64, 64, 300, n_in=257, bias=1 - acc, acc=acc, split=8,
                      reducer='k_sum_splits4'))
        g.append(case(f'split4-shadow-32to128-K8-n257-acc{acc}', 'k_spconv_bf16_fast<128, true, true>', 8, 32, 128, 257, n_in=300, xh=1, acc=acc, split=4,
                      reducer='k_sum_splits4'))
        g.append(case(f'split8-64to64-K27-n300-tail-acc{acc}', 'k_spconv_bf16_fast<64, false, true>', 27, 64, 64, 300, n_in=257, bias=acc, acc=acc, split=8,
                      reducer='split_tail', opts={16: 1}))
    g.append(case('split2-64to64-K8-n300-option8-6', 'k_spconv_bf16_fast<64, false, true>', 8, 64, 64, 300, n_in=257, split=2, reducer='k_sum_splits4',
                  opts={8: 6}))
    g.append(case('split8-64to64-K27-n300-odd-ldy-acc', 'k_spconv_bf16_fast<64, false, true>', 27, 64, 64, 300, n_in=257, acc=1, ldy_pad=3, split=8,
                  reducer='k_sum_splits'))
    g.append(case('split8-64to64-K27-n129-tail-odd-ldy', 'k_spconv_bf16_fast<64, false, true>', 27, 64, 64, 129, n_in=257, bias=1, ldy_pad=1, split=8,
                  reducer='split_tail', opts={16: 1}))
    g.append(case('split-no-workspace-64to64-K27-n300', 'k_spconv_bf16_fast<64, false, true>', 27, 64, 64, 300, n_in=257, ws=False, acc=1))
    g.append(case('split8-64to128-K27-n300-weight-sharing-order', 'k_spconv_bf16_fast<128, false, true>', 27, 64, 128, 300, n_in=257, bias=1, split=8,
                  reducer='k_sum_splits4', opts={20: 1}))
    g.append(case('split8-64to64-K27-n300-two-live-taps-acc', 'k_spconv_bf16_fast<64, false, true>', 27, 64, 64, 300, n_in=257, map='sparse', acc=1, split=8,
                  reducer='k_sum_splits4'))
    g.append(case('split8-64to64-K27-n300-two-live-taps-tail', 'k_spconv_bf16_fast<64, false, true>', 27, 64, 64, 300, n_in=257, map='sparse', bias=1, split=8,
                  reducer='split_tail', opts={16: 1}))
    g.append(case('split8-dma-64to64-K27-n129-two-live-taps', 'k_spconv_bf16_dma<64, 2>', 27, 64, 64, 129, n_in=257, map='sparse', xh=1, split=8,
                  reducer='k_sum_splits4', opts={11: 64}))
    g.append(case('split8-shadow-64to64-K27-n1', 'k_spconv_bf16_fast<64, true, true>', 27, 64, 64, 1, n_in=40, xh=1, split=8, reducer='k_sum_splits4'))
    # the row-GEMM family (K = 1, no map, n_in >= n_out): both generations, every width, every epilogue mode
    widths = [(2, 128, 64, 128), (2, 64, 64, 64), (2, 32, 48, 32), (1, 128, 64, 128), (1, 64, 64, 64), (1, 32, 48, 32), (1, 16, 24, 48), (1, 16, 64, 16)]
    i = 0
    for wi, (gen, nt, cin, cout) in enumerate(widths):
        for m in RG_MODES:
            m = dict(m)
            tag = m.pop('tag')
            o = {13: 0} if (gen == 1 and nt >= 32) else {}
            if cin >= 64 and cout % 64 == 0 and m.get('mode', 'plain') == 'plain':
                o[24] = 0                                                        # (k_lin_small would take the plain f32 launch)
            n = ROWS[(i + wi) % len(ROWS)]                                      # (10 modes, 5 row counts: the width index mixes them)
            i += 1
            g.append(case(f'rowgemm{gen}-{nt}-{cin}to{cout}-n{n}-{tag}', f"k_rowgemm{'2' if gen == 2 else ''}_bf16<{nt}>", 1, cin, cout, n, n_in=n + (i % 3),
                          map=None, opts=o, **m))
    g.append(case('rowgemm2-declined-bf16-y-8bytes-off', 'k_rowgemm_bf16<64>', 1, 64, 64, 129, map=None, mode='io', yh=1, y_off=4, ldy_pad=8))
    g.append(case('rowgemm2-declined-bf16-ldy-4', 'k_rowgemm_bf16<128>', 1, 64, 128, 127, map=None, mode='io', yh=1, res=1, act=1, ldy_pad=4))
    g.append(case('rowgemm2-declined-bf16-res-8bytes-off', 'k_rowgemm_bf16<32>', 1, 48, 32, 129, map=None, mode='io', res=1, rh=1, r_off=4, act=3))
    g.append(case('rowgemm-declined-y-4bytes-off', 'k_spconv_bf16_fast<64, false, true>', 1, 64, 64, 129, map=None, mode='affine', y_off=1))
    g.append(case('rowgemm128-min-cin-option12', 'k_rowgemm2_bf16<64>', 1, 64, 128, 129, map=None, mode='affine', opts={12: 128}))
    g.append(case('rowgemm128-min-wgs-option19', 'k_rowgemm2_bf16<64>', 1, 64, 128, 129, map=None, mode='affine', opts={19: 3}))
    g.append(case('rowgemm-off-option3', 'k_spconv_bf16_fast<64, false, true>', 1, 64, 64, 129, map=None, bias=1, opts={3: 0}))
    # k_lin_small: one and several 256-channel stages are 64 -> 64 and 256 -> 256 here; rows around its 64-row tile
    for j, n in enumerate((1, 63, 64, 65)):
        g.append(case(f'lin-small-64to64-n{n}', 'k_lin_small', 1, 64, 64, n, n_in=n + j, map=None, bias=j & 1, acc=(j >> 1) & 1, ldy_pad=4 * (j & 1)))
        g.append(case(f'lin-small-256to256-n{n}', 'k_lin_small', 1, 256, 256, n, n_in=n + 1, map=None, bias=1 - (j & 1), acc=j & 1, ldx_pad=4))
    g.append(case('lin-small-off-option24', 'k_rowgemm2_bf16<64>', 1, 64, 64, 65, map=None, bias=1, opts={24: 0}))
    # the 320-column tile (from 16 384 rows, hard-coded)
    g.append(case('rowgemm320-64to320-n16384-bias', 'k_rowgemm2_bf16<320>', 1, 64, 320, 16384, map=None, bias=1))
    g.append(case('rowgemm320-64to320-n16385-shadow-affine-act1', 'k_rowgemm2_bf16<320>', 1, 64, 320, 16385, n_in=16386, map=None, xh=1, mode='io', act=1,
                  ldy_pad=4))
    g.append(case('rowgemm320-one-row-fewer', 'k_rowgemm2_bf16<64>', 1, 64, 320, 16383, map=None, bias=1))
    # k_expand_bf16 (option 25 lowered to 1)
    for j, n in enumerate((1, 15, 16, 17, 1000)):
        for cin in (16, 32, 64):
            g.append(case(f'expand-{cin}to{4 * cin}-n{n}', f'k_expand_bf16<{cin}>', 1, cin, 4 * cin, n, n_in=n + (j & 1), map=None, mode='io', xh=1, yh=1,
                          res=(j + cin // 16) & 1, rh=1, act=(j >> 1) & 1, ldx_pad=8 * (j & 1), ldy_pad=8 * ((j >> 1) & 1), ldr_pad=8 * (j & 1), opts={25: 1}))
    g.append(case('expand-few-workgroups-option26', 'k_expand_bf16<32>', 1, 32, 128, 1000, map=None, mode='io', xh=1, yh=1, res=1, rh=1, act=1, opts={25: 1, 26: 3}))
    g.append(case('expand-off-below-option25', 'k_rowgemm2_bf16<128>', 1, 32, 128, 999, map=None, mode='io', xh=1, yh=1, res=1, rh=1, act=1, opts={25: 1000}))
    for i, c in enumerate(g):
        c['seed'] = 2000 + i
    return g


CASES = _grid()
assert len({c['name'] for c in CASES}) == len(CASES)


def _esize(half):
    return 2 if half else 4


def geometry(c):
    """-> ldx, ldy, ldr (elements of the operand's own type).  Unless a case says otherwise every leading dimension is padded by 16 bytes (4 f32 /
    8 bf16 elements): no alignment gate of the plan sees the difference, every kernel's row stride does"""
    ldx = c['cin'] + (c['ldx_pad'] if c['ldx_pad'] is not None else (8 if c['xh'] else 4))
    ldy = c['cout'] + (c['ldy_pad'] if c['ldy_pad'] is not None else (8 if c['yh'] else 4))
    ldr = c['cout'] + (c['ldr_pad'] if c['ldr_pad'] is not None else (8 if c['rh'] else 4))
    return ldx, ldy, ldr


def options(c):
    o = dict(S.DEFAULTS)
    o.update(c['opts'])
    return o


def restated_plan(c, have_ws=None):
    ldx, ldy, ldr = geometry(c)
    o = options(c)
    have_ws = (c['ws'] and c['mode'] == 'plain') if have_ws is None else have_ws
    L = S.launch(xh=c['xh'], yh=c['yh'], rh=c['rh'], ldx=ldx, ldy=ldy, ldr=ldr, x_mod=(c['x_off'] * _esize(c['xh'])) % 16,
                 y_mod=(c['y_off'] * _esize(c['yh'])) % 16, r_mod=(c['r_off'] * _esize(c['rh'])) % 16, has_map=c['map'] is not None, n_out=c['n_out'],
                 n_in=c['n_in'], K=c['K'], cin=c['cin'], cout=c['cout'], bias=bool(c['bias']), scale=c['mode'] != 'plain', shift=bool(c['shift']),
                 res=bool(c['res']), act=c['act'], acc=c['acc'],
                 ws_floats=S.split_workspace_floats(c['n_out'], c['K'], c['cin'], c['cout'], o) if have_ws else 0)
    return S.plan_fwd(L, o)


def promised(c, p):
    """the restated plan must be the one the case's name promises"""
    assert p.kernel == c['kernel'], f"{c['name']}: the restated plan runs {p.kernel}, the case promises {c['kernel']}"
    assert p.split == c['split'], f"{c['name']}: the restated plan splits {p.split} ways, the case promises {c['split']}"
    assert p.reducer == c['reducer'], f"{c['name']}: the restated plan reduces with {p.reducer}, the case promises {c['reducer']}"


def place_map(rng, n_out, n_in, K, sparse=False):
    """the (n_out, K) map of a case.  About 40 % of the (row, tap) pairs, naming rows 1 .. n_in - 1 (X row 0 stays unreferenced), then:
    row n_out // 2 without a pair, the second 128-row tile (rows 128 .. 255, n_out >= 257) without a pair, tap K // 2 (K >= 2) unused, tap
    K - 1 (K >= 3) used by the last row only, rows 0 and n_out - 1 with a pair in tap 0, both naming row n_in - 1.  sparse: taps 0 and 2
    alone carry the random pairs -- a tile's compacted tap list is shorter than a split launch has slices, some slices get no tap"""
    lo = min(1, n_in - 1)
    nbr = np.full((n_out, K), -1, dtype=np.int32)
    m = rng.random((n_out, K)) < (0.4 if K > 1 else 0.9)
    if sparse:
        m[:, [k for k in range(K) if k not in (0, 2)]] = False
    nbr[m] = rng.integers(lo, n_in, size=int(m.sum()))
    if K >= 2:
        nbr[:, K // 2] = -1
    if K >= 3:
        nbr[:, K - 1] = -1
        nbr[n_out - 1, K - 1] = n_in - 1
    if n_out >= 3:
        nbr[n_out // 2] = -1
    if n_out >= 257:
        nbr[128:256] = -1
    nbr[0, 0] = nbr[n_out - 1, 0] = n_in - 1
    return nbr


def rows_buffer(dev, rng, n, C, ld, off, half, live):
    """-> (flat buffer, (n, C) view): normal values in the live rows, NaN in every other row, in the ld - C padding columns and around"""
    m = np.full((n, ld), np.nan, dtype=np.float32)
    m[live, :C] = (rng.standard_normal((int(live.sum()), C)) * np.exp2(rng.integers(-3, 4, size=(1, C)))).astype(np.float32)
    flat = torch.full((off + n * ld + 16,), NAN, dtype=F32)
    flat[off:off + n * ld] = torch.from_numpy(m).reshape(-1)
    flat = (flat.to(B16) if half else flat).to(dev)
    assert flat.data_ptr() % 16 == 0
    return flat, flat[off:off + n * ld].view(n, ld)[:, :C]


def window_buffer(dev, n, C, ld, off, half, fill):
    """-> (flat, window): SENT pads | `off` SENT elements | n rows of ld elements (NaN, the (n, C) window = fill or NaN) | SENT pads"""
    dt = B16 if half else F32
    flat = torch.full((PAD + off + n * ld + PAD,), SENT, dtype=dt, device=dev)
    body = flat[PAD + off:PAD + off + n * ld]
    body.fill_(NAN)
    win = body.view(n, ld)[:, :C]
    if fill is not None:
        win.copy_(fill.to(dt))
    assert flat.data_ptr() % 16 == 0
    return flat, win


def bits(t):
    return t.view(torch.int16 if t.dtype == B16 else torch.int32)


def outside_intact(label, flat, before, n, C, ld, off):
    """everything but the (n, C) window holds its prefill bit for bit: the pads, the ld padding, the elements before a shifted base"""
    a, b = bits(flat).clone(), bits(before).clone()
    for t in (a, b):
        t[PAD + off:PAD + off + n * ld].view(n, ld)[:, :C] = 0
    if not torch.equal(a, b):
        i = int(torch.nonzero(a != b)[0])
        raise AssertionError(f'{label}: a launch wrote outside its output window (flat element {i - PAD - off} relative to the base, ld {ld}, C {C})')


def set_options(opts):
    for k, v in opts.items():
        _hip().call('es_set_option', k, v)


def restore_options(opts):
    for k in opts:
        _hip().call('es_set_option', k, S.DEFAULTS[k])


def _p(t):
    return t.data_ptr() if t is not None else 0


def normalise(expr):
    """a launch-log kernel expression -> the name plan_fwd gives: the row GEMMs keep their width only (MT for the fused transposed taps)"""
    e = expr.strip('()').replace(' ', '')
    m = re.match(r'(k_rowgemm2?_bf16)<(\d+),(\w+)(?:,(\w+))?', e)
    if m:
        return f"{m.group(1)}<{m.group(2)}{', MT' if (m.group(4) == 'true') else ''}>"
    return e.replace(',', ', ')


class Problem:
    """the operands, the map and the f64 specification of a case (built once; run() launches on fresh Y / workspace)"""

    def __init__(self, dev, c):
        self.dev, self.c = dev, c
        self.opts = options(c)
        self.plan = restated_plan(c)
        promised(c, self.plan)
        self.ldx, self.ldy, self.ldr = geometry(c)
        n_out, n_in, K, cin, cout = c['n_out'], c['n_in'], c['K'], c['cin'], c['cout']
        rng = np.random.default_rng(c['seed'])
        self.nbr = place_map(rng, n_out, n_in, K, c['map'] == 'sparse') if c['map'] is not None else None
        rows = max(n_in, n_out) + 1                                                  # rows >= n_in exist and hold NaN
        live = np.zeros(rows, dtype=bool)
        if self.nbr is None:
            live[:min(n_out, n_in)] = True
        else:
            assert int(self.nbr.max()) == n_in - 1 and int(self.nbr.min()) >= -1
            live[np.unique(self.nbr[self.nbr >= 0])] = True
            assert n_in == 1 or not live[0]
        self.xflat, self.x = rows_buffer(dev, rng, rows, cin, self.ldx, c['x_off'], c['xh'], live)
        w = torch.from_numpy((rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)).to(B16)
        self.wt = w.transpose(1, 2).contiguous().to(dev)                              # [K][Cout][Cin]: the reduction index contiguous
        col = lambda lo, hi: torch.from_numpy((rng.random(cout) * (hi - lo) + lo).astype(np.float32)).to(dev)
        self.bias = col(-1, 1) if c['bias'] else None
        self.scale = col(0.5, 1.5) * (1 - 2 * (torch.arange(cout, device=dev) % 3 == 0)) if c['mode'] != 'plain' else None
        self.shift = col(-1, 1) if c['shift'] else None
        self.rflat = self.res = None
        if c['res']:
            r = rng.standard_normal((n_out, cout)).astype(np.float32)
            r.reshape(-1)[::7] = 0.0                                                 # the gate's edge: 0.0 and -0.0 are closed
            r.reshape(-1)[3::14] = -0.0
            self.rflat, self.res = window_buffer(dev, n_out, cout, self.ldr, c['r_off'], c['rh'], torch.from_numpy(r))
        self.prior = torch.from_numpy(rng.standard_normal((n_out, cout)).astype(np.float32)).to(dev) if c['acc'] else None
        self.nbr_d = torch.from_numpy(self.nbr).to(dev) if self.nbr is not None else None
        cv, A, pairs = S.conv(S.operand(self.x), S.operand(w.to(dev)), self.nbr_d, n_out, n_in)
        self.pairs = pairs
        self.spec, self.lin, self.slack = S.specify(cv, A, pairs, cin, self.bias, self.scale, self.shift, self.res, c['act'], self.prior, bool(c['yh']))
        # the inputs alone, before any kernel runs: finite, and a contribution wherever one is intended
        assert bool(torch.isfinite(self.spec).all()) and bool((A[pairs > 0] > 0).all()), f"{c['name']}: the case's inputs leave a live row dead"

    def queries(self):
        c = self.c
        need = int(_hip().raw('es_spconv_split_workspace_floats')(c['n_out'], c['K'], c['cin'], c['cout']))
        want = S.split_workspace_floats(c['n_out'], c['K'], c['cin'], c['cout'], self.opts)
        assert need == want, f"{c['name']}: es_spconv_split_workspace_floats = {need}, the restated plan needs {want}"
        fast = int(_hip().raw('es_spconv_bf16_is_fast')(c['n_in'], self.ldx, c['K'], c['cin'], c['cout']))
        assert fast == S.is_fast(c['n_in'], self.ldx, c['K'], c['cin'], c['cout']), f"{c['name']}: es_spconv_bf16_is_fast = {fast}"
        return need

    def run(self, launches=None):
        """one launch -> (status, Y pad buffer, its prefill, Y window)"""
        c = self.c
        need = self.queries()
        use_ws = c['ws'] and c['mode'] == 'plain' and need > 0
        self.wsflat = None
        if use_ws:
            self.wsflat = torch.full((PAD + need + PAD,), SENT, dtype=F32, device=self.dev)
            self.wsflat[PAD:PAD + need] = NAN
            self.wsflat[PAD:PAD + S.SPLIT_TICKETS] = 0.0
        ws = self.wsflat[PAD:PAD + need] if use_ws else None
        flat, y = window_buffer(self.dev, c['n_out'], c['cout'], self.ldy, c['y_off'], c['yh'], self.prior)
        before = flat.clone()
        if launches is not None:
            launches()
        head = (_p(self.x), c['xh'], self.ldx, _p(self.wt), _p(self.nbr_d), c['n_out'], c['n_in'], c['K'], c['cin'], c['cout'])
        if c['mode'] == 'plain' and use_ws:
            rc = _rc('es_spconv_fwd_bf16_ws', *head, _p(self.bias), _p(y), self.ldy, c['acc'], _p(ws), need, _st())
        elif c['mode'] == 'plain':
            rc = _rc('es_spconv_fwd_bf16', *head, _p(self.bias), _p(y), self.ldy, c['acc'], _st())
        elif c['mode'] == 'affine':
            assert not (c['xh'] or c['yh'] or c['rh'])
            rc = _rc('es_spconv_fwd_bf16_affine', head[0], *head[2:], _p(self.scale), _p(self.shift), _p(self.res), self.ldr, c['act'], _p(y), self.ldy, _st())
        else:
            rc = _rc('es_spconv_fwd_bf16_io', *head, _p(self.scale), _p(self.shift), _p(self.res), c['rh'], self.ldr, c['act'], _p(y), c['yh'], self.ldy, _st())
        _sync()
        if launches is not None and rc == 0:
            ran = [ln for ln in launches()]
            names = [normalise(ln.split(' grid=')[0]) for ln in ran]
            p = self.plan
            want = [p.kernel] + ([p.reducer] if p.reducer in ('k_sum_splits', 'k_sum_splits4') else [])
            assert names == want, f"{c['name']}: launched {names}, the restated plan says {want}"
            z = int(re.search(r'grid=\(?\s*\d+\s*,\s*\d+\s*,\s*(\d+)', ran[0]).group(1))
            assert z == p.split, f"{c['name']}: gridDim.z = {z}, the restated plan splits {p.split} ways"
        if use_ws:
            assert bool((self.wsflat[:PAD] == SENT).all()) and bool((self.wsflat[PAD + need:] == SENT).all()), f"{c['name']}: wrote outside the workspace"
            assert not bool(bits(self.wsflat[PAD:PAD + S.SPLIT_TICKETS]).any()), f"{c['name']}: tile tickets not zero on exit"
        return rc, flat, before, y

    def check(self, y):
        p = self.plan
        cls = p.kernel + (f' + {p.reducer} x{p.split}' if p.reducer else '')
        return S.check(self.c['name'], y, self.spec, self.lin, self.slack, self.prior, cls, STATS)


def conv_case(dev, c, launches=None):
    set_options(c['opts'])
    try:
        pb = Problem(dev, c)
        rc, flat, before, y = pb.run(launches)
        assert rc == 0, (c['name'], rc)
        outside_intact(c['name'], flat, before, c['n_out'], c['cout'], pb.ldy, c['y_off'])
        ratio = pb.check(y)
        rc2, flat2, _, y2 = pb.run()
        assert rc2 == 0 and torch.equal(bits(y2), bits(y)), f"{c['name']}: two runs differ"
        print(f"{c['name']}: {pb.plan.kernel}, split {pb.plan.split}, {pb.plan.reducer}, {int(pb.pairs.sum())} pairs, worst ratio {ratio:.3f}")
    finally:
        restore_options(c['opts'])


@pytest.mark.parametrize('name', [c['name'] for c in CASES])
def test_convolution_per_element(dev, name):
    conv_case(dev, next(c for c in CASES if c['name'] == name))


# ------------------------------------------------------------------------------------------------------------------ es_spconv_fwd
F32_CASES = [  # name, kernel, K, cin, cout, n_out, n_in, map, trans_w, bias, acc, ldx_pad, ldy_pad, opts
    ('f32-3to5-K1-n1', 'k_spconv<false>', 1, 3, 5, 1, 4, 'placed', 0, 1, 0, 2, 1, {}),
    ('f32-24to72-K8-n129', 'k_spconv<false>', 8, 24, 72, 129, 77, 'placed', 0, 1, 0, 1, 3, {}),
    ('f32-24to72-K8-n129-transposed-weights-acc', 'k_spconv<true>', 8, 24, 72, 129, 200, 'placed', 1, 0, 1, 0, 0, {}),
    ('f32-130to67-K27-n257-transposed-weights', 'k_spconv<true>', 27, 130, 67, 257, 300, 'placed', 1, 0, 0, 2, 1, {}),
    ('f32-24to72-identity-nin<nout', 'k_spconv<false>', 1, 24, 72, 129, 77, None, 0, 0, 1, 4, 0, {}),
    ('f32-24to72-identity-nin>nout-transposed-weights', 'k_spconv<true>', 1, 24, 72, 127, 200, None, 1, 1, 0, 0, 4, {}),
    ('narrow-n1', 'k_spconv_narrow_fwd<3>', 27, 3, 64, 1, 9, 'placed', 0, 1, 0, 0, 0, {}),
    ('narrow-n63-acc', 'k_spconv_narrow_fwd<3>', 27, 3, 64, 63, 40, 'placed', 0, 0, 1, 1, 4, {}),
    ('narrow-n64', 'k_spconv_narrow_fwd<3>', 27, 3, 64, 64, 100, 'placed', 0, 0, 0, 0, 0, {}),
    ('narrow-n65-bias-acc', 'k_spconv_narrow_fwd<3>', 27, 3, 64, 65, 64, 'placed', 0, 1, 1, 2, 1, {}),
    ('narrow-n257', 'k_spconv_narrow_fwd<3>', 27, 3, 64, 257, 300, 'placed', 0, 1, 0, 0, 0, {}),
    ('narrow-off-option21', 'k_spconv<false>', 27, 3, 64, 65, 64, 'placed', 0, 1, 0, 0, 0, {21: 0}),
    ('narrow-transposed-weights-keeps-the-tile', 'k_spconv<true>', 27, 3, 64, 65, 64, 'placed', 1, 0, 0, 0, 0, {}),
]


def f32_case(dev, name, kernel, K, cin, cout, n_out, n_in, mp, trans_w, bias, acc, ldx_pad, ldy_pad, opts, launches=None):
    set_options(opts)
    try:
        o = dict(S.DEFAULTS)
        o.update(opts)
        p = S.plan_f32(mp is not None, K, cin, cout, trans_w, o)
        assert p.kernel == kernel, f'{name}: the restated plan runs {p.kernel}, the case promises {kernel}'
        rng = np.random.default_rng(len(name) * 131 + n_out)
        nbr = place_map(rng, n_out, n_in, K) if mp else None
        rows = max(n_in, n_out) + 1
        live = np.zeros(rows, dtype=bool)
        if nbr is None:
            live[:min(n_out, n_in)] = True
        else:
            live[np.unique(nbr[nbr >= 0])] = True
        ldx, ldy = cin + ldx_pad, cout + ldy_pad
        xflat, x = rows_buffer(dev, rng, rows, cin, ldx, 0, 0, live)
        w = torch.from_numpy((rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)).to(dev)
        wk = w.transpose(1, 2).contiguous() if trans_w else w
        b = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).to(dev) if bias else None
        prior = torch.from_numpy(rng.standard_normal((n_out, cout)).astype(np.float32)).to(dev) if acc else None
        nbr_d = torch.from_numpy(nbr).to(dev) if nbr is not None else None
        cv, A, pairs = S.conv(S.operand(x, False), S.operand(w, False), nbr_d, n_out, n_in)
        spec, lin, slack = S.specify(cv, A, pairs, cin, b, prior=prior)
        got = []
        for rep in range(2):
            flat, y = window_buffer(dev, n_out, cout, ldy, 0, 0, prior)
            before = flat.clone()
            if launches is not None:
                launches()
            rc = _rc('es_spconv_fwd', _p(x), ldx, _p(wk), _p(nbr_d), n_out, n_in, K, cin, cout, _p(b), _p(y), ldy, trans_w, acc, _st())
            _sync()
            assert rc == 0, (name, rc)
            if launches is not None:
                ran = [normalise(ln.split(' grid=')[0]) for ln in launches()]
                assert ran == [kernel], f'{name}: launched {ran}'
            outside_intact(name, flat, before, n_out, cout, ldy, 0)
            got.append(y)
        ratio = S.check(name, got[0], spec, lin, slack, prior, f'es_spconv_fwd {kernel}', STATS)
        assert torch.equal(bits(got[0]), bits(got[1])), f'{name}: two runs differ'
        print(f'{name}: {kernel}, worst ratio {ratio:.3f}')
    finally:
        restore_options(opts)


@pytest.mark.parametrize('args', F32_CASES, ids=[a[0] for a in F32_CASES])
def test_exact_f32_convolution_per_element(dev, args):
    f32_case(dev, *args)


# ------------------------------------------------------------------------------------------------------------------ fused transposed taps
GT_CASES = [(cin, cout, n) for cin, cout in ((64, 64), (128, 64), (32, 96)) for n in (1, 127, 129)]


def gen_transpose_case(dev, cin, cout, n, launches=None):
    """es_gen_transpose_fwd_bf16: y[i, t Cout ...] = r(x[i]) r(w[t]) (Y contiguous (n, 8 Cout)); es_gen_transpose_dgrad_bf16:
    dX[i] (+)= sum_t r(dY[i, t Cout ...]) r(w[t])^T, with and without accumulate"""
    rng = np.random.default_rng(cin * 7 + cout + n)
    w = torch.from_numpy((rng.standard_normal((8, cin, cout)) / np.sqrt(cin)).astype(np.float32)).to(B16).to(dev)
    wn, wt = w.contiguous(), w.transpose(1, 2).contiguous()
    live = np.ones(n + 1, dtype=bool)
    live[n] = False
    ldx = cin + 4
    xflat, x = rows_buffer(dev, rng, n + 1, cin, ldx, 0, 0, live)
    label = f'gen-transpose {cin}->{cout} n={n}'
    pf = S.plan_gen_transpose(cout, cin, ldx, 8 * cout, 0, False, cout)
    y_spec, A = S.gen_transpose_fwd(S.operand(x[:n]), S.operand(w))
    lin = S.U * np.sqrt(cin) * A
    outs = []
    for rep in range(2):
        flat, y = window_buffer(dev, n, 8 * cout, 8 * cout, 0, 0, None)
        before = flat.clone()
        if launches is not None:
            launches()
        rc = _rc('es_gen_transpose_fwd_bf16', _p(x), ldx, _p(wt), n, cin, cout, _p(y), _st())
        _sync()
        assert rc == 0, (label, rc)
        if launches is not None:
            ran = launches()
            assert [normalise(ln.split(' grid=')[0]) for ln in ran] == [pf.kernel], (label, ran)
        outside_intact(label, flat, before, n, 8 * cout, 8 * cout, 0)
        outs.append(y)
    S.check(label + ' forward', outs[0], y_spec, lin, torch.zeros_like(lin), None, f'es_gen_transpose_fwd_bf16 {pf.kernel}', STATS)
    assert torch.equal(bits(outs[0]), bits(outs[1])), f'{label}: two forward runs differ'
    # the data gradient: dY is the contiguous (n, 8 Cout) matrix, dX has its own leading dimension
    dyflat, dy = rows_buffer(dev, rng, n + 1, 8 * cout, 8 * cout, 0, 0, live)
    pd = S.plan_gen_transpose(cin, cout, 8 * cout, ldx, 0, True, cout)
    dx_spec, Ad = S.gen_transpose_dgrad(S.operand(dy[:n]), S.operand(w))
    lind = S.U * np.sqrt(8 * cout) * Ad
    for acc in (0, 1):
        prior = torch.from_numpy(rng.standard_normal((n, cin)).astype(np.float32)).to(dev) if acc else None
        outs = []
        for rep in range(2):
            flat, dx = window_buffer(dev, n, cin, ldx, 0, 0, prior)
            before = flat.clone()
            if launches is not None:
                launches()
            rc = _rc('es_gen_transpose_dgrad_bf16', _p(dy), _p(wn), n, cin, cout, _p(dx), ldx, acc, _st())
            _sync()
            assert rc == 0, (label, rc)
            if launches is not None:
                ran = launches()
                assert [normalise(ln.split(' grid=')[0]) for ln in ran] == [pd.kernel], (label, ran)
            outside_intact(label, flat, before, n, cin, ldx, 0)
            outs.append(dx)
        spec = dx_spec + (prior.to(S.F64) if acc else 0)
        slack = S.U * prior.to(S.F64).abs() if acc else torch.zeros_like(lind)
        S.check(label + f' data gradient acc={acc}', outs[0], spec, lind, slack, prior, f'es_gen_transpose_dgrad_bf16 {pd.kernel}', STATS)
        assert torch.equal(bits(outs[0]), bits(outs[1])), f'{label}: two data-gradient runs differ'


@pytest.mark.parametrize('cin,cout,n', GT_CASES)
def test_fused_transposed_taps_per_element(dev, cin, cout, n):
    gen_transpose_case(dev, cin, cout, n)


def gen_transpose_not_served_case(dev):
    """shapes and operands the fused launchers answer 1 for (the caller issues the per-tap launches): nothing is written"""
    rng = np.random.default_rng(5)
    n = 33
    for cin, cout, ldx_pad, x_off, what in ((64, 48, 4, 0, 'Cout % 32'), (20, 64, 4, 0, 'Cin % 8'), (64, 64, 3, 0, 'ldx % 4'), (64, 64, 4, 1, 'X 4 bytes off')):
        ldx = cin + ldx_pad
        xflat, x = rows_buffer(dev, rng, n, cin, ldx, x_off, 0, np.ones(n, dtype=bool))
        w = torch.zeros((8, cout, cin), dtype=B16, device=dev)
        flat, y = window_buffer(dev, n, 8 * cout, 8 * cout, 0, 0, None)
        before = flat.clone()
        assert S.plan_gen_transpose(cout, cin, ldx, 8 * cout, (x_off * 4) % 16, False, cout) is None
        rc = _rc('es_gen_transpose_fwd_bf16', _p(x), ldx, _p(w), n, cin, cout, _p(y), _st())
        _sync()
        assert rc == 1 and torch.equal(bits(flat), bits(before)), f'es_gen_transpose_fwd_bf16 ({what}): status {rc}, or Y written'
    for cin, cout, ldx_pad, what in ((48, 64, 4, 'Cin % 32'), (64, 20, 4, 'Cout % 8'), (64, 64, 3, 'ldx % 4')):
        ldx = cin + ldx_pad
        dyflat, dy = rows_buffer(dev, rng, n, 8 * cout, 8 * cout, 0, 0, np.ones(n, dtype=bool))
        w = torch.zeros((8, cin, cout), dtype=B16, device=dev)
        for acc in (0, 1):
            flat, dx = window_buffer(dev, n, cin, ldx, 0, 0, torch.ones(n, cin) if acc else None)
            before = flat.clone()
            assert S.plan_gen_transpose(cin, cout, 8 * cout, ldx, 0, True, cout) is None
            rc = _rc('es_gen_transpose_dgrad_bf16', _p(dy), _p(w), n, cin, cout, _p(dx), ldx, acc, _st())
            _sync()
            assert rc == 1 and torch.equal(bits(flat), bits(before)), f'es_gen_transpose_dgrad_bf16 ({what}): status {rc}, or dX written'


def test_fused_transposed_taps_not_served(dev):
    gen_transpose_not_served_case(dev)


# ------------------------------------------------------------------------------------------------------------------ refusals
def refusals_case(dev):
    """the status of every refused launch, with Y and the workspace left bit-identical to their prefill"""
    rng = np.random.default_rng(9)
    n, cin, cout = 40, 64, 64
    xflat, x = rows_buffer(dev, rng, n, cin, cin + 8, 0, 0, np.ones(n, dtype=bool))
    xhflat, xh = rows_buffer(dev, rng, n, cin, cin + 8, 0, 1, np.ones(n, dtype=bool))
    w = torch.zeros((28, cout, cin), dtype=B16, device=dev)
    w32 = torch.zeros((28, cin, cout), dtype=F32, device=dev)
    nbr = torch.zeros((n, 28), dtype=torch.int32, device=dev)
    ones = torch.ones(cout, device=dev)
    prior = torch.ones(n, cout)
    ws = torch.full((S.SPLIT_TICKETS + 8 * n * cout,), NAN, device=dev)
    ws[:S.SPLIT_TICKETS] = 0
    ws0 = ws.clone()

    def refused(label, want, fn, half=0, ldy=cout, C=cout, y_off=0, fill=None):
        flat, y = window_buffer(dev, n, C, ldy, y_off, half, fill)
        before = flat.clone()
        rc = fn(y)
        _sync()
        assert rc == want, f'{label}: status {rc}, expected {want}'
        assert torch.equal(bits(flat), bits(before)), f'{label}: Y written by a refused launch'
        assert torch.equal(bits(ws), bits(ws0)), f'{label}: workspace written by a refused launch'

    # K > 27 -> -2, every entry point
    refused('es_spconv_fwd K = 28', -2, lambda y: _rc('es_spconv_fwd', _p(x), cin + 8, _p(w32), _p(nbr), n, n, 28, cin, cout, 0, _p(y), cout, 0, 0, _st()))
    refused('es_spconv_fwd_bf16 K = 28', -2, lambda y: _rc('es_spconv_fwd_bf16', _p(x), 0, cin + 8, _p(w), _p(nbr), n, n, 28, cin, cout, 0, _p(y), cout, 0, _st()))
    refused('es_spconv_fwd_bf16_ws K = 28', -2, lambda y: _rc('es_spconv_fwd_bf16_ws', _p(xh), 1, cin + 8, _p(w), _p(nbr), n, n, 28, cin, cout, 0, _p(y), cout,
                                                              1, _p(ws), ws.numel(), _st()), fill=prior)
    refused('es_spconv_fwd_bf16_affine K = 28', -2, lambda y: _rc('es_spconv_fwd_bf16_affine', _p(x), cin + 8, _p(w), _p(nbr), n, n, 28, cin, cout, _p(ones),
                                                                  _p(ones), 0, 0, 1, _p(y), cout, _st()))
    refused('es_spconv_fwd_bf16_io K = 28', -2, lambda y: _rc('es_spconv_fwd_bf16_io', _p(xh), 1, cin + 8, _p(w), _p(nbr), n, n, 28, cin, cout, _p(ones),
                                                              _p(ones), 0, 0, 0, 1, _p(y), 1, cout, _st()), half=1)
    # bf16 Y: ldy % 4, Cout % 4, a base 4 bytes off -> -7 (accumulation into bf16 rows has no entry point: es_spconv_fwd_bf16_io never accumulates)
    io = lambda y, ldy, C, res=0, rh=0, ldr=0: _rc('es_spconv_fwd_bf16_io', _p(xh), 1, cin + 8, _p(w), _p(nbr), n, n, 8, cin, C, _p(ones), _p(ones), res, rh, ldr,
                                                   1, _p(y), 1, ldy, _st())
    refused('bf16 Y with ldy % 4', -7, lambda y: io(y, cout + 2, cout), half=1, ldy=cout + 2)
    refused('bf16 Y with Cout % 4', -7, lambda y: io(y, cout, cout - 2), half=1, ldy=cout, C=cout - 2)
    refused('bf16 Y 4 bytes off', -7, lambda y: io(y, cout, cout), half=1, y_off=2)
    # a misaligned bf16 res (4 bytes off; ldr % 4) -> -7, f32 and bf16 Y
    rflat, r = window_buffer(dev, n, cout, cout + 2, 2, 1, torch.ones(n, cout))
    refused('bf16 res 4 bytes off, bf16 Y', -7, lambda y: io(y, cout, cout, _p(r), 1, cout + 4), half=1)
    refused('bf16 res with ldr % 4, bf16 Y', -7, lambda y: io(y, cout, cout, _p(rflat), 1, cout + 2), half=1)
    refused('bf16 res 4 bytes off, f32 Y', -7, lambda y: _rc('es_spconv_fwd_bf16_io', _p(x), 0, cin + 8, _p(w), _p(nbr), n, n, 8, cin, cout, _p(ones), _p(ones),
                                                              _p(r), 1, cout + 4, 1, _p(y), 0, cout, _st()))
    # n_out = 0 -> 0, nothing written (K > 27 included: an empty launch is not looked at)
    for K in (8, 28):
        refused(f'n_out = 0, K = {K}', 0, lambda y: _rc('es_spconv_fwd_bf16_ws', _p(xh), 1, cin + 8, _p(w), _p(nbr), 0, n, K, cin, cout, 0, _p(y), cout, 0, _p(ws),
                                                        ws.numel(), _st()))
        refused(f'es_spconv_fwd n_out = 0, K = {K}', 0, lambda y: _rc('es_spconv_fwd', _p(x), cin + 8, _p(w32), _p(nbr), 0, n, K, cin, cout, 0, _p(y), cout, 0, 1,
                                                                     _st()), fill=prior)
    refused('es_gen_transpose_fwd_bf16 n = 0', 0, lambda y: _rc('es_gen_transpose_fwd_bf16', _p(x), cin + 8, _p(w), 0, cin, 8, _p(y), _st()))


def test_refusal_codes_leave_everything_untouched(dev):
    refusals_case(dev)


# ------------------------------------------------------------------------------------------------------------------ implied maps
def grid_map(B, dims, ks, st, pad):
    """the neighbour map an address-arithmetic launcher implies, built on the host: rows in lexicographic grid order, taps in lexicographic
    order of their offsets; output voxel o under tap t reads input voxel o * st + t - pad (absent outside the grid) -> (nbr, output dims)"""
    nd = len(dims)
    odims = [(d + 2 * pad - ks) // st + 1 for d in dims]
    o = np.stack(np.meshgrid(np.arange(B), *[np.arange(d) for d in odims], indexing='ij'), -1).reshape(-1, nd + 1)
    taps = np.stack(np.meshgrid(*[np.arange(ks)] * nd, indexing='ij'), -1).reshape(-1, nd)
    nbr = np.full((len(o), len(taps)), -1, dtype=np.int32)
    for t, off in enumerate(taps):
        src = o[:, 1:] * st + off - pad
        ok = ((src >= 0) & (src < np.array(dims))).all(1)
        row = o[:, 0]
        for a in range(nd):
            row = row * dims[a] + np.clip(src[:, a], 0, dims[a] - 1)
        nbr[ok, t] = row[ok]
    return nbr, odims


def _weights(dev, rng, K, cin, cout):
    """-> w (K, Cin, Cout) bf16 values on dev, its natural and its transposed ([K][Cout][Cin]) copy"""
    w = torch.from_numpy((rng.standard_normal((K, cin, cout)) / np.sqrt(K * cin)).astype(np.float32)).to(B16).to(dev)
    return w, w.contiguous(), w.transpose(1, 2).contiguous()


def _launch_checked(label, fn, dev, n, C, ld, half, prior, launches, kernel, runs=2):
    """`runs` launches of fn(Y pointer) on fresh Y buffers: status 0, nothing outside the window, the promised kernel, the same bits"""
    outs = []
    for rep in range(runs):
        flat, y = window_buffer(dev, n, C, ld, 0, half, prior)
        before = flat.clone()
        if launches is not None:
            launches()
        rc = fn(_p(y))
        _sync()
        assert rc == 0, (label, rc)
        if launches is not None:
            ran = [normalise(ln.split(' grid=')[0]) for ln in launches()]
            assert len(ran) >= 1 and kernel in ran[0], f'{label}: launched {ran}, expected {kernel}'
        outside_intact(label, flat, before, n, C, ld, 0)
        outs.append(y)
    assert all(torch.equal(bits(outs[0]), bits(o)) for o in outs[1:]), f'{label}: two runs differ'
    return outs[0]


# ------------------------------------------------------------------------------------------------------------------ es_spconv_halo_bf16
HALO_CASES = [  # n_out, n_in, cin, cout, mirror, bias, acc, ldy_pad, sparse
    (257, 300, 64, 128, 0, 1, 0, 4, False),
    (300, 200, 128, 256, 1, 0, 1, 0, True),
    (1, 40, 64, 128, 0, 0, 0, 0, False),
    (129, 129, 64, 128, 1, 1, 1, 4, True),
]


def halo_case(dev, n_out, n_in, cin, cout, mirror, bias, acc, ldy_pad, sparse, launches=None):
    """es_halo_plan + es_spconv_halo_bf16 on a placed 27-tap map (256-row tiles: one ragged, one with an all -1 half), both mirror values:
    mirror 1 reads the plan's column 26 - k under tap k"""
    rng = np.random.default_rng(n_out * 3 + cin + mirror)
    K = 27
    nbr = place_map(rng, n_out, n_in, K, sparse)
    live = np.zeros(n_in + 1, dtype=bool)
    live[np.unique(nbr[nbr >= 0])] = True
    ldx, ldy = cin + 8, cout + ldy_pad
    xflat, x = rows_buffer(dev, rng, n_in + 1, cin, ldx, 0, 1, live)
    w, wn, wt = _weights(dev, rng, K, cin, cout)
    b = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).to(dev) if bias else None
    prior = torch.from_numpy(rng.standard_normal((n_out, cout)).astype(np.float32)).to(dev) if acc else None
    nbr_d = torch.from_numpy(nbr).to(dev)
    rows = int(_hip().raw('es_halo_plan_rows')(n_out))
    assert rows == S.cdiv(n_out, 256) * 256
    loc = torch.full((rows, K), -2, dtype=torch.int16, device=dev)
    hrows = torch.full((rows // 256, 256 * K), -7, dtype=torch.int32, device=dev)
    hcnt = torch.full((rows // 256,), -7, dtype=torch.int32, device=dev)
    assert _rc('es_halo_plan', _p(nbr_d), n_out, K, _p(loc), _p(hrows), _p(hcnt), _st()) == 0
    _sync()
    eff = torch.from_numpy(np.ascontiguousarray(nbr[:, ::-1])).to(dev) if mirror else nbr_d
    cv, A, pairs = S.conv(S.operand(x), S.operand(w), eff, n_out, n_in)
    spec, lin, slack = S.specify(cv, A, pairs, cin, b, prior=prior)
    label = f'halo {cin}->{cout} n_out={n_out} mirror={mirror}'
    y = _launch_checked(label, lambda yp: _rc('es_spconv_halo_bf16', _p(x), ldx, _p(wt), _p(loc), _p(hrows), _p(hcnt), n_out, n_in, K, cin, cout, _p(b), yp,
                                               ldy, acc, mirror, _st()), dev, n_out, cout, ldy, 0, prior, launches, 'k_spconv_halo')
    ratio = S.check(label, y, spec, lin, slack, prior, 'es_spconv_halo_bf16 k_spconv_halo<128>', STATS)
    print(f'{label}: worst ratio {ratio:.3f}')


@pytest.mark.parametrize('args', HALO_CASES, ids=[f'n{a[0]}-{a[2]}to{a[3]}-mirror{a[4]}' for a in HALO_CASES])
def test_halo_convolution_per_element(dev, args):
    halo_case(dev, *args)


# ------------------------------------------------------------------------------------------------------------------ es_dconv_fwd_bf16
DCONV_CASES = [  # B, X, Y, Z, stride, mode, cin, cout, acc, ldy_pad
    (2, 5, 4, 3, 1, 0, 64, 128, 0, 4),
    (1, 6, 4, 4, 2, 0, 64, 256, 1, 0),
    (1, 5, 4, 3, 1, 1, 128, 64, 0, 4),
    (2, 3, 4, 5, 1, 1, 128, 128, 1, 0),
]


def dconv_case(dev, B, X, Y, Z, st, mode, cin, cout, acc, ldy_pad, launches=None):
    """es_dconv_fwd_bf16, nn.Conv3d(3, stride, 1): mode 0 forward; mode 1 (stride 1) its data gradient = the same map with the taps mirrored
    and the natural weight copy read transposed"""
    import ctypes
    rng = np.random.default_rng(B * 100 + X * 10 + mode + st)
    K = 27
    g = (ctypes.c_int * 7)(B, X, Y, Z, 3, st, 1)
    nbr, (Xo, Yo, Zo) = grid_map(B, (X, Y, Z), 3, st, 1)
    n_in, n_out = B * X * Y * Z, B * Xo * Yo * Zo
    kd, n = (cin, cout) if mode == 0 else (cout, cin)                     # reduction / result channels
    if mode == 1:
        assert st == 1 and n_out == n_in
    assert int(_hip().raw('es_dconv_supported')(g, mode, cin, cout)) == 1
    ldx, ldy = kd + 8, n + ldy_pad
    xflat, x = rows_buffer(dev, rng, n_in + 1, kd, ldx, 0, 1, np.arange(n_in + 1) < n_in)
    w, wn, wt = _weights(dev, rng, K, cin, cout)
    w_eff = w if mode == 0 else w.flip(0).transpose(1, 2)                 # (K, reduction, result)
    prior = torch.from_numpy(rng.standard_normal((n_out, n)).astype(np.float32)).to(dev) if acc else None
    cv, A, pairs = S.conv(S.operand(x), S.operand(w_eff), torch.from_numpy(nbr).to(dev), n_out, n_in)
    spec, lin, slack = S.specify(cv, A, pairs, kd, prior=prior)
    need = int(_hip().raw('es_dconv_workspace_floats')(g, mode, cin, cout))
    wsflat = torch.full((PAD + max(need, 4) + PAD,), SENT, dtype=F32, device=dev)
    wsflat[PAD:PAD + max(need, 4)] = NAN
    label = f'dconv mode {mode} {B}x{X}x{Y}x{Z} stride {st} {cin}->{cout}'
    y = _launch_checked(label, lambda yp: _rc('es_dconv_fwd_bf16', _p(x), ldx, _p(wt if mode == 0 else wn), g, mode, cin, cout, yp, ldy, acc,
                                               _p(wsflat[PAD:]) if need else 0, need, _st()), dev, n_out, n, ldy, 0, prior, launches, 'k_dconv')
    assert bool((wsflat[:PAD] == SENT).all()) and bool((wsflat[PAD + max(need, 4):] == SENT).all()), f'{label}: wrote outside the workspace'
    ratio = S.check(label, y, spec, lin, slack, prior, f'es_dconv_fwd_bf16 mode {mode}', STATS)
    print(f'{label}: worst ratio {ratio:.3f}')


@pytest.mark.parametrize('args', DCONV_CASES, ids=[f'mode{a[5]}-stride{a[4]}-{a[6]}to{a[7]}' for a in DCONV_CASES])
def test_dense_convolution_per_element(dev, args):
    dconv_case(dev, *args)


# ------------------------------------------------------------------------------------------------------------------ es_img_conv3_bf16
IMG_CASES = [  # C, W (output width decides the tile), stride, mode, H, y_half, act, workgroups option (0: default)   -- the IC_LAUNCH table
    (16, 70, 1, 0, 5, 1, 1, 4), (16, 20, 1, 0, 5, 0, 0, 0), (32, 20, 1, 0, 5, 1, 1, 4), (64, 12, 1, 0, 5, 1, 0, 2), (32, 24, 2, 0, 10, 1, 1, 4),
    (16, 70, 1, 1, 5, 0, 3, 4), (16, 20, 1, 1, 5, 0, 3, 0), (32, 20, 1, 1, 5, 0, 3, 4), (64, 12, 1, 1, 5, 0, 3, 2),
]


def img_conv_case(dev, C, W, st, mode, H, y_half, act, wgs, launches=None):
    """es_img_conv3_bf16 on two images: mode 0 = act(scale conv + shift) on the 3x3 / pad 1 / stride map (bf16 or f32 rows out); mode 1 = the
    gated data gradient of a stride-1 layer (f32 gradient rows in, the natural weight copy, taps mirrored, scale, gate = bf16 activation rows)"""
    rng = np.random.default_rng(C + W + 7 * mode + st)
    n_img, K = 2, 9
    nbr, (Ho, Wo) = grid_map(n_img, (H, W), 3, st, 1)
    n_in, n_out = n_img * H * W, n_img * Ho * Wo
    assert int(_hip().raw('es_img_conv3_supported')(n_img, H, W, C, st, mode)) == 1
    ldx = C + (8 if mode == 0 else 4)
    ldy = C + (2 if y_half else 1)
    xflat, x = rows_buffer(dev, rng, n_in + 1, C, ldx, 0, int(mode == 0), np.arange(n_in + 1) < n_in)
    w, wn, wt = _weights(dev, rng, K, C, C)
    w_eff = w if mode == 0 else w.flip(0).transpose(1, 2)
    scale = torch.from_numpy((rng.random(C) + 0.5).astype(np.float32)).to(dev) * (1 - 2 * (torch.arange(C, device=dev) % 3 == 0))
    shift = torch.from_numpy(rng.standard_normal(C).astype(np.float32)).to(dev) if mode == 0 else None
    gflat = gate = None
    ldg = 0
    if mode == 1:
        r = rng.standard_normal((n_out, C)).astype(np.float32)
        r.reshape(-1)[::7] = 0.0
        r.reshape(-1)[3::14] = -0.0
        ldg = C + 8
        gflat, gate = window_buffer(dev, n_out, C, ldg, 0, 1, torch.from_numpy(r))
    cv, A, pairs = S.conv(S.operand(x), S.operand(w_eff), torch.from_numpy(nbr).to(dev), n_out, n_in)
    spec, lin, slack = S.specify(cv, A, pairs, C, scale=scale, shift=shift, res=gate, act=act, out_bf16=bool(y_half))
    label = f'img-conv3 C={C} {H}x{W} stride {st} mode {mode}'
    if wgs:
        _hip().raw('es_img_conv_set_option')(51, wgs)
    try:
        y = _launch_checked(label, lambda yp: _rc('es_img_conv3_bf16', _p(x), ldx, _p(wt if mode == 0 else wn), n_img, H, W, C, st, mode, _p(scale), _p(shift),
                                                   _p(gate), ldg, act if mode == 0 else 0, yp, y_half, ldy, _st()), dev, n_out, C, ldy, y_half, None, launches,
                            f'k_img_conv3<{C}, {128 if (C == 16 and Wo > 64) else 64 if C <= 32 else 32}, {st}, {mode}>')
    finally:
        _hip().raw('es_img_conv_set_option')(51, 1024)
    ratio = S.check(label, y, spec, lin, slack, None, f'es_img_conv3_bf16 C={C} stride {st} mode {mode}', STATS)
    print(f'{label}: worst ratio {ratio:.3f}')


@pytest.mark.parametrize('args', IMG_CASES, ids=[f'C{a[0]}-W{a[1]}-stride{a[2]}-mode{a[3]}' for a in IMG_CASES])
def test_image_convolution_per_element(dev, args):
    img_conv_case(dev, *args)


def not_taken_case(dev):
    """-4 of the halo and image launchers for operands their *_supported query cannot see (it answers 1): a base pointer 8 bytes off, a
    leading dimension the kernel cannot take; Y stays bit-identical to its prefill"""
    rng = np.random.default_rng(17)
    n, K, cin, cout = 40, 27, 64, 128
    nbr = torch.from_numpy(place_map(rng, n, n, K)).to(dev)
    loc = torch.zeros((256, K), dtype=torch.int16, device=dev)
    hrows = torch.zeros((1, 256 * K), dtype=torch.int32, device=dev)
    hcnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    assert _rc('es_halo_plan', _p(nbr), n, K, _p(loc), _p(hrows), _p(hcnt), _st()) == 0
    w = torch.zeros((K, cout, cin), dtype=B16, device=dev)
    _hip().raw('es_halo_set_option')(30, 1)
    try:
        assert int(_hip().raw('es_spconv_halo_supported')(n, n, cin + 8, K, cin, cout)) == 1
        for x_off, ldx, what in ((4, cin + 8, 'X 8 bytes off'), (0, cin + 4, 'ldx % 8')):
            xflat, x = rows_buffer(dev, rng, n, cin, ldx, x_off, 1, np.ones(n, dtype=bool))
            flat, y = window_buffer(dev, n, cout, cout, 0, 0, None)
            before = flat.clone()
            rc = _rc('es_spconv_halo_bf16', _p(x), ldx, _p(w), _p(loc), _p(hrows), _p(hcnt), n, n, K, cin, cout, 0, _p(y), cout, 0, 0, _st())
            _sync()
            assert rc == -4 and torch.equal(bits(flat), bits(before)), f'es_spconv_halo_bf16 ({what}): status {rc}, or Y written'
        wflat = torch.zeros(K * cout * cin + 8, dtype=B16, device=dev)
        xflat, x = rows_buffer(dev, rng, n, cin, cin + 8, 0, 1, np.ones(n, dtype=bool))
        flat, y = window_buffer(dev, n, cout, cout, 0, 0, None)
        before = flat.clone()
        rc = _rc('es_spconv_halo_bf16', _p(x), cin + 8, _p(wflat[4:]), _p(loc), _p(hrows), _p(hcnt), n, n, K, cin, cout, 0, _p(y), cout, 0, 0, _st())
        _sync()
        assert rc == -4 and torch.equal(bits(flat), bits(before)), f'es_spconv_halo_bf16 (weights 8 bytes off): status {rc}, or Y written'
    finally:
        _hip().raw('es_halo_set_option')(30, 192)
    n_img, H, W, C = 2, 5, 20, 32
    rows = n_img * H * W
    assert int(_hip().raw('es_img_conv3_supported')(n_img, H, W, C, 1, 0)) == 1
    wc = torch.zeros((9, C, C), dtype=B16, device=dev)
    ones = torch.ones(C, device=dev)
    for x_off, ldx, y_off, ldy, what in ((4, C + 8, 0, C, 'X 8 bytes off'), (0, C + 4, 0, C, 'ldx % 8'), (0, C + 8, 1, C, 'bf16 Y 2 bytes off'), (0, C + 8, 0, C + 1, 'bf16 ldy odd')):
        xflat, x = rows_buffer(dev, rng, rows, C, ldx, x_off, 1, np.ones(rows, dtype=bool))
        flat, y = window_buffer(dev, rows, C, ldy, y_off, 1, None)
        before = flat.clone()
        rc = _rc('es_img_conv3_bf16', _p(x), ldx, _p(wc), n_img, H, W, C, 1, 0, _p(ones), _p(ones), 0, 0, 1, _p(y), 1, ldy, _st())
        _sync()
        assert rc == -4 and torch.equal(bits(flat), bits(before)), f'es_img_conv3_bf16 ({what}): status {rc}, or Y written'
    # a forward activation its epilogue does not know (ELU, 2; the gate, 3): -4, the caller takes the map kernels
    for act in (2, 3):
        xflat, x = rows_buffer(dev, rng, rows, C, C + 8, 0, 1, np.ones(rows, dtype=bool))
        flat, y = window_buffer(dev, rows, C, C, 0, 1, None)
        before = flat.clone()
        rc = _rc('es_img_conv3_bf16', _p(x), C + 8, _p(wc), n_img, H, W, C, 1, 0, _p(ones), _p(ones), 0, 0, act, _p(y), 1, C, _st())
        _sync()
        assert rc == -4 and torch.equal(bits(flat), bits(before)), f'es_img_conv3_bf16 (act {act}): status {rc}, or Y written'
    # the gated data gradient without its gate: a missing operand, -4
    xflat, x = rows_buffer(dev, rng, rows, C, C + 4, 0, 0, np.ones(rows, dtype=bool))
    flat, y = window_buffer(dev, rows, C, C, 0, 0, None)
    before = flat.clone()
    rc = _rc('es_img_conv3_bf16', _p(x), C + 4, _p(wc), n_img, H, W, C, 1, 1, _p(ones), 0, 0, 0, 0, _p(y), 0, C, _st())
    _sync()
    assert rc == -4 and torch.equal(bits(flat), bits(before)), f'es_img_conv3_bf16 (no gate): status {rc}, or Y written'


def test_halo_and_image_launchers_answer_minus_4_for_operands_the_query_cannot_see(dev):
    not_taken_case(dev)
