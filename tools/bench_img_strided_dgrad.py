"""A/B of the stride-2 data-gradient kernels (csrc/imgconv.hip: es_img_dgrad3_s2_bf16, es_img_dgrad1_s2_bf16) against the map-kernel launches
they replace, at the image backbone's shapes of an mv-3ddet step (80 images, 480 x 480 input): five repetitions of a 10-launch timing each,
achieved GB/s of the compulsory bytes (gradient rows + gate rows + output rows), bit-identity (dev tool)"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from embodiedscan_amd.hip import P, call, raw

dev = torch.device('cuda:0')
st = torch.cuda.current_stream().cuda_stream


def timeit(fn, n=10):
    fn(); fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def five(fn):
    ts = sorted(timeit(fn) for _ in range(5))
    return ts


def fmt(ts, nbytes):
    return f'median {ts[2]:6.1f} us (min {ts[0]:6.1f}, max {ts[4]:6.1f}; {nbytes / ts[2] / 1e3:5.0f} GB/s = {nbytes / ts[2] / 1e3 / 8000 * 100:4.1f} % of 8 TB/s)'


def maps(n_img, H, W, k, pad):
    n, n_o = n_img * H * W, n_img * (H // 2) * (W // 2)
    nbr = torch.empty((n_o, k * k), dtype=torch.int32, device=dev)
    inv = torch.empty((n, k * k), dtype=torch.int32, device=dev)
    call('es_image_map', n_img, H, W, H // 2, W // 2, k, k, 2, pad, P(nbr), st)
    call('es_inverse_map', P(nbr), n_o, k * k, n, P(inv), st)
    return inv


print('gated 3x3 / stride-2 data gradient (n_img x H x W input grid x C)')
for name, n_img, H, W, C in (('layer2.0.conv2', 80, 120, 120, 32), ('layer3.0.conv2', 80, 60, 60, 64), ('layer4.0.conv2', 80, 30, 30, 128)):
    n, n_o = n_img * H * W, n_img * (H // 2) * (W // 2)
    gy, act = torch.randn(n_o, C, device=dev), torch.randn(n, C, device=dev).to(torch.bfloat16)
    w = torch.randn(9, C, C, device=dev) * 0.05
    wn, wt = torch.empty((9, C, C), dtype=torch.bfloat16, device=dev), torch.empty((9, C, C), dtype=torch.bfloat16, device=dev)
    call('es_cast_weight_bf16', P(w), 9, C, C, P(wn), P(wt), st)
    scale = torch.rand(C, device=dev) + 0.5
    inv = maps(n_img, H, W, 3, 1)
    nbytes = n_o * C * 4 + n * C * 2 + n * C * 4
    d1, d2 = torch.zeros(n, C, device=dev), torch.full((n, C), float('nan'), device=dev)
    t1 = five(lambda: call('es_spconv_fwd_bf16_io', P(gy), 0, C, P(wn), P(inv), n, n_o, 9, C, C, P(scale), 0, P(act), 1, C, 3, P(d1), 0, C, st))
    print(f'{name} {n_img} x {H} x {W} x {C}: compulsory {nbytes / 1e6:.0f} MB\n   map kernel   {fmt(t1, nbytes)}')
    if raw('es_img_dgrad3_s2_supported')(n_img, H, W, C) != 1:
        print('   image kernel: shape refused by the plan (stays on the map kernel)')
        continue
    for wgs in (512, 1024, 2048, 4096):
        call('es_img_stride_set_option', 53, wgs)
        t2 = five(lambda: call('es_img_dgrad3_s2_bf16', P(gy), C, P(wn), n_img, H, W, C, P(scale), P(act), C, P(d2), C, st))
        torch.cuda.synchronize()
        print(f'   image kernel {fmt(t2, nbytes)}  workgroups aimed for {wgs}  bit-identical {torch.equal(d1.view(torch.int32), d2.view(torch.int32))}'
              f'  faster by more than the spread {t2[4] < t1[0]}')
    call('es_img_stride_set_option', 53, 2048)

print('1x1 / stride-2 data gradient (n_img x H x W input grid, gradient channels -> input channels)')
for name, n_img, H, W, cg, cx in (('layer3.0.downsample', 80, 60, 60, 256, 128), ('layer4.0.downsample', 80, 30, 30, 512, 256)):
    n, n_o = n_img * H * W, n_img * (H // 2) * (W // 2)
    gy = torch.randn(n_o, cg, device=dev)
    w = torch.randn(1, cx, cg, device=dev) * 0.05
    wn, wt = torch.empty((1, cx, cg), dtype=torch.bfloat16, device=dev), torch.empty((1, cg, cx), dtype=torch.bfloat16, device=dev)
    call('es_cast_weight_bf16', P(w), 1, cx, cg, P(wn), P(wt), st)
    inv = maps(n_img, H, W, 1, 0)
    nbytes = n_o * cg * 4 + n * cx * 4
    print(f'{name} {n_img} x {H} x {W}, {cg} -> {cx}: compulsory {nbytes / 1e6:.0f} MB')
    for accumulate in (0, 1):
        d1, d2 = torch.ones(n, cx, device=dev), torch.ones(n, cx, device=dev)
        call('es_spconv_fwd_bf16', P(gy), 0, cg, P(wn), P(inv), n, n_o, 1, cg, cx, 0, P(d1), cx, accumulate, st)
        call('es_img_dgrad1_s2_bf16', P(gy), cg, P(wn), n_img, H, W, cg, cx, P(d2), cx, accumulate, st)
        torch.cuda.synchronize()
        same = torch.equal(d1.view(torch.int32), d2.view(torch.int32))
        t1 = five(lambda: call('es_spconv_fwd_bf16', P(gy), 0, cg, P(wn), P(inv), n, n_o, 1, cg, cx, 0, P(d1), cx, accumulate, st))
        t2 = five(lambda: call('es_img_dgrad1_s2_bf16', P(gy), cg, P(wn), n_img, H, W, cg, cx, P(d2), cx, accumulate, st))
        print(f'   accumulate {accumulate}: map kernel   {fmt(t1, nbytes)}\n'
              f'                 image kernel {fmt(t2, nbytes)}  bit-identical {same}  faster by more than the spread {t2[4] < t1[0]}')
