"""The stride-2 data-gradient kernels of the image backbone (embodiedscan_amd/csrc/imgconv.hip: k_img_dgrad3_s2, gradient rows in an LDS
ring, only the taps of a pixel's parity class; k_img_dgrad1_s2, a row GEMM over the gradient rows stored to the even pixels) under the CDNA
emulator of tests/emu: against numpy f64 evaluations on the bf16-rounded operands and, bit for bit, against the map-kernel launches they
replace (es_spconv_fwd_bf16_io gated / es_spconv_fwd_bf16 on es_image_map -> es_inverse_map); NaN-prefilled outputs, accumulate 0 / 1,
several bands per image, the launchers' refusals.  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import numpy as np

from test_emu_kernels import P, bf16_bits, bf16_round, emu  # noqa: F401  (the fixture)

CASES3 = [  # n_img, H, W (input grid), C, workgroups aimed for
    (2, 10, 22, 32, 4),
    (2, 8, 12, 64, 2),
    (1, 2, 2, 32, 1),
    (3, 6, 34, 32, 9),
]
CASES1 = [  # n_img, H, W (input grid), gradient channels, input channels
    (2, 10, 22, 64, 32),
    (1, 4, 6, 256, 128),
]


def _dgrad3_ref(gb, wb, n_img, H, W, C):
    """f64 transposed 3x3 / stride-2 / pad-1 convolution on channels-last rows: gb (n_img*H/2*W/2, C), wb (9, Cin, Cout) -> (n_img*H*W, C)"""
    Ho, Wo = H // 2, W // 2
    g = gb.reshape(n_img, Ho, Wo, C).astype(np.float64)
    dx = np.zeros((n_img, H + 2, W + 2, C))
    for ky in range(3):
        for kx in range(3):                 # output (oy, ox) read input (2 oy + ky - 1, 2 ox + kx - 1)
            dx[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] += g @ wb[ky * 3 + kx].astype(np.float64).T
    return dx[:, 1:H + 1, 1:W + 1].reshape(-1, C)


def _maps(emu, n_img, H, W, k, pad):
    n, n_o = n_img * H * W, n_img * (H // 2) * (W // 2)
    nbr, inv = np.zeros((n_o, k * k), np.int32), np.zeros((n, k * k), np.int32)
    emu('es_image_map', n_img, H, W, H // 2, W // 2, k, k, 2, pad, P(nbr), 0)
    emu('es_inverse_map', P(nbr), n_o, k * k, n, P(inv), 0)
    return inv


def test_gated_3x3_stride2_data_gradient(emu):
    rng = np.random.default_rng(21)
    try:
        for n_img, H, W, C, wgs in CASES3:
            assert emu.fns['es_img_dgrad3_s2_supported'](n_img, H, W, C) == 1
            emu('es_img_stride_set_option', 53, wgs)
            n, n_o = n_img * H * W, n_img * (H // 2) * (W // 2)
            gy = rng.standard_normal((n_o, C)).astype(np.float32)
            act = rng.standard_normal((n, C)).astype(np.float32)
            w = (rng.standard_normal((9, C, C)) / np.sqrt(9 * C)).astype(np.float32)
            scale = (0.5 + rng.random(C)).astype(np.float32)
            wt, wn = np.zeros((9, C, C), np.uint16), np.zeros((9, C, C), np.uint16)
            emu('es_cast_weight_bf16', P(w), 9, C, C, P(wn), P(wt), 0)
            ah = bf16_bits(act)
            want = np.where(bf16_round(act) > 0, _dgrad3_ref(bf16_round(gy), bf16_round(w), n_img, H, W, C) * scale, 0.0)
            out = np.full((n, C), np.nan, np.float32)
            emu('es_img_dgrad3_s2_bf16', P(gy), C, P(wn), n_img, H, W, C, P(scale), P(ah), C, P(out), C, 0)
            assert np.isfinite(out).all(), (n_img, H, W, C)
            err = np.abs(out - want).max() / np.abs(want).max()
            assert err < 2e-6, (n_img, H, W, C, err)
            inv = _maps(emu, n_img, H, W, 3, 1)
            out2 = np.zeros((n, C), np.float32)
            emu('es_spconv_fwd_bf16_io', P(gy), 0, C, P(wn), P(inv), n, n_o, 9, C, C, P(scale), 0, P(ah), 1, C, 3, P(out2), 0, C, 0)
            assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), (n_img, H, W, C, int((out != out2).sum()))
    finally:
        emu('es_img_stride_set_option', 53, 2048)


def test_1x1_stride2_data_gradient(emu):
    rng = np.random.default_rng(22)
    for n_img, H, W, cg, cx in CASES1:
        assert emu.fns['es_img_dgrad1_s2_supported'](n_img, H, W, cg, cx) == 1
        n, n_o = n_img * H * W, n_img * (H // 2) * (W // 2)
        gy = rng.standard_normal((n_o, cg)).astype(np.float32)
        w = (rng.standard_normal((1, cx, cg)) / np.sqrt(cg)).astype(np.float32)        # (1, Cin, Cout) of the layer
        wt, wn = np.zeros((1, cg, cx), np.uint16), np.zeros((1, cx, cg), np.uint16)
        emu('es_cast_weight_bf16', P(w), 1, cx, cg, P(wn), P(wt), 0)
        even = np.zeros((n_img, H, W, cx))
        even[:, ::2, ::2] = (bf16_round(gy).astype(np.float64) @ bf16_round(w)[0].astype(np.float64).T).reshape(n_img, H // 2, W // 2, cx)
        even = even.reshape(n, cx)
        inv = _maps(emu, n_img, H, W, 1, 0)
        pat = rng.standard_normal((n, cx)).astype(np.float32)
        for accumulate in (0, 1):
            out = np.full((n, cx), np.nan, np.float32) if not accumulate else pat.copy()
            emu('es_img_dgrad1_s2_bf16', P(gy), cg, P(wn), n_img, H, W, cg, cx, P(out), cx, accumulate, 0)
            want = even + (pat if accumulate else 0.0)
            assert np.isfinite(out).all()
            assert np.abs(out - want).max() < 2e-6 * np.abs(want).max(), (n_img, H, W, cg, cx, accumulate)
            odd = np.ones((n_img, H, W), bool)
            odd[:, ::2, ::2] = False
            odd = odd.reshape(n)
            if accumulate:
                assert np.array_equal(out[odd].view(np.uint32), pat[odd].view(np.uint32))       # not touched
            else:
                assert not out[odd].any()
            out2 = np.zeros((n, cx), np.float32) if not accumulate else pat.copy()
            emu('es_spconv_fwd_bf16', P(gy), 0, cg, P(wn), P(inv), n, n_o, 1, cg, cx, 0, P(out2), cx, accumulate, 0)
            assert np.array_equal(out.view(np.uint32), out2.view(np.uint32)), (n_img, H, W, cg, cx, accumulate)


def test_strided_data_gradient_refusals(emu):
    """odd H / W, a leading dimension that is no multiple of 4, a pointer 8 bytes off a 16-byte boundary, rows x ld >= 2^31 and channel counts
    outside the plan: -4 and an untouched output"""
    d3, d1 = emu.fns['es_img_dgrad3_s2_bf16'], emu.fns['es_img_dgrad1_s2_bf16']
    s3, s1 = emu.fns['es_img_dgrad3_s2_supported'], emu.fns['es_img_dgrad1_s2_supported']
    buf = np.full(1 << 16, 7.0, np.float32)
    a = (P(buf) + 15) // 16 * 16
    assert s3(80, 120, 120, 32) == 1 and s3(80, 60, 60, 64) == 1 and s3(80, 30, 30, 128) == 0 and s3(80, 60, 60, 32) == 1
    assert s3(80, 120, 160, 32) == 0 and s3(2, 9, 10, 32) == 0 and s3(2, 10, 9, 32) == 0 and s3(80, 120, 120, 16) == 0
    assert s3(1 << 13, 64, 128, 32) == 0                      # 2^26 rows x 32 channels
    assert s1(80, 60, 60, 256, 128) == 1 and s1(80, 30, 30, 512, 256) == 1 and s1(2, 5, 6, 64, 32) == 0 and s1(2, 6, 6, 48, 32) == 0
    assert s1(1 << 13, 64, 128, 64, 32) == 0
    for args in ((a, 32, a, 2, 9, 10, 32, a, a, 32, a, 32), (a, 32, a, 2, 10, 9, 32, a, a, 32, a, 32), (a, 34, a, 2, 10, 10, 32, a, a, 32, a, 32),
                 (a, 32, a, 2, 10, 10, 32, a, a, 32, a, 34), (a + 8, 32, a, 2, 10, 10, 32, a, a, 32, a, 32),
                 (a, 32, a, 2, 10, 10, 32, a, a, 32, a + 8, 32), (a, 32, a, 1 << 13, 64, 128, 32, a, a, 32, a, 32),
                 (a, 32, a, 2, 10, 10, 32, a, 0, 32, a, 32)):
        assert d3(*args, 0) == -4, args
    for args in ((a, 64, a, 2, 9, 10, 64, 32, a, 32), (a, 66, a, 2, 10, 10, 64, 32, a, 32), (a, 64, a, 2, 10, 10, 64, 32, a, 34),
                 (a + 8, 64, a, 2, 10, 10, 64, 32, a, 32), (a, 64, a, 2, 10, 10, 64, 32, a + 8, 32), (a, 64, a, 1 << 13, 64, 128, 64, 32, a, 32)):
        for accumulate in (0, 1):
            assert d1(*args, accumulate, 0) == -4, args
    assert (buf == 7.0).all()
