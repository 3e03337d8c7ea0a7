// 3x3 convolutions of the image backbone by address arithmetic (round 6; SURVEY 8a row A7: mmdet.ResNet depth 50, base_channels 16,
// configs/detection/mv-det3d_8xb4_embodiedscan-3d-284class-9dof.py:24-34 -- Bottleneck.conv2 of layer1 .. layer3: 16 / 32 / 64
// channels on 120^2 / 60^2 / 30^2 feature maps, 80 images per mv-3ddet step; the fused launches of engine.conv_affine):
//   MODE 0  forward:  Y = act((X * W) * scale[c] + shift[c])   X bf16 rows, Y bf16 (or f32) rows, stride 1 or 2, pad 1
//   MODE 1  gated data gradient of a stride-1 layer:  dX = (A > 0) ? (G * W^T mirrored) * scale[c] : 0
//           G f32 rows (rounded to bf16 on the way into LDS, like every gradient shadow), A = the layer input's bf16 activation rows
// The map kernels (k_spconv_bf16_fast / k_spconv_bf16<64>, spconv.hip) gather every tap's rows through a 9-wide int32 map: 59 us for
// a 37 MB problem (32 channels), 153 us at 16 channels (no fast path below 32 input channels).  On an image grid the neighbour of pixel
// x under tap tx is pixel x + tx - 1 of an image row that is already in LDS (the scheme of imgwgrad.hip):
//   * a workgroup owns a band of output rows of ONE image; the input rows live in a 4- (stride 2: 8-) slot LDS ring of W + 2 pixels
//     whose pad pixels stay zero (no border test in the loop), filled one output row ahead (MODE 0: LDS-DMA; MODE 1: f32 loads ->
//     bf16 -> ds_write); one barrier per output row;
//   * the 9 x C x C weights stay in REGISTERS for the whole launch (18 B fragments per wave at 32 / 64 channels; 16 channels: two taps
//     share one K = 32 MFMA: 5 fragments); A fragments are plain 16-byte LDS reads of [pixel][channel] rows;
//   * C <= 32: the four waves split the 16-pixel blocks of a row (each all output channels); C = 64: the waves split the output-channel
//     blocks (each all pixel blocks);
//   * the epilogue of the map kernels, fused: folded-BN scale / shift + ReLU + bf16 rows (forward), BN scale + ReLU gate (data gradient).
// Arithmetic: bf16 operands, f32 accumulation, taps in (ty, tx) order then channel chunks -- a fixed order: bit-reproducible.
#include "common.h"
#include "../../include/es_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

__device__ __attribute__((aligned(16))) unsigned short g_ic_zero[8];

template <int C, int WP, int S, int MODE>
__global__ __launch_bounds__(256) void k_img_conv3(const void* __restrict__ Xv, int ldx, const unsigned short* __restrict__ Wt,
                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                   const unsigned short* __restrict__ gate, int ldg, void* __restrict__ Yv, int ldy,
                                                   int y_half, int act, int H, int W, int rows_per_wg, int bands) {
  static_assert(MODE == 0 || S == 1, "the gated data gradient is built for stride 1");
  constexpr int RB = C * 2;                                 // bytes per pixel row of the ring
  constexpr int XP = S * WP + 2, X_BYTES = XP * RB;
  constexpr int NS = S == 1 ? 4 : 8;                        // ring slots
  constexpr int GX = RB / 16;                               // 16-byte granules per pixel
  constexpr int NCB = C / 16;                               // output-channel blocks
  constexpr bool CO_SPLIT = NCB >= 4;                       // waves split output-channel blocks (else: pixel blocks)
  constexpr int CBW = CO_SPLIT ? NCB / 4 : NCB;             // channel blocks per wave
  constexpr bool PAIR = C == 16;                            // two taps per K = 32 MFMA
  constexpr int KS = PAIR ? 1 : C / 32;                     // MFMA k steps per tap
  constexpr int NT = PAIR ? 5 : 9;                          // tap groups
  constexpr int NPB = WP / 16;                              // 16-pixel blocks per output row
  __shared__ __attribute__((aligned(16))) unsigned char smem[NS * X_BYTES];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, li = lane & 15, kq = lane >> 4;
  const int im = blockIdx.x / bands, band = blockIdx.x - im * bands;
  const int Ho = H / S, Wo = W / S;
  const int oy0 = band * rows_per_wg, oy1 = min(Ho, oy0 + rows_per_wg);
  if (oy0 >= oy1) return;
  for (int i = t; i < NS * X_BYTES / 16; i += 256) ((uint4*)smem)[i] = make_uint4(0u, 0u, 0u, 0u);

  // weights -> registers.  Forward: Wt = [tap][Cout][Cin] (Cin contiguous), tap t of the loop reads tap t.  Data gradient: Wt = the natural
  // [tap][Cin][Cout] copy read as [tap][N = Cin][K = Cout], and tap t of the loop (offset (ty - 1, tx - 1) on the GRADIENT grid) multiplies the
  // weights of the mirrored tap 8 - t.
  bf16x8_t Bf[NT][KS][CBW];
#pragma unroll
  for (int g = 0; g < NT; ++g)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int cw = 0; cw < CBW; ++cw) {
        const int cb = CO_SPLIT ? wv * CBW + cw : cw;
        int tap = PAIR ? 2 * g + (kq >> 1) : g;
        const int kc = PAIR ? (kq & 1) * 8 : ks * 32 + kq * 8;
        const bool ok = tap < 9;
        if (MODE == 1) tap = 8 - tap;
        const uint4 v = ok ? *(const uint4*)(Wt + ((size_t)(ok ? tap : 0) * C + cb * 16 + li) * C + kc) : make_uint4(0u, 0u, 0u, 0u);
        Bf[g][ks][cw] = __builtin_bit_cast(bf16x8_t, v);
      }
  __syncthreads();                                            // the ring is zero

  const unsigned short* Xh = (const unsigned short*)Xv;
  const float* Xf = (const float*)Xv;
  constexpr int NPX = (S * WP * GX + 255) / 256;            // 16-byte pieces per thread and image row
  // MODE 0: image row iy -> ring slot by LDS-DMA (pixels 0 .. W - 1 at LDS pixels 1 .. W; granules past W copy a zero granule)
  auto issue_x = [&](int iy) {
    if (iy < 0 || iy >= H) return;                          // (uniform)
    const unsigned short* src = Xh + ((size_t)im * H + iy) * W * ldx;
    unsigned char* dst = smem + (iy & (NS - 1)) * X_BYTES + RB;
#pragma unroll
    for (int j = 0; j < NPX; ++j) {
      const int e = (j * 4 + wv) * 64 + lane;
      if ((j * 4 + wv) * 64 < S * WP * GX) {                // (wave-uniform: whole 1 KB pieces)
        const int px = e / GX, g = e - px * GX;
        const unsigned short* p = px < W ? (src + (size_t)px * ldx + g * 8) : g_ic_zero;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)p,
                                         (__attribute__((address_space(3))) void*)(dst + (j * 4 + wv) * 1024), 16, 0, 0);
      }
    }
  };
  // MODE 1: gradient row iy (f32) -> registers -> bf16 -> ring slot
  constexpr int NLG = MODE == 1 ? (WP * C / 4 + 255) / 256 : 1;
  float4 greg[NLG];
  auto load_g = [&](int iy) {
    const float* src = Xf + ((size_t)im * H + iy) * W * ldx;
#pragma unroll
    for (int j = 0; j < NLG; ++j) {
      const int e = j * 256 + t, px = e / (C / 4), c4 = e - px * (C / 4);
      greg[j] = (iy >= 0 && iy < H && px < W) ? *(const float4*)(src + (size_t)px * ldx + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_g = [&](int iy) {
    if (iy < 0 || iy >= H) return;
    unsigned char* dst = smem + (iy & (NS - 1)) * X_BYTES + RB;
#pragma unroll
    for (int j = 0; j < NLG; ++j) {
      const int e = j * 256 + t, px = e / (C / 4), c4 = e - px * (C / 4);
      if (px < WP) {
        uint2 v;
        v.x = es_pack_bf16(greg[j].x, greg[j].y);
        v.y = es_pack_bf16(greg[j].z, greg[j].w);
        *(uint2*)(dst + px * RB + c4 * 8) = v;
      }
    }
  };

  // prologue: the input rows of the first output row and the rows the second one adds
  if (MODE == 0) {
    for (int r = -1; r <= 1 + (S - 1); ++r) issue_x(S * oy0 + r);
  } else {
    for (int r = -1; r <= 0; ++r) { load_g(oy0 + r); store_g(oy0 + r); }
    load_g(oy0 + 1);
  }
  for (int oy = oy0; oy < oy1; ++oy) {
    if (MODE == 1) store_g(oy + 1);                          // (its slot held row oy - 3: nobody reads it any more)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // this wave's pieces of the rows of output row oy have landed ...
    __syncthreads();                                          // ... everybody's; output row oy - 1 has been consumed
    if (MODE == 0) {
      if (S == 1) issue_x(oy + 2);
      else { issue_x(2 * oy + 3); issue_x(2 * oy + 4); }
    } else {
      load_g(oy + 2);
    }
#pragma unroll 1
    for (int pb = CO_SPLIT ? 0 : wv; pb < NPB; pb += CO_SPLIT ? 1 : 4) {
      const int p0 = pb * 16;
      if (p0 >= Wo) break;
      f32x4 acc[CBW];
#pragma unroll
      for (int cw = 0; cw < CBW; ++cw) acc[cw] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g = 0; g < NT; ++g) {
        // this lane's tap: 16 channels share one K = 32 step between two taps (lanes kq < 2: tap 2 g, kq >= 2: tap 2 g + 1)
        const int tap = PAIR ? 2 * g + (kq >> 1) : g;
        const int ty = tap / 3, tx = tap - ty * 3;
        const int iy = S * oy + ty - 1;
        const bool rowok = tap < 9 && iy >= 0 && iy < H;    // (a row outside the image contributes nothing: its slot may hold another row)
        const unsigned char* xr = smem + ((iy < 0 ? 0 : iy) & (NS - 1)) * X_BYTES + ((p0 + li) * S + tx) * RB;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int kc = PAIR ? (kq & 1) * 8 : ks * 32 + kq * 8;
          uint4 av = *(const uint4*)(xr + kc * 2);
          if (!rowok) av = make_uint4(0u, 0u, 0u, 0u);
          const bf16x8_t a = __builtin_bit_cast(bf16x8_t, av);
#pragma unroll
          for (int cw = 0; cw < CBW; ++cw) acc[cw] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, Bf[g][ks][cw], acc[cw], 0, 0, 0);
        }
      }
      // epilogue: lane (li, kq) holds pixels p0 + kq * 4 + r of channel cb * 16 + li
#pragma unroll
      for (int cw = 0; cw < CBW; ++cw) {
        const int col = (CO_SPLIT ? wv * CBW + cw : cw) * 16 + li;
        const float sc = scale ? scale[col] : 1.f, sh = (MODE == 0 && shift) ? shift[col] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int px = p0 + kq * 4 + r;
          const size_t row = ((size_t)im * Ho + oy) * Wo + px;
          float v = acc[cw][r] * sc + sh;
          if (MODE == 0) {
            if (act) v = fmaxf(v, 0.f);
            if (y_half) {                                    // bf16 rows: lanes (li, li ^ 1) share one 4-byte store
              const float vn = __shfl_xor(v, 1, 64);
              if (!(li & 1) && px < Wo) *(uint32_t*)((unsigned short*)Yv + row * ldy + col) = es_pack_bf16(v, vn);
            } else if (px < Wo) {
              ((float*)Yv)[row * ldy + col] = v;
            }
          } else if (px < Wo) {
            const float gt = __uint_as_float((uint32_t)gate[row * ldg + col] << 16);
            ((float*)Yv)[row * ldy + col] = gt > 0.f ? v : 0.f;
          }
        }
      }
    }
  }
}

static int ES_OPT_IMG_CONV = 1;
static int ES_OPT_IMG_CONV_WGS = 1024;
extern "C" int es_img_conv_set_option(int key, int value) {
  if (key == 50) { ES_OPT_IMG_CONV = value; return 0; }
  if (key == 51) { ES_OPT_IMG_CONV_WGS = value; return 0; }
  return -1;
}

static bool img_conv_plan(int n_img, int H, int W, int C, int stride, int mode, int& wp, int& rows, int& bands) {
  if (!ES_OPT_IMG_CONV || n_img <= 0 || H <= 0 || W <= 0) return false;
  if (mode == 1 && stride != 1) return false;
  if (stride != 1 && !(stride == 2 && H % 2 == 0 && W % 2 == 0)) return false;
  const int Ho = H / stride, Wo = W / stride;
  if (C == 16 && Wo <= 128 && stride == 1) wp = Wo <= 64 ? 64 : 128;
  else if (C == 32 && Wo <= 64) wp = 64;
  else if (C == 64 && Wo <= 32) wp = 32;
  else return false;
  if (C == 64 && stride == 2) return false;                 // (A/B, profiles/r6g_imgconv_ab.txt: 32 us against the map kernel's 26.5)
  // workgroups aimed for (A/B on 80 images): 1 024 at 16 / 32 channels, 512 for the 64-channel and the stride-2 launches
  const int target = (C == 64 || stride == 2) ? ES_OPT_IMG_CONV_WGS / 2 : ES_OPT_IMG_CONV_WGS;
  bands = target / n_img;
  if (bands < 1) bands = 1;
  if (bands > Ho) bands = Ho;
  rows = es_cdiv(Ho, bands);
  bands = es_cdiv(Ho, rows);
  return true;
}

// the whole gate of the path: the plan plus the operands' layout, alignment and 32-bit index range (a null pointer: a fresh buffer)
static bool img_conv_check(int n_img, int H, int W, int C, int stride, int mode, const void* X, int ldx, const void* W_bf16,
                           const void* Y, int y_half, int ldy, int& wp, int& rows, int& bands) {
  if (!img_conv_plan(n_img, H, W, C, stride, mode, wp, rows, bands)) return false;
  if ((ldx % (mode ? 4 : 8)) || ((((uintptr_t)X) | ((uintptr_t)W_bf16)) & 15) || (y_half ? ((ldy % 2) || (((uintptr_t)Y) & 3)) : 0)) return false;
  if (mode == 1 && y_half) return false;
  return (long long)n_img * H * W * (ldx > ldy ? ldx : ldy) < (1ll << 31);
}

// (for fresh contiguous operands; the launcher answers for the caller's own with -4)
extern "C" int es_img_conv3_supported(int n_img, int H, int W, int C, int stride, int mode) {
  int wp, rows, bands;
  return img_conv_check(n_img, H, W, C, stride, mode, nullptr, C, nullptr, nullptr, 0, C, wp, rows, bands) ? 1 : 0;
}

extern "C" int es_img_conv3_bf16(const void* X, int ldx, const void* W_bf16, int n_img, int H, int W, int C, int stride, int mode,
                                 const float* scale, const float* shift, const void* gate, int ldg, int act, void* Y, int y_half,
                                 int ldy, void* stream) {
  int wp, rows, bands;
  if (!img_conv_check(n_img, H, W, C, stride, mode, X, ldx, W_bf16, Y, y_half, ldy, wp, rows, bands)) return -4;
  if (mode == 1 && gate == nullptr) return -4;                 // (a missing operand, not a shape the query rejects)
  if (mode == 0 && act != 0 && act != 1) return -4;            // (the epilogue here knows ReLU only: ELU (2) stays with the map kernels)
  hipStream_t st = (hipStream_t)stream;
  const unsigned short* Wt = (const unsigned short*)W_bf16;
  const unsigned short* G = (const unsigned short*)gate;
#define IC_LAUNCH(C_, WP_, S_, M_)                                                                                           \
  hipLaunchKernelGGL((k_img_conv3<C_, WP_, S_, M_>), dim3(n_img * bands), dim3(256), 0, st, X, ldx, Wt, scale, shift, G, ldg, Y, ldy, \
                     y_half, act, H, W, rows, bands)
  if (mode == 0 && stride == 1) {
    if (C == 16 && wp == 128) IC_LAUNCH(16, 128, 1, 0);
    else if (C == 16) IC_LAUNCH(16, 64, 1, 0);
    else if (C == 32) IC_LAUNCH(32, 64, 1, 0);
    else IC_LAUNCH(64, 32, 1, 0);
  } else if (mode == 0) {
    if (C == 32) IC_LAUNCH(32, 64, 2, 0);
    else if (C == 64) IC_LAUNCH(64, 32, 2, 0);
    else return -4;
  } else {
    if (C == 16 && wp == 128) IC_LAUNCH(16, 128, 1, 1);
    else if (C == 16) IC_LAUNCH(16, 64, 1, 1);
    else if (C == 32) IC_LAUNCH(32, 64, 1, 1);
    else IC_LAUNCH(64, 32, 1, 1);
  }
#undef IC_LAUNCH
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ stride-2 data gradients by address arithmetic
// The data gradient of a stride-2 layer through the inverse map is mostly work on absent taps: a pixel (y, x) of the input grid receives
// from tap (ky, kx) only where y + 1 - ky and x + 1 - kx are even -- 1, 2, 2 or 4 of the nine taps by the parity of (y, x) -- and a 128-row
// tile of the map kernels holds every parity, so it runs all nine taps on every row (zero rows for the absent ones); the 1x1 / stride-2
// layers multiply and store four rows for every one that has a source.  Here the address arithmetic names the present taps:
//   k_img_dgrad3_s2  gated data gradient of a 3x3 / stride-2 / pad-1 layer: dX = (A > 0) ? (sum_taps G[o(p, tap)] W[tap]^T) * scale[c] : 0.
//     A workgroup owns a band of 2-row cells of ONE image; the gradient rows (f32 -> bf16 on the way in) sit in a 4-slot LDS ring of
//     Wo + 1 pixels whose pad pixel stays zero; cell cy needs gradient rows cy (input row 2 cy: ky = 1; row 2 cy + 1: ky = 2) and cy + 1
//     (row 2 cy + 1: ky = 0).  Per 16-pixel block of one x parity only the taps of that (y, x) parity class are issued, in ascending tap
//     order and 32-channel chunks with v_mfma_f32_16x16x32_bf16: the order of the map kernels, whose skipped taps added exact zeros --
//     bit-identical.  Weights ([9][Cin][Cout] natural copy) in registers, waves split as in k_img_conv3.
//   k_img_dgrad1_s2  data gradient of a 1x1 / stride-2 layer: a row GEMM over the (H/2 x W/2) gradient rows only, stored to pixel
//     (2 oy, 2 ox); accumulate = 0: the workgroup also stores zeros (16-byte stores) to the other three pixels of the 2x2 cell.
template <int C, int WPO>
__global__ __launch_bounds__(256) void k_img_dgrad3_s2(const float* __restrict__ G, int ldg, const unsigned short* __restrict__ Wn,
                                                       const float* __restrict__ scale, const unsigned short* __restrict__ gate, int lda,
                                                       float* __restrict__ dX, int ldx, int H, int W, int cells_per_wg, int bands) {
  constexpr int RB = C * 2;                                 // bytes per pixel row of the ring
  constexpr int XP = WPO + 1, X_BYTES = XP * RB;            // (pixel WPO: the zero pad read by the last odd pixel's kx = 0 tap)
  constexpr int NS = 4;
  constexpr int NCB = C / 16;
  constexpr bool CO_SPLIT = NCB >= 4;
  constexpr int CBW = CO_SPLIT ? NCB / 4 : NCB;
  constexpr int KS = C / 32;
  constexpr int NPB = WPO / 16;
  __shared__ __attribute__((aligned(16))) unsigned char smem[NS * X_BYTES];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, li = lane & 15, kq = lane >> 4;
  const int im = blockIdx.x / bands, band = blockIdx.x - im * bands;
  const int Ho = H / 2, Wo = W / 2;
  const int c0 = band * cells_per_wg, c1 = min(Ho, c0 + cells_per_wg);
  if (c0 >= c1) return;
  for (int i = t; i < NS * X_BYTES / 16; i += 256) ((uint4*)smem)[i] = make_uint4(0u, 0u, 0u, 0u);

  // weights -> registers: tap k of the natural [tap][Cin][Cout] copy read as [N = Cin][K = Cout]
  bf16x8_t Bf[9][KS][CBW];
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int cw = 0; cw < CBW; ++cw) {
        const int cb = CO_SPLIT ? wv * CBW + cw : cw;
        const uint4 v = *(const uint4*)(Wn + ((size_t)k * C + cb * 16 + li) * C + ks * 32 + kq * 8);
        Bf[k][ks][cw] = __builtin_bit_cast(bf16x8_t, v);
      }
  __syncthreads();                                            // the ring is zero

  constexpr int NLG = (WPO * C / 4 + 255) / 256;
  float4 greg[NLG];
  auto load_g = [&](int oy) {
    const float* src = G + ((size_t)im * Ho + oy) * Wo * ldg;
#pragma unroll
    for (int j = 0; j < NLG; ++j) {
      const int e = j * 256 + t, px = e / (C / 4), c4 = e - px * (C / 4);
      greg[j] = (oy < Ho && px < Wo) ? *(const float4*)(src + (size_t)px * ldg + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store_g = [&](int oy) {
    if (oy >= Ho) return;                                     // (a row outside the image: its reads are zeroed below)
    unsigned char* dst = smem + (oy & (NS - 1)) * X_BYTES;
#pragma unroll
    for (int j = 0; j < NLG; ++j) {
      const int e = j * 256 + t, px = e / (C / 4), c4 = e - px * (C / 4);
      if (px < WPO) {
        uint2 v;
        v.x = es_pack_bf16(greg[j].x, greg[j].y);
        v.y = es_pack_bf16(greg[j].z, greg[j].w);
        *(uint2*)(dst + px * RB + c4 * 8) = v;
      }
    }
  };

  load_g(c0);
  store_g(c0);
  load_g(c0 + 1);
  for (int cy = c0; cy < c1; ++cy) {
    store_g(cy + 1);                                          // (its slot held row cy - 3: nobody reads it any more)
    __syncthreads();                                          // rows cy, cy + 1 are in the ring; cell cy - 1 has been consumed
    load_g(cy + 2);
#pragma unroll 1
    for (int pb = CO_SPLIT ? 0 : wv; pb < NPB; pb += CO_SPLIT ? 1 : 4) {
      const int q0 = pb * 16;
      if (q0 >= Wo) break;
#pragma unroll
      for (int cls = 0; cls < 4; ++cls) {                    // the four parity classes of the cell: (row 2 cy + yr, pixels 2 q + px)
        const int yr = cls >> 1, px = cls & 1;
        f32x4 acc[CBW];
#pragma unroll
        for (int cw = 0; cw < CBW; ++cw) acc[cw] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          if ((ky == 1) != (yr == 0)) continue;              // even rows: ky = 1; odd rows: ky = 0, 2
          const int oy = (yr == 1 && ky == 0) ? cy + 1 : cy;
          const bool rowok = oy < Ho;                        // (the last odd row has no ky = 0 tap: the slot may hold another row)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            if ((kx == 1) != (px == 0)) continue;            // even pixels: kx = 1; odd pixels: kx = 0, 2
            const int k = ky * 3 + kx;
            const int ox = q0 + li + ((px == 1 && kx == 0) ? 1 : 0);
            const unsigned char* xr = smem + (oy & (NS - 1)) * X_BYTES + ox * RB;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
              uint4 av = *(const uint4*)(xr + (ks * 32 + kq * 8) * 2);
              if (!rowok) av = make_uint4(0u, 0u, 0u, 0u);
              const bf16x8_t a = __builtin_bit_cast(bf16x8_t, av);
#pragma unroll
              for (int cw = 0; cw < CBW; ++cw) acc[cw] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, Bf[k][ks][cw], acc[cw], 0, 0, 0);
            }
          }
        }
        // epilogue of the map kernels' gated launch: lane (li, kq) holds pixels 2 (q0 + kq * 4 + r) + px of channel cb * 16 + li
        const size_t rowy = ((size_t)im * H + 2 * cy + yr) * W;
#pragma unroll
        for (int cw = 0; cw < CBW; ++cw) {
          const int col = (CO_SPLIT ? wv * CBW + cw : cw) * 16 + li;
          const float sc = scale ? scale[col] : 1.f;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int q = q0 + kq * 4 + r;
            if (q < Wo) {
              const size_t row = rowy + 2 * q + px;
              const float v = (acc[cw][r] + 0.f) * sc + 0.f;
              const float gt = __uint_as_float((uint32_t)gate[row * lda + col] << 16);
              dX[row * ldx + col] = gt > 0.f ? v : 0.f;
            }
          }
        }
      }
    }
  }
}

#define ES_S2_LD 48                                         // bf16 elements per padded LDS row (96 B, as HLD of spconv.hip)
template <bool GH, int NB> struct S2Regs { float4 a[4]; uint4 b[NB]; };              // one thread's piece of a chunk: 16 f32 ...
template <int NB> struct S2Regs<true, NB> { uint4 a[2]; uint4 b[NB]; };             // ... or 16 bf16 gradient channels, and the weights
// GH: G holds bf16 rows (the pre-rounded values of the same gradient matrix, ldg in elements): staged as they are, same chunks and sums
template <int NT, bool GH = false>
__global__ __launch_bounds__(256) void k_img_dgrad1_s2(const float* __restrict__ G, int ldg, const unsigned short* __restrict__ Wn, int n_g,
                                                       int Kred, int Wo, float* __restrict__ dX, int ldx, int accumulate) {
  constexpr int NF = NT / 16;
  constexpr int NB = (NT + 63) / 64;
  constexpr int LD = ES_S2_LD;
  __shared__ __attribute__((aligned(16))) unsigned short As[2 * 128 * LD];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[2 * NT * LD];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, li = lane & 15, kq = lane >> 4;
  const int row0 = blockIdx.x * 128, n0 = blockIdx.y * NT;
  // gradient row (im, oy, ox) = q * Wo + ox with q = im * Ho + oy  ->  pixel (2 oy, 2 ox) of the input grid = row 4 q Wo + 2 ox
  if (!accumulate) {                                          // the three pixels of the 2x2 cell that have no source
    constexpr int C4 = NT / 4;
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e = t; e < 128 * C4; e += 256) {
      const int r = e / C4, c4 = e - r * C4, row = row0 + r;
      if (row < n_g) {
        const int q = row / Wo, ox = row - q * Wo;
        float* p = dX + ((size_t)4 * q * Wo + 2 * ox) * ldx + n0 + c4 * 4;
        *(float4*)(p + ldx) = z;
        *(float4*)(p + (size_t)2 * Wo * ldx) = z;
        *(float4*)(p + ((size_t)2 * Wo + 1) * ldx) = z;
      }
    }
  }
  f32x4 acc[2][NF];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < NF; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nC = Kred / 32;
  const int a_r = t >> 1, a_kk = (t & 1) * 16;               // A: one row, 16 consecutive channels
  const int b_n = t >> 2, b_kk = (t & 3) * 8;                // B: output channel b_n (+ 64), 8 consecutive reduction elements
  const int b_w = ((NT % 64 == 0) || b_n < NT) ? b_n : 0;    // (NT = 32: the upper threads re-read column 0 and store nothing)
  const bool a_ok = row0 + a_r < n_g;
  const float* a_src = G + (size_t)(a_ok ? row0 + a_r : 0) * ldg + a_kk;
  const unsigned short* a_srch = (const unsigned short*)G + (size_t)(a_ok ? row0 + a_r : 0) * ldg + a_kk;
  using Regs = S2Regs<GH, NB>;
  auto load_chunk = [&](Regs& R, int c) {
    if constexpr (GH) {
      const uint4* ph = (const uint4*)(a_srch + c * 32);
      R.a[0] = ph[0];
      R.a[1] = ph[1];
    } else {
      const float4* pa = (const float4*)(a_src + c * 32);
#pragma unroll
      for (int q = 0; q < 4; ++q) R.a[q] = pa[q];
    }
#pragma unroll
    for (int h = 0; h < NB; ++h) R.b[h] = *(const uint4*)(Wn + (size_t)(n0 + b_w + h * 64) * Kred + c * 32 + b_kk);
  };
  auto store_chunk = [&](const Regs& R, int buf) {
    uint4 v0, v1;
    if constexpr (GH) {
      v0 = R.a[0];
      v1 = R.a[1];
    } else {
      v0 = make_uint4(es_pack_bf16(R.a[0].x, R.a[0].y), es_pack_bf16(R.a[0].z, R.a[0].w), es_pack_bf16(R.a[1].x, R.a[1].y),
                      es_pack_bf16(R.a[1].z, R.a[1].w));
      v1 = make_uint4(es_pack_bf16(R.a[2].x, R.a[2].y), es_pack_bf16(R.a[2].z, R.a[2].w), es_pack_bf16(R.a[3].x, R.a[3].y),
                      es_pack_bf16(R.a[3].z, R.a[3].w));
    }
    if (!a_ok) v0 = v1 = make_uint4(0u, 0u, 0u, 0u);
    uint4* pa = (uint4*)&As[buf * 128 * LD + a_r * LD + a_kk];
    pa[0] = v0;
    pa[1] = v1;
#pragma unroll
    for (int h = 0; h < NB; ++h)
      if ((NT % 64 == 0) || b_n < NT) *(uint4*)&Bs[buf * NT * LD + (b_n + h * 64) * LD + b_kk] = R.b[h];
  };
  auto compute = [&](int buf) {
    bf16x8_t a[2], b[NF];
#pragma unroll
    for (int mf = 0; mf < 2; ++mf) a[mf] = *(const bf16x8_t*)&As[buf * 128 * LD + (wv * 32 + mf * 16 + li) * LD + kq * 8];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) b[nf] = *(const bf16x8_t*)&Bs[buf * NT * LD + (nf * 16 + li) * LD + kq * 8];
#pragma unroll
    for (int mf = 0; mf < 2; ++mf)
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mf], b[nf], acc[mf][nf], 0, 0, 0);
  };
  // chunk c is computed from buffer c & 1 while chunk c + 1 is written to the other one and chunk c + 2 is in flight: one barrier per chunk
  Regs R;
  load_chunk(R, 0);
  store_chunk(R, 0);
  load_chunk(R, nC > 1 ? 1 : 0);
  __syncthreads();
  for (int c = 0; c < nC; ++c) {
    if (c + 1 < nC) store_chunk(R, (c + 1) & 1);
    load_chunk(R, c + 2 < nC ? c + 2 : c);                    // (unconditional: past the end it re-reads a chunk that is never stored)
    compute(c & 1);
    __syncthreads();
  }
#pragma unroll
  for (int mf = 0; mf < 2; ++mf)
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + wv * 32 + mf * 16 + kq * 4 + r;
        if (row < n_g) {
          const int q = row / Wo, ox = row - q * Wo;
          float* p = dX + ((size_t)4 * q * Wo + 2 * ox) * ldx + n0 + nf * 16 + li;
          const float v = acc[mf][nf][r] + 0.f;               // (the map kernels' `+ bias`, absent: -0 -> +0)
          *p = accumulate ? (*p + v) : v;
        }
      }
}

static int ES_OPT_IMG_S2 = 1;
static int ES_OPT_IMG_S2_WGS = 2048;     // (A/B on 80 images, profiles/img_strided_dgrad_ab.txt: 32 channels 99 us at 1 024, 90 at 2 048; 64 channels 84 / 67)
extern "C" int es_img_stride_set_option(int key, int value) {
  if (key == 52) { ES_OPT_IMG_S2 = value; return 0; }
  if (key == 53) { ES_OPT_IMG_S2_WGS = value; return 0; }
  return -1;
}

// C = 32 (gradient width <= 64) and C = 64 (<= 32): the register-resident weights of k_img_conv3.  C = 128 (layer4.0.conv2, 30 -> 15) is not
// built: 9 x 128 x 128 bf16 does not fit in registers; it stays on the map kernel (below the 71 us cut of profiles/r6j_slowest_launches.txt).
static bool img_dgrad3_s2_check(int n_img, int H, int W, int C, const void* G, int ldg, const void* Wn, const void* gate, int lda,
                                const void* dX, int ldx, int& cells, int& bands) {
  if (!ES_OPT_IMG_S2 || n_img <= 0 || H <= 0 || W <= 0 || (H % 2) || (W % 2)) return false;
  const int Ho = H / 2, Wo = W / 2;
  if (!((C == 32 && Wo <= 64) || (C == 64 && Wo <= 32))) return false;
  if ((ldg % 4) || (ldx % 4) || ldg < C || ldx < C || lda < C) return false;
  if ((((uintptr_t)G) | ((uintptr_t)Wn) | ((uintptr_t)dX)) & 15) return false;
  const int ldm = ldx > lda ? ldx : lda;
  if ((long long)n_img * H * W * ldm >= (1ll << 31) || (long long)n_img * Ho * Wo * ldg >= (1ll << 31)) return false;
  bands = ES_OPT_IMG_S2_WGS / n_img;
  if (bands < 1) bands = 1;
  if (bands > Ho) bands = Ho;
  cells = es_cdiv(Ho, bands);
  bands = es_cdiv(Ho, cells);
  return true;
}

extern "C" int es_img_dgrad3_s2_supported(int n_img, int H, int W, int C) {
  int cells, bands;
  return img_dgrad3_s2_check(n_img, H, W, C, nullptr, C, nullptr, nullptr, C, nullptr, C, cells, bands) ? 1 : 0;
}

extern "C" int es_img_dgrad3_s2_bf16(const float* G, int ldg, const void* Wn_bf16, int n_img, int H, int W, int C, const float* scale,
                                     const void* gate, int lda, float* dX, int ldx, void* stream) {
  int cells, bands;
  if (!img_dgrad3_s2_check(n_img, H, W, C, G, ldg, Wn_bf16, gate, lda, dX, ldx, cells, bands)) return -4;
  if (G == nullptr || Wn_bf16 == nullptr || gate == nullptr || dX == nullptr) return -4;
  hipStream_t st = (hipStream_t)stream;
  const unsigned short* Wn = (const unsigned short*)Wn_bf16;
  const unsigned short* A = (const unsigned short*)gate;
  if (C == 32)
    hipLaunchKernelGGL((k_img_dgrad3_s2<32, 64>), dim3(n_img * bands), dim3(256), 0, st, G, ldg, Wn, scale, A, lda, dX, ldx, H, W, cells, bands);
  else
    hipLaunchKernelGGL((k_img_dgrad3_s2<64, 32>), dim3(n_img * bands), dim3(256), 0, st, G, ldg, Wn, scale, A, lda, dX, ldx, H, W, cells, bands);
  ES_CHECK_LAUNCH();
  return 0;
}

static bool img_dgrad1_s2_check(int n_img, int H, int W, int Cg, int Cx, const void* G, int ldg, const void* Wn, const void* dX, int ldx) {
  if (!ES_OPT_IMG_S2 || n_img <= 0 || H <= 0 || W <= 0 || (H % 2) || (W % 2)) return false;
  if (Cg <= 0 || Cx <= 0 || (Cg % 32) || (Cx % 32)) return false;
  if ((ldg % 4) || (ldx % 4) || ldg < Cg || ldx < Cx) return false;
  if ((((uintptr_t)G) | ((uintptr_t)Wn) | ((uintptr_t)dX)) & 15) return false;
  return (long long)n_img * H * W * ldx < (1ll << 31) && (long long)n_img * (H / 2) * (W / 2) * ldg < (1ll << 31);
}

extern "C" int es_img_dgrad1_s2_supported(int n_img, int H, int W, int Cg, int Cx) {
  return img_dgrad1_s2_check(n_img, H, W, Cg, Cx, nullptr, Cg, nullptr, nullptr, Cx) ? 1 : 0;
}

extern "C" int es_img_dgrad1_s2_bf16(const float* G, int ldg, const void* Wn_bf16, int n_img, int H, int W, int Cg, int Cx, float* dX, int ldx,
                                     int accumulate, void* stream) {
  const bool gh = (accumulate & ES_ACC_ROWS_BF16) != 0;       // bit 1: G holds bf16 rows, the pre-rounded values of the f32 matrix (ldg in elements)
  accumulate &= 1;
  if (!img_dgrad1_s2_check(n_img, H, W, Cg, Cx, G, ldg, Wn_bf16, dX, ldx)) return -4;
  if (G == nullptr || Wn_bf16 == nullptr || dX == nullptr || (gh && (ldg % 8))) return -4;
  hipStream_t st = (hipStream_t)stream;
  const unsigned short* Wn = (const unsigned short*)Wn_bf16;
  const int n_g = n_img * (H / 2) * (W / 2), Wo = W / 2;
  const dim3 g128(es_cdiv(n_g, 128), Cx / 128), g32(es_cdiv(n_g, 128), Cx / 32);
  if (Cx % 128 == 0 && gh)
    hipLaunchKernelGGL((k_img_dgrad1_s2<128, true>), g128, dim3(256), 0, st, G, ldg, Wn, n_g, Cg, Wo, dX, ldx, accumulate);
  else if (Cx % 128 == 0)
    hipLaunchKernelGGL((k_img_dgrad1_s2<128>), g128, dim3(256), 0, st, G, ldg, Wn, n_g, Cg, Wo, dX, ldx, accumulate);
  else if (gh)
    hipLaunchKernelGGL((k_img_dgrad1_s2<32, true>), g32, dim3(256), 0, st, G, ldg, Wn, n_g, Cg, Wo, dX, ldx, accumulate);
  else
    hipLaunchKernelGGL((k_img_dgrad1_s2<32>), g32, dim3(256), 0, st, G, ldg, Wn, n_g, Cg, Wo, dX, ldx, accumulate);
  ES_CHECK_LAUNCH();
  return 0;
}
