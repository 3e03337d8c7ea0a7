// Grounding-transformer kernels (BASELINE config 4): multi-head attention forward / backward on the
// matrix cores, LayerNorm (+ residual), ReLU, the contrastive text-visual logits and the 9-DoF "baseline" box coder.
//
// Replaces, for embodiedscan/models/layers/ground_transformer/decoder.py:103-179,224-297:
//   mmcv MultiheadAttention -> torch.nn.MultiheadAttention (scaled dot-product core)   -> es_attn_fwd / es_attn_bwd
//   nn.LayerNorm (+ the residual add of mmcv's MultiheadAttention / FFN wrappers)       -> es_layernorm_fwd / _bwd
//   ContrastiveEmbed (dense_heads/grounding_head.py:20-99)                              -> es_contrastive_fwd / _bwd
//   GroundingHead._bbox_pred_to_bbox, box_coder='baseline', 9 outputs (:267-296)        -> es_ground_decode_fwd / _bwd
// The projections (in_proj / out_proj / FFN / reg branch) are row GEMMs on the convolution engine (K = 1).
//
// Attention: head_dim is fixed to 32 (embed 256 / 8 heads, configs/grounding/...py:48-61) = exactly the reduction depth
// of one v_mfma_f32_16x16x32_bf16, so a 16x16 score tile is ONE matrix instruction.  A workgroup (4 waves) owns 64 query
// rows (forward, dQ) or 64 key rows (dK / dV) of one (sample, head); operand tiles are staged k-contiguous in LDS, every
// GEMM of the forward and backward pass (QK^T, PV, dO V^T, dS K, P^T dO, dS^T Q) is the same "16x16 tile = sum_k A[m][k]
// B[n][k]" primitive.  Online softmax in f32; probabilities are rounded to bf16 only as MFMA operands.  BF = false
// selects the exact-f32 matrix instruction (v_mfma_f32_16x16x4_f32) for the f32 parity mode.  Keys are masked by a
// per-sample valid length (the reference's key_padding_mask is always a prefix mask: padded texts / padded point sets).
#include "common.h"
#include "../../include/es_hip.h"
extern int ES_OPT_ELECT_SAFE;           // rowops.hip (es_set_option key 18): fenced last-workgroup elections

typedef __bf16 tbf16x8_t __attribute__((ext_vector_type(8)));
typedef float tf32x4_t __attribute__((ext_vector_type(4)));

#define AT_D 32          // head dim
#define AT_R 64          // rows owned by a workgroup
#define AT_S 32          // rows of the streamed operand per step

template <bool BF> struct AtT;
template <> struct AtT<true> { typedef unsigned short T; static constexpr int LD = 40; };
template <> struct AtT<false> { typedef float T; static constexpr int LD = 33; };

__device__ inline unsigned short f2bf(float f) {          // round to nearest even
  unsigned int u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
template <bool BF> __device__ inline typename AtT<BF>::T at_cvt(float f);
template <> __device__ inline unsigned short at_cvt<true>(float f) { return f2bf(f); }
template <> __device__ inline float at_cvt<false>(float f) { return f; }

// acc (16x16, D layout: row = kq*4 + r, col = li) += sum_{k<32} A[li][k] * B[li][k]; arow / brow point at row li of the
// 16-row A / B sub-tiles (k-contiguous)
template <bool BF>
__device__ inline tf32x4_t tile_mma(const typename AtT<BF>::T* arow, const typename AtT<BF>::T* brow, int kq, tf32x4_t acc) {
  if constexpr (BF) {
    tbf16x8_t a = *(const tbf16x8_t*)(arow + kq * 8);
    tbf16x8_t b = *(const tbf16x8_t*)(brow + kq * 8);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
  } else {
#pragma unroll
    for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[4 * s + kq], brow[4 * s + kq], acc, 0, 0, 0);
    return acc;
  }
}

// stage `rows` x 32 floats (global rows r0.., leading dim ld, column offset applied by the caller) into LDS [rows][LD],
// rows >= n_valid zero-filled, values multiplied by `mul`
template <bool BF>
__device__ inline void stage_rows(typename AtT<BF>::T* dst, const float* __restrict__ src, int ld, int r0, int n_valid,
                                  int rows, float mul) {
  constexpr int LD = AtT<BF>::LD;
  for (int e = threadIdx.x; e < rows * 8; e += 256) {
    int r = e >> 3, c = (e & 7) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < n_valid) v = *(const float4*)(src + (size_t)(r0 + r) * ld + c);
    typename AtT<BF>::T* d = dst + r * LD + c;
    d[0] = at_cvt<BF>(v.x * mul); d[1] = at_cvt<BF>(v.y * mul); d[2] = at_cvt<BF>(v.z * mul); d[3] = at_cvt<BF>(v.w * mul);
  }
}
// the same tile transposed: dst [32][LD] with dst[c][r] = src[r0 + r][c]   (rows <= 32)
template <bool BF>
__device__ inline void stage_rows_t(typename AtT<BF>::T* dst, const float* __restrict__ src, int ld, int r0, int n_valid,
                                    int rows, float mul) {
  constexpr int LD = AtT<BF>::LD;
  for (int e = threadIdx.x; e < rows * 8; e += 256) {
    int r = e >> 3, c = (e & 7) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < n_valid) v = *(const float4*)(src + (size_t)(r0 + r) * ld + c);
    dst[(c + 0) * LD + r] = at_cvt<BF>(v.x * mul);
    dst[(c + 1) * LD + r] = at_cvt<BF>(v.y * mul);
    dst[(c + 2) * LD + r] = at_cvt<BF>(v.z * mul);
    dst[(c + 3) * LD + r] = at_cvt<BF>(v.w * mul);
  }
}

__device__ inline float group16_max(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------ forward
// grid (ceil(Lq/64), H, B).  Q/K/V/O: row (b*L + i), columns h*32.. of matrices with leading dims ldq/ldk/ldv/ldo.
template <bool BF>
__global__ __launch_bounds__(256) void k_attn_fwd(const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk,
                                                  const float* __restrict__ V, int ldv, int Lq, int Lk,
                                                  const int* __restrict__ klen, float scale, float* __restrict__ O, int ldo,
                                                  float* __restrict__ lse, int H) {
  typedef typename AtT<BF>::T T;
  constexpr int LD = AtT<BF>::LD;
  __shared__ __attribute__((aligned(16))) T Qs[AT_R * LD], Ks[AT_S * LD], Vt[AT_D * LD], Ps[AT_R * LD];
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * AT_R;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
  const int kvalid = klen ? min(klen[b], Lk) : Lk;
  const float* Qb = Q + (size_t)b * Lq * ldq + h * AT_D;
  const float* Kb = K + (size_t)b * Lk * ldk + h * AT_D;
  const float* Vb = V + (size_t)b * Lk * ldv + h * AT_D;
  stage_rows<BF>(Qs, Qb, ldq, q0, Lq, AT_R, scale);
  float m[4], l[4];
  tf32x4_t o[2];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; }
  o[0] = o[1] = (tf32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kvalid; k0 += AT_S) {
    __syncthreads();                                   // previous step's readers of Ks / Vt / Ps are done (and Qs is staged)
    stage_rows<BF>(Ks, Kb, ldk, k0, kvalid, AT_S, 1.f);
    stage_rows_t<BF>(Vt, Vb, ldv, k0, kvalid, AT_S, 1.f);
    __syncthreads();
    tf32x4_t s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = (tf32x4_t){0.f, 0.f, 0.f, 0.f};
      s[t] = tile_mma<BF>(Qs + (wv * 16 + li) * LD, Ks + (t * 16 + li) * LD, kq, s[t]);
    }
    const bool ok0 = (k0 + li) < kvalid, ok1 = (k0 + 16 + li) < kvalid;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s0 = ok0 ? s[0][r] : -INFINITY, s1 = ok1 ? s[1][r] : -INFINITY;
      float mx = group16_max(fmaxf(s0, s1));
      float mn = fmaxf(m[r], mx);                      // finite: every step has at least one valid key (a sample WITHOUT a step: below)
      float corr = __expf(m[r] - mn);
      float p0 = __expf(s0 - mn), p1 = __expf(s1 - mn);
      l[r] = l[r] * corr + group16_sum(p0 + p1);
      m[r] = mn;
      o[0][r] *= corr;
      o[1][r] *= corr;
      T* prow = Ps + (wv * 16 + kq * 4 + r) * LD;
      prow[li] = at_cvt<BF>(p0);
      prow[16 + li] = at_cvt<BF>(p1);
    }
    __syncthreads();
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) o[nf] = tile_mma<BF>(Ps + (wv * 16 + li) * LD, Vt + (nf * 16 + li) * LD, kq, o[nf]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int q = q0 + wv * 16 + kq * 4 + r;
    if (q >= Lq) continue;
    // A sample without a valid key (klen[b] <= 0) never entered the loop: l = 0, o = 0, m = -inf.  It gets O = 0 and lse = -inf.
    // Deliberate divergence: the reference's softmax over a fully masked row is NaN there (grounding section).  The
    // backward kernels skip their key loops for such a sample as well (kvalid <= 0; lse is never read) and write exact zeros.
    const bool any = l[r] > 0.f;
    float inv = any ? 1.f / l[r] : 0.f;
    float* orow = O + ((size_t)b * Lq + q) * ldo + h * AT_D;
    orow[li] = o[0][r] * inv;
    orow[16 + li] = o[1][r] * inv;
    if (li == 0) lse[((size_t)b * H + h) * Lq + q] = any ? m[r] + __logf(l[r]) : -INFINITY;
  }
}

// delta[b,h,q] = sum_d dO[q, h*32 + d] * O[q, h*32 + d]
__global__ void k_attn_delta(const float* __restrict__ O, int ldo, const float* __restrict__ dO, int ldd, int B, int H, int Lq,
                             float* __restrict__ delta) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * H * Lq) return;
  int q = (int)(i % Lq), h = (int)((i / Lq) % H), b = (int)(i / ((long long)Lq * H));
  const float* o = O + ((size_t)b * Lq + q) * ldo + h * AT_D;
  const float* g = dO + ((size_t)b * Lq + q) * ldd + h * AT_D;
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < AT_D; d += 4) {
    float4 a = *(const float4*)(o + d), c = *(const float4*)(g + d);
    s += a.x * c.x + a.y * c.y + a.z * c.z + a.w * c.w;
  }
  delta[i] = s;
}

// ------------------------------------------------------------------ backward: dQ
template <bool BF>
__global__ __launch_bounds__(256) void k_attn_bwd_dq(const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk,
                                                     const float* __restrict__ V, int ldv, const float* __restrict__ dO, int ldd,
                                                     const float* __restrict__ lse, const float* __restrict__ delta, int Lq,
                                                     int Lk, const int* __restrict__ klen, float scale, float* __restrict__ dQ,
                                                     int ldg, int accumulate, int H) {
  typedef typename AtT<BF>::T T;
  constexpr int LD = AtT<BF>::LD;
  __shared__ __attribute__((aligned(16))) T Qs[AT_R * LD], dOs[AT_R * LD], Ks[AT_S * LD], Vs[AT_S * LD], Kt[AT_D * LD], dSs[AT_R * LD];
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * AT_R;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
  const int kvalid = klen ? min(klen[b], Lk) : Lk;
  const float* Kb = K + (size_t)b * Lk * ldk + h * AT_D;
  const float* Vb = V + (size_t)b * Lk * ldv + h * AT_D;
  stage_rows<BF>(Qs, Q + (size_t)b * Lq * ldq + h * AT_D, ldq, q0, Lq, AT_R, scale);
  stage_rows<BF>(dOs, dO + (size_t)b * Lq * ldd + h * AT_D, ldd, q0, Lq, AT_R, 1.f);
  float ls[4], dl[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int q = q0 + wv * 16 + kq * 4 + r;
    bool in = q < Lq;
    ls[r] = in ? lse[((size_t)b * H + h) * Lq + q] : 0.f;
    dl[r] = in ? delta[((size_t)b * H + h) * Lq + q] : 0.f;
  }
  tf32x4_t dq[2];
  dq[0] = dq[1] = (tf32x4_t){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kvalid; k0 += AT_S) {
    __syncthreads();
    stage_rows<BF>(Ks, Kb, ldk, k0, kvalid, AT_S, 1.f);
    stage_rows<BF>(Vs, Vb, ldv, k0, kvalid, AT_S, 1.f);
    stage_rows_t<BF>(Kt, Kb, ldk, k0, kvalid, AT_S, 1.f);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      tf32x4_t s = (tf32x4_t){0.f, 0.f, 0.f, 0.f}, dp = s;
      s = tile_mma<BF>(Qs + (wv * 16 + li) * LD, Ks + (t * 16 + li) * LD, kq, s);
      dp = tile_mma<BF>(dOs + (wv * 16 + li) * LD, Vs + (t * 16 + li) * LD, kq, dp);
      const bool ok = (k0 + t * 16 + li) < kvalid;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = ok ? __expf(s[r] - ls[r]) : 0.f;
        dSs[(wv * 16 + kq * 4 + r) * LD + t * 16 + li] = at_cvt<BF>(p * (dp[r] - dl[r]));
      }
    }
    __syncthreads();
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) dq[nf] = tile_mma<BF>(dSs + (wv * 16 + li) * LD, Kt + (nf * 16 + li) * LD, kq, dq[nf]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int q = q0 + wv * 16 + kq * 4 + r;
    if (q >= Lq) continue;
    float* g = dQ + ((size_t)b * Lq + q) * ldg + h * AT_D;
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      float v = dq[nf][r] * scale;
      g[nf * 16 + li] = accumulate ? g[nf * 16 + li] + v : v;
    }
  }
}

// ------------------------------------------------------------------ backward: dK, dV   (grid (ceil(Lk/64), H, B))
template <bool BF>
__global__ __launch_bounds__(256) void k_attn_bwd_dkv(const float* __restrict__ Q, int ldq, const float* __restrict__ K, int ldk,
                                                      const float* __restrict__ V, int ldv, const float* __restrict__ dO,
                                                      int ldd, const float* __restrict__ lse, const float* __restrict__ delta,
                                                      int Lq, int Lk, const int* __restrict__ klen, float scale,
                                                      float* __restrict__ dK, int ldgk, float* __restrict__ dV, int ldgv,
                                                      int accumulate, int H) {
  typedef typename AtT<BF>::T T;
  constexpr int LD = AtT<BF>::LD;
  __shared__ __attribute__((aligned(16))) T Ks[AT_R * LD], Vs[AT_R * LD], Qs[AT_S * LD], dOs[AT_S * LD], Qt[AT_D * LD], dOt[AT_D * LD],
      PTs[AT_R * LD], dSTs[AT_R * LD];
  __shared__ float lseS[AT_S], delS[AT_S];
  const int b = blockIdx.z, h = blockIdx.y, kbase = blockIdx.x * AT_R;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
  const int kvalid = klen ? min(klen[b], Lk) : Lk;
  const float* Qb = Q + (size_t)b * Lq * ldq + h * AT_D;
  const float* dOb = dO + (size_t)b * Lq * ldd + h * AT_D;
  tf32x4_t dk[2], dv[2];
  dk[0] = dk[1] = dv[0] = dv[1] = (tf32x4_t){0.f, 0.f, 0.f, 0.f};
  if (kbase < kvalid) {                                 // workgroup-uniform: tiles made of padding only skip the loop
    stage_rows<BF>(Ks, K + (size_t)b * Lk * ldk + h * AT_D, ldk, kbase, kvalid, AT_R, 1.f);
    stage_rows<BF>(Vs, V + (size_t)b * Lk * ldv + h * AT_D, ldv, kbase, kvalid, AT_R, 1.f);
    for (int q0 = 0; q0 < Lq; q0 += AT_S) {
      __syncthreads();
      stage_rows<BF>(Qs, Qb, ldq, q0, Lq, AT_S, scale);
      stage_rows<BF>(dOs, dOb, ldd, q0, Lq, AT_S, 1.f);
      stage_rows_t<BF>(Qt, Qb, ldq, q0, Lq, AT_S, scale);
      stage_rows_t<BF>(dOt, dOb, ldd, q0, Lq, AT_S, 1.f);
      if (threadIdx.x < AT_S) {
        int q = q0 + threadIdx.x;
        lseS[threadIdx.x] = q < Lq ? lse[((size_t)b * H + h) * Lq + q] : INFINITY;        // exp(s - inf) = 0 for padding rows
        delS[threadIdx.x] = q < Lq ? delta[((size_t)b * H + h) * Lq + q] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 2; ++t) {                      // S^T / dP^T tiles: rows = this wave's 16 keys, cols = 16 queries
        tf32x4_t st = (tf32x4_t){0.f, 0.f, 0.f, 0.f}, dpt = st;
        st = tile_mma<BF>(Ks + (wv * 16 + li) * LD, Qs + (t * 16 + li) * LD, kq, st);
        dpt = tile_mma<BF>(Vs + (wv * 16 + li) * LD, dOs + (t * 16 + li) * LD, kq, dpt);
        const float lq = lseS[t * 16 + li], dq_ = delS[t * 16 + li];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          bool ok = (kbase + wv * 16 + kq * 4 + r) < kvalid;
          float p = ok ? __expf(st[r] - lq) : 0.f;
          PTs[(wv * 16 + kq * 4 + r) * LD + t * 16 + li] = at_cvt<BF>(p);
          dSTs[(wv * 16 + kq * 4 + r) * LD + t * 16 + li] = at_cvt<BF>(p * (dpt[r] - dq_));
        }
      }
      __syncthreads();
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        dv[nf] = tile_mma<BF>(PTs + (wv * 16 + li) * LD, dOt + (nf * 16 + li) * LD, kq, dv[nf]);
        dk[nf] = tile_mma<BF>(dSTs + (wv * 16 + li) * LD, Qt + (nf * 16 + li) * LD, kq, dk[nf]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int k = kbase + wv * 16 + kq * 4 + r;
    if (k >= Lk) continue;                               // padded keys (k >= kvalid) get exact zeros
    float* gk = dK + ((size_t)b * Lk + k) * ldgk + h * AT_D;
    float* gv = dV + ((size_t)b * Lk + k) * ldgv + h * AT_D;
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      gk[nf * 16 + li] = accumulate ? gk[nf * 16 + li] + dk[nf][r] : dk[nf][r];     // Qs / Qt already carry `scale`
      gv[nf * 16 + li] = accumulate ? gv[nf * 16 + li] + dv[nf][r] : dv[nf][r];
    }
  }
}

extern "C" int es_attn_fwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, int B, int H, int Lq,
                           int Lk, const int* klen_dev, float* O, int ldo, float* lse, int bf16, void* stream) {
  if (B <= 0 || Lq <= 0 || Lk <= 0) return 0;
  if ((ldq | ldk | ldv | ldo) & 3) return -3;
  dim3 grid(es_cdiv(Lq, AT_R), H, B);
  const float scale = 0.17677669529663687f;              // 1 / sqrt(32)
  if (bf16)
    hipLaunchKernelGGL(k_attn_fwd<true>, grid, dim3(256), 0, (hipStream_t)stream, Q, ldq, K, ldk, V, ldv, Lq, Lk, klen_dev,
                       scale, O, ldo, lse, H);
  else
    hipLaunchKernelGGL(k_attn_fwd<false>, grid, dim3(256), 0, (hipStream_t)stream, Q, ldq, K, ldk, V, ldv, Lq, Lk, klen_dev,
                       scale, O, ldo, lse, H);
  ES_CHECK_LAUNCH();
  return 0;
}

extern "C" int es_attn_bwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo,
                           const float* dO, int ldd, const float* lse, int B, int H, int Lq, int Lk, const int* klen_dev,
                           float* delta_scratch, float* dQ, int ldgq, float* dK, int ldgk, float* dV, int ldgv, int accumulate,
                           int bf16, void* stream) {
  if (B <= 0 || Lq <= 0 || Lk <= 0) return 0;
  if ((ldq | ldk | ldv | ldo | ldd | ldgq | ldgk | ldgv) & 3) return -3;
  hipStream_t st = (hipStream_t)stream;
  const float scale = 0.17677669529663687f;
  hipLaunchKernelGGL(k_attn_delta, dim3(es_cdiv((long long)B * H * Lq, 256)), dim3(256), 0, st, O, ldo, dO, ldd, B, H, Lq,
                     delta_scratch);
  dim3 gq(es_cdiv(Lq, AT_R), H, B), gk(es_cdiv(Lk, AT_R), H, B);
  if (bf16) {
    hipLaunchKernelGGL(k_attn_bwd_dq<true>, gq, dim3(256), 0, st, Q, ldq, K, ldk, V, ldv, dO, ldd, lse, delta_scratch, Lq, Lk,
                       klen_dev, scale, dQ, ldgq, accumulate, H);
    hipLaunchKernelGGL(k_attn_bwd_dkv<true>, gk, dim3(256), 0, st, Q, ldq, K, ldk, V, ldv, dO, ldd, lse, delta_scratch, Lq, Lk,
                       klen_dev, scale, dK, ldgk, dV, ldgv, accumulate, H);
  } else {
    hipLaunchKernelGGL(k_attn_bwd_dq<false>, gq, dim3(256), 0, st, Q, ldq, K, ldk, V, ldv, dO, ldd, lse, delta_scratch, Lq, Lk,
                       klen_dev, scale, dQ, ldgq, accumulate, H);
    hipLaunchKernelGGL(k_attn_bwd_dkv<false>, gk, dim3(256), 0, st, Q, ldq, K, ldk, V, ldv, dO, ldd, lse, delta_scratch, Lq, Lk,
                       klen_dev, scale, dK, ldgk, dV, ldgv, accumulate, H);
  }
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ attention over ONE prepared key / value set
// (SparseFeatureFusion3DGrounder.ground: the queries of many prompts over the point tokens of one scene.)  k_attn_fwd stages,
// converts and transposes every K / V tile once per 64 query rows; here that work is done once per (scene, layer) by
// es_attn_kv_prepare and the forward kernel copies finished tiles.
//
// Operand layout of `kv` (element type: bf16 in bf16 mode, f32 in the parity mode; nt = ceil(Lk / 64) key tiles):
//   block (h, j) at element ((h * nt + j) * 4096), 4096 = 2 * 64 * 32 elements:
//     [   0, 2048)  K tile, k-contiguous:  element key * 32 + d        = K[j * 64 + key][h * 32 + d]
//     [2048, 4096)  V tile, TRANSPOSED:    element 2048 + d * 64 + key = V[j * 64 + key][h * 32 + d]
//   keys >= Lk are exact zeros (the forward masks their scores; zero keeps 0 * p finite in the PV product).
// One block is one contiguous run of 16-byte pieces: the forward kernel stages it with two (bf16) / four (f32) 16-byte loads per
// thread, issued BEFORE the products of the current tile and written to LDS after them (loads in flight under the MFMAs).
// A workgroup owns 128 query rows of one head (wave w: rows 32 w .. 32 w + 31 as two 16-row tiles; the Q fragments live in
// registers for the whole key loop), a step is 64 keys: 16 matrix instructions per wave between barriers instead of 4.
// Rounding points as in k_attn_fwd: f32(q * scale) -> operand type, K / V once (in prepare), online softmax in f32, unnormalised
// probabilities -> operand type as MFMA operands only.
#define AK_S 64                         // keys per tile
#define AK_R 128                        // query rows per workgroup
#define AK_TILE (2 * AK_S * AT_D)       // elements of one (head, tile) block

template <bool BF> struct AkT;
template <> struct AkT<true> { typedef unsigned short T; static constexpr int LDK = 40, LDV = 72, EPP = 8; };
template <> struct AkT<false> { typedef float T; static constexpr int LDK = 36, LDV = 68, EPP = 4; };

// grid (nt, H)
template <bool BF>
__global__ __launch_bounds__(256) void k_attn_kv_prepare(const float* __restrict__ K, int ldk, const float* __restrict__ V, int ldv,
                                                         int Lk, typename AkT<BF>::T* __restrict__ kv) {
  const int j = blockIdx.x, h = blockIdx.y;
  typename AkT<BF>::T* dst = kv + ((size_t)h * gridDim.x + j) * AK_TILE;
  for (int e = threadIdx.x; e < AK_TILE; e += 256) {
    int key, d;
    const float* src;
    int ld;
    if (e < AK_S * AT_D) { key = e >> 5; d = e & 31; src = K; ld = ldk; }
    else { d = (e - AK_S * AT_D) >> 6; key = e & 63; src = V; ld = ldv; }
    const int kg = j * AK_S + key;
    dst[e] = at_cvt<BF>(kg < Lk ? src[(size_t)kg * ld + h * AT_D + d] : 0.f);
  }
}

// the 16-byte pieces of block j that this thread stages: global -> registers ...
template <bool BF>
__device__ inline void ak_load(tf32x4_t (&pre)[AK_TILE / AkT<BF>::EPP / 256], const typename AkT<BF>::T* __restrict__ src, int j) {
  const tf32x4_t* s4 = (const tf32x4_t*)(src + (size_t)j * AK_TILE);
#pragma unroll
  for (int u = 0; u < AK_TILE / AkT<BF>::EPP / 256; ++u) pre[u] = s4[u * 256 + threadIdx.x];
}
// ... registers -> the padded LDS images Ks [64][LDK], Vt [32][LDV]
template <bool BF>
__device__ inline void ak_store(const tf32x4_t (&pre)[AK_TILE / AkT<BF>::EPP / 256], typename AkT<BF>::T* Ks, typename AkT<BF>::T* Vt) {
  constexpr int LDK = AkT<BF>::LDK, LDV = AkT<BF>::LDV, EPP = AkT<BF>::EPP;
#pragma unroll
  for (int u = 0; u < AK_TILE / EPP / 256; ++u) {
    const int e = (u * 256 + threadIdx.x) * EPP;
    // (block-uniform per u: pieces u * 256 .. u * 256 + 255 lie on one side of the K / V^T boundary)
    typename AkT<BF>::T* d;
    if (u * 256 * EPP < AK_S * AT_D) d = Ks + (e >> 5) * LDK + (e & 31);
    else d = Vt + ((e - AK_S * AT_D) >> 6) * LDV + (e & 63);
    *(tf32x4_t*)d = pre[u];                              // 16 bytes: LDK, LDV and the column are multiples of 8 bf16 / 4 f32
  }
}

// acc (16x16) += sum_{k<32} A[li][k] B[li][k] with lane (li, kq) supplying k = 8 kq .. 8 kq + 7 of both rows in BOTH modes (the exact-f32
// instruction sums four lanes' k per step: any assignment of k to (step, lane quarter) is a valid one as long as A and B agree), so a
// lane's operands are 16 (bf16) / 32 (f32) contiguous bytes of LDS, read as one / two 16-byte loads
template <bool BF>
__device__ inline tf32x4_t ak_mma(const typename AkT<BF>::T* arow, const typename AkT<BF>::T* brow, int kq, tf32x4_t acc) {
  if constexpr (BF) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const tbf16x8_t*)(arow + kq * 8), *(const tbf16x8_t*)(brow + kq * 8), acc, 0, 0, 0);
  } else {
    const tf32x4_t a0 = *(const tf32x4_t*)(arow + kq * 8), a1 = *(const tf32x4_t*)(arow + kq * 8 + 4);
    const tf32x4_t b0 = *(const tf32x4_t*)(brow + kq * 8), b1 = *(const tf32x4_t*)(brow + kq * 8 + 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[c], b0[c], acc, 0, 0, 0);
#pragma unroll
    for (int c = 0; c < 4; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[c], b1[c], acc, 0, 0, 0);
    return acc;
  }
}

// grid (ceil(Lq / 128), H).  Q / O: row i, columns h*32.. of matrices with leading dims ldq / ldo; lse (H, Lq).
template <bool BF>
__global__ __launch_bounds__(256) void k_attn_kv_fwd(const float* __restrict__ Q, int ldq, const typename AkT<BF>::T* __restrict__ kv,
                                                     int Lq, int Lk, float scale, float* __restrict__ O, int ldo,
                                                     float* __restrict__ lse) {
  typedef typename AkT<BF>::T T;
  constexpr int LDK = AkT<BF>::LDK, LDV = AkT<BF>::LDV;
  __shared__ __attribute__((aligned(16))) T Ks[AK_S * LDK], Vt[AT_D * LDV], Ps[AK_R * LDV];
  const int h = blockIdx.y, q0 = blockIdx.x * AK_R;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
  const int nt = (Lk + AK_S - 1) / AK_S;
  const T* src = kv + (size_t)h * nt * AK_TILE;
  // the A fragments of this wave's two query tiles: lane (li, kq) holds row li, k = 8 kq + j (see ak_mma)
  typedef short ts16x8_t __attribute__((ext_vector_type(8)));
  tbf16x8_t qv[2];
  ts16x8_t qb[2] = {};
  float qs[2][8];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int q = q0 + wv * 32 + qt * 16 + li;
    const float* qr = Q + (size_t)(q < Lq ? q : 0) * ldq + h * AT_D;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = q < Lq ? qr[kq * 8 + j] * scale : 0.f;
      if constexpr (BF) qb[qt][j] = (short)f2bf(x);
      else qs[qt][j] = x;
    }
    qv[qt] = __builtin_bit_cast(tbf16x8_t, qb[qt]);
  }
  float m[2][4], l[2][4];
  tf32x4_t o[2][2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[qt][r] = -INFINITY; l[qt][r] = 0.f; }
    o[qt][0] = o[qt][1] = (tf32x4_t){0.f, 0.f, 0.f, 0.f};
  }
  tf32x4_t pre[AK_TILE / AkT<BF>::EPP / 256];
  ak_load<BF>(pre, src, 0);
  for (int j = 0; j < nt; ++j) {
    const int k0 = j * AK_S;
    __syncthreads();                                   // the previous step's readers of Ks / Vt / Ps are done
    ak_store<BF>(pre, Ks, Vt);
    if (j + 1 < nt) ak_load<BF>(pre, src, j + 1);      // in flight under this step's products
    __syncthreads();
    tf32x4_t s[2][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const T* brow = Ks + (t * 16 + li) * LDK;
      s[0][t] = s[1][t] = (tf32x4_t){0.f, 0.f, 0.f, 0.f};
      if constexpr (BF) {
        const tbf16x8_t b = *(const tbf16x8_t*)(brow + kq * 8);
        s[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qv[0], b, s[0][t], 0, 0, 0);
        s[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qv[1], b, s[1][t], 0, 0, 0);
      } else {
        const tf32x4_t b0 = *(const tf32x4_t*)(brow + kq * 8), b1 = *(const tf32x4_t*)(brow + kq * 8 + 4);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const float b = c < 4 ? b0[c & 3] : b1[c & 3];
          s[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(qs[0][c], b, s[0][t], 0, 0, 0);
          s[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(qs[1][c], b, s[1][t], 0, 0, 0);
        }
      }
    }
    bool ok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) ok[t] = (k0 + t * 16 + li) < Lk;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) sv[t] = ok[t] ? s[qt][t][r] : -INFINITY;
        const float mx = group16_max(fmaxf(fmaxf(sv[0], sv[1]), fmaxf(sv[2], sv[3])));
        const float mn = fmaxf(m[qt][r], mx);          // finite: every tile holds at least one key < Lk
        const float corr = __expf(m[qt][r] - mn);
        float p[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) p[t] = __expf(sv[t] - mn);
        l[qt][r] = l[qt][r] * corr + group16_sum((p[0] + p[1]) + (p[2] + p[3]));
        m[qt][r] = mn;
        o[qt][0][r] *= corr;
        o[qt][1][r] *= corr;
        T* prow = Ps + (wv * 32 + qt * 16 + kq * 4 + r) * LDV;
#pragma unroll
        for (int t = 0; t < 4; ++t) prow[t * 16 + li] = at_cvt<BF>(p[t]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int nf = 0; nf < 2; ++nf)
#pragma unroll
        for (int c = 0; c < 2; ++c)
          o[qt][nf] = ak_mma<BF>(Ps + (wv * 32 + qt * 16 + li) * LDV + c * 32, Vt + (nf * 16 + li) * LDV + c * 32, kq, o[qt][nf]);
  }
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + wv * 32 + qt * 16 + kq * 4 + r;
      if (q >= Lq) continue;
      const bool any = l[qt][r] > 0.f;
      const float inv = any ? 1.f / l[qt][r] : 0.f;
      float* orow = O + (size_t)q * ldo + h * AT_D;
      orow[li] = o[qt][0][r] * inv;
      orow[16 + li] = o[qt][1][r] * inv;
      if (li == 0) lse[(size_t)h * Lq + q] = any ? m[qt][r] + __logf(l[qt][r]) : -INFINITY;
    }
  }
}

extern "C" size_t es_attn_kv_bytes(int H, int Lk, int bf16) {
  if (H <= 0 || Lk <= 0) return 0;
  return (size_t)H * es_cdiv(Lk, AK_S) * AK_TILE * (bf16 ? 2 : 4);
}
extern "C" int es_attn_kv_prepare(const float* K, int ldk, const float* V, int ldv, int H, int Lk, int bf16, void* kv, void* stream) {
  if (H <= 0 || Lk <= 0) return 0;
  if ((ldk | ldv) & 3) return -3;
  dim3 grid(es_cdiv(Lk, AK_S), H);
  if (bf16)
    hipLaunchKernelGGL(k_attn_kv_prepare<true>, grid, dim3(256), 0, (hipStream_t)stream, K, ldk, V, ldv, Lk, (unsigned short*)kv);
  else
    hipLaunchKernelGGL(k_attn_kv_prepare<false>, grid, dim3(256), 0, (hipStream_t)stream, K, ldk, V, ldv, Lk, (float*)kv);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_attn_kv_fwd(const float* Q, int ldq, const void* kv, int H, int Lq, int Lk, float* O, int ldo, float* lse, int bf16,
                              void* stream) {
  if (H <= 0 || Lq <= 0 || Lk <= 0) return 0;
  if ((ldq | ldo) & 3) return -3;
  dim3 grid(es_cdiv(Lq, AK_R), H);
  const float scale = 0.17677669529663687f;              // 1 / sqrt(32)
  if (bf16)
    hipLaunchKernelGGL(k_attn_kv_fwd<true>, grid, dim3(256), 0, (hipStream_t)stream, Q, ldq, (const unsigned short*)kv, Lq, Lk, scale,
                       O, ldo, lse);
  else
    hipLaunchKernelGGL(k_attn_kv_fwd<false>, grid, dim3(256), 0, (hipStream_t)stream, Q, ldq, (const float*)kv, Lq, Lk, scale, O, ldo,
                       lse);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ backward of es_attn_kv_fwd: many query rows, one key / value set
// The shape is the mirror image of the forward: Lq = P * Q is the long axis (3 072 rows at 12 prompts), there is one key set.
// k_attn_bwd_dkv re-stages Q and dO from f32 -- converted, and scattered into LDS a second time transposed -- every 32 query rows in
// each of its ceil(Lk / 64) * H workgroups, for 8 matrix instructions per wave.  Here the QUERY side is treated the way the forward treats
// the key side: k_attn_kv_bwd_prep converts Q * scale and dO ONCE per call into finished tiles, in both orientations the products
// consume; k_attn_kv_bwd_dkv keeps its 64 keys' K / V tile resident in LDS and streams those tiles with 16-byte copies, 64 query rows a
// step in bf16 mode: 16 matrix instructions per wave between the same three barriers, no conversion in the loop.
// Workspace layout (element type as the mode; nq = ceil(Lq / QS) query steps, QS = 64 in bf16 / 32 in f32 mode -- the parity mode
// keeps the 32-row step so that its f32 tiles stay inside the 64 KiB of static LDS):
//   block (h, j) at element (h * nq + j) * 4 * QS * 32:  [Qn QS x 32][dOn QS x 32][Qt 32 x QS][dOt 32 x QS]
//   Qn[r][d] = cvt(f32(Q[j QS + r][h 32 + d] * scale)), dOn likewise without the scale, Qt / dOt their transposes; rows >= Lq are zeros.
// dK / dV are deterministic: a (key tile, head) is owned by one workgroup that walks the query steps in ascending order.  dQ is
// k_attn_bwd_dq with one sample: its workgroups own the query rows already, what they stream is the one key set.
// Rounding points are those of es_attn_bwd: operands -> operand type, probabilities recomputed from lse in f32, f32 accumulation.
template <bool BF> struct AbT;
template <> struct AbT<true> { static constexpr int QS = 64, LDT = 72, EPP = 8; };
template <> struct AbT<false> { static constexpr int QS = 32, LDT = 33, EPP = 4; };

template <bool BF>
__global__ __launch_bounds__(256) void k_attn_kv_bwd_prep(const float* __restrict__ Q, int ldq, const float* __restrict__ dO, int ldd,
                                                          int Lq, float scale, typename AtT<BF>::T* __restrict__ ws) {
  typedef typename AtT<BF>::T T;
  constexpr int QS = AbT<BF>::QS;
  const int j = blockIdx.x, h = blockIdx.y, nq = gridDim.x;
  T* blk = ws + ((size_t)h * nq + j) * (4 * QS * AT_D);
  T *Qn = blk, *dOn = blk + QS * AT_D, *Qt = blk + 2 * QS * AT_D, *dOt = blk + 3 * QS * AT_D;
  for (int e = threadIdx.x; e < QS * 8; e += 256) {
    const int r = e >> 3, c = (e & 7) * 4, q = j * QS + r;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), g = a;
    if (q < Lq) {
      a = *(const float4*)(Q + (size_t)q * ldq + h * AT_D + c);
      g = *(const float4*)(dO + (size_t)q * ldd + h * AT_D + c);
    }
    const float av[4] = {a.x * scale, a.y * scale, a.z * scale, a.w * scale}, gv[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const T qa = at_cvt<BF>(av[i]), ga = at_cvt<BF>(gv[i]);
      Qn[r * AT_D + c + i] = qa;
      dOn[r * AT_D + c + i] = ga;
      Qt[(c + i) * QS + r] = qa;
      dOt[(c + i) * QS + r] = ga;
    }
  }
}

// dst [rows][ldd] <- the dense finished tile src [rows][cols] (16-byte pieces; f32 LDS rows are not 16-byte aligned: scalar stores)
template <bool BF>
__device__ inline void copy_tile(typename AtT<BF>::T* dst, int ldd, const typename AtT<BF>::T* __restrict__ src, int rows, int cols) {
  constexpr int EPP = AbT<BF>::EPP;
  const int ppr = cols / EPP;
  for (int e = threadIdx.x; e < rows * ppr; e += 256) {
    const int r = e / ppr, c = (e - r * ppr) * EPP;
    if constexpr (BF) {
      *(uint4*)(dst + r * ldd + c) = *(const uint4*)(src + (size_t)r * cols + c);
    } else {
      const float4 v = *(const float4*)(src + (size_t)r * cols + c);
      float* d = dst + r * ldd + c;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  }
}

// grid (ceil(Lk / 64), H).  Wave w owns keys kbase + 16 w .. + 15.
template <bool BF>
__global__ __launch_bounds__(256) void k_attn_kv_bwd_dkv(const float* __restrict__ K, int ldk, const float* __restrict__ V, int ldv,
                                                         const typename AtT<BF>::T* __restrict__ ws, const float* __restrict__ lse,
                                                         const float* __restrict__ delta, int Lq, int Lk, float* __restrict__ dK,
                                                         int ldgk, float* __restrict__ dV, int ldgv, int accumulate) {
  typedef typename AtT<BF>::T T;
  constexpr int LD = AtT<BF>::LD, QS = AbT<BF>::QS, LDT = AbT<BF>::LDT;
  __shared__ __attribute__((aligned(16))) T Ks[AT_R * LD], Vs[AT_R * LD], Qs[QS * LD], dOs[QS * LD], Qt[AT_D * LDT], dOt[AT_D * LDT],
      PTs[AT_R * LDT], dSTs[AT_R * LDT];
  __shared__ float lseS[QS], delS[QS];
  const int h = blockIdx.y, kbase = blockIdx.x * AT_R;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
  const int nq = (Lq + QS - 1) / QS;
  tf32x4_t dk[2], dv[2];
  dk[0] = dk[1] = dv[0] = dv[1] = (tf32x4_t){0.f, 0.f, 0.f, 0.f};
  stage_rows<BF>(Ks, K + h * AT_D, ldk, kbase, Lk, AT_R, 1.f);          // resident for the whole query walk
  stage_rows<BF>(Vs, V + h * AT_D, ldv, kbase, Lk, AT_R, 1.f);
  for (int j = 0; j < nq; ++j) {
    const T* blk = ws + ((size_t)h * nq + j) * (4 * QS * AT_D);
    __syncthreads();                                                   // the previous step's readers are done (and Ks / Vs are staged)
    copy_tile<BF>(Qs, LD, blk, QS, AT_D);
    copy_tile<BF>(dOs, LD, blk + QS * AT_D, QS, AT_D);
    copy_tile<BF>(Qt, LDT, blk + 2 * QS * AT_D, AT_D, QS);
    copy_tile<BF>(dOt, LDT, blk + 3 * QS * AT_D, AT_D, QS);
    if (threadIdx.x < QS) {
      const int q = j * QS + threadIdx.x;
      lseS[threadIdx.x] = q < Lq ? lse[(size_t)h * Lq + q] : INFINITY;   // exp(s - inf) = 0 for padding rows
      delS[threadIdx.x] = q < Lq ? delta[(size_t)h * Lq + q] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < QS / 16; ++t) {                                // S^T / dP^T tiles: rows = this wave's 16 keys, cols = 16 queries
      tf32x4_t st = (tf32x4_t){0.f, 0.f, 0.f, 0.f}, dpt = st;
      st = tile_mma<BF>(Ks + (wv * 16 + li) * LD, Qs + (t * 16 + li) * LD, kq, st);
      dpt = tile_mma<BF>(Vs + (wv * 16 + li) * LD, dOs + (t * 16 + li) * LD, kq, dpt);
      const float lq = lseS[t * 16 + li], dq_ = delS[t * 16 + li];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = (kbase + wv * 16 + kq * 4 + r) < Lk;
        const float p = ok ? __expf(st[r] - lq) : 0.f;
        PTs[(wv * 16 + kq * 4 + r) * LDT + t * 16 + li] = at_cvt<BF>(p);
        dSTs[(wv * 16 + kq * 4 + r) * LDT + t * 16 + li] = at_cvt<BF>(p * (dpt[r] - dq_));
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < QS / 32; ++kk) {                             // reduction over the step's queries, 32 at a time, ascending
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        dv[nf] = tile_mma<BF>(PTs + (wv * 16 + li) * LDT + kk * 32, dOt + (nf * 16 + li) * LDT + kk * 32, kq, dv[nf]);
        dk[nf] = tile_mma<BF>(dSTs + (wv * 16 + li) * LDT + kk * 32, Qt + (nf * 16 + li) * LDT + kk * 32, kq, dk[nf]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = kbase + wv * 16 + kq * 4 + r;
    if (k >= Lk) continue;
    float* gk = dK + (size_t)k * ldgk + h * AT_D;
    float* gv = dV + (size_t)k * ldgv + h * AT_D;
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      gk[nf * 16 + li] = accumulate ? gk[nf * 16 + li] + dk[nf][r] : dk[nf][r];     // Qt already carries `scale`
      gv[nf * 16 + li] = accumulate ? gv[nf * 16 + li] + dv[nf][r] : dv[nf][r];
    }
  }
}

extern "C" size_t es_attn_kv_bwd_workspace_bytes(int H, int Lq, int bf16) {
  if (H <= 0 || Lq <= 0) return 0;
  const int QS = bf16 ? AbT<true>::QS : AbT<false>::QS;
  return (size_t)H * es_cdiv(Lq, QS) * 4 * QS * AT_D * (bf16 ? 2 : 4);
}
extern "C" int es_attn_kv_bwd(const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv, const float* O, int ldo,
                              const float* dO, int ldd, const float* lse, int H, int Lq, int Lk, float* delta_scratch, void* workspace,
                              size_t workspace_bytes, float* dQ, int ldgq, float* dK, int ldgk, float* dV, int ldgv, int accumulate,
                              int bf16, void* stream) {
  if (H <= 0 || Lq <= 0 || Lk <= 0) return 0;
  if ((ldq | ldk | ldv | ldo | ldd | ldgq | ldgk | ldgv) & 3) return -3;
  if (!workspace || (((uintptr_t)workspace) & 15) || workspace_bytes < es_attn_kv_bwd_workspace_bytes(H, Lq, bf16)) return -5;
  hipStream_t st = (hipStream_t)stream;
  const float scale = 0.17677669529663687f;
  hipLaunchKernelGGL(k_attn_delta, dim3(es_cdiv((long long)H * Lq, 256)), dim3(256), 0, st, O, ldo, dO, ldd, 1, H, Lq, delta_scratch);
  dim3 gq(es_cdiv(Lq, AT_R), H, 1), gk(es_cdiv(Lk, AT_R), H);
  if (bf16) {
    hipLaunchKernelGGL(k_attn_kv_bwd_prep<true>, dim3(es_cdiv(Lq, AbT<true>::QS), H), dim3(256), 0, st, Q, ldq, dO, ldd, Lq, scale,
                       (unsigned short*)workspace);
    hipLaunchKernelGGL(k_attn_bwd_dq<true>, gq, dim3(256), 0, st, Q, ldq, K, ldk, V, ldv, dO, ldd, lse, delta_scratch, Lq, Lk,
                       (const int*)nullptr, scale, dQ, ldgq, accumulate, H);
    hipLaunchKernelGGL(k_attn_kv_bwd_dkv<true>, gk, dim3(256), 0, st, K, ldk, V, ldv, (const unsigned short*)workspace, lse,
                       delta_scratch, Lq, Lk, dK, ldgk, dV, ldgv, accumulate);
  } else {
    hipLaunchKernelGGL(k_attn_kv_bwd_prep<false>, dim3(es_cdiv(Lq, AbT<false>::QS), H), dim3(256), 0, st, Q, ldq, dO, ldd, Lq, scale,
                       (float*)workspace);
    hipLaunchKernelGGL(k_attn_bwd_dq<false>, gq, dim3(256), 0, st, Q, ldq, K, ldk, V, ldv, dO, ldd, lse, delta_scratch, Lq, Lk,
                       (const int*)nullptr, scale, dQ, ldgq, accumulate, H);
    hipLaunchKernelGGL(k_attn_kv_bwd_dkv<false>, gk, dim3(256), 0, st, K, ldk, V, ldv, (const float*)workspace, lse, delta_scratch, Lq,
                       Lk, dK, ldgk, dV, ldgv, accumulate);
  }
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ gather backward with rows shared between prompts
// (SparseFeatureFusion3DGrounder.loss_shared: the query rows of P prompts are gathered from ONE scene's L token rows, and different
// prompts select overlapping rows -- es_row_move mode 1, a plain `+=`, would race on them.)  Two launches, no float atomics:
//   k_scatter_table: workgroup p clears row p of the (P, L) position table to -1 and then writes pos[p][idx[p][q]] = q.  The indices
//     of one prompt are distinct (top-k), so no two lanes write one slot, and nobody but workgroup p touches row p;
//   k_scatter_sum: one lane per (scene row l, channel quad) walks p upward: s = +0, s += dy[p*Q + pos[p][l]] for the prompts that
//     selected l.  The order of the additions is the order of p -- the result is a function of the inputs alone.
// Indices outside [0, L) select nothing (as es_row_move skips negative rows).
__global__ __launch_bounds__(256) void k_scatter_table(const int* __restrict__ idx, int Q, int L, int* __restrict__ pos) {
  const int p = blockIdx.x;
  int* row = pos + (size_t)p * L;
  for (int l = threadIdx.x; l < L; l += 256) row[l] = -1;
  __syncthreads();
  for (int q = threadIdx.x; q < Q; q += 256) {
    int l = idx[(size_t)p * Q + q];
    if (l >= 0 && l < L) row[l] = q;
  }
}
template <int VEC>
__global__ __launch_bounds__(256) void k_scatter_sum(const float* __restrict__ dy, int ldy, const int* __restrict__ pos, int P, int Q,
                                                     int L, int Cv, float* __restrict__ dx, int ldx, int accumulate) {
  const size_t tot = (size_t)L * Cv;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (size_t)gridDim.x * 256) {
    const int l = (int)(e / Cv), c = (int)(e - (size_t)l * Cv) * VEC;
    float s[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s[j] = 0.f;
    for (int p = 0; p < P; ++p) {
      const int q = pos[(size_t)p * L + l];
      if (q < 0) continue;
      const float* src = dy + ((size_t)p * Q + q) * ldy + c;
      if constexpr (VEC == 4) {
        const float4 v = *(const float4*)src;
        s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
      } else {
        s[0] += src[0];
      }
    }
    float* dst = dx + (size_t)l * ldx + c;
    if constexpr (VEC == 4) {
      float4 o = make_float4(s[0], s[1], s[2], s[3]);
      if (accumulate) {
        const float4 a = *(const float4*)dst;
        o = make_float4(a.x + o.x, a.y + o.y, a.z + o.z, a.w + o.w);
      }
      *(float4*)dst = o;
    } else {
      dst[0] = accumulate ? dst[0] + s[0] : s[0];
    }
  }
}
extern "C" size_t es_rows_scatter_sum_workspace_ints(int P, int L) {
  if (P <= 0 || L <= 0) return 0;
  return (size_t)P * L;
}
extern "C" int es_rows_scatter_sum(const float* dy, int ldy, const int* idx, int P, int Q, int L, int C, float* dx, int ldx,
                                   int accumulate, int* workspace, size_t workspace_ints, void* stream) {
  if (P < 0 || Q < 0 || L <= 0 || C <= 0) return 0;
  if (Q > L) return -4;                                     // distinct rows per prompt: at most L of them
  if (ldy < C || ldx < C) return -3;
  const bool vec = (C % 4 == 0) && (((((uintptr_t)dy) | ((uintptr_t)dx)) & 15) == 0);
  if (vec && ((ldy | ldx) & 3)) return -3;
  if (P > 0 && (!workspace || workspace_ints < es_rows_scatter_sum_workspace_ints(P, L))) return -5;
  if ((long long)P * Q > 0x7fffffffLL) return -4;
  if (P > 0) {
    hipLaunchKernelGGL(k_scatter_table, dim3(P), dim3(256), 0, (hipStream_t)stream, idx, Q, L, workspace);
    ES_CHECK_LAUNCH();
  }
  const int Cv = vec ? C / 4 : C;
  int g = es_cdiv((long long)L * Cv, 256);
  if (g > 8192) g = 8192;
  if (vec)
    hipLaunchKernelGGL(k_scatter_sum<4>, dim3(g), dim3(256), 0, (hipStream_t)stream, dy, ldy, workspace, P, Q, L, Cv, dx, ldx, accumulate);
  else
    hipLaunchKernelGGL(k_scatter_sum<1>, dim3(g), dim3(256), 0, (hipStream_t)stream, dy, ldy, workspace, P, Q, L, Cv, dx, ldx, accumulate);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ LayerNorm over the channel dim of (n, C) rows
// z = x (+ res); y = (z - mean) * rstd * w + b.  One wave per row, C <= 512.  z is written out when res != NULL (backward
// needs the normalised input); mean / rstd saved per row.
__global__ __launch_bounds__(256) void k_ln_fwd(const float* __restrict__ x, const float* __restrict__ res, int n, int C,
                                                const float* __restrict__ w, const float* __restrict__ bia, float eps,
                                                float* __restrict__ y, float* __restrict__ z, float* __restrict__ mean,
                                                float* __restrict__ rstd) {
  int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  float v[8];
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    int c = lane + q * 64;
    v[q] = 0.f;
    if (c < C) {
      v[q] = x[(size_t)i * C + c] + (res ? res[(size_t)i * C + c] : 0.f);
      s += v[q];
    }
  }
  float mu = es_wave_sum(s) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    int c = lane + q * 64;
    if (c < C) { float d = v[q] - mu; ss += d * d; }
  }
  float rs = rsqrtf(es_wave_sum(ss) / (float)C + eps);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    int c = lane + q * 64;
    if (c < C) {
      y[(size_t)i * C + c] = (v[q] - mu) * rs * w[c] + bia[c];
      if (z) z[(size_t)i * C + c] = v[q];
    }
  }
  if (lane == 0) { mean[i] = mu; rstd[i] = rs; }
}
extern "C" int es_layernorm_fwd(const float* x, const float* res, int n, int C, const float* w, const float* b, float eps,
                                float* y, float* z, float* mean, float* rstd, void* stream) {
  if (n <= 0) return 0;
  if (C > 512) return -4;
  hipLaunchKernelGGL(k_ln_fwd, dim3(es_cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, x, res, n, C, w, b, eps, y, z, mean, rstd);
  ES_CHECK_LAUNCH();
  return 0;
}
// dz = rstd * (g - mean_c(g) - xhat * mean_c(g * xhat)), g = dy * w;  dw += sum_rows dy * xhat, db += sum_rows dy
// Parameter gradients (round 4, deterministic): every workgroup stores the partial sums of its slice of rows in the workspace,
// the last workgroup to arrive (es_last_block_light, common.h) adds them in workgroup order into dw / db -- one writer, fixed order, no float
// atomics (rounds 2-3 used unsafeAtomicAdd here: the grounder's gradients were reproducible to ~1e-6 only).
#define LN_ROWS_PER_BLOCK 32
__global__ __launch_bounds__(256) void k_ln_bwd(const float* __restrict__ dy, const float* __restrict__ z, int n, int C,
                                                const float* __restrict__ w, const float* __restrict__ mean,
                                                const float* __restrict__ rstd, float* __restrict__ dz, int accumulate,
                                                float* __restrict__ dw, float* __restrict__ db, int rows_per_block,
                                                float* __restrict__ ws, int safe) {
  __shared__ float sw[4][512], sb[4][512];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float aw[8], ab[8], wc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    int c = lane + q * 64;
    aw[q] = ab[q] = 0.f;
    wc[q] = c < C ? w[c] : 0.f;
  }
  int r_end = min(n, (int)(blockIdx.x + 1) * rows_per_block);
  // two rows of this wave per iteration (i and i + 4): their loads are independent, so one memory latency serves both (round 6: a wave walked
  // its 8 rows one dependent latency at a time -- 32 us per launch on the decoder's 3 072 x 256 matrices); sums accumulate in the old row order
  for (int i0 = blockIdx.x * rows_per_block + wv; i0 < r_end; i0 += 8) {
    float d[2][8], zz[2][8], mu[2], rs[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = i0 + 4 * h;
      const bool ok = i < r_end;
      mu[h] = ok ? mean[i] : 0.f;
      rs[h] = ok ? rstd[i] : 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int c = lane + q * 64;
        d[h][q] = zz[h][q] = 0.f;
        if (ok && c < C) { d[h][q] = dy[(size_t)i * C + c]; zz[h][q] = z[(size_t)i * C + c]; }
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = i0 + 4 * h;
      if (i >= r_end) break;
      float g[8], xh[8], s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int c = lane + q * 64;
        g[q] = xh[q] = 0.f;
        if (c < C) {
          xh[q] = (zz[h][q] - mu[h]) * rs[h];
          g[q] = d[h][q] * wc[q];
          s1 += g[q];
          s2 += g[q] * xh[q];
          aw[q] += d[h][q] * xh[q];
          ab[q] += d[h][q];
        }
      }
      s1 = es_wave_sum(s1) / (float)C;
      s2 = es_wave_sum(s2) / (float)C;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int c = lane + q * 64;
        if (c < C) {
          const float v = rs[h] * (g[q] - s1 - xh[q] * s2);
          float* p = dz + (size_t)i * C + c;
          *p = accumulate ? *p + v : v;
        }
      }
    }
  }
  if (!dw && !db) return;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    int c = lane + q * 64;
    if (c < C) { sw[wv][c] = aw[q]; sb[wv][c] = ab[q]; }
  }
  __syncthreads();
  float* part = ws + ES_TICKET_FLOATS;                              // [block][2][C]
  for (int c = threadIdx.x; c < C; c += 256) {                       // (coherent stores / loads: see es_last_block_light)
    es_coh_store(part + ((size_t)blockIdx.x * 2) * C + c, sw[0][c] + sw[1][c] + sw[2][c] + sw[3][c]);
    es_coh_store(part + ((size_t)blockIdx.x * 2 + 1) * C + c, sb[0][c] + sb[1][c] + sb[2][c] + sb[3][c]);
  }
  if (!es_last_block_sel((unsigned int*)ws, gridDim.x, safe)) return;
  for (int c = threadIdx.x; c < C; c += 256) {
    float a, bsum;
    es_coh_sum2(part + c, part + C + c, (int)gridDim.x, (size_t)2 * C, a, bsum);
    if (dw) dw[c] += a;
    if (db) db[c] += bsum;
  }
}
extern "C" size_t es_layernorm_bwd_workspace_floats(int n, int C) {
  return (size_t)ES_TICKET_FLOATS + (size_t)es_cdiv(n > 0 ? n : 1, LN_ROWS_PER_BLOCK) * 2 * C;
}
extern "C" int es_layernorm_bwd(const float* dy, const float* z, int n, int C, const float* w, const float* mean,
                                const float* rstd, float* dz, int accumulate, float* dw, float* db, float* workspace,
                                size_t workspace_floats, void* stream) {
  if (n <= 0) return 0;
  if (C > 512) return -4;
  if ((dw || db) && (!workspace || workspace_floats < es_layernorm_bwd_workspace_floats(n, C))) return -5;
  int rpb = LN_ROWS_PER_BLOCK;
  hipLaunchKernelGGL(k_ln_bwd, dim3(es_cdiv(n, rpb)), dim3(256), 0, (hipStream_t)stream, dy, z, n, C, w, mean, rstd, dz, accumulate,
                     dw, db, rpb, workspace, ES_OPT_ELECT_SAFE);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ ReLU (in place) and its backward through the output
__global__ void k_relu_fwd(float* __restrict__ x, size_t n) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) x[e] = fmaxf(x[e], 0.f);
}
__global__ void k_relu_bwd(float* __restrict__ dy, const float* __restrict__ y, size_t n) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x)
    if (!(y[e] > 0.f)) dy[e] = 0.f;
}
extern "C" int es_relu_fwd(float* x, size_t n, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_relu_fwd, dim3(min(es_cdiv(n, 256), 4096)), dim3(256), 0, (hipStream_t)stream, x, n);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_relu_bwd(float* dy, const float* y, size_t n, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_relu_bwd, dim3(min(es_cdiv(n, 256), 4096)), dim3(256), 0, (hipStream_t)stream, dy, y, n);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ ContrastiveEmbed (grounding_head.py:62-99)
// logits[b, i, t] = <v[b,i,:], text[b,t,:]> / sqrt(C) + bias   for t < tlen[b] (and i < vlen[b]); -inf elsewhere, up to Tmax.
// One wave per visual row; the sample's text block sits in LDS.  rowmax (optional): max_t logits (query selection,
// sparse_featfusion_grounder.py:370-376).
// the per-element arithmetic of ContrastiveEmbed, shared by k_contrastive_fwd and k_contrastive_shared_fwd so that the two cannot drift:
// lane-strided partial sums over C (vv / tt: this lane's channels lane + 64 q of the visual row and of the text token), then the xor
// butterfly 32, 16, .. 1 over the wave (es_wave_sum, or its 8-row form below), * 1 / sqrt(C), + bias
__device__ inline float contrastive_partial(const float (&vv)[8], const float (&tt)[8], int C, int lane) {
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) if ((lane + q * 64) < C) s += vv[q] * tt[q];
  return s;
}
__device__ inline float contrastive_logit(const float (&vv)[8], const float (&tt)[8], int C, int lane, float inv, float bv) {
  return es_wave_sum(contrastive_partial(vv, tt, C, lane)) * inv + bv;
}
// es_wave_sum of EIGHT values at once: 10 shuffles instead of 48.  The butterfly steps 32, 16, 8 each halve the number of values a lane
// carries (a lane keeps the half its lane bit selects and hands the other half to its partner), steps 4, 2, 1 finish the one value left.
// Every step adds the same two partial sums as es_wave_sum does at that step (a + b = b + a bit for bit), so the result equals
// es_wave_sum(s[r]) exactly; it arrives in the lanes with ((lane >> 3) & 7) == bit-reversed r, i.e. r = 4 b5 + 2 b4 + b3 of the lane.
__device__ inline float wave_sum8(const float (&s)[8], int lane) {
  float a[4], b[2], c;
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) a[i] = (h5 ? s[i + 4] : s[i]) + __shfl_xor(h5 ? s[i] : s[i + 4], 32, 64);
#pragma unroll
  for (int i = 0; i < 2; ++i) b[i] = (h4 ? a[i + 2] : a[i]) + __shfl_xor(h4 ? a[i] : a[i + 2], 16, 64);
  c = (h3 ? b[1] : b[0]) + __shfl_xor(h3 ? b[0] : b[1], 8, 64);
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}
__global__ __launch_bounds__(256) void k_contrastive_fwd(const float* __restrict__ v, int L, const float* __restrict__ text, int T,
                                                         int C, const int* __restrict__ tlen, const int* __restrict__ vlen,
                                                         const float* __restrict__ bias, float* __restrict__ logits, int Tout,
                                                         float* __restrict__ rowmax) {
  extern __shared__ float ts[];                         // T * C
  const int b = blockIdx.y;
  const int tl = min(min(tlen[b], T), Tout);            // tokens beyond the Tout written columns are not staged (nor in rowmax)
  for (int e = threadIdx.x; e < tl * C; e += 256) ts[e] = text[(size_t)b * T * C + e];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const float inv = 1.f / sqrtf((float)C), bv = bias ? bias[0] : 0.f;
  const int vl = vlen ? min(vlen[b], L) : L;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < L; i += gridDim.x * 4) {
    const float* vr = v + ((size_t)b * L + i) * C;
    float vv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) vv[q] = (lane + q * 64) < C ? vr[lane + q * 64] : 0.f;
    float best = -INFINITY;
    for (int t = 0; t < Tout; ++t) {
      float out = -INFINITY;
      if (t < tl && i < vl) {
        float tt[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) tt[q] = (lane + q * 64) < C ? ts[t * C + lane + q * 64] : 0.f;
        out = contrastive_logit(vv, tt, C, lane, inv, bv);
      }
      best = fmaxf(best, out);
      if (logits && lane == 0) logits[((size_t)b * L + i) * Tout + t] = out;
    }
    if (rowmax && lane == 0) rowmax[(size_t)b * L + i] = best;
  }
}
extern "C" int es_contrastive_fwd(const float* v, int B, int L, const float* text, int T, int C, const int* tlen_dev,
                                  const int* vlen_dev, const float* bias_dev, float* logits, int Tout, float* rowmax,
                                  void* stream) {
  if (B <= 0 || L <= 0) return 0;
  if (C > 512 || (size_t)T * C * 4 > 160 * 1024 - 1024) return -4;
  size_t sh = (size_t)T * C * sizeof(float);
  if (sh > 64 * 1024) ES_TRY(hipFuncSetAttribute((const void*)k_contrastive_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
  hipLaunchKernelGGL(k_contrastive_fwd, dim3(min(es_cdiv(L, 4), 256), B), dim3(256), sh, (hipStream_t)stream, v, L, text, T, C,
                     tlen_dev, vlen_dev, bias_dev, logits, Tout, rowmax);
  ES_CHECK_LAUNCH();
  return 0;
}
// ContrastiveEmbed of ONE scene's L rows against P prompts' text blocks (SparseFeatureFusion3DGrounder.ground): logits (P, L, Tout),
// rowmax (P, L), bit-identical to es_contrastive_fwd on P copies of the rows (same partial sums, same butterfly: see wave_sum8).  A wave
// holds CS_R = 8 visual rows in registers (a workgroup: 32 consecutive rows, loaded ONCE) while the prompts' text blocks stream through
// LDS; a staged text channel is read from LDS once for the wave's 8 rows and the 8 wave sums of a token are one 10-shuffle reduction --
// the composition it replaces pays 8 LDS reads and 6 shuffles per logit, which is where its time goes.  After the reduction the lanes
// with lane >> 3 == (b5 b4 b3) hold row r = 4 b5 + 2 b4 + b3 of the wave; the lane with (lane & 7) == 0 of each group writes.
// grid (ceil(L / 32), ny): workgroup (x, y) takes the prompts y, y + ny, ... (ny > 1 only when the rows alone would not fill the chip).
// tlen[p] <= 0: a row of -inf.
#define CS_R 8
__global__ __launch_bounds__(256) void k_contrastive_shared_fwd(const float* __restrict__ v, int L, const float* __restrict__ text, int P,
                                                                int T, int C, const int* __restrict__ tlen,
                                                                const float* __restrict__ bias, float* __restrict__ logits, int Tout,
                                                                float* __restrict__ rowmax) {
  extern __shared__ float ts[];                         // T * C
  const int lane = threadIdx.x & 63;
  const float inv = 1.f / sqrtf((float)C), bv = bias ? bias[0] : 0.f;
  const int i0 = blockIdx.x * (4 * CS_R) + (threadIdx.x >> 6) * CS_R;
  float vv[CS_R][8];
#pragma unroll
  for (int r = 0; r < CS_R; ++r) {
#pragma unroll
    for (int q = 0; q < 8; ++q) vv[r][q] = (i0 + r < L && (lane + q * 64) < C) ? v[(size_t)(i0 + r) * C + lane + q * 64] : 0.f;
  }
  const int mine = i0 + ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);      // the row this lane ends up holding
  const bool writer = (lane & 7) == 0 && mine < L;
  for (int p = blockIdx.y; p < P; p += gridDim.y) {
    const int tl = min(min(tlen[p], T), Tout);          // tokens beyond the Tout written columns are not staged (nor in rowmax)
    __syncthreads();                                    // the previous prompt's readers are done
    for (int e = threadIdx.x; e < tl * C; e += 256) ts[e] = text[(size_t)p * T * C + e];
    __syncthreads();
    float best = -INFINITY;
    for (int t = 0; t < Tout; ++t) {
      float out = -INFINITY;
      if (t < tl) {                                     // (workgroup-uniform)
        float tt[8], s[CS_R];
#pragma unroll
        for (int q = 0; q < 8; ++q) tt[q] = (lane + q * 64) < C ? ts[t * C + lane + q * 64] : 0.f;
#pragma unroll
        for (int r = 0; r < CS_R; ++r) s[r] = contrastive_partial(vv[r], tt, C, lane);
        out = wave_sum8(s, lane) * inv + bv;
      }
      best = fmaxf(best, out);
      if (logits && writer) logits[((size_t)p * L + mine) * Tout + t] = out;
    }
    if (rowmax && writer) rowmax[(size_t)p * L + mine] = best;
  }
}
extern "C" int es_contrastive_shared_fwd(const float* v, int L, const float* text, int P, int T, int C, const int* tlen_dev,
                                         const float* bias_dev, float* logits, int Tout, float* rowmax, void* stream) {
  if (P <= 0 || L <= 0) return 0;
  if (C > 512 || (size_t)T * C * 4 > 160 * 1024 - 1024) return -4;
  size_t sh = (size_t)T * C * sizeof(float);
  if (sh > 64 * 1024) ES_TRY(hipFuncSetAttribute((const void*)k_contrastive_shared_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
  const int nx = es_cdiv(L, 4 * CS_R);
  const int ny = min(P, max(1, es_cdiv(512, nx)));
  hipLaunchKernelGGL(k_contrastive_shared_fwd, dim3(nx, ny), dim3(256), sh, (hipStream_t)stream, v, L, text, P, T, C, tlen_dev, bias_dev,
                     logits, Tout, rowmax);
  ES_CHECK_LAUNCH();
  return 0;
}
// backward: dv[b,i,:] = sum_t dl[b,i,t] text[b,t,:] / sqrt(C);  dtext[b,t,:] += sum_i dl[b,i,t] v[b,i,:] / sqrt(C);
// dbias += sum dl.  dlogits must be 0 at masked positions.  One launch, two kinds of workgroups (round 4, deterministic: no
// float atomics): blockIdx.x < nA -> one wave per visual row for dv (the sample's text block in LDS); blockIdx.x >= nA -> ONE
// workgroup per (sample, text token) walks the sample's rows in ascending order, threads over channels, and is the only
// writer of its dtext row; its sum of dl goes to the workspace and the last workgroup to arrive (es_last_block) adds those B * T
// partials in index order into dbias.
__global__ __launch_bounds__(256) void k_contrastive_bwd(const float* __restrict__ dl, int Tout, const float* __restrict__ v, int L,
                                                         const float* __restrict__ text, int T, int C,
                                                         const int* __restrict__ tlen, float* __restrict__ dv, int acc_v,
                                                         float* __restrict__ dtext, float* __restrict__ dbias, int nA,
                                                         float* __restrict__ ws, int safe) {
  extern __shared__ float sh[];                         // dv workgroups: the sample's text block [tl * C]
  const int b = blockIdx.y;
  const int tl = min(min(tlen[b], T), Tout);            // a dlogits row holds Tout columns: the forward wrote no more
  const float inv = 1.f / sqrtf((float)C);
  const bool reduce = (dtext != nullptr) || (dbias != nullptr);
  if ((int)blockIdx.x < nA) {
    if (dv) {
      float* ts = sh;
      for (int e = threadIdx.x; e < tl * C; e += 256) ts[e] = text[(size_t)b * T * C + e];
      __syncthreads();
      const int lane = threadIdx.x & 63;
      for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < L; i += nA * 4) {
        const float* dr = dl + ((size_t)b * L + i) * Tout;
        float g[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) g[q] = 0.f;
        for (int t = 0; t < tl; ++t) {
          float d = dr[t];
          if (d == 0.f) continue;
          d *= inv;
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            int c = lane + q * 64;
            if (c < C) g[q] += d * ts[t * C + c];
          }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          int c = lane + q * 64;
          if (c < C) { float* p = dv + ((size_t)b * L + i) * C + c; *p = acc_v ? *p + g[q] : g[q]; }
        }
      }
    }
  } else if (reduce) {
    const int t = (int)blockIdx.x - nA;
    float a0 = 0.f, a1 = 0.f, bs = 0.f;
    const int c0 = threadIdx.x, c1 = threadIdx.x + 256;
    if (t < tl) {
      for (int i0 = 0; i0 < L; i0 += 8) {                  // 8 rows in flight, added in ascending row order
        float d[8], x0[8], x1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int i = i0 + u;
          const bool in = i < L;
          d[u] = in ? dl[((size_t)b * L + i) * Tout + t] : 0.f;
          const float* vr = v + ((size_t)b * L + (in ? i : 0)) * C;
          x0[u] = (in && c0 < C) ? vr[c0] : 0.f;
          x1[u] = (in && c1 < C) ? vr[c1] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (d[u] == 0.f) continue;                       // (uniform across the workgroup)
          bs += d[u];
          const float ds = d[u] * inv;
          a0 += ds * x0[u];
          a1 += ds * x1[u];
        }
      }
      if (dtext) {
        float* o = dtext + ((size_t)b * T + t) * C;
        if (c0 < C) o[c0] += a0;
        if (c1 < C) o[c1] += a1;
      }
    }
    if (threadIdx.x == 0) es_coh_store(ws + ES_TICKET_FLOATS + (size_t)b * T + t, bs);
  }
  if (!reduce) return;
  if (!es_last_block_sel((unsigned int*)ws, gridDim.x * gridDim.y, safe)) return;
  if (dbias && threadIdx.x == 0) {
    dbias[0] += es_coh_sum(ws + ES_TICKET_FLOATS, (int)(gridDim.y * T), 1);
  }
}
extern "C" size_t es_contrastive_bwd_workspace_floats(int B, int T) { return (size_t)ES_TICKET_FLOATS + (size_t)(B > 0 ? B : 1) * T; }
extern "C" int es_contrastive_bwd(const float* dlogits, int Tout, const float* v, int B, int L, const float* text, int T, int C,
                                  const int* tlen_dev, float* dv, int acc_v, float* dtext, float* dbias, float* workspace,
                                  size_t workspace_floats, void* stream) {
  if (B <= 0 || L <= 0) return 0;
  size_t sh = (size_t)T * C * sizeof(float);
  if (C > 512 || sh > 160 * 1024 - 1024) return -4;
  const bool reduce = dtext || dbias;
  if (reduce && (!workspace || workspace_floats < es_contrastive_bwd_workspace_floats(B, T))) return -5;
  if (sh > 64 * 1024) ES_TRY(hipFuncSetAttribute((const void*)k_contrastive_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
  const int nA = dv ? min(es_cdiv(L, 4), 64) : 0;
  const int nx = nA + (reduce ? T : 0);
  if (nx <= 0) return 0;
  hipLaunchKernelGGL(k_contrastive_bwd, dim3(nx, B), dim3(256), sh, (hipStream_t)stream, dlogits, Tout, v, L, text, T, C, tlen_dev,
                     dv, acc_v, dtext, dbias, nA, workspace, ES_OPT_ELECT_SAFE);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ 9-DoF "baseline" box coder (grounding_head.py:286-296)
// box = (pred[:3] + point, clamp(exp(pred[3:6]), 2e-2), pred[6:9])
__global__ void k_ground_decode_fwd(const float* __restrict__ pred, int ldp, const float* __restrict__ pts, int n,
                                    float* __restrict__ box) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = pred + (size_t)i * ldp;
  float* o = box + (size_t)i * 9;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[c] = p[c] + pts[(size_t)i * 3 + c];
    o[3 + c] = fmaxf(expf(p[3 + c]), 2e-2f);
    o[6 + c] = p[6 + c];
  }
}
extern "C" int es_ground_decode_fwd(const float* pred, int ldp, const float* points, int n, float* box, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_ground_decode_fwd, dim3(es_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, pred, ldp, points, n, box);
  ES_CHECK_LAUNCH();
  return 0;
}
__global__ void k_ground_decode_bwd(const float* __restrict__ pred, int ldp, const float* __restrict__ dbox, int n,
                                    float* __restrict__ dpred, int ldg, int accumulate) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = pred + (size_t)i * ldp;
  const float* g = dbox + (size_t)i * 9;
  float* o = dpred + (size_t)i * ldg;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float e = expf(p[3 + c]);
    float v0 = g[c], v1 = e > 2e-2f ? g[3 + c] * e : 0.f, v2 = g[6 + c];     // clamp(min): gradient passes where exp > min
    o[c] = accumulate ? o[c] + v0 : v0;
    o[3 + c] = accumulate ? o[3 + c] + v1 : v1;
    o[6 + c] = accumulate ? o[6 + c] + v2 : v2;
  }
}
extern "C" int es_ground_decode_bwd(const float* pred, int ldp, const float* dbox, int n, float* dpred, int ldg, int accumulate,
                                    void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_ground_decode_bwd, dim3(es_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, pred, ldp, dbox, n, dpred, ldg,
                     accumulate);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ 9-DoF "FCAF" box coder (grounding_head.py:308-363;
// configs/grounding/mv-grounding_8xb12_embodiedscan-vg-9dof_fcaf-coder.py:64)
// d = clamp(exp(pred[0:6]), 2e-2) (log distances to the six faces); s = ((d1 - d0) / 2, (d3 - d2) / 2, (d5 - d4) / 2);
// box = (point + R(euler) s, (d0 + d1, d2 + d3, d4 + d5), euler), euler = pred[6:9], R = Rz(a) Rx(b) Ry(c) (rotation_3d_in_euler
// multiplies the row vector by R^T).  The reference writes d in place into bbox_pred; nothing reads bbox_pred afterwards, so this
// is a pure function of (pred, point) and autograd differentiates through exp / clamp (gradient passes where exp >= 2e-2).
struct FcafRot { float c0[3], c1[3], c2[3], sa, ca, sb, cb, sc, cc; };
__device__ inline FcafRot fcaf_rot(float a, float b, float c) {
  FcafRot r;
  r.sa = sinf(a); r.ca = cosf(a); r.sb = sinf(b); r.cb = cosf(b); r.sc = sinf(c); r.cc = cosf(c);
  r.c0[0] = r.ca * r.cc - r.sa * r.sb * r.sc; r.c0[1] = r.sa * r.cc + r.ca * r.sb * r.sc; r.c0[2] = -(r.cb * r.sc);
  r.c1[0] = -(r.sa * r.cb);                   r.c1[1] = r.ca * r.cb;                      r.c1[2] = r.sb;
  r.c2[0] = r.ca * r.sc + r.sa * r.sb * r.cc; r.c2[1] = r.sa * r.sc - r.ca * r.sb * r.cc; r.c2[2] = r.cb * r.cc;
  return r;
}
__global__ void k_ground_decode_fcaf_fwd(const float* __restrict__ pred, int ldp, const float* __restrict__ pts, int n,
                                         float* __restrict__ box) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = pred + (size_t)i * ldp;
  float* o = box + (size_t)i * 9;
  float d[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) d[j] = fmaxf(expf(p[j]), 2e-2f);
  const float s0 = (d[1] - d[0]) * 0.5f, s1 = (d[3] - d[2]) * 0.5f, s2 = (d[5] - d[4]) * 0.5f;
  const FcafRot r = fcaf_rot(p[6], p[7], p[8]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[c] = pts[(size_t)i * 3 + c] + (r.c0[c] * s0 + r.c1[c] * s1 + r.c2[c] * s2);
    o[3 + c] = d[2 * c] + d[2 * c + 1];
    o[6 + c] = p[6 + c];
  }
}
extern "C" int es_ground_decode_fcaf_fwd(const float* pred, int ldp, const float* points, int n, float* box, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_ground_decode_fcaf_fwd, dim3(es_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, pred, ldp, points, n, box);
  ES_CHECK_LAUNCH();
  return 0;
}
__global__ void k_ground_decode_fcaf_bwd(const float* __restrict__ pred, int ldp, const float* __restrict__ dbox, int n,
                                         float* __restrict__ dpred, int ldg, int accumulate) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* p = pred + (size_t)i * ldp;
  const float* g = dbox + (size_t)i * 9;
  float* o = dpred + (size_t)i * ldg;
  float e[6], d[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) { e[j] = expf(p[j]); d[j] = fmaxf(e[j], 2e-2f); }
  const float s0 = (d[1] - d[0]) * 0.5f, s1 = (d[3] - d[2]) * 0.5f, s2 = (d[5] - d[4]) * 0.5f;
  const FcafRot r = fcaf_rot(p[6], p[7], p[8]);
  // gradient w.r.t. the shift: R^T g_center
  const float gs0 = r.c0[0] * g[0] + r.c0[1] * g[1] + r.c0[2] * g[2];
  const float gs1 = r.c1[0] * g[0] + r.c1[1] * g[1] + r.c1[2] * g[2];
  const float gs2 = r.c2[0] * g[0] + r.c2[1] * g[1] + r.c2[2] * g[2];
  const float gs[3] = {gs0, gs1, gs2};
  float out[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float lo = -0.5f * gs[c] + g[3 + c], hi = 0.5f * gs[c] + g[3 + c];       // d d[2c], d d[2c+1]
    out[2 * c] = e[2 * c] >= 2e-2f ? lo * e[2 * c] : 0.f;
    out[2 * c + 1] = e[2 * c + 1] >= 2e-2f ? hi * e[2 * c + 1] : 0.f;
  }
  // v = R s; dv/da = (-v.y, v.x, 0); dv/dc = col0 * s2 - col2 * s0; dv/db from the element-wise derivative of Rz Rx Ry
  const float v0 = r.c0[0] * s0 + r.c1[0] * s1 + r.c2[0] * s2, v1 = r.c0[1] * s0 + r.c1[1] * s1 + r.c2[1] * s2;
  const float da = g[0] * (-v1) + g[1] * v0;
  const float b0 = (-(r.sa * r.cb * r.sc)) * s0 + (r.sa * r.sb) * s1 + (r.sa * r.cb * r.cc) * s2;
  const float b1 = (r.ca * r.cb * r.sc) * s0 + (-(r.ca * r.sb)) * s1 + (-(r.ca * r.cb * r.cc)) * s2;
  const float b2 = (r.sb * r.sc) * s0 + r.cb * s1 + (-(r.sb * r.cc)) * s2;
  const float db = g[0] * b0 + g[1] * b1 + g[2] * b2;
  const float dc = g[0] * (r.c0[0] * s2 - r.c2[0] * s0) + g[1] * (r.c0[1] * s2 - r.c2[1] * s0) + g[2] * (r.c0[2] * s2 - r.c2[2] * s0);
  out[6] = g[6] + da; out[7] = g[7] + db; out[8] = g[8] + dc;
#pragma unroll
  for (int j = 0; j < 9; ++j) o[j] = accumulate ? o[j] + out[j] : out[j];
}
extern "C" int es_ground_decode_fcaf_bwd(const float* pred, int ldp, const float* dbox, int n, float* dpred, int ldg, int accumulate,
                                         void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_ground_decode_fcaf_bwd, dim3(es_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, pred, ldp, dbox, n, dpred,
                     ldg, accumulate);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ frozen RoBERTa text encoder (forward only; embodiedscan_amd/text.py
// HipTextEncoder): embedding gather + position rule + LayerNorm, residual LayerNorm up to C = 1024, exact-erf bias + GELU, and a masked
// self-attention with head dimension 64 on a packed [q | k | v] projection.  The projections themselves are K = 1 row GEMMs.
#define TX_MAXQ 16       // channels per lane of a row held by one wave: C <= 64 * TX_MAXQ = 1024

// y[c] = (v - mean) * rstd * w[c] + b[c] for the row a wave holds as v[q] = row[lane + 64 q] (k_ln_fwd's arithmetic: two passes)
__device__ inline void tx_ln_row(const float (&v)[TX_MAXQ], int C, int lane, const float* __restrict__ w, const float* __restrict__ bia,
                                 float eps, float* __restrict__ yrow) {
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < TX_MAXQ; ++q) if (lane + q * 64 < C) s += v[q];
  const float mu = es_wave_sum(s) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int q = 0; q < TX_MAXQ; ++q) if (lane + q * 64 < C) { float d = v[q] - mu; ss += d * d; }
  const float rs = rsqrtf(es_wave_sum(ss) / (float)C + eps);
#pragma unroll
  for (int q = 0; q < TX_MAXQ; ++q) {
    const int c = lane + q * 64;
    if (c < C) yrow[c] = (v[q] - mu) * rs * w[c] + bia[c];
  }
}

// One wave per token row (b, t).  ids outside [0, vocab) count as pad_id everywhere.  Position (modeling_roberta.py
// create_position_ids_from_input_ids): pad_id + (id != pad_id ? #{t' <= t : id[t'] != pad_id} : 0).
__global__ __launch_bounds__(256) void k_text_embed_ln(const long long* __restrict__ ids, int n, int T, int pad_id,
                                                       const float* __restrict__ word, const float* __restrict__ pos,
                                                       const float* __restrict__ type0, int C, int vocab, const float* __restrict__ w,
                                                       const float* __restrict__ bia, float eps, float* __restrict__ y,
                                                       int* __restrict__ pos_ids) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  const int t = i % T;
  const long long* row = ids + (size_t)(i - t);
  int cnt = 0;
  for (int u = lane; u <= t; u += 64) {
    const long long v = row[u];
    cnt += (v >= 0 && v < vocab && v != pad_id) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  long long id = row[t];
  if (id < 0 || id >= vocab) id = pad_id;
  const int p = pad_id + (id != pad_id ? cnt : 0);         // <= pad_id + T < max_pos (checked by the entry point)
  if (pos_ids && lane == 0) pos_ids[i] = p;
  const float* wr = word + (size_t)id * C;
  const float* pr = pos + (size_t)p * C;
  float v[TX_MAXQ];
#pragma unroll
  for (int q = 0; q < TX_MAXQ; ++q) {
    const int c = lane + q * 64;
    v[q] = c < C ? (wr[c] + pr[c]) + type0[c] : 0.f;
  }
  tx_ln_row(v, C, lane, w, bia, eps, y + (size_t)i * C);
}
extern "C" int es_text_embed_ln(const long long* ids, int B, int T, int pad_id, const float* word, const float* pos,
                                const float* type0, int C, int vocab, int max_pos, const float* ln_w, const float* ln_b, float eps,
                                float* y, int* pos_ids, void* stream) {
  if (B <= 0 || T <= 0) return 0;
  if (!ids || !word || !pos || !type0 || !ln_w || !ln_b || !y) return -4;
  if (C <= 0 || C > 64 * TX_MAXQ || vocab <= 0 || pad_id < 0 || pad_id >= vocab) return -4;
  if ((long long)pad_id + T >= max_pos || (long long)B * T > 0x7fffffffLL) return -4;
  const int n = B * T;
  hipLaunchKernelGGL(k_text_embed_ln, dim3(es_cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, ids, n, T, pad_id, word, pos, type0, C,
                     vocab, ln_w, ln_b, eps, y, pos_ids);
  ES_CHECK_LAUNCH();
  return 0;
}

// y = LayerNorm(x (+ res)) for C <= 1024, no saved statistics (es_layernorm_fwd stops at 512 and feeds a backward pass).  A wave
// holds its whole row before it writes: y may alias x or res.
__global__ __launch_bounds__(256) void k_text_add_ln(const float* x, const float* res, int n, int C, const float* __restrict__ w,
                                                     const float* __restrict__ bia, float eps, float* y) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  float v[TX_MAXQ];
#pragma unroll
  for (int q = 0; q < TX_MAXQ; ++q) {
    const int c = lane + q * 64;
    v[q] = 0.f;
    if (c < C) v[q] = x[(size_t)i * C + c] + (res ? res[(size_t)i * C + c] : 0.f);
  }
  tx_ln_row(v, C, lane, w, bia, eps, y + (size_t)i * C);
}
extern "C" int es_text_add_ln(const float* x, const float* res, int n, int C, const float* w, const float* b, float eps, float* y,
                              void* stream) {
  if (n <= 0) return 0;
  if (!x || !w || !b || !y || C <= 0 || C > 64 * TX_MAXQ) return -4;
  hipLaunchKernelGGL(k_text_add_ln, dim3(es_cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, x, res, n, C, w, b, eps, y);
  ES_CHECK_LAUNCH();
  return 0;
}

// x[r, c] <- gelu(x[r, c] + bias[c]), the exact form 0.5 z (1 + erf(z / sqrt 2)) (transformers' "gelu"), in place, c < C of rows with
// leading dimension ld
__global__ void k_bias_gelu(float* __restrict__ x, int ld, int n, int C, const float* __restrict__ bias) {
  const size_t total = (size_t)n * C;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t r = e / C;
    const int c = (int)(e - r * C);
    float* p = x + r * ld + c;
    const float z = *p + bias[c];
    *p = (0.5f * z) * (1.f + erff(z * 0.70710678118654752f));
  }
}
extern "C" int es_bias_gelu(float* x, int ld, int n, int C, const float* bias, void* stream) {
  if (n <= 0) return 0;
  if (!x || !bias || C <= 0 || ld < C) return -4;
  hipLaunchKernelGGL(k_bias_gelu, dim3(min(es_cdiv((long long)n * C, 256), 4096)), dim3(256), 0, (hipStream_t)stream, x, ld, n, C,
                     bias);
  ES_CHECK_LAUNCH();
  return 0;
}

// Self-attention with head dimension 64 on the packed projection: row (b T + t) holds [q | k | v], head h in columns 64 h .. of
// each third.  Prompts are short (T = 10 .. 40) and B H is large, so the unit of work is ONE WAVE = one (sample, head, 16-query
// tile), launched as a one-wave workgroup: nothing is shared between waves, a barrier costs nothing, and the chip sees
// B H ceil(T / 16) independent workgroups (several per CU: 22.5 KiB of LDS in bf16, 40.6 KiB in f32).  Keys are walked in steps
// of 64 with the online softmax; for T <= 64 that is one step, the whole K and V^T of the (sample, head) resident in LDS.
// A score tile (16 queries x 16 keys) is two 16x16x32 k-steps.  mask: (B, T) int32, 0 = key masked (any pattern), NULL = all live.
#define TA_D 64
#define TA_KS 64
template <bool BF> struct TaT;
template <> struct TaT<true> { static constexpr int LD = 72; };       // 144-byte rows: the 16-byte fragments stay aligned
template <> struct TaT<false> { static constexpr int LD = 65; };

template <bool BF>
__global__ __launch_bounds__(64) void k_text_attn_fwd(const float* __restrict__ qkv, int ld, int H, int T,
                                                      const int* __restrict__ mask, float* __restrict__ O, int ldo, int nqt) {
  typedef typename AtT<BF>::T S;
  constexpr int LD = TaT<BF>::LD;
  __shared__ __attribute__((aligned(16))) S Qs[16 * LD], Ks[TA_KS * LD], Vt[TA_D * LD], Ps[16 * LD];
  const int item = blockIdx.x;
  const int qt = item % nqt, h = (item / nqt) % H, b = item / (nqt * H);
  const int lane = threadIdx.x, li = lane & 15, kq = lane >> 4;
  const int q0 = qt * 16, E = H * TA_D;
  const float* base = qkv + (size_t)b * T * ld + h * TA_D;
  const int* mrow = mask ? mask + (size_t)b * T : nullptr;
  for (int e = lane; e < 16 * 16; e += 64) {               // Q tile, scaled by 1/8 (a power of two: commutes with the rounding)
    const int r = e >> 4, c = (e & 15) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + r < T) v = *(const float4*)(base + (size_t)(q0 + r) * ld + c);
    S* d = Qs + r * LD + c;
    d[0] = at_cvt<BF>(v.x * 0.125f); d[1] = at_cvt<BF>(v.y * 0.125f); d[2] = at_cvt<BF>(v.z * 0.125f); d[3] = at_cvt<BF>(v.w * 0.125f);
  }
  float m[4], l[4];
  tf32x4_t o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; l[r] = 0.f; o[r] = (tf32x4_t){0.f, 0.f, 0.f, 0.f}; }
  for (int k0 = 0; k0 < T; k0 += TA_KS) {
    __syncthreads();                                       // the previous step's readers of Ks / Vt / Ps are done
    for (int e = lane; e < TA_KS * 16; e += 64) {
      const int r = e >> 4, c = (e & 15) * 4;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (k0 + r < T) {
        const float* p = base + (size_t)(k0 + r) * ld + c;
        kv = *(const float4*)(p + E);
        vv = *(const float4*)(p + 2 * E);
      }
      S* d = Ks + r * LD + c;
      d[0] = at_cvt<BF>(kv.x); d[1] = at_cvt<BF>(kv.y); d[2] = at_cvt<BF>(kv.z); d[3] = at_cvt<BF>(kv.w);
      Vt[(c + 0) * LD + r] = at_cvt<BF>(vv.x);
      Vt[(c + 1) * LD + r] = at_cvt<BF>(vv.y);
      Vt[(c + 2) * LD + r] = at_cvt<BF>(vv.z);
      Vt[(c + 3) * LD + r] = at_cvt<BF>(vv.w);
    }
    __syncthreads();
    tf32x4_t s[4];
    bool ok[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = (tf32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) s[t] = tile_mma<BF>(Qs + li * LD + ks * 32, Ks + (t * 16 + li) * LD + ks * 32, kq, s[t]);
      const int j = k0 + t * 16 + li;
      ok[t] = j < T && (!mrow || mrow[j] != 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float sv[4], mx = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t) { sv[t] = ok[t] ? s[t][r] : -INFINITY; mx = fmaxf(mx, sv[t]); }
      mx = group16_max(mx);
      const float mn = fmaxf(m[r], mx);
      const float ref = mn == -INFINITY ? 0.f : mn;        // no live key so far: every exponential below is exp(-inf) = 0
      const float corr = BF ? __expf(m[r] - ref) : expf(m[r] - ref);
      float ps = 0.f;
      S* prow = Ps + (kq * 4 + r) * LD;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float p = BF ? __expf(sv[t] - ref) : expf(sv[t] - ref);
        ps += p;
        prow[t * 16 + li] = at_cvt<BF>(p);
      }
      l[r] = l[r] * corr + group16_sum(ps);
      m[r] = mn;
#pragma unroll
      for (int nf = 0; nf < 4; ++nf) o[nf][r] *= corr;
    }
    __syncthreads();
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) o[nf] = tile_mma<BF>(Ps + li * LD + ks * 32, Vt + (nf * 16 + li) * LD + ks * 32, kq, o[nf]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + kq * 4 + r;
    if (q >= T) continue;
    const float inv = l[r] > 0.f ? 1.f / l[r] : 0.f;       // a sample without a live key: O = 0 (the file's convention, k_attn_fwd)
    float* orow = O + ((size_t)b * T + q) * ldo + h * TA_D;
#pragma unroll
    for (int nf = 0; nf < 4; ++nf) orow[nf * 16 + li] = o[nf][r] * inv;
  }
}
extern "C" int es_text_attn_fwd(const float* qkv, int ld, int B, int H, int T, const int* mask_dev, float* O, int ldo, int bf16,
                                void* stream) {
  if (B <= 0 || H <= 0) return 0;
  if (!qkv || !O || T < 1 || T > 512) return -4;
  if ((long long)H * TA_D * 3 > ld || (long long)H * TA_D > ldo || ((ld | ldo) & 3)) return -4;
  if (((size_t)qkv & 15) != 0) return -4;                  // rows are read as float4
  const int nqt = es_cdiv(T, 16);
  const long long items = (long long)B * H * nqt;
  if (items > 0x7fffffffLL || (long long)B * T > 0x7fffffffLL) return -4;
  if (bf16)
    hipLaunchKernelGGL(k_text_attn_fwd<true>, dim3((unsigned)items), dim3(64), 0, (hipStream_t)stream, qkv, ld, H, T, mask_dev, O, ldo,
                       nqt);
  else
    hipLaunchKernelGGL(k_text_attn_fwd<false>, dim3((unsigned)items), dim3(64), 0, (hipStream_t)stream, qkv, ld, H, T, mask_dev, O, ldo,
                       nqt);
  ES_CHECK_LAUNCH();
  return 0;
}
