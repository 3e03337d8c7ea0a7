// Inference post-processing of the FCAF3D 9-DoF head:
//   scores = sigmoid(cls) * sigmoid(centerness), 12-d -> 9-DoF box decode, per-class greedy NMS on the rotated
//   bird's-eye-view IoU.  Replaces FCAF3DHeadRotMat._predict_by_feat_single / _single_scene_multiclass_nms
//   (embodiedscan/models/dense_heads/fcaf3d_head.py:1352-1399,1666-1725) and mmcv.ops.nms3d (iou3d_nms3d_forward).
#include "common.h"
#include "../../include/es_hip.h"

__global__ void k_predict_scores(const float* __restrict__ ho, int ldh, int n, int C, float* __restrict__ scores,
                                 float* __restrict__ maxs) {
  int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n) return;
  const float* h = ho + (size_t)row * ldh;
  float sc = 1.f / (1.f + expf(-h[0]));
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) {
    float s = (1.f / (1.f + expf(-h[13 + c]))) * sc;
    scores[(size_t)row * C + c] = s;
    m = fmaxf(m, s);
  }
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) maxs[row] = m;
}
extern "C" int es_predict_scores(const float* ho, int ldh, int n, int C, float* scores, float* max_scores, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_predict_scores, dim3(es_cdiv(n, 4)), dim3(256), 0, (hipStream_t)stream, ho, ldh, n, C, scores,
                     max_scores);
  ES_CHECK_LAUNCH();
  return 0;
}

// rows selected by idx: 12-d prediction + location -> (cx,cy,cz,dx,dy,dz,alpha,beta,gamma)   (fcaf3d_head.py:1454-1525)
__global__ void k_decode_boxes(const float* __restrict__ points, const float* __restrict__ bbox,
                               const int* __restrict__ idx, int m, float* __restrict__ out) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  int i = idx ? idx[t] : t;
  const float* b = bbox + (size_t)i * 12;
  const float* p = points + (size_t)i * 3;
  float xr[3] = {b[6], b[7], b[8]}, yr[3] = {b[9], b[10], b[11]};
  float ny = sqrtf(yr[0] * yr[0] + yr[1] * yr[1] + yr[2] * yr[2]) + 1e-8f;
  float y[3] = {yr[0] / ny, yr[1] / ny, yr[2] / ny};
  float z[3] = {xr[1] * y[2] - xr[2] * y[1], xr[2] * y[0] - xr[0] * y[2], xr[0] * y[1] - xr[1] * y[0]};
  float nz = sqrtf(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]) + 1e-8f;
  z[0] /= nz; z[1] /= nz; z[2] /= nz;
  float x[3] = {y[1] * z[2] - y[2] * z[1], y[2] * z[0] - y[0] * z[2], y[0] * z[1] - y[1] * z[0]};
  float e0 = atan2f(-y[0], y[1]), e1 = asinf(y[2]), e2 = atan2f(-x[2], z[2]);
  float ca = cosf(e0), sa = sinf(e0), cb = cosf(e1), sb = sinf(e1), cc = cosf(e2), sc = sinf(e2);
  float R[9] = {ca * cc - sa * sb * sc, -sa * cb, ca * sc + sa * sb * cc, sa * cc + ca * sb * sc, ca * cb,
                sa * sc - ca * sb * cc, -cb * sc, sb, cb * cc};
  float s0 = (b[1] - b[0]) / 2, s1 = (b[3] - b[2]) / 2, s2 = (b[5] - b[4]) / 2;
  float* o = out + (size_t)t * 9;
  o[0] = p[0] + (s0 * R[0] + s1 * R[1] + s2 * R[2]);
  o[1] = p[1] + (s0 * R[3] + s1 * R[4] + s2 * R[5]);
  o[2] = p[2] + (s0 * R[6] + s1 * R[7] + s2 * R[8]);
  o[3] = b[0] + b[1]; o[4] = b[2] + b[3]; o[5] = b[4] + b[5];
  o[6] = e0; o[7] = e1; o[8] = e2;
}
extern "C" int es_decode_boxes(const float* points, const float* bbox, const int* idx, int m, float* out, void* stream) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_decode_boxes, dim3(es_cdiv(m, 128)), dim3(128), 0, (hipStream_t)stream, points, bbox, idx, m, out);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ rotated BEV IoU (float64, see oracle/predict.py)
struct P2 { double x, y; };
__device__ inline double crs(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }
__device__ inline void bev_corners(const float* b, P2* c) {
  double x = b[0], y = b[1], dx = b[3], dy = b[4], ang = b[6];
  double cs = cos(ang), sn = sin(ang);
  double x1 = x - dx / 2, y1 = y - dy / 2, x2 = x + dx / 2, y2 = y + dy / 2;
  double px[4] = {x1, x2, x2, x1}, py[4] = {y1, y1, y2, y2};
  for (int k = 0; k < 4; ++k) {
    c[k].x = (px[k] - x) * cs + (py[k] - y) * (-sn) + x;
    c[k].y = (px[k] - x) * sn + (py[k] - y) * cs + y;
  }
  c[4] = c[0];
}
__device__ inline bool seg_isect(P2 p1, P2 p0, P2 q1, P2 q0, P2& out) {
  if (!(fmin(p0.x, p1.x) <= fmax(q0.x, q1.x) && fmin(q0.x, q1.x) <= fmax(p0.x, p1.x) &&
        fmin(p0.y, p1.y) <= fmax(q0.y, q1.y) && fmin(q0.y, q1.y) <= fmax(p0.y, p1.y)))
    return false;
  double s1 = crs(q0.x - p0.x, q0.y - p0.y, p1.x - p0.x, p1.y - p0.y);
  double s2 = crs(p1.x - p0.x, p1.y - p0.y, q1.x - p0.x, q1.y - p0.y);
  double s3 = crs(p0.x - q0.x, p0.y - q0.y, q1.x - q0.x, q1.y - q0.y);
  double s4 = crs(q1.x - q0.x, q1.y - q0.y, p1.x - q0.x, p1.y - q0.y);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  double s5 = crs(q1.x - p0.x, q1.y - p0.y, p1.x - p0.x, p1.y - p0.y);
  if (fabs(s5 - s1) > 1e-8) {
    out.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    out.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    double a0 = p0.y - p1.y, a1 = q0.y - q1.y, b0 = p1.x - p0.x, b1 = q1.x - q0.x;
    double c0 = p0.x * p1.y - p1.x * p0.y, c1 = q0.x * q1.y - q1.x * q0.y;
    double D = a0 * b1 - a1 * b0;
    out.x = (b0 * c1 - b1 * c0) / D;
    out.y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}
__device__ inline bool in_box(const float* b, P2 p) {
  double cx = b[0], cy = b[1], dx = b[3], dy = b[4], ang = b[6];
  double cs = cos(-ang), sn = sin(-ang);
  double rx = (p.x - cx) * cs + (p.y - cy) * (-sn), ry = (p.x - cx) * sn + (p.y - cy) * cs;
  return fabs(rx) < dx / 2 + 1e-2 && fabs(ry) < dy / 2 + 1e-2;
}
__device__ double iou_bev(const float* a, const float* b) {
  P2 ca[5], cb[5], pts[16];
  bev_corners(a, ca);
  bev_corners(b, cb);
  int cnt = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      P2 o;
      if (seg_isect(ca[i + 1], ca[i], cb[j + 1], cb[j], o)) pts[cnt++] = o;
    }
  for (int k = 0; k < 4; ++k) {
    if (in_box(a, cb[k])) pts[cnt++] = cb[k];
    if (in_box(b, ca[k])) pts[cnt++] = ca[k];
  }
  double so = 0.0;
  if (cnt >= 3) {
    double mx = 0, my = 0;
    for (int k = 0; k < cnt; ++k) { mx += pts[k].x; my += pts[k].y; }
    mx /= cnt; my /= cnt;
    double ang[16];
    for (int k = 0; k < cnt; ++k) ang[k] = atan2(pts[k].y - my, pts[k].x - mx);
    for (int i = 1; i < cnt; ++i) {                    // insertion sort (stable, like the oracle's list.sort)
      P2 p = pts[i]; double g = ang[i];
      int j = i - 1;
      while (j >= 0 && ang[j] > g) { pts[j + 1] = pts[j]; ang[j + 1] = ang[j]; --j; }
      pts[j + 1] = p; ang[j + 1] = g;
    }
    double area = 0;
    for (int k = 0; k < cnt - 1; ++k)
      area += crs(pts[k].x - pts[0].x, pts[k].y - pts[0].y, pts[k + 1].x - pts[0].x, pts[k + 1].y - pts[0].y);
    so = fabs(area) / 2.0;
  }
  double sa = (double)a[3] * (double)a[4], sb = (double)b[3] * (double)b[4];
  return so / fmax(sa + sb - so, 1e-8);
}

#define NMS_CAP 4096
// one workgroup per class: candidates (score > thr) -> bitonic sort by (score desc, index asc) -> greedy suppression.
// keep_idx[c*M + k] = k-th kept box (descending score), keep_cnt[c] = number kept.
__global__ __launch_bounds__(256) void k_nms3d_multiclass(const float* __restrict__ boxes /* (M,9) */,
                                                          const float* __restrict__ scores /* (M,C) */, int M, int C,
                                                          float score_thr, float iou_thr, int* __restrict__ keep_idx,
                                                          int* __restrict__ keep_cnt) {
  __shared__ float s_key[NMS_CAP];
  __shared__ int s_idx[NMS_CAP];
  __shared__ unsigned char s_sup[NMS_CAP];
  __shared__ int s_n, s_keep;
  const int c = blockIdx.x, t = threadIdx.x;
  if (t == 0) { s_n = 0; s_keep = 0; }
  __syncthreads();
  for (int i = t; i < M; i += 256) {
    float s = scores[(size_t)i * C + c];
    if (s > score_thr) {
      int p = atomicAdd(&s_n, 1);
      if (p < NMS_CAP) { s_key[p] = s; s_idx[p] = i; }
    }
  }
  __syncthreads();
  int n = min(s_n, NMS_CAP);
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int i = n + t; i < np2; i += 256) { s_key[i] = -INFINITY; s_idx[i] = 0x7fffffff; }
  __syncthreads();
  for (int k = 2; k <= np2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < np2; i += 256) {
        int l = i ^ j;
        if (l > i) {
          bool up = ((i & k) == 0);
          float ki = s_key[i], kl = s_key[l];
          int ii = s_idx[i], il = s_idx[l];
          bool i_first = (ki > kl) || (ki == kl && ii < il);     // i should come before l in the final order
          if (up ? !i_first : i_first) { s_key[i] = kl; s_key[l] = ki; s_idx[i] = il; s_idx[l] = ii; }
        }
      }
      __syncthreads();
    }
  for (int i = t; i < n; i += 256) s_sup[i] = 0;
  __syncthreads();
  for (int p = 0; p < n; ++p) {
    if (s_sup[p]) continue;                                      // uniform: LDS value read by all threads
    if (t == 0) { keep_idx[(size_t)c * M + s_keep] = s_idx[p]; s_keep++; }
    const float* bp = boxes + (size_t)s_idx[p] * 9;
    for (int q = p + 1 + t; q < n; q += 256)
      if (!s_sup[q] && iou_bev(bp, boxes + (size_t)s_idx[q] * 9) > (double)iou_thr) s_sup[q] = 1;
    __syncthreads();
  }
  if (t == 0) keep_cnt[c] = s_keep;
}
extern "C" int es_nms3d_multiclass(const float* boxes, const float* scores, int M, int C, float score_thr, float iou_thr,
                                   int* keep_idx, int* keep_cnt, void* stream) {
  if (C <= 0) return 0;
  if (M > NMS_CAP) return -10;
  hipLaunchKernelGGL(k_nms3d_multiclass, dim3(C), dim3(256), 0, (hipStream_t)stream, boxes, scores, M, C, score_thr,
                     iou_thr, keep_idx, keep_cnt);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ overlays on the recording's frames
// Predictions drawn onto the u8 frames the model consumed: 9-DoF boxes (es_render_project + es_render_boxes) and an occupancy
// volume (es_render_occupancy).  Every decision is int32 / int64 arithmetic or plain f64 (+ - * / floor, compares; no FMA
// contraction in this build), there are no atomics and no f32 arithmetic: tests/render_spec.py restates each kernel and the
// output is held to it byte for byte.  The only library calls are the six f64 cos / sin of a box's Euler angles; the spec keeps
// every projected coordinate 1e-6 away from a rounding boundary, which absorbs their last-bit differences.
#define RND_TW 64                  // a workgroup owns RND_TH rows of RND_TW pixels: one wave per row, 192 contiguous bytes per row
#define RND_TH 4
#define RND_CHUNK 64               // box records staged through LDS per round: one lane of wave 0 per record
#define RND_MAX 4096               // H, W and the guard band |u|, |v| <= RND_MAX
#define RND_SKIP 256               // mask bit: the camera centre lies inside the box

// Box i seen from view v -> rec[(v*n + i)*ES_RENDER_REC ...] (layout: include/es_hip.h).  Operation order, all f64:
//   half = dims * 0.5;  R = Rz(a) Rx(b) Ry(g) as make_box of ground.hip (columns = the box axes)
//   C_j  = -((E[0][j]*E[0][3] + E[1][j]*E[1][3]) + E[2][j]*E[2][3]);  d = C - centre;  loc_j = (R[0][j]*d0 + R[1][j]*d1) + R[2][j]*d2
//   skip = |loc_j| <= half_j for j = 0, 1, 2
//   corner c: l_a = bit a of c ? half_a : -half_a;  X_i = centre_i + ((R[i][0]*l0 + R[i][1]*l1) + R[i][2]*l2)
//   cam_i = ((E[i][0]*X0 + E[i][1]*X1) + E[i][2]*X2) + E[i][3];  z = cam_2
//   p_r = ((K[r][0]*cam0 + K[r][1]*cam1) + K[r][2]*cam2) + K[r][3] for r = 0, 1;  u = p_0 / z, v = p_1 / z  (only where z >= 1e-4)
//   usable = z >= 1e-4 and -4096 <= u <= 4096 and -4096 <= v <= 4096;  q = (int)floor(4*u + 0.5), (int)floor(4*v + 0.5), else 0, 0
__global__ void k_render_project(const float* __restrict__ boxes, int n, const float* __restrict__ ext,
                                 const float* __restrict__ intr, int V, int* __restrict__ rec) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= V * n) return;
  const int v = t / n, i = t - v * n;
  const float* b = boxes + (size_t)i * 9;
  const float* E = ext + (size_t)v * 16;
  const float* K = intr + (size_t)v * 16;
  const double c[3] = {b[0], b[1], b[2]};
  const double h[3] = {(double)b[3] * 0.5, (double)b[4] * 0.5, (double)b[5] * 0.5};
  const double ca = cos((double)b[6]), sa = sin((double)b[6]), cb = cos((double)b[7]), sb = sin((double)b[7]);
  const double cc = cos((double)b[8]), sc = sin((double)b[8]);
  const double R[3][3] = {{ca * cc - sa * sb * sc, -(sa * cb), ca * sc + sa * sb * cc},
                          {sa * cc + ca * sb * sc, ca * cb, sa * sc - ca * sb * cc},
                          {-(cb * sc), sb, cb * cc}};
  double e[3][4];
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 4; ++k) e[r][k] = (double)E[r * 4 + k];
  double d[3];
  for (int j = 0; j < 3; ++j) d[j] = -((e[0][j] * e[0][3] + e[1][j] * e[1][3]) + e[2][j] * e[2][3]) - c[j];
  bool inside = true;
  for (int j = 0; j < 3; ++j) {
    const double loc = (R[0][j] * d[0] + R[1][j] * d[1]) + R[2][j] * d[2];
    inside = inside && (loc <= h[j]) && (loc >= -h[j]);
  }
  int* o = rec + (size_t)t * ES_RENDER_REC;
  int mask = inside ? RND_SKIP : 0;
  int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = -0x7fffffff - 1, by1 = -0x7fffffff - 1;
  for (int k = 0; k < 8; ++k) {
    const double l0 = (k & 1) ? h[0] : -h[0], l1 = (k & 2) ? h[1] : -h[1], l2 = (k & 4) ? h[2] : -h[2];
    double X[3], cam[3];
    for (int r = 0; r < 3; ++r) X[r] = c[r] + ((R[r][0] * l0 + R[r][1] * l1) + R[r][2] * l2);
    for (int r = 0; r < 3; ++r) cam[r] = ((e[r][0] * X[0] + e[r][1] * X[1]) + e[r][2] * X[2]) + e[r][3];
    const double z = cam[2];
    int qx = 0, qy = 0;
    if (z >= 1e-4) {
      const double u = (((double)K[0] * cam[0] + (double)K[1] * cam[1]) + (double)K[2] * cam[2] + (double)K[3]) / z;
      const double w = (((double)K[4] * cam[0] + (double)K[5] * cam[1]) + (double)K[6] * cam[2] + (double)K[7]) / z;
      if (u <= (double)RND_MAX && u >= -(double)RND_MAX && w <= (double)RND_MAX && w >= -(double)RND_MAX) {
        qx = (int)floor(4.0 * u + 0.5);
        qy = (int)floor(4.0 * w + 0.5);
        mask |= 1 << k;
        bx0 = min(bx0, qx); bx1 = max(bx1, qx); by0 = min(by0, qy); by1 = max(by1, qy);
      }
    }
    o[2 * k] = qx;
    o[2 * k + 1] = qy;
  }
  o[16] = mask;
  o[17] = bx0; o[18] = by0; o[19] = bx1; o[20] = by1;
  o[21] = 0; o[22] = 0; o[23] = 0;
}

// (byte loads / stores on purpose: the 192-byte row of a wave moved as 48 dwords with lane shuffles measured SLOWER)
__device__ inline void rnd_load(const unsigned char* src, int chw, int v, int H, int W, int y, int x, int& r, int& g, int& b) {
  if (chw) {
    const size_t pl = (size_t)H * W, p = (size_t)v * 3 * pl + (size_t)y * W + x;
    r = src[p]; g = src[p + pl]; b = src[p + 2 * pl];
  } else {
    const size_t p = (((size_t)v * H + y) * W + x) * 3;
    r = src[p]; g = src[p + 1]; b = src[p + 2];
  }
}
__device__ inline void rnd_store(unsigned char* dst, int v, int H, int W, int y, int x, int r, int g, int b) {
  const size_t p = (((size_t)v * H + y) * W + x) * 3;
  dst[p] = (unsigned char)r; dst[p + 1] = (unsigned char)g; dst[p + 2] = (unsigned char)b;
}
__device__ inline int rnd_blend(int c, int col, int alpha) { return (c * alpha + col * (256 - alpha) + 128) >> 8; }

// edge (lo, a): from corner lo (bit a clear) to lo | 1 << a; its slot = a * 4 + (lo with bit a squeezed out)
__host__ __device__ constexpr int rnd_edge(int lo, int a) { return a * 4 + (a == 0 ? lo >> 1 : a == 1 ? ((lo & 1) | ((lo >> 2) << 1)) : (lo & 3)); }

// Pixel (x, y) has the centre (px, py) = (4x + 2, 4y + 2) in quarter-pixels.  Boxes in ascending row order; for box i:
//   edge (A -> B drawable: both ends usable): d = B - A, e = P - A, cross = d.x*e.y - d.y*e.x, dot = d.x*e.x + d.y*e.y, len2 = d.d (int64)
//     near = dot <= 0 ? e.e <= r^2 : dot >= len2 ? (e - d).(e - d) <= r^2 : cross^2 <= r^2 * len2        (len2 = 0: the disc round A)
//   face (fixed axis a at s, other axes b < c; P0 = s << a, P1 = P0 | 1 << b, P2 = P1 | 1 << c, P3 = P0 | 1 << c; all four usable):
//     f0 = cross(P0 -> P1), f1 = cross(P1 -> P2), f2 = cross(P2 -> P3) = -cross(P3 -> P2), f3 = cross(P3 -> P0) = -cross(P0 -> P3)
//     covered = (all f >= 0 or all f <= 0) and not all f == 0
//   any edge near: c = colour_i;  else any face covered: c = (c*alpha + colour_i*(256 - alpha) + 128) >> 8 per channel
// A record whose rectangle (grown by radius_q) misses the tile's pixel centres, or with the skip bit, or with no usable corner, is
// dropped by wave 0's ballot before the pixel loop -- a face lies inside the rectangle of its corners and a near edge inside the
// grown one, so the cull changes no byte -- and the surviving records keep their order.
__global__ __launch_bounds__(RND_TW * RND_TH) void k_render_boxes(const unsigned char* src, int chw, int H, int W,
                                                                  const int* __restrict__ rec, const unsigned char* __restrict__ colors,
                                                                  int n, int radius_q, int alpha, unsigned char* dst /* may be src */) {
  __shared__ int s_rec[RND_CHUNK][18];            // 16 coordinates, the usable mask, the colour
  __shared__ int s_cnt;
  const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
  const int v = blockIdx.z, x0 = blockIdx.x * RND_TW, y0 = blockIdx.y * RND_TH;
  const int x = x0 + lane, y = y0 + row;
  const bool live = x < W && y < H;
  int cr = 0, cg = 0, cbl = 0;
  if (live) rnd_load(src, chw, v, H, W, y, x, cr, cg, cbl);
  const int px = 4 * x + 2, py = 4 * y + 2;
  const int tx0 = 4 * x0 + 2, tx1 = 4 * min(x0 + RND_TW - 1, W - 1) + 2, ty0 = 4 * y0 + 2, ty1 = 4 * min(y0 + RND_TH - 1, H - 1) + 2;
  const long long r2 = (long long)radius_q * radius_q;
  for (int base = 0; base < n; base += RND_CHUNK) {
    __syncthreads();                              // the previous round's readers are done with s_rec
    if (row == 0) {
      const int i = base + lane;
      const int* rc = rec + ((size_t)v * n + min(i, n - 1)) * ES_RENDER_REC;
      bool keep = false;
      if (i < n) {
        const int m = rc[16];
        keep = !(m & RND_SKIP) && (m & 255) && rc[17] - radius_q <= tx1 && rc[19] + radius_q >= tx0 && rc[18] - radius_q <= ty1 &&
               rc[20] + radius_q >= ty0;
      }
      const unsigned long long bal = __ballot(keep);
      if (keep) {
        const int k = __popcll(bal & ((1ull << lane) - 1ull));
        for (int j = 0; j < 17; ++j) s_rec[k][j] = rc[j];
        s_rec[k][17] = (int)colors[(size_t)i * 3] | ((int)colors[(size_t)i * 3 + 1] << 8) | ((int)colors[(size_t)i * 3 + 2] << 16);
      }
      if (lane == 0) s_cnt = __popcll(bal);
    }
    __syncthreads();
    const int cnt = s_cnt;
    for (int k = 0; k < cnt; ++k) {               // uniform over the workgroup: every branch on the mask below is too
      const int* q = s_rec[k];
      const int m = q[16];
      long long cross[12];
      bool near = false, covered = false;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int lo = 0; lo < 8; ++lo) {
          if (lo & (1 << a)) continue;
          const int hi = lo | (1 << a), e = rnd_edge(lo, a);
          cross[e] = 0;
          if ((m >> lo) & (m >> hi) & 1) {
            const int ax = q[2 * lo], ay = q[2 * lo + 1];
            const int dx = q[2 * hi] - ax, dy = q[2 * hi + 1] - ay, ex = px - ax, ey = py - ay;
            const long long c = (long long)dx * ey - (long long)dy * ex;
            const long long dot = (long long)dx * ex + (long long)dy * ey, len2 = (long long)dx * dx + (long long)dy * dy;
            const int fx = ex - dx, fy = ey - dy;
            const bool hit = dot <= 0 ? ((long long)ex * ex + (long long)ey * ey <= r2)
                                      : dot >= len2 ? ((long long)fx * fx + (long long)fy * fy <= r2) : (c * c <= r2 * len2);
            cross[e] = c;
            near = near || hit;
          }
        }
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int bb = a == 0 ? 1 : 0, cx = a == 2 ? 1 : 2;
          const int p0 = s << a, p1 = p0 | (1 << bb), p2 = p1 | (1 << cx), p3 = p0 | (1 << cx);
          const int fm = (1 << p0) | (1 << p1) | (1 << p2) | (1 << p3);
          if ((m & fm) == fm) {
            const long long f0 = cross[rnd_edge(p0, bb)], f1 = cross[rnd_edge(p1, cx)], f2 = -cross[rnd_edge(p3, bb)],
                            f3 = -cross[rnd_edge(p0, cx)];
            const bool in = ((f0 >= 0 && f1 >= 0 && f2 >= 0 && f3 >= 0) || (f0 <= 0 && f1 <= 0 && f2 <= 0 && f3 <= 0)) &&
                            (f0 | f1 | f2 | f3) != 0;
            covered = covered || in;
          }
        }
      const int col = q[17], r = col & 255, g = (col >> 8) & 255, b = (col >> 16) & 255;
      if (near) { cr = r; cg = g; cbl = b; }
      else if (covered) { cr = rnd_blend(cr, r, alpha); cg = rnd_blend(cg, g, alpha); cbl = rnd_blend(cbl, b, alpha); }
    }
  }
  if (live) rnd_store(dst, v, H, W, y, x, cr, cg, cbl);
}

struct RndGrid { double rmin[3], size[3]; int n[3]; };
// One thread per pixel, f64 with + - * / floor and compares only.  M = rays[v][0..8] (row-major R^T K^-1), o = rays[v][9..11]:
//   d_i = (M[i][0]*(x + 0.5) + M[i][1]*(y + 0.5)) + M[i][2]
//   slab: tmin = 0, tmax = +inf, axis = 0; for i = 0, 1, 2: lo = rmin_i, hi = rmin_i + n_i*size_i;
//     d_i == 0: miss unless lo <= o_i < hi;  else t0 = (lo - o_i)/d_i, t1 = (hi - o_i)/d_i, swapped if t0 > t1;
//     t0 > tmin: tmin = t0, axis = i;  t1 < tmax: tmax = t1.          miss if tmin > tmax
//   entry: idx_i = clamp((int)floor(((o_i + tmin*d_i) - rmin_i) / size_i), 0, n_i - 1)
//   step_i = d_i > 0 ? 1 : d_i < 0 ? -1 : 0;  tnext_i = d_i == 0 ? +inf : ((rmin_i + (idx_i + (d_i > 0 ? 1 : 0))*size_i) - o_i)/d_i
//   dt_i = d_i == 0 ? +inf : size_i / (d_i > 0 ? d_i : -d_i)
//   at most X + Y + Z times: label = occ[idx]; 1 <= label < C: hit.  a = (tnext_0 <= tnext_1 and tnext_0 <= tnext_2) ? 0 :
//     tnext_1 <= tnext_2 ? 1 : 2;  idx_a += step_a; outside 0 .. n_a - 1: miss;  tnext_a += dt_a;  axis = a
//   hit: col = (palette[label] * shade[axis]) >> 8, shade = {256, 208, 160};  c = (c*alpha + col*(256 - alpha) + 128) >> 8
__global__ __launch_bounds__(RND_TW * RND_TH) void k_render_occupancy(const unsigned char* src, int chw, int H, int W,
                                                                      const double* __restrict__ rays, const unsigned char* __restrict__ occ,
                                                                      RndGrid G, const unsigned char* __restrict__ palette, int C, int alpha,
                                                                      unsigned char* dst /* may be src */) {
  const int lane = threadIdx.x & 63, row = threadIdx.x >> 6;
  const int v = blockIdx.z, x = blockIdx.x * RND_TW + lane, y = blockIdx.y * RND_TH + row;
  if (x >= W || y >= H) return;
  int cr, cg, cbl;
  rnd_load(src, chw, v, H, W, y, x, cr, cg, cbl);
  const double* M = rays + (size_t)v * 12;
  const double fx = (double)x + 0.5, fy = (double)y + 0.5, inf = __builtin_inf();
  double d[3], o[3];
  for (int i = 0; i < 3; ++i) { d[i] = (M[i * 3] * fx + M[i * 3 + 1] * fy) + M[i * 3 + 2]; o[i] = M[9 + i]; }
  double tmin = 0.0, tmax = inf;
  int axis = 0;
  bool miss = false;
  for (int i = 0; i < 3; ++i) {
    const double lo = G.rmin[i], hi = G.rmin[i] + (double)G.n[i] * G.size[i];
    if (d[i] == 0.0) {
      if (!(o[i] >= lo && o[i] < hi)) miss = true;
    } else {
      double t0 = (lo - o[i]) / d[i], t1 = (hi - o[i]) / d[i];
      if (t0 > t1) { const double s = t0; t0 = t1; t1 = s; }
      if (t0 > tmin) { tmin = t0; axis = i; }
      if (t1 < tmax) tmax = t1;
    }
  }
  if (!(tmin <= tmax)) miss = true;
  int label = 0;
  if (!miss) {
    int idx[3], step[3];
    double tnext[3], dt[3];
    for (int i = 0; i < 3; ++i) {
      int k = (int)floor(((o[i] + tmin * d[i]) - G.rmin[i]) / G.size[i]);
      k = k < 0 ? 0 : k > G.n[i] - 1 ? G.n[i] - 1 : k;
      idx[i] = k;
      step[i] = d[i] > 0.0 ? 1 : d[i] < 0.0 ? -1 : 0;
      tnext[i] = d[i] == 0.0 ? inf : ((G.rmin[i] + (double)(k + (d[i] > 0.0 ? 1 : 0)) * G.size[i]) - o[i]) / d[i];
      dt[i] = d[i] == 0.0 ? inf : G.size[i] / (d[i] > 0.0 ? d[i] : -d[i]);
    }
    const int steps = G.n[0] + G.n[1] + G.n[2];
    for (int s = 0; s < steps; ++s) {
      const int l = occ[((size_t)idx[0] * G.n[1] + idx[1]) * G.n[2] + idx[2]];
      if (l >= 1 && l < C) { label = l; break; }
      const int a = (tnext[0] <= tnext[1] && tnext[0] <= tnext[2]) ? 0 : (tnext[1] <= tnext[2]) ? 1 : 2;
      const int k = (a == 0 ? idx[0] : a == 1 ? idx[1] : idx[2]) + (a == 0 ? step[0] : a == 1 ? step[1] : step[2]);
      if (k < 0 || k > (a == 0 ? G.n[0] : a == 1 ? G.n[1] : G.n[2]) - 1) break;
      if (a == 0) { idx[0] = k; tnext[0] += dt[0]; } else if (a == 1) { idx[1] = k; tnext[1] += dt[1]; } else { idx[2] = k; tnext[2] += dt[2]; }
      axis = a;
    }
  }
  if (label) {
    const int shade = axis == 0 ? 256 : axis == 1 ? 208 : 160;
    cr = rnd_blend(cr, ((int)palette[label * 3] * shade) >> 8, alpha);
    cg = rnd_blend(cg, ((int)palette[label * 3 + 1] * shade) >> 8, alpha);
    cbl = rnd_blend(cbl, ((int)palette[label * 3 + 2] * shade) >> 8, alpha);
  }
  rnd_store(dst, v, H, W, y, x, cr, cg, cbl);
}

static inline bool rnd_frame_ok(int H, int W) { return H >= 1 && H <= RND_MAX && W >= 1 && W <= RND_MAX; }
extern "C" int es_render_project(const float* boxes, int n, const float* extrinsic, const float* intrinsic, int V, int H, int W, int* rec,
                                 void* stream) {
  if (n < 0 || V < 0) return -5;
  if (!rnd_frame_ok(H, W) || V > 65535 || (long long)V * n > (1ll << 30)) return -4;
  if (n == 0 || V == 0) return 0;
  hipLaunchKernelGGL(k_render_project, dim3(es_cdiv((long long)V * n, 64)), dim3(64), 0, (hipStream_t)stream, boxes, n, extrinsic,
                     intrinsic, V, rec);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_render_boxes(const unsigned char* src, int chw, int V, int H, int W, const int* rec, const unsigned char* colors, int n,
                               int radius_q, int alpha, unsigned char* dst, void* stream) {
  if (n < 0 || V < 0) return -5;
  if (!rnd_frame_ok(H, W) || V > 65535 || (long long)V * n > (1ll << 30) || radius_q < 1 || radius_q > 64 || alpha < 0 || alpha > 256 ||
      (chw && (const void*)src == (const void*)dst))
    return -4;
  if (V == 0) return 0;
  hipLaunchKernelGGL(k_render_boxes, dim3(es_cdiv(W, RND_TW), es_cdiv(H, RND_TH), V), dim3(RND_TW * RND_TH), 0, (hipStream_t)stream, src,
                     chw, H, W, rec, colors, n, radius_q, alpha, dst);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_render_occupancy(const unsigned char* src, int chw, int V, int H, int W, const double* rays, const unsigned char* occ, int X,
                                   int Y, int Z, const double* grid_host, const unsigned char* palette, int C, int alpha,
                                   unsigned char* dst, void* stream) {
  if (V < 0) return -5;
  if (!rnd_frame_ok(H, W) || V > 65535 || alpha < 0 || alpha > 256 || C < 1 || C > 256 || X < 1 || Y < 1 || Z < 1 ||
      (long long)X * Y * Z > (1ll << 30) || (chw && (const void*)src == (const void*)dst))
    return -4;
  if (V == 0) return 0;
  RndGrid G;
  for (int i = 0; i < 3; ++i) { G.rmin[i] = grid_host[i]; G.size[i] = grid_host[3 + i]; }
  G.n[0] = X; G.n[1] = Y; G.n[2] = Z;
  hipLaunchKernelGGL(k_render_occupancy, dim3(es_cdiv(W, RND_TW), es_cdiv(H, RND_TH), V), dim3(RND_TW * RND_TH), 0, (hipStream_t)stream,
                     src, chw, H, W, rays, occ, G, palette, C, alpha, dst);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ the scene seen from above
// A bird's-eye map of the aligned frame: Wm x Hm cells of `cell` metres, lower-left corner (x0, y0), image row = Hm - 1 - iy (+y up).
// es_map_splat z-buffers the recording's own depth pixels from above into one u64 key per cell, es_map_resolve turns the keys into an
// image (and a height map), es_map_project writes the ES_RENDER_REC record of a box for the orthographic view -- k_render_boxes then draws
// footprints and the camera trail unchanged -- and es_map_occupancy blends the top surface of a label volume.  As above: int32 / int64
// and plain f64 only; the one atomic is an integer max, which does not depend on arrival order.  tests/scene_map_spec.py restates all four.
struct MapGrid { double x0, y0, cell, zmin, zmax, maxd; int Wm, Hm, nz; };

// One thread per depth pixel (x, y) of view v, f64.  M = rays[v][0..8] (row-major R^T K^-1 at the DEPTH maps' resolution), c = rays[v][9..11]:
//   d = (double)depth[v][y][x];  kept iff d > 0 and d <= max_depth   (drops NaN, +-inf, 0 and negatives)
//   r_k = (M[k][0]*x + M[k][1]*y) + M[k][2];  p_k = c_k + d*r_k      ((x, y, 1), no half pixel: the cloud of k_depth_to_points)
//   kept iff p_z >= z_min and p_z < z_max;  zq = (int)floor((p_z - z_min) * 1024)
//   fx = floor((p_x - x0) / cell), fy = floor((p_y - y0) / cell);  kept iff 0 <= fx < Wm and 0 <= fy < Hm, compared in f64
//   colour = frame pixel (cx, cy) = ((2x + 1)*w / (2W), (2y + 1)*h / (2H)), integer division
//   key = (u64)(zq + 1) << 24 | r << 16 | g << 8 | b;  keys[(Hm - 1 - fy)*Wm + fx] = max(itself, key)
// The cell is read first (relaxed, agent scope) and the atomic is skipped when it already holds at least our key: a stale value can only
// be too small, so no key that should win is ever skipped.  Measured against the same kernel without the load: 1.27 x on an
// empty map, 5.3 x on a map that already holds the scene -- most pixels lose -- with bit-equal keys; the variant without it is gone.
__global__ __launch_bounds__(256) void k_map_splat(const float* __restrict__ depth, int H, int W, const unsigned char* __restrict__ frames,
                                                   int chw, int h, int w, const double* __restrict__ rays, MapGrid G,
                                                   unsigned long long* keys) {
  const int v = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int y = p / W, x = p - y * W;
  const double d = (double)depth[(size_t)v * H * W + p];
  if (!(d > 0.0 && d <= G.maxd)) return;
  const double* M = rays + (size_t)v * 12;
  const double fx = (double)x, fy = (double)y;
  double q[3];
  for (int k = 0; k < 3; ++k) q[k] = M[9 + k] + d * ((M[k * 3] * fx + M[k * 3 + 1] * fy) + M[k * 3 + 2]);
  if (!(q[2] >= G.zmin && q[2] < G.zmax)) return;
  const int zq = (int)floor((q[2] - G.zmin) * 1024.0);
  const double cx = floor((q[0] - G.x0) / G.cell), cy = floor((q[1] - G.y0) / G.cell);
  if (!(cx >= 0.0 && cx < (double)G.Wm && cy >= 0.0 && cy < (double)G.Hm)) return;
  const int ix = (int)cx, iy = (int)cy;
  int r, g, b;
  rnd_load(frames, chw, v, h, w, ((2 * y + 1) * h) / (2 * H), ((2 * x + 1) * w) / (2 * W), r, g, b);
  const unsigned long long key = ((unsigned long long)(zq + 1) << 24) | ((unsigned long long)r << 16) | ((unsigned long long)g << 8) |
                                 (unsigned long long)b;
  unsigned long long* cellp = keys + (size_t)(G.Hm - 1 - iy) * G.Wm + ix;
  if (__hip_atomic_load(cellp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= key) return;
  atomicMax(cellp, key);
}

// One thread per cell, tiled as k_render_boxes.  key == 0: background.  Else zq = (key >> 24) - 1, c = the three colour bytes;
//   shade != 0: c = (c*s + 128) >> 8, s = 160 + (96 * min(zq, span)) / span, span = max(1, nz - 1), nz = ceil((z_max - z_min) * 1024)
//   height != NULL: (float)(z_min + (zq + 0.5) / 1024), NaN for an empty cell;  image == NULL: only the height map is written
__global__ __launch_bounds__(RND_TW * RND_TH) void k_map_resolve(const unsigned long long* __restrict__ keys, MapGrid G, int bg, int shade,
                                                                 unsigned char* __restrict__ image, float* __restrict__ height) {
  const int x = blockIdx.x * RND_TW + (threadIdx.x & 63), y = blockIdx.y * RND_TH + (threadIdx.x >> 6);
  if (x >= G.Wm || y >= G.Hm) return;
  const unsigned long long key = keys[(size_t)y * G.Wm + x];
  int r = (bg >> 16) & 255, g = (bg >> 8) & 255, b = bg & 255;
  float hz = __builtin_nanf("");
  if (key) {
    const int zq = (int)(key >> 24) - 1;
    r = (int)(key >> 16) & 255; g = (int)(key >> 8) & 255; b = (int)key & 255;
    if (shade) {
      const int span = max(1, G.nz - 1), s = 160 + (96 * min(zq, span)) / span;
      r = (r * s + 128) >> 8; g = (g * s + 128) >> 8; b = (b * s + 128) >> 8;
    }
    hz = (float)(G.zmin + ((double)zq + 0.5) / 1024.0);
  }
  if (image) rnd_store(image, 0, G.Hm, G.Wm, y, x, r, g, b);
  if (height) height[(size_t)y * G.Wm + x] = hz;
}

// One thread per box, f64: the record of k_render_project for the orthographic view from above.  half, R and the corner order as there;
//   X_i = centre_i + ((R[i][0]*l0 + R[i][1]*l1) + R[i][2]*l2);  u = (X_0 - x0) / cell;  v = Hm - (X_1 - y0) / cell
//   usable = -4096 <= u <= 4096 and -4096 <= v <= 4096;  q = (int)floor(4*u + 0.5), (int)floor(4*v + 0.5), else 0, 0;  the skip bit is 0
__global__ void k_map_project(const float* __restrict__ boxes, int n, MapGrid G, int* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* b = boxes + (size_t)i * 9;
  const double c[3] = {b[0], b[1], b[2]};
  const double h[3] = {(double)b[3] * 0.5, (double)b[4] * 0.5, (double)b[5] * 0.5};
  const double ca = cos((double)b[6]), sa = sin((double)b[6]), cb = cos((double)b[7]), sb = sin((double)b[7]);
  const double cc = cos((double)b[8]), sc = sin((double)b[8]);
  const double R[2][3] = {{ca * cc - sa * sb * sc, -(sa * cb), ca * sc + sa * sb * cc}, {sa * cc + ca * sb * sc, ca * cb, sa * sc - ca * sb * cc}};
  int* o = rec + (size_t)i * ES_RENDER_REC;
  int mask = 0;
  int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = -0x7fffffff - 1, by1 = -0x7fffffff - 1;
  for (int k = 0; k < 8; ++k) {
    const double l0 = (k & 1) ? h[0] : -h[0], l1 = (k & 2) ? h[1] : -h[1], l2 = (k & 4) ? h[2] : -h[2];
    const double X = c[0] + ((R[0][0] * l0 + R[0][1] * l1) + R[0][2] * l2), Y = c[1] + ((R[1][0] * l0 + R[1][1] * l1) + R[1][2] * l2);
    const double u = (X - G.x0) / G.cell, w = (double)G.Hm - (Y - G.y0) / G.cell;
    int qx = 0, qy = 0;
    if (u <= (double)RND_MAX && u >= -(double)RND_MAX && w <= (double)RND_MAX && w >= -(double)RND_MAX) {
      qx = (int)floor(4.0 * u + 0.5);
      qy = (int)floor(4.0 * w + 0.5);
      mask |= 1 << k;
      bx0 = min(bx0, qx); bx1 = max(bx1, qx); by0 = min(by0, qy); by1 = max(by1, qy);
    }
    o[2 * k] = qx;
    o[2 * k + 1] = qy;
  }
  o[16] = mask;
  o[17] = bx0; o[18] = by0; o[19] = bx1; o[20] = by1;
  o[21] = 0; o[22] = 0; o[23] = 0;
}

// One thread per map pixel (px, py), f64 compares: Xc = x0 + (px + 0.5)*cell, Yc = y0 + ((Hm - 1 - py) + 0.5)*cell;
//   i = floor((Xc - rmin_x) / size_x), j = floor((Yc - rmin_y) / size_y); accepted iff 0 <= i <= X - 1 and 0 <= j <= Y - 1
//   the highest k with 1 <= occ[i][j][k] < C: c = (c*alpha + palette[label]*(256 - alpha) + 128) >> 8;  no such k: nothing is written
__global__ __launch_bounds__(RND_TW * RND_TH) void k_map_occupancy(unsigned char* image, MapGrid G, const unsigned char* __restrict__ occ,
                                                                   RndGrid O, const unsigned char* __restrict__ palette, int C, int alpha) {
  const int px = blockIdx.x * RND_TW + (threadIdx.x & 63), py = blockIdx.y * RND_TH + (threadIdx.x >> 6);
  if (px >= G.Wm || py >= G.Hm) return;
  const double Xc = G.x0 + ((double)px + 0.5) * G.cell, Yc = G.y0 + ((double)(G.Hm - 1 - py) + 0.5) * G.cell;
  const double fi = floor((Xc - O.rmin[0]) / O.size[0]), fj = floor((Yc - O.rmin[1]) / O.size[1]);
  if (!(fi >= 0.0 && fi <= (double)(O.n[0] - 1) && fj >= 0.0 && fj <= (double)(O.n[1] - 1))) return;
  const unsigned char* col = occ + ((size_t)(int)fi * O.n[1] + (int)fj) * O.n[2];
  int label = 0;
  for (int k = O.n[2] - 1; k >= 0; --k) {
    const int l = col[k];
    if (l >= 1 && l < C) { label = l; break; }
  }
  if (!label) return;
  int r, g, b;
  rnd_load(image, 0, 0, G.Hm, G.Wm, py, px, r, g, b);
  rnd_store(image, 0, G.Hm, G.Wm, py, px, rnd_blend(r, palette[label * 3], alpha), rnd_blend(g, palette[label * 3 + 1], alpha),
            rnd_blend(b, palette[label * 3 + 2], alpha));
}

// grid_host = x0, y0, cell, z_min, z_max, max_depth (f64, read on the host at the call)
static inline bool map_grid(const double* g, int Wm, int Hm, MapGrid& G) {
  G.x0 = g[0]; G.y0 = g[1]; G.cell = g[2]; G.zmin = g[3]; G.zmax = g[4]; G.maxd = g[5];
  G.Wm = Wm; G.Hm = Hm;
  if (!rnd_frame_ok(Hm, Wm) || !(G.cell > 0.0 && G.cell < __builtin_inf()) || !(G.zmax > G.zmin) || !(G.zmax - G.zmin <= 4096.0) || !(G.maxd > 0.0)) return false;
  G.nz = (int)ceil((G.zmax - G.zmin) * 1024.0);
  return true;
}
extern "C" int es_map_splat(const float* depth, int V, int H, int W, const unsigned char* frames, int chw, int h, int w, const double* rays,
                            const double* grid_host, int Wm, int Hm, long long* keys, void* stream) {
  MapGrid G;
  if (V < 0 || V > 65535 || !rnd_frame_ok(H, W) || !rnd_frame_ok(h, w) || !map_grid(grid_host, Wm, Hm, G)) return -4;
  if (V == 0) return 0;
  hipLaunchKernelGGL(k_map_splat, dim3(es_cdiv(H * W, 256), V), dim3(256), 0, (hipStream_t)stream, depth, H, W, frames, chw, h, w, rays, G,
                     (unsigned long long*)keys);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_map_resolve(const long long* keys, int Wm, int Hm, const double* grid_host, int background, int shade, unsigned char* image,
                              float* height, void* stream) {
  MapGrid G;
  if (!map_grid(grid_host, Wm, Hm, G) || background < 0 || background > 0xffffff || (!image && !height)) return -4;
  hipLaunchKernelGGL(k_map_resolve, dim3(es_cdiv(Wm, RND_TW), es_cdiv(Hm, RND_TH)), dim3(RND_TW * RND_TH), 0, (hipStream_t)stream,
                     (const unsigned long long*)keys, G, background, shade, image, height);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_map_project(const float* boxes, int n, const double* grid_host, int Wm, int Hm, int* rec, void* stream) {
  MapGrid G;
  if (n < 0 || n > (1 << 30) || !map_grid(grid_host, Wm, Hm, G)) return -4;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_map_project, dim3(es_cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, boxes, n, G, rec);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_map_occupancy(unsigned char* image, int Wm, int Hm, const double* grid_host, const unsigned char* occ, int X, int Y, int Z,
                                const double* volume_host, const unsigned char* palette, int C, int alpha, void* stream) {
  MapGrid G;
  if (!map_grid(grid_host, Wm, Hm, G) || alpha < 0 || alpha > 256 || C < 1 || C > 256 || X < 1 || Y < 1 || Z < 1 ||
      (long long)X * Y * Z > (1ll << 30) || !(volume_host[3] > 0.0) || !(volume_host[4] > 0.0))
    return -4;
  RndGrid O;
  for (int i = 0; i < 3; ++i) { O.rmin[i] = volume_host[i]; O.size[i] = volume_host[3 + i]; }
  O.n[0] = X; O.n[1] = Y; O.n[2] = Z;
  hipLaunchKernelGGL(k_map_occupancy, dim3(es_cdiv(Wm, RND_TW), es_cdiv(Hm, RND_TH)), dim3(RND_TW * RND_TH), 0, (hipStream_t)stream, image, G,
                     occ, O, palette, C, alpha);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ the scene in three dimensions
// The recording's depth pixels fused into ONE de-duplicated coloured cloud: es_cloud_splat inserts every pixel's voxel key into an open
// addressing table (tkeys / tvals / thits), es_cloud_mask marks the occupied slots with enough hits -- es_compact_mask and es_sort_u64
// then list them in ascending key order, whatever the table layout --, es_cloud_points turns the sorted rows into voxel centres, colours
// and hit counts, es_cloud_label gives every point the first 9-DoF box that holds it and every box its number of points, and
// es_occ_face_mask / es_occ_face_quads list the exposed faces of a label volume as quads.  As above: int32 / int64 and plain f64 only;
// the atomics are a CAS that can only turn -1 into a key, an integer max and integer adds, none of which depends on arrival order as
// long as no pixel is dropped (a dropped pixel is COUNTED: counters[1]).  tests/scene_cloud_spec.py restates all six.
struct CloudGrid { double cell, zmin, zmax, maxd; };

// One thread per depth pixel (x, y) of view v, f64.  d, p_k and the colour pixel exactly as k_map_splat; kept iff z_min <= p_z < z_max;
//   i_k = floor(p_k / cell), kept iff -2^17 <= i_k < 2^17 (compared in f64);  key = es_pack(0, i_x, i_y, i_z)
//   dq = (int)floor(d * 256);  val = (u64)(2^21 - dq) << 24 | r << 16 | g << 8 | b      (max_depth <= 4096: dq <= 2^20)
// Neighbouring pixels of an image row mostly fall into one voxel, so the lanes of a wave first combine their RUNS of equal keys: lane l
// starts a run when l == 0 or the key of lane l - 1 differs (a dropped pixel carries key -1: its runs are never inserted); the start
// lane takes the run's max val by a segmented shuffle reduction and its length from the boundary ballot, and alone probes the table:
//   s = es_hash(key, cap - 1); up to `probes` = min(64, cap) slots, linearly: CAS(tkeys[s], -1, key) returns -1 or key ->
//   tvals[s] = max(itself, val), thits[s] += length, done;  after the last probe the run is dropped and nothing is written for it.
// counters[0] / [1] += the wave's inserted / dropped pixels, one add per wave each (ballot + popcount).  Max and add are associative:
// the table bits equal those of one CAS / max / add per pixel (that variant was measured and is gone).  A slot is read
// before the CAS and the max (relaxed, agent scope): a key never changes once set and a stale val can only be too small.
__global__ __launch_bounds__(256) void k_cloud_splat(const float* __restrict__ depth, int H, int W, const unsigned char* __restrict__ frames,
                                                     int chw, int h, int w, const double* __restrict__ rays, CloudGrid G,
                                                     unsigned long long* tkeys, unsigned long long* tvals, unsigned int* thits,
                                                     uint32_t mask, int probes, unsigned int* counters) {
  const int v = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  long long key = -1;
  unsigned long long val = 0;
  if (p < H * W) {
    const int y = p / W, x = p - y * W;
    const double d = (double)depth[(size_t)v * H * W + p];
    if (d > 0.0 && d <= G.maxd) {
      const double* M = rays + (size_t)v * 12;
      const double fx = (double)x, fy = (double)y;
      double q[3], c[3];
      for (int k = 0; k < 3; ++k) q[k] = M[9 + k] + d * ((M[k * 3] * fx + M[k * 3 + 1] * fy) + M[k * 3 + 2]);
      for (int k = 0; k < 3; ++k) c[k] = floor(q[k] / G.cell);
      const double lo = -(double)ES_OFF, hi = (double)ES_OFF;
      if (q[2] >= G.zmin && q[2] < G.zmax && c[0] >= lo && c[0] < hi && c[1] >= lo && c[1] < hi && c[2] >= lo && c[2] < hi) {
        int r, g, b;
        rnd_load(frames, chw, v, h, w, ((2 * y + 1) * h) / (2 * H), ((2 * x + 1) * w) / (2 * W), r, g, b);
        const int dq = (int)floor(d * 256.0);
        key = es_pack(0, (int)c[0], (int)c[1], (int)c[2]);
        val = ((unsigned long long)((1 << 21) - dq) << 24) | ((unsigned long long)r << 16) | ((unsigned long long)g << 8) | (unsigned long long)b;
      }
    }
  }
  // every lane of the wave is here (no early return above): the run boundaries, then the run's max in its start lane
  const long long prev = __shfl_up(key, 1);
  const unsigned long long bounds = __ballot(lane == 0 || prev != key);
  const int start = 63 - __builtin_clzll(bounds & (~0ull >> (63 - lane)));
  const unsigned long long above = (bounds >> start) >> 1;
  const int end = above ? start + 1 + __builtin_ctzll(above) : 64;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long other = __shfl_down(val, o);
    if (lane + o < end && other > val) val = other;
  }
  int placed = 0;
  if (key >= 0 && lane == start) {
    uint32_t s = es_hash(key, mask);
    for (int it = 0; it < probes; ++it) {
      unsigned long long o = __hip_atomic_load(tkeys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (o == ~0ull) o = atomicCAS(tkeys + s, ~0ull, (unsigned long long)key);
      if (o == ~0ull || o == (unsigned long long)key) {
        if (__hip_atomic_load(tvals + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < val) atomicMax(tvals + s, val);
        atomicAdd(thits + s, (unsigned int)(end - start));
        placed = 1;
        break;
      }
      s = (s + 1) & mask;
    }
  }
  placed = __shfl(placed, start);
  const unsigned long long in = __ballot(key >= 0 && placed), out = __ballot(key >= 0 && !placed);
  if (lane == 0) {
    if (in) atomicAdd(counters, (unsigned int)__popcll(in));
    if (out) atomicAdd(counters + 1, (unsigned int)__popcll(out));
  }
}

// mask[s] = 1 iff slot s holds a key and thits[s] >= min_hits, else 0
__global__ void k_cloud_mask(const long long* __restrict__ tkeys, const unsigned int* __restrict__ thits, int cap, unsigned int min_hits,
                             int* __restrict__ mask) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= cap) return;
  mask[s] = (tkeys[s] != ES_EMPTY_KEY && thits[s] >= min_hits) ? 1 : 0;
}

// Row j of the sorted cloud, slot s = src[j]: xyz = the voxel's centre (float)(((double)i_k + 0.5) * cell), rgb = the low three bytes of
// tvals[s], hits = min(thits[s], 2^31 - 1)
__global__ void k_cloud_points(const long long* __restrict__ keys, const int* __restrict__ src, int n,
                               const unsigned long long* __restrict__ tvals, const unsigned int* __restrict__ thits, double cell,
                               float* __restrict__ xyz, unsigned char* __restrict__ rgb, int* __restrict__ hits) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int b, i[3];
  es_unpack(keys[j], b, i[0], i[1], i[2]);
  const int s = src[j];
  const unsigned long long val = tvals[s];
  for (int k = 0; k < 3; ++k) xyz[(size_t)j * 3 + k] = (float)(((double)i[k] + 0.5) * cell);
  rgb[(size_t)j * 3] = (unsigned char)(val >> 16);
  rgb[(size_t)j * 3 + 1] = (unsigned char)(val >> 8);
  rgb[(size_t)j * 3 + 2] = (unsigned char)val;
  const unsigned int t = thits[s];
  hits[j] = t > 0x7fffffffu ? 0x7fffffff : (int)t;
}

// One thread per point, the boxes staged through LDS RND_CHUNK at a time (lane i of wave 0 stages box i of the chunk, f64: centre,
// half + grow, and R with half, R, cos / sin as k_render_project), so m is not limited by LDS.  dx = (double)p - c;
//   l_k = (R[0][k]*dx_0 + R[1][k]*dx_1) + R[2][k]*dx_2;  inside iff -(half_k + grow) <= l_k <= half_k + grow for k = 0, 1, 2
// label[i] = the smallest such j, else -1 (a point stops testing at its first hit); support[j] += 1 through a per-workgroup LDS count
// that is flushed once per chunk: integer adds only.
__global__ __launch_bounds__(256) void k_cloud_label(const float* __restrict__ xyz, int n, const float* __restrict__ boxes, int m, double grow,
                                                     int* __restrict__ label, int* __restrict__ support) {
  __shared__ double s_box[RND_CHUNK][15];
  __shared__ int s_cnt[RND_CHUNK];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double pt[3] = {0.0, 0.0, 0.0};
  if (i < n)
    for (int k = 0; k < 3; ++k) pt[k] = (double)xyz[(size_t)i * 3 + k];
  int found = -1;
  for (int j0 = 0; j0 < m; j0 += RND_CHUNK) {
    const int cnt = min(RND_CHUNK, m - j0);
    if ((int)threadIdx.x < cnt) {
      const float* b = boxes + (size_t)(j0 + threadIdx.x) * 9;
      double* o = s_box[threadIdx.x];
      const double ca = cos((double)b[6]), sa = sin((double)b[6]), cb = cos((double)b[7]), sb = sin((double)b[7]);
      const double cc = cos((double)b[8]), sc = sin((double)b[8]);
      for (int k = 0; k < 3; ++k) { o[k] = (double)b[k]; o[3 + k] = (double)b[3 + k] * 0.5 + grow; }
      o[6] = ca * cc - sa * sb * sc; o[7] = -(sa * cb); o[8] = ca * sc + sa * sb * cc;
      o[9] = sa * cc + ca * sb * sc; o[10] = ca * cb; o[11] = sa * sc - ca * sb * cc;
      o[12] = -(cb * sc); o[13] = sb; o[14] = cb * cc;
      s_cnt[threadIdx.x] = 0;
    }
    __syncthreads();
    if (i < n && found < 0) {
      for (int j = 0; j < cnt; ++j) {
        const double* o = s_box[j];
        const double dx[3] = {pt[0] - o[0], pt[1] - o[1], pt[2] - o[2]};
        bool inside = true;
        for (int k = 0; k < 3; ++k) {
          const double l = (o[6 + k] * dx[0] + o[9 + k] * dx[1]) + o[12 + k] * dx[2];
          inside = inside && (l <= o[3 + k]) && (l >= -o[3 + k]);
        }
        if (inside) { found = j0 + j; atomicAdd(&s_cnt[j], 1); break; }
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < cnt && s_cnt[threadIdx.x]) atomicAdd(support + j0 + threadIdx.x, s_cnt[threadIdx.x]);
    __syncthreads();
  }
  if (i < n) label[i] = found;
}

// Element e = 6 * ((i*Y + j)*Z + k) + f, f = -x, +x, -y, +y, -z, +z: set iff 1 <= occ[i][j][k] < C and the neighbour across face f lies
// outside the volume or holds no such label
__global__ void k_occ_face_mask(const unsigned char* __restrict__ occ, int X, int Y, int Z, int C, int* __restrict__ mask) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 6 * X * Y * Z) return;
  const int f = e % 6, cell = e / 6, k = cell % Z, j = (cell / Z) % Y, i = cell / (Y * Z);
  const int l = occ[cell];
  int set = 0;
  if (l >= 1 && l < C) {
    const int a = f >> 1, step = (f & 1) ? 1 : -1;
    const int ni = i + (a == 0 ? step : 0), nj = j + (a == 1 ? step : 0), nk = k + (a == 2 ? step : 0);
    set = 1;
    if (ni >= 0 && ni < X && nj >= 0 && nj < Y && nk >= 0 && nk < Z) {
      const int o = occ[((size_t)ni * Y + nj) * Z + nk];
      set = !(o >= 1 && o < C);
    }
  }
  mask[e] = set;
}

// the corners of face f as bits (x | y << 1 | z << 2) of the voxel's unit cube, counter-clockwise seen from outside, three bits per corner
#define OCC_QUAD(a, b, c, d) ((a) | (b) << 3 | (c) << 6 | (d) << 9)
__host__ __device__ constexpr int occ_face_corners(int f) {
  return f == 0 ? OCC_QUAD(0, 4, 6, 2) : f == 1 ? OCC_QUAD(1, 3, 7, 5) : f == 2 ? OCC_QUAD(0, 1, 5, 4) : f == 3 ? OCC_QUAD(2, 6, 7, 3)
       : f == 4 ? OCC_QUAD(0, 2, 3, 1) : OCC_QUAD(4, 5, 7, 6);
}

// Face row r = element e = src[r]: verts[4r + q][a] = (float)(rmin_a + (double)(index_a + bit_a) * size_a), face_label[r] = the voxel's label
__global__ void k_occ_face_quads(const unsigned char* __restrict__ occ, RndGrid O, const int* __restrict__ src, int n, float* __restrict__ verts,
                                 unsigned char* __restrict__ face_label) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int e = src[r], f = e % 6, cell = e / 6;
  const int idx[3] = {cell / (O.n[1] * O.n[2]), (cell / O.n[2]) % O.n[1], cell % O.n[2]};
  const int corners = occ_face_corners(f);
  for (int q = 0; q < 4; ++q) {
    const int bits = (corners >> (3 * q)) & 7;
    for (int a = 0; a < 3; ++a) verts[((size_t)r * 4 + q) * 3 + a] = (float)(O.rmin[a] + (double)(idx[a] + ((bits >> a) & 1)) * O.size[a]);
  }
  face_label[r] = occ[cell];
}

extern "C" int es_cloud_splat(const float* depth, int V, int H, int W, const unsigned char* frames, int chw, int h, int w, const double* rays,
                              const double* grid_host, int64_t* tkeys, uint64_t* tvals, unsigned int* thits, int cap, unsigned int* counters,
                              void* stream) {
  if (V < 0) return -5;
  CloudGrid G = {grid_host[0], grid_host[1], grid_host[2], grid_host[3]};
  if (V > 65535 || !rnd_frame_ok(H, W) || !rnd_frame_ok(h, w) || cap < 2 || cap > (1 << 30) || (cap & (cap - 1)) ||
      !(G.cell > 0.0 && G.cell < __builtin_inf()) || !(G.maxd > 0.0 && G.maxd <= 4096.0) || !(G.zmax > G.zmin))
    return -4;
  if (V == 0) return 0;
  hipLaunchKernelGGL(k_cloud_splat, dim3(es_cdiv(H * W, 256), V), dim3(256), 0, (hipStream_t)stream, depth, H, W, frames, chw, h, w, rays, G,
                     (unsigned long long*)tkeys, (unsigned long long*)tvals, thits, (uint32_t)cap - 1, cap < ES_CLOUD_PROBES ? cap : ES_CLOUD_PROBES,
                     counters);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_cloud_mask(const int64_t* tkeys, const unsigned int* thits, int cap, int min_hits, int* mask, void* stream) {
  if (cap < 2 || cap > (1 << 30) || (cap & (cap - 1)) || min_hits < 0) return -4;
  hipLaunchKernelGGL(k_cloud_mask, dim3(es_cdiv(cap, 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)tkeys, thits, cap,
                     (unsigned int)min_hits, mask);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_cloud_points(const int64_t* sorted_keys, const int* src, int n, const uint64_t* tvals, const unsigned int* thits, double cell,
                               float* xyz, unsigned char* rgb, int* hits, void* stream) {
  if (n < 0) return -5;
  if (n > (1 << 30) || !(cell > 0.0 && cell < __builtin_inf())) return -4;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_cloud_points, dim3(es_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, (const long long*)sorted_keys, src, n,
                     (const unsigned long long*)tvals, thits, cell, xyz, rgb, hits);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_cloud_label(const float* xyz, int n, const float* boxes, int m, double grow, int* label, int* support, void* stream) {
  if (n < 0 || m < 0) return -5;
  if (n > (1 << 30) || m > 65535 || !(grow >= 0.0 && grow < __builtin_inf())) return -4;
  if (m > 0) ES_TRY(hipMemsetAsync(support, 0, (size_t)m * 4, (hipStream_t)stream));
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_cloud_label, dim3(es_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, xyz, n, boxes, m, grow, label, support);
  ES_CHECK_LAUNCH();
  return 0;
}
static inline bool occ_volume_ok(int X, int Y, int Z) { return X >= 1 && Y >= 1 && Z >= 1 && 6ll * X * Y * Z <= (1ll << 30); }
extern "C" int es_occ_face_mask(const unsigned char* occ, int X, int Y, int Z, int C, int* mask, void* stream) {
  if (C < 1 || C > 256 || !occ_volume_ok(X, Y, Z)) return -4;
  hipLaunchKernelGGL(k_occ_face_mask, dim3(es_cdiv(6ll * X * Y * Z, 256)), dim3(256), 0, (hipStream_t)stream, occ, X, Y, Z, C, mask);
  ES_CHECK_LAUNCH();
  return 0;
}
extern "C" int es_occ_face_quads(const unsigned char* occ, int X, int Y, int Z, const double* vol_host, const int* src, int n, float* verts,
                                 unsigned char* face_label, void* stream) {
  if (n < 0) return -5;
  if (!occ_volume_ok(X, Y, Z) || n > 6ll * X * Y * Z) return -4;
  if (n == 0) return 0;
  RndGrid O;
  for (int i = 0; i < 3; ++i) { O.rmin[i] = vol_host[i]; O.size[i] = vol_host[3 + i]; }
  O.n[0] = X; O.n[1] = Y; O.n[2] = Z;
  hipLaunchKernelGGL(k_occ_face_quads, dim3(es_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, occ, O, src, n, verts, face_label);
  ES_CHECK_LAUNCH();
  return 0;
}
