// Grounding-side assignment and classification loss on the device (SURVEY 8a row A19 + 8f row N2):
//   * es_box3d_iou        : exact IoU of two oriented (9-DoF Euler ZXY) boxes -- EulerInstance3DBoxes.overlaps
//                           (structures/bbox_3d/euler_box3d.py:103-135 -> pytorch3d.ops.box3d_overlap), IoU3DCost
//                           (models/losses/match_cost.py:95-113);
//   * es_ground_match     : BinaryFocalLossCost + BBox3DL1Cost + IoU3DCost (match_cost.py:49-75,213-265), nan_to_num and
//                           the rectangular linear-sum-assignment of HungarianAssigner3D.assign
//                           (task_modules/assigners/hungarian_assigner.py:56-138; scipy.optimize.linear_sum_assignment)
//                           for every sample of a decoder layer in ONE launch -- the reference does a D2H copy and a scipy
//                           call per sample per layer;
//   * es_ground_focal     : GroundingHead._get_targets_single label construction + mmdet FocalLoss on the un-padded text
//                           tokens (dense_heads/grounding_head.py:365-425,717-748), value + gradient;
//   * es_topk_sorted      : per-sample top-k indices in descending score order (query selection,
//                           detectors/sparse_featfusion_grounder.py:374-376).
//   * es_det_best_gt / es_det_mark / es_det_ap : IndoorDetMetric on the device (8f row N5; eval/indoor_eval.py:8-182): best
//                           ground-truth box of every prediction inside its (scene, class) group, TP marking by the lowest
//                           rank that claims a box, and the area under the precision envelope per (class, threshold).
// All geometry and the assignment run in f64 (scipy casts the cost matrix to double as well).
//
// box3d_overlap: pytorch3d (un-vendored) clips the triangulated faces of each box against the other box and sums
// tetrahedra.  Here: the intersection polytope's faces lie in the 12 face planes of the two boxes; each face is that box
// face (a rectangle) clipped by the six half-spaces of the OTHER box (Sutherland-Hodgman in 3-D), and the volume follows
// from the divergence theorem  V = 1/3 sum_f (n_f . x_f) A_f.  Faces of A are clipped inclusively, faces of B exclusively,
// so a pair of coincident faces is counted once (and faces of two boxes that only touch contribute nothing).
#include "common.h"
#include "../../include/es_hip.h"

struct V3 { double x, y, z; };
__device__ inline V3 v3(double x, double y, double z) { V3 r = {x, y, z}; return r; }
__device__ inline V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ inline V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ inline V3 operator*(V3 a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ inline double dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline V3 cross3(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

struct OBox { V3 c; V3 ax[3]; double h[3]; };
// R = Rz(a) Rx(b) Ry(g) (pytorch3d euler_angles_to_matrix 'ZXY'); the box axes are R's columns
__device__ inline OBox make_box(const double* b) {
  OBox o;
  o.c = v3(b[0], b[1], b[2]);
  o.h[0] = b[3] * 0.5; o.h[1] = b[4] * 0.5; o.h[2] = b[5] * 0.5;
  double ca = cos(b[6]), sa = sin(b[6]), cb = cos(b[7]), sb = sin(b[7]), cc = cos(b[8]), sc = sin(b[8]);
  o.ax[0] = v3(ca * cc - sa * sb * sc, sa * cc + ca * sb * sc, -(cb * sc));
  o.ax[1] = v3(-(sa * cb), ca * cb, sb);
  o.ax[2] = v3(ca * sc + sa * sb * cc, sa * sc - ca * sb * cc, cb * cc);
  return o;
}
#define MAXV 16
// sum over the 6 faces of P (clipped by Q) of (n . (x - O)) * area
__device__ inline double faces_flux(const OBox& P, const OBox& Q, V3 O, bool inclusive) {
  double total = 0.0;
  for (int f = 0; f < 6; ++f) {
    const int j = f >> 1, k = (j + 1) % 3, l = (j + 2) % 3;
    const double sgn = (f & 1) ? -1.0 : 1.0;
    V3 n = P.ax[j] * sgn;
    V3 fc = P.c + P.ax[j] * (sgn * P.h[j]);
    V3 ek = P.ax[k] * P.h[k], el = P.ax[l] * P.h[l];
    V3 poly[MAXV], tmp[MAXV];
    int np = 4;
    poly[0] = fc + ek + el; poly[1] = fc - ek + el; poly[2] = fc - ek - el; poly[3] = fc + ek - el;
    for (int g = 0; g < 6 && np > 0; ++g) {
      const int jj = g >> 1;
      const double sg = (g & 1) ? -1.0 : 1.0;
      V3 m = Q.ax[jj] * sg;
      const double off = Q.h[jj];
      int nt = 0;
      for (int i = 0; i < np; ++i) {
        V3 a = poly[i], b = poly[(i + 1) % np];
        double da = dot3(m, a - Q.c) - off, db = dot3(m, b - Q.c) - off;
        // a vertex ON the clipping plane (|d| <= tol) is inside only for P = A's faces and only when the two planes face
        // the same way: coincident faces are then counted once, faces of two boxes that merely touch not at all
        const bool same = inclusive && dot3(m, n) > 0.5;
        bool ia = (da < -1e-12) || (same && da <= 1e-12), ib = (db < -1e-12) || (same && db <= 1e-12);
        if (ia) { if (nt < MAXV) tmp[nt++] = a; }
        if (ia != ib) {
          double t = da / (da - db);
          if (nt < MAXV) tmp[nt++] = a + (b - a) * t;
        }
      }
      np = nt;
      for (int i = 0; i < np; ++i) poly[i] = tmp[i];
    }
    if (np < 3) continue;
    V3 av = v3(0, 0, 0);
    for (int i = 1; i + 1 < np; ++i) av = av + cross3(poly[i] - poly[0], poly[i + 1] - poly[0]);
    double area = 0.5 * sqrt(dot3(av, av));
    total += dot3(n, fc - O) * area;
  }
  return total;
}
__device__ inline double box_iou3d(const double* a9, const double* b9) {
  OBox A = make_box(a9), B = make_box(b9);
  double va = a9[3] * a9[4] * a9[5], vb = b9[3] * b9[4] * b9[5];
  // quick reject on bounding spheres
  V3 d = A.c - B.c;
  double ra = sqrt(A.h[0] * A.h[0] + A.h[1] * A.h[1] + A.h[2] * A.h[2]), rb = sqrt(B.h[0] * B.h[0] + B.h[1] * B.h[1] + B.h[2] * B.h[2]);
  if (dot3(d, d) > (ra + rb) * (ra + rb)) return 0.0;
  double v = (faces_flux(A, B, A.c, true) + faces_flux(B, A, A.c, false)) / 3.0;
  if (v < 0.0) v = 0.0;
  return v / (va + vb - v);
}

__global__ void k_box3d_iou(const float* __restrict__ b1, int N, const float* __restrict__ b2, int M, float* __restrict__ iou) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * M) return;
  int i = e / M, j = e % M;
  double a[9], b[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) { a[c] = b1[(size_t)i * 9 + c]; b[c] = b2[(size_t)j * 9 + c]; }
  iou[e] = (float)box_iou3d(a, b);
}
extern "C" int es_box3d_iou(const float* boxes1, int N, const float* boxes2, int M, float* iou, void* stream) {
  if (N <= 0 || M <= 0) return 0;
  hipLaunchKernelGGL(k_box3d_iou, dim3(es_cdiv((long long)N * M, 64)), dim3(64), 0, (hipStream_t)stream, boxes1, N, boxes2, M, iou);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ scene inventory filter (demo/demo.py:84-130, nms_filter)
// The demo's object list: walk the rows by descending score (order = es_topk_sorted: ties to the lower row); skip a row whose class
// already holds topk_per_class kept rows, whose score is below score_thr, or whose 9-DoF IoU with ANY kept row (whatever its class)
// exceeds iou_thr; keep the others.  The reference builds the whole n x n matrix and loops on the host; here the greedy is
// sequential in the KEPT rows only: one workgroup holds a dead flag per sorted position and the class counters in LDS, and every
// kept row costs one pass over the later positions that are still alive -- iou(candidate, kept), the candidate as the first
// (inclusive) argument, rounded to f32 and compared in f32: the [candidate][kept] element es_box3d_iou stores.  A NaN IoU (a
// zero-volume pair) compares false and does not suppress.  Rows below the score threshold (a suffix after the sort), rows with a
// label outside [0, n_classes) and order entries outside [0, n) are dead from the start; m bounds the live positions.  A class's
// counter only grows, so a row met over quota is dead for good -- it never suppresses anything, exactly as in the reference.
// A pass has two phases.  One clipping takes a wave about 0.2 ms (f64, two 16-vertex polygons per lane in scratch), and a wave
// waits for its slowest lane, so lanes that walk their share of the positions and clip where they must make the pass as long as
// the number of loop trips in which SOME lane clips.  Phase 1 therefore only restates box_iou3d's bounding-sphere test -- the same
// f64 expressions on the same values, no FMA contraction in this file, so it rejects exactly the pairs box_iou3d returns 0.0 for --
// and collects the surviving positions in an LDS list (in arrival order: every entry is judged on its own, so the order does not
// reach the result); phase 2 deals the list out one entry per lane.
#define FILT_MAX 16384             // rows: what es_topk_sorted orders
#define FILT_MAX_CLS 4096
#define FILT_T 256
// the bounding-sphere radius as box_iou3d forms it: half sizes b[3..5] * 0.5, sqrt of the sum of their squares in that order
__device__ inline double filt_radius(const double* b) {
  const double h0 = b[3] * 0.5, h1 = b[4] * 0.5, h2 = b[5] * 0.5;
  return sqrt(h0 * h0 + h1 * h1 + h2 * h2);
}
__global__ __launch_bounds__(FILT_T) void k_box3d_iou_filter(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                             const int* __restrict__ labels, const int* __restrict__ order, int n,
                                                             int n_classes, float iou_thr, float score_thr, int topk,
                                                             int* __restrict__ keep_idx, int* __restrict__ keep_cnt) {
  __shared__ unsigned char s_dead[FILT_MAX];
  __shared__ unsigned short s_list[FILT_MAX];      // positions whose sphere meets the kept row's (a position is < 16384)
  __shared__ unsigned short s_cnt[FILT_MAX_CLS];   // kept rows per class (<= n <= 16384)
  __shared__ int s_first[FILT_T / 64];
  __shared__ int s_m, s_nlist;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int c = tid; c < n_classes; c += FILT_T) s_cnt[c] = 0;
  if (tid == 0) s_m = 0;
  __syncthreads();
  int mine = 0;
  for (int p = tid; p < n; p += FILT_T) {
    const int r = order[p];
    bool live = r >= 0 && r < n;
    if (live) {
      const int l = labels[r];
      live = l >= 0 && l < n_classes && !(scores[r] < score_thr);
    }
    s_dead[p] = live ? 0 : 1;
    if (live) mine = p + 1;
  }
  if (mine) atomicMax(&s_m, mine);
  __syncthreads();
  const int m = s_m;                       // one past the last live position
  int nk = 0, cur = 0;
  while (true) {
    // the first live position at or after `cur` whose class has room (the same value in every lane)
    int found = -1;
    for (int base = cur; base < m; base += FILT_T) {
      const int p = base + tid;
      bool ok = false;
      if (p < m && !s_dead[p]) {
        if ((int)s_cnt[labels[order[p]]] < topk) ok = true;
        else s_dead[p] = 1;
      }
      const unsigned long long bal = __ballot(ok);
      if (lane == 0) s_first[w] = bal ? base + w * 64 + __ffsll(bal) - 1 : 0x7fffffff;
      __syncthreads();
      int f = s_first[0];
#pragma unroll
      for (int k = 1; k < FILT_T / 64; ++k) f = min(f, s_first[k]);
      __syncthreads();                     // every lane has read s_first before the next chunk rewrites it
      if (f != 0x7fffffff) { found = f; break; }
    }
    if (found < 0) break;
    const int rk = order[found];
    if (tid == 0) { keep_idx[nk] = rk; s_cnt[labels[rk]] += 1; s_nlist = 0; }
    ++nk;
    __syncthreads();
    double kb[9], a[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) kb[c] = boxes[(size_t)rk * 9 + c];
    const V3 kc = v3(kb[0], kb[1], kb[2]);
    const double kr = filt_radius(kb);
    for (int p = found + 1 + tid; p < m; p += FILT_T) {
      if (s_dead[p]) continue;
      const int r = order[p];
      const V3 d = v3((double)boxes[(size_t)r * 9], (double)boxes[(size_t)r * 9 + 1], (double)boxes[(size_t)r * 9 + 2]) - kc;
      a[3] = boxes[(size_t)r * 9 + 3]; a[4] = boxes[(size_t)r * 9 + 4]; a[5] = boxes[(size_t)r * 9 + 5];
      const double rs = filt_radius(a) + kr;
      if (dot3(d, d) > rs * rs) {          // box_iou3d returns 0.0 here
        if (0.0f > iou_thr) s_dead[p] = 1;
      } else {
        s_list[atomicAdd(&s_nlist, 1)] = (unsigned short)p;
      }
    }
    __syncthreads();
    const int nl = s_nlist;
    for (int i = tid; i < nl; i += FILT_T) {
      const int p = s_list[i];
      const int r = order[p];
#pragma unroll
      for (int c = 0; c < 9; ++c) a[c] = boxes[(size_t)r * 9 + c];
      if ((float)box_iou3d(a, kb) > iou_thr) s_dead[p] = 1;
    }
    cur = found + 1;
    __syncthreads();                       // the flags, the counter and the list of this pass are settled before the next search
  }
  if (tid == 0) keep_cnt[0] = nk;
}
extern "C" int es_box3d_iou_filter(const float* boxes, const float* scores, const int* labels, const int* order, int n, int n_classes,
                                   float iou_thr, float score_thr, int topk_per_class, int* keep_idx, int* keep_cnt, void* stream) {
  if (n > FILT_MAX || n_classes < 1 || n_classes > FILT_MAX_CLS || topk_per_class < 1) return -4;
  if (n < 0) return -5;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    ES_TRY(hipMemsetAsync(keep_cnt, 0, sizeof(int), st));
    return 0;
  }
  hipLaunchKernelGGL(k_box3d_iou_filter, dim3(1), dim3(FILT_T), 0, st, boxes, scores, labels, order, n, n_classes, iou_thr, score_thr,
                     topk_per_class, keep_idx, keep_cnt);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ track table: one frame's detections against the tracks
// Stable identities over a walk (embodiedscan_amd/tracks.py; the reference has no tracker, the definition is include/es_hip.h's).
// iou (n, ld) is what es_box3d_iou(det_boxes, n, trk_boxes, m) stored: the clipping stays in that all-CU kernel, this one clips
// nothing.  A pair (j, i) is a candidate when i < min(m, n_tracks), the track is alive, iou[j][i] > iou_thr (f32, a NaN never is)
// and, with same_class, the labels agree.  The greedy walks the candidates by descending IoU, ties to the lower row, then the lower
// slot, and takes a pair whose two ends are free.  That order is strict and total, so the greedy equals repeated rounds of MUTUAL
// BEST pairs: a pair that is the best free candidate of its row and of its column is taken by the greedy before anything that shares
// an end with it, and taking it changes nothing for the other pairs of the round.  A round is parallel in the pairs: the key
// iou_bits << 32 | (2047 - j) << 12 | (4095 - i) (positive floats order like their bits) goes into rowbest[j] and colbest[i] by
// 64-bit LDS atomicMax, a pair is taken iff rowbest[j] == colbest[i] != 0, and the loop ends on a round that takes nothing (the
// largest key left is always mutual, so nothing is left then).  A free row without a candidate never gets one again (columns only
// leave) and is not scanned again: after the first round only the contested rows are read.  Then the unmatched rows are numbered in
// row order by a workgroup prefix sum (births), every row writes its track, and the tracks nobody matched age.
#define TRK_MAX_DET 2048
#define TRK_MAX_CAP 4096
#define TRK_T 1024
__global__ __launch_bounds__(TRK_T) void k_track_assign(const float* __restrict__ iou, int n, int m, int ld, const float* __restrict__ det_boxes,
                                                        const float* __restrict__ det_scores, const int* __restrict__ det_labels,
                                                        float* trk_boxes, float* trk_f, int* trk_i, int* counts, int cap, int t,
                                                        float iou_thr, int same_class, int max_age, int* __restrict__ det_track) {
  __shared__ unsigned long long s_rowbest[TRK_MAX_DET];    // 16 KB
  __shared__ unsigned long long s_colbest[TRK_MAX_CAP];    // 32 KB
  __shared__ short s_row[TRK_MAX_DET];                     // -1 free, -2 free for good (no candidate left), else the matched slot
  __shared__ unsigned char s_col[TRK_MAX_CAP];             // 0 not a column (dead), 1 free, 2 taken
  __shared__ int s_wcnt[TRK_T / 64];
  __shared__ int s_taken;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nt0 = min(max(counts[0], 0), cap);
  const int mm = min(m, nt0);                              // columns at or above hold whatever the host's bound left there
  for (int j = tid; j < n; j += TRK_T) s_row[j] = -1;
  for (int i = tid; i < mm; i += TRK_T) s_col[i] = trk_i[(size_t)i * 5 + 4] != 0 ? 1 : 0;
  __syncthreads();
  if (n > 0 && mm > 0) {
    while (true) {
      for (int j = tid; j < n; j += TRK_T) s_rowbest[j] = 0ull;
      for (int i = tid; i < mm; i += TRK_T) s_colbest[i] = 0ull;
      if (tid == 0) s_taken = 0;
      __syncthreads();
      for (int j = w; j < n; j += TRK_T / 64) {            // a wave per free row, its lanes along the columns
        if (s_row[j] != -1) continue;
        const float* __restrict__ row = iou + (size_t)j * ld;
        const int dl = same_class ? det_labels[j] : 0;
        unsigned long long best = 0ull;
        for (int i0 = lane; i0 < mm; i0 += 256) {
          float v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = i0 + 64 * u < mm ? row[i0 + 64 * u] : 0.f;     // (0 is no candidate: iou_thr >= 0)
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int i = i0 + 64 * u;
            if (!(v[u] > iou_thr) || s_col[i] != 1) continue;
            if (same_class && trk_i[(size_t)i * 5] != dl) continue;
            const unsigned long long key = ((unsigned long long)__float_as_uint(v[u]) << 32) | ((unsigned long long)(2047 - j) << 12) |
                                           (unsigned long long)(4095 - i);
            atomicMax(&s_colbest[i], key);
            if (key > best) best = key;
          }
        }
        if (best) atomicMax(&s_rowbest[j], best);
      }
      __syncthreads();
      for (int j = tid; j < n; j += TRK_T) {
        if (s_row[j] != -1) continue;
        const unsigned long long k = s_rowbest[j];
        if (!k) { s_row[j] = -2; continue; }
        const int i = 4095 - (int)(k & 4095ull);
        if (s_colbest[i] == k) { s_row[j] = (short)i; s_col[i] = 2; s_taken = 1; }
      }
      __syncthreads();
      const int taken = s_taken;
      __syncthreads();                                     // every lane has read s_taken before the next round clears it
      if (!taken) break;
    }
  }
  // matched rows update their track; unmatched rows are born in row order into nt0, nt0 + 1, ... while the table has room
  int born = 0;
  for (int base = 0; base < n; base += TRK_T) {
    const int j = base + tid;
    const int r = j < n ? (int)s_row[j] : 0;
    const bool un = j < n && r < 0;
    const unsigned long long bal = __ballot(un);
    if (lane == 0) s_wcnt[w] = __popcll(bal);
    __syncthreads();
    int before = born, total = 0;
#pragma unroll
    for (int k = 0; k < TRK_T / 64; ++k) {
      const int c = s_wcnt[k];
      if (k < w) before += c;
      total += c;
    }
    __syncthreads();                                       // every lane has read s_wcnt before the next chunk rewrites it
    born += total;
    if (j >= n) continue;
    int slot = r;
    if (un) {
      slot = nt0 + before + __popcll(bal & ((1ull << lane) - 1ull));
      if (slot >= cap) slot = -1;                          // the table is full: the detection is dropped
    }
    det_track[j] = slot;
    if (slot < 0) continue;
    const float sc = det_scores[j];
    const int lb = det_labels[j];
#pragma unroll
    for (int c = 0; c < 9; ++c) trk_boxes[(size_t)slot * 9 + c] = det_boxes[(size_t)j * 9 + c];
    trk_f[(size_t)slot * 2] = sc;
    int* ti = trk_i + (size_t)slot * 5;
    if (un) {
      trk_f[(size_t)slot * 2 + 1] = sc;
      ti[0] = lb; ti[1] = t; ti[2] = t; ti[3] = 1; ti[4] = 1;
    } else {
      if (sc >= trk_f[(size_t)slot * 2 + 1]) { trk_f[(size_t)slot * 2 + 1] = sc; ti[0] = lb; }
      ti[2] = t;
      ti[3] += 1;
    }
  }
  // ageing, after the births: a track matched or born now has last_seen = t and stays; the others are rows nobody wrote in this launch
  if (max_age >= 0) {
    for (int i = tid; i < nt0; i += TRK_T) {
      if (i < mm && s_col[i] == 2) continue;
      int* ti = trk_i + (size_t)i * 5;
      if (ti[4] != 0 && (long long)t - (long long)ti[2] > (long long)max_age) ti[4] = 0;
    }
  }
  if (tid == 0) {
    const int want = nt0 + born;
    counts[0] = min(want, cap);
    if (want > cap) counts[1] += want - cap;
  }
}
extern "C" int es_track_assign(const float* iou, int n, int m, int ld, const float* det_boxes, const float* det_scores, const int* det_labels,
                               float* trk_boxes, float* trk_f, int* trk_i, int* counts, int cap, int t, float iou_thr, int same_class,
                               int max_age, int* det_track, void* stream) {
  if (n < 0 || n > TRK_MAX_DET || cap < 1 || cap > TRK_MAX_CAP || m < 0 || m > cap || ld < m || !(iou_thr >= 0.0f)) return -4;
  hipLaunchKernelGGL(k_track_assign, dim3(1), dim3(TRK_T), 0, (hipStream_t)stream, iou, n, m, ld, det_boxes, det_scores, det_labels, trk_boxes,
                     trk_f, trk_i, counts, cap, t, iou_thr, same_class, max_age, det_track);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ box_iou3d with its two polygons in LDS
// faces_flux keeps two 16-vertex polygons per lane in scratch (1 KB).  The same routine with the polygons in an LDS column per lane
// -- vertex i, component c of lane q at [(i * 3 + c) * CLIP_LANES + q], so that a wave's accesses are conflict free -- and the two
// face loops unrolled, so that every box axis is indexed statically and nothing is left for scratch.  The SAME expressions in the
// same order on the same values (no FMA contraction in this file): bit for bit the value box_iou3d returns.  The clipped polygon is
// written to the other column set and the two swap, where faces_flux copies it back: the values read are the same.
#define CLIP_LANES 64
__device__ inline V3 lp_get(const double* p, int i) {
  return v3(p[(i * 3 + 0) * CLIP_LANES], p[(i * 3 + 1) * CLIP_LANES], p[(i * 3 + 2) * CLIP_LANES]);
}
__device__ inline void lp_set(double* p, int i, V3 v) {
  p[(i * 3 + 0) * CLIP_LANES] = v.x; p[(i * 3 + 1) * CLIP_LANES] = v.y; p[(i * 3 + 2) * CLIP_LANES] = v.z;
}
__device__ inline double faces_flux_lds(const OBox& P, const OBox& Q, V3 O, bool inclusive, double* poly, double* tmp) {
  double total = 0.0;
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    const int j = f >> 1, k = (j + 1) % 3, l = (j + 2) % 3;
    const double sgn = (f & 1) ? -1.0 : 1.0;
    V3 n = P.ax[j] * sgn;
    V3 fc = P.c + P.ax[j] * (sgn * P.h[j]);
    V3 ek = P.ax[k] * P.h[k], el = P.ax[l] * P.h[l];
    int np = 4;
    lp_set(poly, 0, fc + ek + el); lp_set(poly, 1, fc - ek + el); lp_set(poly, 2, fc - ek - el); lp_set(poly, 3, fc + ek - el);
#pragma unroll
    for (int g = 0; g < 6; ++g) {
      if (np > 0) {
        const int jj = g >> 1;
        const double sg = (g & 1) ? -1.0 : 1.0;
        V3 m = Q.ax[jj] * sg;
        const double off = Q.h[jj];
        int nt = 0;
        for (int i = 0; i < np; ++i) {
          V3 a = lp_get(poly, i), b = lp_get(poly, (i + 1) % np);
          double da = dot3(m, a - Q.c) - off, db = dot3(m, b - Q.c) - off;
          const bool same = inclusive && dot3(m, n) > 0.5;
          bool ia = (da < -1e-12) || (same && da <= 1e-12), ib = (db < -1e-12) || (same && db <= 1e-12);
          if (ia) { if (nt < MAXV) lp_set(tmp, nt++, a); }
          if (ia != ib) {
            double t = da / (da - db);
            if (nt < MAXV) lp_set(tmp, nt++, a + (b - a) * t);
          }
        }
        np = nt;
        double* sw = poly; poly = tmp; tmp = sw;
      }
    }
    if (np < 3) continue;
    V3 av = v3(0, 0, 0);
    const V3 p0 = lp_get(poly, 0);
    for (int i = 1; i + 1 < np; ++i) av = av + cross3(lp_get(poly, i) - p0, lp_get(poly, i + 1) - p0);
    double area = 0.5 * sqrt(dot3(av, av));
    total += dot3(n, fc - O) * area;
  }
  return total;
}
// make_box on the six values make_box computes first (t = cos, sin of b[6], b[7], b[8]): the same three axis expressions
__device__ inline OBox make_box_trig(const double* b, const double* t, int ld) {
  OBox o;
  o.c = v3(b[0], b[1], b[2]);
  o.h[0] = b[3] * 0.5; o.h[1] = b[4] * 0.5; o.h[2] = b[5] * 0.5;
  double ca = t[0], sa = t[ld], cb = t[2 * ld], sb = t[3 * ld], cc = t[4 * ld], sc = t[5 * ld];
  o.ax[0] = v3(ca * cc - sa * sb * sc, sa * cc + ca * sb * sc, -(cb * sc));
  o.ax[1] = v3(-(sa * cb), ca * cb, sb);
  o.ax[2] = v3(ca * sc + sa * sb * cc, sa * sc - ca * sb * cc, cb * cc);
  return o;
}
__device__ inline double box_iou3d_lds(const double* a9, const OBox& A, const double* b9, const OBox& B, double* poly, double* tmp) {
  double va = a9[3] * a9[4] * a9[5], vb = b9[3] * b9[4] * b9[5];
  V3 d = A.c - B.c;
  double ra = sqrt(A.h[0] * A.h[0] + A.h[1] * A.h[1] + A.h[2] * A.h[2]), rb = sqrt(B.h[0] * B.h[0] + B.h[1] * B.h[1] + B.h[2] * B.h[2]);
  if (dot3(d, d) > (ra + rb) * (ra + rb)) return 0.0;
  double v = (faces_flux_lds(A, B, A.c, true, poly, tmp) + faces_flux_lds(B, A, A.c, false, poly, tmp)) / 3.0;
  if (v < 0.0) v = 0.0;
  return v / (va + vb - v);
}

// ------------------------------------------------------------------ answers of a grounder: distinct boxes per prompt, all prompts in one launch
// ground() returns Q boxes and scores per prompt; an answer is the short list the greedy above leaves of them with ONE class:
// rows by descending score (ties to the lower row), a row below score_thr or with a NaN score is never an answer, a row whose
// 9-DoF IoU with an already kept row exceeds iou_thr is skipped (candidate first, f64 rounded to f32, f32 compare, a NaN IoU does
// not suppress), and the walk stops at topk kept rows.  One workgroup per prompt; the order is made here: position of row i = the
// number of rows j with s_j > s_i, or s_j == s_i and j < i (counted over the keys in LDS; a NaN score takes the key -inf, which
// keeps the positions a permutation).  Then the two-phase pass of k_box3d_iou_filter without class counters.  The pass behind the
// last kept row is not run (topk = 1 computes no IoU).  ans_idx[k] = -1 for k >= ans_cnt: every entry of the prompt's row is written.
// Phase 2 clips with box_iou3d_lds on the first wave, one list entry per lane and 64 per round: the kernel uses no scratch and
// spills nothing.  What makes that possible is the table s_trig (dynamic LDS, 48 Q bytes): the six sin / cos of every row, made
// once in a loop of its own before the greedy -- the f64 sin / cos keep some fifty scalar registers of constants alive around
// them, and inside the greedy loop those would stay live through the clipping (10 scalar spills measured with make_box there).
#define GANS_MAX 1024              // rows per prompt: positions and keys of one prompt stay in LDS (9 KB)
__global__ __launch_bounds__(FILT_T) void k_ground_answers(const float* __restrict__ boxes, const float* __restrict__ scores, int Q,
                                                           float iou_thr, float score_thr, int topk, int* __restrict__ ans_idx,
                                                           int* __restrict__ ans_cnt) {
  __shared__ float s_key[GANS_MAX];
  __shared__ unsigned short s_ord[GANS_MAX];       // row at each sorted position
  __shared__ unsigned char s_dead[GANS_MAX];       // per sorted position
  __shared__ unsigned short s_list[GANS_MAX];      // positions whose sphere meets the kept row's
  __shared__ int s_first[FILT_T / 64];
  __shared__ int s_m, s_nlist;
  __shared__ double s_poly[2][MAXV * 3 * CLIP_LANES];      // the clipping's two polygons, one column per lane of the first wave (48 KB)
  extern __shared__ double s_trig[];       // (6, Q): cos, sin of every row's three angles -- made once, in a loop of its own: the f64
                                           // sin / cos hold ~50 scalar registers of constants, which must not stay live through the clipping
  __shared__ float s_kb[9];                // the kept row's box: read back per lane, so that what is derived from it stays in vector registers
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  boxes += (size_t)blockIdx.x * Q * 9;
  scores += (size_t)blockIdx.x * Q;
  int* __restrict__ out = ans_idx + (size_t)blockIdx.x * topk;
  for (int i = tid; i < Q; i += FILT_T) {
    const float v = scores[i];
    s_key[i] = (v != v) ? -__builtin_huge_valf() : v;
  }
  if (tid == 0) s_m = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < Q; i += FILT_T) {
    const float v = s_key[i];
    int r = 0;
    for (int j = 0; j < Q; ++j) {          // (every lane reads the same key: an LDS broadcast)
      const float u = s_key[j];
      r += (u > v || (u == v && j < i)) ? 1 : 0;
    }
    const float raw = scores[i];
    const bool live = raw == raw && !(raw < score_thr);
    s_ord[r] = (unsigned short)i;
    s_dead[r] = live ? 0 : 1;
    if (live) mine = max(mine, r + 1);
  }
  if (mine) atomicMax(&s_m, mine);
  if (topk > 1) {                          // (topk = 1 computes no IoU)
    for (int i = tid; i < Q; i += FILT_T) {
      const double ea = boxes[(size_t)i * 9 + 6], eb = boxes[(size_t)i * 9 + 7], ec = boxes[(size_t)i * 9 + 8];
      s_trig[i] = cos(ea); s_trig[Q + i] = sin(ea); s_trig[2 * Q + i] = cos(eb); s_trig[3 * Q + i] = sin(eb);
      s_trig[4 * Q + i] = cos(ec); s_trig[5 * Q + i] = sin(ec);
    }
  }
  __syncthreads();
  const int m = s_m;                       // one past the last live position
  int nk = 0, cur = 0;
  while (nk < topk) {
    // the first live position at or after `cur` (the same value in every lane)
    int found = -1;
    for (int base = cur; base < m; base += FILT_T) {
      const int p = base + tid;
      const bool ok = p < m && !s_dead[p];
      const unsigned long long bal = __ballot(ok);
      if (lane == 0) s_first[w] = bal ? base + w * 64 + __ffsll(bal) - 1 : 0x7fffffff;
      __syncthreads();
      int f = s_first[0];
#pragma unroll
      for (int k = 1; k < FILT_T / 64; ++k) f = min(f, s_first[k]);
      __syncthreads();                     // every lane has read s_first before the next chunk rewrites it
      if (f != 0x7fffffff) { found = f; break; }
    }
    if (found < 0) break;
    const int rk = s_ord[found];
    if (tid == 0) { out[nk] = rk; s_nlist = 0; }
    ++nk;
    if (nk == topk) break;                 // nothing is selected behind the last answer: its pass is not run
    if (tid < 9) s_kb[tid] = boxes[(size_t)rk * 9 + tid];
    __syncthreads();
    double kb[9], a[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) kb[c] = s_kb[c];
    const V3 kc = v3(kb[0], kb[1], kb[2]);
    const double kr = filt_radius(kb);
    for (int p = found + 1 + tid; p < m; p += FILT_T) {
      if (s_dead[p]) continue;
      const int r = s_ord[p];
      const V3 d = v3((double)boxes[(size_t)r * 9], (double)boxes[(size_t)r * 9 + 1], (double)boxes[(size_t)r * 9 + 2]) - kc;
      a[3] = boxes[(size_t)r * 9 + 3]; a[4] = boxes[(size_t)r * 9 + 4]; a[5] = boxes[(size_t)r * 9 + 5];
      const double rs = filt_radius(a) + kr;
      if (dot3(d, d) > rs * rs) {          // box_iou3d returns 0.0 here
        if (0.0f > iou_thr) s_dead[p] = 1;
      } else {
        s_list[atomicAdd(&s_nlist, 1)] = (unsigned short)p;
      }
    }
    __syncthreads();
    const int nl = s_nlist;
    if (tid < CLIP_LANES && tid < nl) {
      const OBox K = make_box_trig(kb, s_trig + rk, Q);      // once per kept row, not once per pair                // one entry per lane of the first wave: the polygons of 64 clippings fill the LDS
      for (int i = tid; i < nl; i += CLIP_LANES) {
        const int p = s_list[i];
        const int r = s_ord[p];
#pragma unroll
        for (int c = 0; c < 9; ++c) a[c] = boxes[(size_t)r * 9 + c];
        if ((float)box_iou3d_lds(a, make_box_trig(a, s_trig + r, Q), kb, K, &s_poly[0][tid], &s_poly[1][tid]) > iou_thr) s_dead[p] = 1;
      }
    }
    cur = found + 1;
    __syncthreads();                       // the flags and the list of this pass are settled before the next search
  }
  for (int k = nk + tid; k < topk; k += FILT_T) out[k] = -1;
  if (tid == 0) ans_cnt[blockIdx.x] = nk;
}
extern "C" int es_ground_answers(const float* boxes, const float* scores, int P, int Q, float iou_thr, float score_thr, int topk,
                                 int* ans_idx, int* ans_cnt, void* stream) {
  if (P < 0 || Q < 0) return -5;
  if (Q > GANS_MAX || P > 65535 || topk < 1 || topk > (Q > 1 ? Q : 1)) return -4;
  if (P == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (Q == 0) {                            // no row, no answer: counts 0, every index -1
    ES_TRY(hipMemsetAsync(ans_cnt, 0, (size_t)P * sizeof(int), st));
    ES_TRY(hipMemsetAsync(ans_idx, 0xff, (size_t)P * topk * sizeof(int), st));
    return 0;
  }
  const size_t sh = (size_t)6 * Q * sizeof(double);      // the trigonometry table: 48 KB at Q = 1024, next to 58 KB of static LDS
  ES_TRY(hipFuncSetAttribute((const void*)k_ground_answers, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
  hipLaunchKernelGGL(k_ground_answers, dim3(P), dim3(FILT_T), sh, st, boxes, scores, Q, iou_thr, score_thr, topk, ans_idx, ans_cnt);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ detection metric (IndoorDetMetric, eval/indoor_eval.py)
// eval_det_cls:111-132,145-158: one lane per prediction walks the ground-truth boxes of its (scene, class) group in the scene's
// order.  A prediction with a face below 2e-4 m^2 (f32 products) has its three sizes clamped to 2e-2 first; the IoU is the f64
// polyhedral one rounded to f32, and the FIRST box that attains the maximum wins (strict >).  No group: iou_max = -inf, gt_best
// = -1.  No (prediction, box) matrix exists: the work is the number of same-scene same-class pairs.
__global__ __launch_bounds__(64) void k_box3d_iou_best(const float* __restrict__ pred, int P, const int* __restrict__ pred_grp,
                                                       const float* __restrict__ gt, const int* __restrict__ grp_off, int n_grp,
                                                       float* __restrict__ iou_max, int* __restrict__ gt_best) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  float best = -INFINITY;
  int jbest = -1;
  const int g = pred_grp[i];
  if (g >= 0 && g < n_grp) {
    float p[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) p[c] = pred[(size_t)i * 9 + c];
    if (p[3] * p[4] < 2e-4f || p[3] * p[5] < 2e-4f || p[5] * p[4] < 2e-4f) {
      p[3] = fmaxf(p[3], 2e-2f); p[4] = fmaxf(p[4], 2e-2f); p[5] = fmaxf(p[5], 2e-2f);
    }
    double a[9], b[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) a[c] = p[c];
    const int j1 = grp_off[g + 1];
    for (int j = grp_off[g]; j < j1; ++j) {
#pragma unroll
      for (int c = 0; c < 9; ++c) b[c] = gt[(size_t)j * 9 + c];
      const float v = (float)box_iou3d(a, b);
      if (v > best) { best = v; jbest = j; }
    }
  }
  iou_max[i] = best;
  gt_best[i] = jbest;
}
extern "C" int es_det_best_gt(const float* pred_boxes, int P, const int* pred_grp, const float* gt_boxes, const int* grp_off_dev,
                              int n_grp, float* iou_max, int* gt_best, void* stream) {
  if (P < 0 || n_grp < 0) return -5;
  if (P == 0) return 0;
  hipLaunchKernelGGL(k_box3d_iou_best, dim3(es_cdiv(P, 64)), dim3(64), 0, (hipStream_t)stream, pred_boxes, P, pred_grp, gt_boxes,
                     grp_off_dev, n_grp, iou_max, gt_best);
  ES_CHECK_LAUNCH();
  return 0;
}

// eval_det_cls:160-168 without the walk down the ranks: at threshold t a ground-truth box goes to the LOWEST rank among the
// predictions with iou_max > t that point at it (integer atomicMin: the result does not depend on the order of arrival), and a
// prediction is a true positive iff that rank is its own.  order[r] = prediction at rank r (classes ascending, score descending).
struct DetThr { float v[ES_DET_MAX_THR]; };
__global__ void k_det_claim(const float* __restrict__ iou_max, const int* __restrict__ gt_best, const int* __restrict__ order, int P,
                            DetThr thr, int T, int G, int* __restrict__ claim) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= P) return;
  const int i = order[r];
  const int g = gt_best[i];
  if (g < 0 || g >= G) return;
  const float v = iou_max[i];
  for (int t = 0; t < T; ++t)
    if (v > thr.v[t]) atomicMin(&claim[(size_t)t * G + g], r);
}
__global__ void k_det_flag(const float* __restrict__ iou_max, const int* __restrict__ gt_best, const int* __restrict__ order, int P,
                           DetThr thr, int T, int G, const int* __restrict__ claim, unsigned char* __restrict__ tp) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= P) return;
  const int i = order[r];
  const int g = gt_best[i];
  const float v = iou_max[i];
  for (int t = 0; t < T; ++t)
    tp[(size_t)t * P + r] = (g >= 0 && g < G && v > thr.v[t] && claim[(size_t)t * G + g] == r) ? 1 : 0;
}
extern "C" int es_det_mark(const float* iou_max, const int* gt_best, const int* order, int P, const float* thr_host, int T, int G,
                           int* claim, unsigned char* tp, void* stream) {
  if (P < 0 || G < 0 || T < 1 || T > ES_DET_MAX_THR) return -5;
  if (P == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  DetThr thr;
  for (int t = 0; t < ES_DET_MAX_THR; ++t) thr.v[t] = t < T ? thr_host[t] : 0.f;
  if (G > 0) {
    ES_TRY(hipMemsetAsync(claim, 0x7f, (size_t)T * G * sizeof(int), st));     // 0x7f7f7f7f: above every rank
    hipLaunchKernelGGL(k_det_claim, dim3(es_cdiv(P, 256)), dim3(256), 0, st, iou_max, gt_best, order, P, thr, T, G, claim);
  }
  hipLaunchKernelGGL(k_det_flag, dim3(es_cdiv(P, 256)), dim3(256), 0, st, iou_max, gt_best, order, P, thr, T, G, claim, tp);
  ES_CHECK_LAUNCH();
  return 0;
}

// eval_det_cls:170-180 + average_precision:33-42 for one (class, threshold) per workgroup.  Ranks cls_off[c] .. cls_off[c+1] hold
// the class's predictions in rank order; every one that is not a TP is an FP, so at position j (0-based) tp + fp = j + 1 and
//   precision_j = cumtp_j / (j + 1),   recall_j = cumtp_j / npos        (f64 quotients, as numpy forms them).
// Recall takes a new value exactly at the TPs, so the area is  sum over TPs j of (recall_j - recall_(j-1)) * max_(k >= j)
// precision_k  (the appended point (1, 0) adds a zero).  Pass 1 counts the TPs; pass 2 walks the chunks of DET_CHUNK ranks from
// the last to the first with a block scan of the flags (cumtp) and a block suffix maximum (the envelope), carrying the count and
// the maximum of the later chunks.  The terms are the reference's own f64 values; only the order of the f64 sum differs.
#define DET_CHUNK 256
__global__ __launch_bounds__(DET_CHUNK) void k_det_ap(const unsigned char* __restrict__ tp, int P, const int* __restrict__ cls_off,
                                                      const int* __restrict__ npos, int C, float* __restrict__ ap,
                                                      int* __restrict__ tp_total) {
  __shared__ int s_cnt[DET_CHUNK / 64];
  __shared__ double s_max[DET_CHUNK / 64];
  __shared__ double s_acc[DET_CHUNK / 64];
  const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int s = cls_off[c], n = cls_off[c + 1] - s;
  const unsigned char* f = tp + (size_t)t * P + s;
  int cnt = 0;
  for (int j = tid; j < n; j += DET_CHUNK) cnt += f[j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) s_cnt[w] = cnt;
  __syncthreads();
  int total = 0;
#pragma unroll
  for (int k = 0; k < DET_CHUNK / 64; ++k) total += s_cnt[k];
  __syncthreads();
  const double np = (double)npos[c];
  int after = 0;               // TPs of the later chunks
  double env = 0.0;            // highest precision of the later chunks (the appended precision is 0)
  double acc = 0.0;
  for (int ch = (n + DET_CHUNK - 1) / DET_CHUNK - 1; ch >= 0; --ch) {
    const int j = ch * DET_CHUNK + tid;
    const int flag = j < n ? f[j] : 0;
    const unsigned long long bal = __ballot(flag);
    const int incl = __popcll(bal & (~0ull >> (63 - lane)));
    if (lane == 0) s_cnt[w] = __popcll(bal);
    __syncthreads();
    int chunk = 0, before = 0;
#pragma unroll
    for (int k = 0; k < DET_CHUNK / 64; ++k) { chunk += s_cnt[k]; if (k < w) before += s_cnt[k]; }
    const int cum = total - after - chunk + before + incl;          // cumulative TPs up to and including position j
    double m = j < n ? (double)cum / (double)(j + 1) : 0.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double v = __shfl_down(m, o, 64);
      if (lane + o < 64) m = fmax(m, v);
    }
    if (lane == 0) s_max[w] = m;
    __syncthreads();
    double all = env;
#pragma unroll
    for (int k = 0; k < DET_CHUNK / 64; ++k) { all = fmax(all, s_max[k]); if (k > w) m = fmax(m, s_max[k]); }
    m = fmax(m, env);
    if (flag) acc += ((double)cum / np - (double)(cum - 1) / np) * m;
    env = all;
    after += chunk;
    __syncthreads();
  }
  acc = es_wave_sum_d(acc);
  if (lane == 0) s_acc[w] = acc;
  __syncthreads();
  if (tid == 0) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < DET_CHUNK / 64; ++k) a += s_acc[k];
    ap[(size_t)t * C + c] = npos[c] > 0 ? (float)a : __builtin_nanf("");     // no ground truth: NaN, as the reference's 0 / 0
    tp_total[(size_t)t * C + c] = total;
  }
}
extern "C" int es_det_ap(const unsigned char* tp, int P, const int* cls_off_dev, const int* npos_dev, int C, int T, float* ap,
                         int* tp_total, void* stream) {
  if (P < 0 || C < 0 || T < 1 || T > ES_DET_MAX_THR) return -5;
  if (C == 0) return 0;
  hipLaunchKernelGGL(k_det_ap, dim3(C, T), dim3(DET_CHUNK), 0, (hipStream_t)stream, tp, P, cls_off_dev, npos_dev, C, ap, tp_total);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ grounding metric (GroundingMetric, grounding_metric.py:70-152)
// ground_eval:103-110 for a whole batch: lane e = (sample s, slot k) takes the box the sorted top-k put in that slot and walks the
// sample's ground-truth boxes.  The IoU is the f64 polyhedral one rounded to f32 and compared in f32; there is no thin-box clamp
// here (the reference calls `overlaps` directly).  `hit[s]` collects one bit per threshold with an integer atomic OR, so the
// word does not depend on the order in which the slots arrive.  An index outside the sample's rows counts as an empty slot.
__global__ __launch_bounds__(64) void k_box3d_iou_hits(const float* __restrict__ boxes, const int* __restrict__ box_off,
                                                       const int* __restrict__ topk, int S, int K, const float* __restrict__ gt,
                                                       const int* __restrict__ gt_off, DetThr thr, int T, int* __restrict__ hit,
                                                       float* __restrict__ iou_top) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S * K) return;
  const int s = e / K;
  const int q = topk[e];
  const int q0 = box_off[s], nq = box_off[s + 1] - q0;
  float best = -INFINITY;
  int bits = 0;
  if (q >= 0 && q < nq) {
    double a[9], b[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) a[c] = boxes[(size_t)(q0 + q) * 9 + c];
    const int j1 = gt_off[s + 1];
    for (int j = gt_off[s]; j < j1; ++j) {
#pragma unroll
      for (int c = 0; c < 9; ++c) b[c] = gt[(size_t)j * 9 + c];
      const float v = (float)box_iou3d(a, b);
      best = fmaxf(best, v);
      for (int t = 0; t < T; ++t)
        if (v > thr.v[t]) bits |= 1 << t;
    }
  }
  iou_top[e] = best;
  if (bits) atomicOr(&hit[s], bits);
}
extern "C" int es_ground_hits(const float* boxes, const int* box_off_dev, const int* topk_idx, int S, int K, const float* gt_boxes,
                              const int* gt_off_dev, const float* thr_host, int T, int* hit, float* iou_top, void* stream) {
  if (S < 0 || K < 0 || T < 1 || T > ES_DET_MAX_THR || (long long)S * K > 0x7fffffffLL) return -5;
  if (S == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  ES_TRY(hipMemsetAsync(hit, 0, (size_t)S * sizeof(int), st));
  if (K == 0) return 0;
  DetThr thr;
  for (int t = 0; t < ES_DET_MAX_THR; ++t) thr.v[t] = t < T ? thr_host[t] : 0.f;
  hipLaunchKernelGGL(k_box3d_iou_hits, dim3(es_cdiv((long long)S * K, 64)), dim3(64), 0, st, boxes, box_off_dev, topk_idx, S, K,
                     gt_boxes, gt_off_dev, thr, T, hit, iou_top);
  ES_CHECK_LAUNCH();
  return 0;
}

// ground_eval:108-131 over the gathered samples: every sample counts in Overall and in one type of each pair.  Types in the
// reference's order: 0 Easy, 1 Hard, 2 View-Dep, 3 View-Indep, 4 Unique, 5 Multi, 6 Overall.  counts (T,7,2) = [found, samples].
// Each workgroup counts in LDS (integer atomics) and flushes its non-zero counters with one integer atomic each.
#define GT_TYPES 7
__global__ __launch_bounds__(256) void k_ground_tally(const int* __restrict__ hit, const unsigned char* __restrict__ flags, int N,
                                                      int T, int* __restrict__ counts) {
  __shared__ int s_found[ES_DET_MAX_THR * GT_TYPES];
  __shared__ int s_n[GT_TYPES];
  for (int i = threadIdx.x; i < ES_DET_MAX_THR * GT_TYPES; i += blockDim.x) s_found[i] = 0;
  if (threadIdx.x < GT_TYPES) s_n[threadIdx.x] = 0;
  __syncthreads();
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    const int f = flags[i], h = hit[i];
    const int ty[4] = {(f & 2) ? 1 : 0, (f & 1) ? 2 : 3, (f & 4) ? 4 : 5, 6};
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicAdd(&s_n[ty[k]], 1);
    for (int t = 0; t < T; ++t)
      if ((h >> t) & 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicAdd(&s_found[t * GT_TYPES + ty[k]], 1);
      }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T * GT_TYPES; i += blockDim.x) {
    if (s_found[i]) atomicAdd(&counts[i * 2], s_found[i]);
    if (s_n[i % GT_TYPES]) atomicAdd(&counts[i * 2 + 1], s_n[i % GT_TYPES]);
  }
}
extern "C" int es_ground_tally(const int* hit, const unsigned char* flags, int N, int T, int* counts, void* stream) {
  if (N < 0 || T < 1 || T > ES_DET_MAX_THR) return -5;
  hipStream_t st = (hipStream_t)stream;
  ES_TRY(hipMemsetAsync(counts, 0, (size_t)T * GT_TYPES * 2 * sizeof(int), st));
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_ground_tally, dim3(min(es_cdiv(N, 256), 256)), dim3(256), 0, st, hit, flags, N, T, counts);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ matching costs
// cost[b][g][q] (G rows, Q columns: the orientation scipy's solver works in after its own transpose, nr <= nc)
__global__ void k_ground_cost(const float* __restrict__ logits, int Tout, const float* __restrict__ boxes, int Q,
                              const float* __restrict__ gt_boxes, const unsigned char* __restrict__ pos_map,
                              const int* __restrict__ gt_off, const int* __restrict__ tlen, int T, float w_cls, float w_l1,
                              float w_iou, float alpha, float gamma, float eps, double* __restrict__ cost, int Gmax) {
  const int b = blockIdx.y;
  const int g0 = gt_off[b], G = gt_off[b + 1] - g0;
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= G * Q) return;
  const int g = e / Q, q = e % Q;
  const float* lg = logits + ((size_t)b * Q + q) * Tout;
  const unsigned char* pm = pos_map + (size_t)(g0 + g) * T;
  const int tl = min(tlen[b], T);
  // BinaryFocalLossCost on the un-padded tokens (f32 like the reference; summed in double)
  double c_cls = 0.0;
  for (int t = 0; t < tl; ++t) {
    float p = 1.f / (1.f + expf(-lg[t]));
    float neg = -logf(1.f - p + eps) * (1.f - alpha) * powf(p, gamma);
    float pos = -logf(p + eps) * alpha * powf(1.f - p, gamma);
    c_cls += pm[t] ? (double)pos : (double)neg;
  }
  const float* pb = boxes + ((size_t)b * Q + q) * 9;
  const float* gb = gt_boxes + (size_t)(g0 + g) * 9;
  double l1 = 0.0, a9[9], b9[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) { a9[c] = pb[c]; b9[c] = gb[c]; l1 += fabs((double)pb[c] - (double)gb[c]); }
  double iou = box_iou3d(a9, b9);
  double c = (double)w_cls * c_cls + (double)w_l1 * (double)(float)l1 + (double)w_iou * -(double)(float)iou;
  if (isnan(c)) c = 100.0;                               // torch.nan_to_num(cost, nan=100, posinf=100, neginf=-100)
  else if (isinf(c)) c = c > 0 ? 100.0 : -100.0;
  cost[((size_t)b * Gmax + g) * Q + q] = c;
}

// ------------------------------------------------------------------ rectangular linear sum assignment
// One thread per sample: the shortest-augmenting-path algorithm scipy.optimize.linear_sum_assignment uses (Crouse 2016),
// including its tie rule (among equal path costs prefer an unassigned column) and its column visiting order, so that
// equal-cost cases resolve the same way.  nr = G rows, nc = Q columns, nr <= nc.  work (doubles): u[G] v[Q] sp[Q];
// iwork (ints): path[Q] col4row[G] row4col[Q] remaining[Q] SR[G] SC[Q].
__global__ void k_lsa(const double* __restrict__ cost, int Gmax, int Q, const int* __restrict__ gt_off, double* __restrict__ work,
                      int* __restrict__ iwork, int* __restrict__ q2g /* (B,Q): matched gt (local index) or -1 */, int B) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int nr = gt_off[b + 1] - gt_off[b], nc = Q;
  const double* C = cost + (size_t)b * Gmax * Q;
  double* u = work + (size_t)b * (Gmax + 2 * Q);
  double* v = u + Gmax;
  double* sp = v + Q;
  int* path = iwork + (size_t)b * (4 * Q + 2 * Gmax);
  int* col4row = path + Q;
  int* row4col = col4row + Gmax;
  int* remaining = row4col + Q;
  int* SR = remaining + Q;
  int* SC = SR + Gmax;
  for (int j = 0; j < nc; ++j) { v[j] = 0.0; row4col[j] = -1; q2g[(size_t)b * Q + j] = -1; }
  for (int i = 0; i < nr; ++i) { u[i] = 0.0; col4row[i] = -1; }
  for (int cur = 0; cur < nr; ++cur) {
    double minVal = 0.0;
    int i = cur, num_remaining = nc, sink = -1;
    for (int it = 0; it < nc; ++it) { remaining[it] = nc - it - 1; SC[it] = 0; sp[it] = INFINITY; }
    for (int it = 0; it < nr; ++it) SR[it] = 0;
    while (sink == -1) {
      int index = -1;
      double lowest = INFINITY;
      SR[i] = 1;
      for (int it = 0; it < num_remaining; ++it) {
        int j = remaining[it];
        double r = minVal + C[(size_t)i * Q + j] - u[i] - v[j];
        if (r < sp[j]) { path[j] = i; sp[j] = r; }
        if (sp[j] < lowest || (sp[j] == lowest && row4col[j] == -1)) { lowest = sp[j]; index = it; }
      }
      minVal = lowest;
      if (!(minVal < INFINITY)) { sink = -2; break; }   // infeasible (cannot happen after nan_to_num)
      int j = remaining[index];
      if (row4col[j] == -1) sink = j; else i = row4col[j];
      SC[j] = 1;
      remaining[index] = remaining[--num_remaining];
    }
    if (sink < 0) break;
    u[cur] += minVal;
    for (int r = 0; r < nr; ++r) if (SR[r] && r != cur) u[r] += minVal - sp[col4row[r]];
    for (int j = 0; j < nc; ++j) if (SC[j]) v[j] -= minVal - sp[j];
    int j = sink;
    while (true) {
      int r = path[j];
      row4col[j] = r;
      int t = col4row[r]; col4row[r] = j; j = t;
      if (r == cur) break;
    }
  }
  for (int r = 0; r < nr; ++r) if (col4row[r] >= 0) q2g[(size_t)b * Q + col4row[r]] = r;
}

// The same algorithm with one WAVE per sample and the solver state in LDS: the column scan of every augmenting step runs
// 64-wide and the argmin is a shuffle reduction that reproduces the sequential tie rule (first column of the minimum
// value, replaced by the LAST unassigned column among the ties).  The single-thread version above spends ~0.5 ms per
// decoder layer in dependent global loads; this one a few tens of microseconds.  Q <= LSA_MAXQ.
#define LSA_MAXQ 1024
__global__ __launch_bounds__(64) void k_lsa_wave(const double* __restrict__ cost, int Gmax, int Q, const int* __restrict__ gt_off,
                                                 int* __restrict__ q2g) {
  __shared__ double u[LSA_MAXQ], v[LSA_MAXQ], sp[LSA_MAXQ];
  __shared__ int path[LSA_MAXQ], col4row[LSA_MAXQ], row4col[LSA_MAXQ], rem[LSA_MAXQ];
  __shared__ unsigned char SR[LSA_MAXQ], SC[LSA_MAXQ];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int nr = gt_off[b + 1] - gt_off[b], nc = Q;
  const double* C = cost + (size_t)b * Gmax * Q;
  for (int j = lane; j < nc; j += 64) { v[j] = 0.0; row4col[j] = -1; }
  for (int i = lane; i < nr; i += 64) { u[i] = 0.0; col4row[i] = -1; }
  __syncthreads();
  for (int cur = 0; cur < nr; ++cur) {
    for (int it = lane; it < nc; it += 64) { rem[it] = nc - it - 1; SC[it] = 0; sp[it] = INFINITY; }
    for (int it = lane; it < nr; it += 64) SR[it] = 0;
    __syncthreads();
    double minVal = 0.0;
    int i = cur, num_remaining = nc, sink = -1;
    while (sink == -1) {
      if (lane == 0) SR[i] = 1;
      const double ui = u[i];
      double lowest = INFINITY;
      int first = 0x7fffffff, lastU = -1;
      for (int it = lane; it < num_remaining; it += 64) {
        int j = rem[it];
        double r = minVal + C[(size_t)i * Q + j] - ui - v[j];
        if (r < sp[j]) { path[j] = i; sp[j] = r; }
        double val = sp[j];
        bool un = row4col[j] == -1;
        if (val < lowest) { lowest = val; first = it; lastU = un ? it : -1; }
        else if (val == lowest && un) lastU = it;           // `it` grows within a lane: a later tie
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        double ol = __shfl_xor(lowest, o, 64);
        int of = __shfl_xor(first, o, 64), ou = __shfl_xor(lastU, o, 64);
        if (ol < lowest) { lowest = ol; first = of; lastU = ou; }
        else if (ol == lowest) { first = min(first, of); lastU = max(lastU, ou); }
      }
      minVal = lowest;
      if (!(minVal < INFINITY)) { sink = -2; break; }
      const int index = lastU >= 0 ? lastU : first;
      const int j = rem[index];
      const int r4 = row4col[j];
      __syncthreads();                                      // every lane has read rem[] / row4col[] of this step
      if (r4 == -1) sink = j; else i = r4;
      if (lane == 0) { SC[j] = 1; rem[index] = rem[num_remaining - 1]; }
      --num_remaining;
      __syncthreads();
    }
    if (sink < 0) break;
    if (lane == 0) u[cur] += minVal;
    for (int r = lane; r < nr; r += 64) if (SR[r] && r != cur) u[r] += minVal - sp[col4row[r]];
    for (int j = lane; j < nc; j += 64) if (SC[j]) v[j] -= minVal - sp[j];
    __syncthreads();
    if (lane == 0) {
      int j = sink;
      while (true) {
        int r = path[j];
        row4col[j] = r;
        int t = col4row[r]; col4row[r] = j; j = t;
        if (r == cur) break;
      }
    }
    __syncthreads();
  }
  for (int j = lane; j < nc; j += 64) q2g[(size_t)b * Q + j] = -1;
  __syncthreads();
  for (int r = lane; r < nr; r += 64) if (col4row[r] >= 0) q2g[(size_t)b * Q + col4row[r]] = r;
}

extern "C" int es_ground_match(const float* logits, int Tout, const float* boxes, int B, int Q, const float* gt_boxes,
                               const unsigned char* pos_map, const int* gt_off_dev, int Gmax, const int* tlen_dev, int T,
                               float w_cls, float w_l1, float w_iou, double* cost, double* work, int* iwork, int* q2g,
                               void* stream) {
  if (B <= 0 || Q <= 0) return 0;
  if (Gmax > Q) return -5;                               // the solver is written for nr <= nc (more queries than boxes)
  hipStream_t st = (hipStream_t)stream;
  if (Gmax > 0)
    hipLaunchKernelGGL(k_ground_cost, dim3(es_cdiv((long long)Gmax * Q, 64), B), dim3(64), 0, st, logits, Tout, boxes, Q, gt_boxes,
                       pos_map, gt_off_dev, tlen_dev, T, w_cls, w_l1, w_iou, 0.25f, 2.0f, 1e-12f, cost, Gmax);
  if (Q <= LSA_MAXQ)
    hipLaunchKernelGGL(k_lsa_wave, dim3(B), dim3(64), 0, st, cost, Gmax, Q, gt_off_dev, q2g);
  else
    hipLaunchKernelGGL(k_lsa, dim3(es_cdiv(B, 64)), dim3(64), 0, st, cost, Gmax, Q, gt_off_dev, work, iwork, q2g, B);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ labels + focal loss on the valid tokens
// labels[b,q,t] = pos_map[g][t] for the matched box g of query q, else 0; loss = sum over (b, q, t < tlen[b]) of
// BCEwithlogits(x, y) * (alpha y + (1-alpha)(1-y)) * pt^gamma, pt = (1-p) y + p (1-y)   (mmdet py_sigmoid_focal_loss),
// divided by (avg_factor + eps32); gradient written to dlogits (0 at padded tokens).  One wave per (b, q) row.
__global__ __launch_bounds__(256) void k_ground_focal(const float* __restrict__ logits, int Tout, int B, int Q,
                                                      const int* __restrict__ q2g, const unsigned char* __restrict__ pos_map,
                                                      const int* __restrict__ gt_off, const int* __restrict__ tlen, int T,
                                                      float alpha, float gamma, const float* __restrict__ avg_factor,
                                                      float grad_scale, float* __restrict__ dlogits,
                                                      double* __restrict__ loss_sum) {
  int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  double acc = 0.0;
  if (row < B * Q) {
    const int b = row / Q;
    const int g = q2g[row];
    const unsigned char* pm = g >= 0 ? pos_map + (size_t)(gt_off[b] + g) * T : nullptr;
    const int tl = min(tlen[b], T);
    const float inv = 1.f / (avg_factor[0] + 1.1920929e-07f);
    for (int t = lane; t < Tout; t += 64) {
      float gout = 0.f;
      if (t < tl) {
        float x = logits[(size_t)row * Tout + t];
        bool y = pm && pm[t];
        float p = 1.f / (1.f + expf(-x));
        float bce = fmaxf(x, 0.f) - (y ? x : 0.f) + log1pf(expf(-fabsf(x)));
        float pt = y ? (1.f - p) : p;
        float fw = (y ? alpha : (1.f - alpha)) * powf(pt, gamma);
        acc += (double)(bce * fw);
        // d/dx [bce * fw]: dbce/dx = p - y ; dfw/dx = w_a * gamma * pt^(gamma-1) * dpt/dx, dpt/dx = (y ? -1 : 1) * p (1-p)
        float dfw = (y ? alpha : (1.f - alpha)) * gamma * powf(pt, gamma - 1.f) * (y ? -1.f : 1.f) * p * (1.f - p);
        gout = ((p - (y ? 1.f : 0.f)) * fw + bce * dfw) * inv * grad_scale;
      }
      if (dlogits) dlogits[(size_t)row * Tout + t] = gout;
    }
  }
  acc = es_wave_sum_d(acc);
  if (lane == 0 && acc != 0.0) unsafeAtomicAdd(loss_sum, acc);
}
extern "C" int es_ground_focal(const float* logits, int Tout, int B, int Q, const int* q2g, const unsigned char* pos_map,
                               const int* gt_off_dev, const int* tlen_dev, int T, float alpha, float gamma,
                               const float* avg_factor_dev, float grad_scale, float* dlogits, double* loss_sum, void* stream) {
  if (B * Q <= 0) return 0;
  hipLaunchKernelGGL(k_ground_focal, dim3(es_cdiv(B * Q, 4)), dim3(256), 0, (hipStream_t)stream, logits, Tout, B, Q, q2g, pos_map,
                     gt_off_dev, tlen_dev, T, alpha, gamma, avg_factor_dev, grad_scale, dlogits, loss_sum);
  ES_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ per-sample sorted top-k (one workgroup per sample)
// idx[b, 0..k) = rows (local to the sample) of the k largest values in descending order, ties: lower row first.
// Segment length <= 16384 (bitonic sort of (value, row) keys in dynamic LDS: 8 B per key of the next power of two >= L; the
// reference's token lists hold at most 4 levels x pts_prune_threshold = 4000 rows, 128 KB of the CU's 160 KB cover 16384).
#define TK_MAX 16384
__global__ __launch_bounds__(1024) void k_topk_sorted(const float* __restrict__ vals, int L, const int* __restrict__ vlen, int k,
                                                      int* __restrict__ idx) {
  extern __shared__ unsigned long long key[];
  const int b = blockIdx.x;
  const int n = vlen ? min(vlen[b], L) : L;
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = threadIdx.x; i < P; i += blockDim.x) {
    unsigned long long kk = ~0ull;                      // padding sorts last
    if (i < n) {
      unsigned int u = __float_as_uint(vals[(size_t)b * L + i]);
      if (u == 0x80000000u) u = 0u;                     // -0.0 == +0.0: the two zeros tie, and ties go to the lower row
      u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);   // ascending order-preserving map
      kk = ((unsigned long long)(~u) << 32) | (unsigned int)i;    // descending value, ascending row
    }
    key[i] = kk;
  }
  __syncthreads();
  for (int sz = 2; sz <= P; sz <<= 1)
    for (int st = sz >> 1; st > 0; st >>= 1) {
      for (int i = threadIdx.x; i < P; i += blockDim.x) {
        int j = i ^ st;
        if (j > i) {
          bool up = (i & sz) == 0;
          unsigned long long a = key[i], c = key[j];
          if ((a > c) == up) { key[i] = c; key[j] = a; }
        }
      }
      __syncthreads();
    }
  for (int i = threadIdx.x; i < k; i += blockDim.x) idx[(size_t)b * k + i] = i < n ? (int)(key[i] & 0xffffffffu) : -1;
}
extern "C" int es_topk_sorted(const float* vals, int B, int L, const int* vlen_dev, int k, int* idx, void* stream) {
  if (B <= 0 || k <= 0) return 0;
  if (L > TK_MAX) return -4;
  int P2 = 1;
  while (P2 < L) P2 <<= 1;
  const size_t sh = (size_t)P2 * sizeof(unsigned long long);
  if (sh > 64 * 1024) ES_TRY(hipFuncSetAttribute((const void*)k_topk_sorted, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
  hipLaunchKernelGGL(k_topk_sorted, dim3(B), dim3(1024), sh, (hipStream_t)stream, vals, L, vlen_dev, k, idx);
  ES_CHECK_LAUNCH();
  return 0;
}
