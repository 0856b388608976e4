// ba.hip — bundle adjustment over the point registry (Runner.py:294-306, SFM.py:405-464): the
// library's own Levenberg-Marquardt rule with the Schur complement (DESIGN.md §13E;
// include/sfmfeat.h sfm_bundle_adjust_dev).  Parity with scipy's least_squares(method='trf')
// is not pinned: the minimum is.
//
// Once per call (the plan):
// * k_ba_init: R = Rodrigues(camera_params) (linalg3.h rodrigues), t and X copied into
//   slot 0 of the two-slot state; the LM state (lambda, counters) reset.
// * k_ba_count / k_ba_scan / k_ba_fill_pt / k_ba_sort_pt: per-point observation lists as offsets
//   + observation indices.  Integer atomics count and hand out slots; every list is then sorted
//   ascending by its own thread, so the order never depends on the atomics.
// * k_ba_fill_cam, one workgroup per camera: its observations compacted in ascending order
//   (an ordered scan over all M; no atomics).
// Per LM iteration, eight launches, each returning at once when the device `done` word is set:
// * k_ba_lin, one thread per observation: r, J_c (2 x 6), J_p (2 x 3) at the current state.
// * k_ba_point, one thread per point: V_j, g_j over its list in order, the 3 x 3 Cholesky
//   inverse of V*_j, V*_j^-1 g_j; W_cj merged over duplicate observations of one (c, j) at the
//   first of them (the others, and fixed cameras, carry camera -1), and Y_cj = W_cj V*_j^-1.
// * k_ba_schur, one wave per (camera a, segment of its list): the 6 x 6 n_cam row of S and b_a in
//   LDS, the segment's points in list order, each point's (camera, element) addresses spread
//   over the lanes — one thread per address per point; segment 0 also adds U*_a and -g_a (per-lane
//   sums in list order, then a butterfly).  The list is cut into ba_schur_split(n_cam) segments of
//   equal length; k_ba_schur_sum adds the segments' rows in order.
// * k_ba_solve, one workgroup: right-looking Cholesky of S in its global workspace (column k
//   staged in LDS for the trailing update), then the two triangular solves with b in LDS.  A
//   pivot that is not positive and finite ends the factorisation: the step is rejected.
// * k_ba_update: the candidate state (other slot): dX_j = -V*_j^-1 (g_j + W_j^T d_c),
//   R <- exp([d omega]x) R, t <- t + d t; per-row |d|^2 and |params|^2.
// * k_ba_resid: squared residual per observation at the candidate.
// * k_ba_decide, one workgroup: the candidate cost and the two norms by block_sum256_tree;
//   thread 0 accepts or rejects, moves lambda, the counters, the slot and `done`.
// Finally k_ba_finish: R -> principal Rodrigues vector (linalg3.h rodrigues_inv); rows
// that never moved return their input bits.
// No cooperative launch, no grid barrier, no wait on memory: every loop is bounded by a size
// passed in.  Float64 throughout; -ffp-contract=off.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "f64_dev.h"
#include "kernels.h"
#include "linalg3.h"

namespace sfm {

constexpr int kBaThreads = 256;
constexpr int kBaSolveThreads = 1024;
constexpr int kBaLin = 20;  // per observation: r (2), J_c rows (6 + 6), J_p rows (3 + 3)

// ---------------- the plan ----------------

__global__ void __launch_bounds__(kBaThreads) k_ba_init(BaProblem p) {
  const int64_t i = (int64_t)blockIdx.x * kBaThreads + threadIdx.x;
  if (i == 0) {
    BaState* s = p.st;
    s->lam = 1e-3;
    s->cost = s->cost0 = 0.0;
    s->cur = 0, s->done = 0, s->status = kRefineMaxIter, s->accepted = 0, s->iters = 0, s->rejected = 0;
    s->fail = 0;
  }
  if (i < p.n_pts) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p.Xs[3 * i + k] = p.X_in[3 * i + k];
  } else if (i < (int64_t)p.n_pts + p.n_cam) {
    const int c = (int)(i - p.n_pts);
    const double* cp = p.cams_in + 6 * c;
    double R[9];
    rodrigues(cp[0], cp[1], cp[2], R);
    double* o = p.Rt + 12 * c;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[9 + k] = cp[3 + k];
  }
}

// pt_cnt, cam_cnt zeroed by the caller
__global__ void __launch_bounds__(kBaThreads) k_ba_count(BaProblem p) {
  const int o = blockIdx.x * kBaThreads + threadIdx.x;
  if (o >= p.M) return;
  atomicAdd(&p.pt_cnt[clamp_index(p.pt_idx[o], p.n_pts)], 1);
  atomicAdd(&p.cam_cnt[clamp_index(p.cam_idx[o], p.n_cam)], 1);
}

// one workgroup: exclusive scans of both counts; pt_cnt becomes the fill cursor
__global__ void __launch_bounds__(kBaThreads) k_ba_scan(BaProblem p) {
  __shared__ uint32_t s_scan[kBaThreads / 64 + 1];
  const int tid = threadIdx.x;
  uint32_t base = 0;
  for (int i0 = 0; i0 < p.n_pts; i0 += kBaThreads) {
    const int i = i0 + tid;
    const uint32_t v = i < p.n_pts ? (uint32_t)p.pt_cnt[i] : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(v, s_scan, &total);
    if (i < p.n_pts) {
      p.pt_off[i] = (int32_t)(base + ex);
      p.pt_cnt[i] = 0;
    }
    base += total;
  }
  if (tid == 0) p.pt_off[p.n_pts] = (int32_t)base;
  const uint32_t v = tid < p.n_cam ? (uint32_t)p.cam_cnt[tid] : 0u;  // n_cam <= 256
  uint32_t total;
  const uint32_t ex = block_exclusive_scan(v, s_scan, &total);
  if (tid < p.n_cam) {
    p.cam_off[tid] = (int32_t)ex;
    p.cam_active[tid] = v > 0 && !(p.cam_fixed && p.cam_fixed[tid]) ? 1 : 0;
  }
  if (tid == 0) p.cam_off[p.n_cam] = (int32_t)total;
}

__global__ void __launch_bounds__(kBaThreads) k_ba_fill_pt(BaProblem p) {
  const int o = blockIdx.x * kBaThreads + threadIdx.x;
  if (o >= p.M) return;
  const int j = clamp_index(p.pt_idx[o], p.n_pts);
  const int slot = atomicAdd(&p.pt_cnt[j], 1);
  const int k = p.pt_off[j + 1] - p.pt_off[j];
  if (slot < k) p.pt_list[p.pt_off[j] + slot] = o;  // (always: the counts are this launch's)
}

// one thread per point: its list ascending (insertion sort, bounded by the list's length), then
// each observation's position
__global__ void __launch_bounds__(kBaThreads) k_ba_sort_pt(BaProblem p) {
  const int j = blockIdx.x * kBaThreads + threadIdx.x;
  if (j >= p.n_pts) return;
  const int off = p.pt_off[j], k = p.pt_off[j + 1] - off;
  int32_t* L = p.pt_list + off;
  for (int e = 1; e < k; ++e) {
    const int32_t v = L[e];
    int q = e;
    for (; q > 0 && L[q - 1] > v; --q) L[q] = L[q - 1];
    L[q] = v;
  }
  for (int e = 0; e < k; ++e)
    if ((uint32_t)L[e] < (uint32_t)p.M) p.pos[L[e]] = off + e;
}

// one workgroup per camera: its observations in ascending order
__global__ void __launch_bounds__(kBaThreads) k_ba_fill_cam(BaProblem p) {
  __shared__ uint32_t s_scan[kBaThreads / 64 + 1];
  const int c = blockIdx.x, tid = threadIdx.x;
  uint32_t base = (uint32_t)p.cam_off[c];
  const uint32_t end = (uint32_t)p.cam_off[c + 1];
  for (int o0 = 0; o0 < p.M; o0 += kBaThreads) {
    const int o = o0 + tid;
    const bool f = o < p.M && clamp_index(p.cam_idx[o], p.n_cam) == c;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(f ? 1u : 0u, s_scan, &total);
    if (f && base + ex < end) p.cam_list[base + ex] = o;
    base += total;
  }
}

// ---------------- one LM iteration ----------------

// observation o at state slot `slot`: residual, and with kJac the Jacobian rows
template <bool kJac>
SFM_DEV void ba_observe(const BaProblem& p, int o, int slot, double (&r)[2], double (&Jc)[2][6], double (&Jp)[2][3]) {
  const int c = clamp_index(p.cam_idx[o], p.n_cam), j = clamp_index(p.pt_idx[o], p.n_pts);
  const double* Rt = p.Rt + ((int64_t)slot * p.n_cam + c) * 12;
  const double* Xp = p.Xs + ((int64_t)slot * p.n_pts + j) * 3;
  const double* K = p.K + 9 * c;
  double R[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = Rt[k];
  double Y[3];
  rotate3(R, Xp[0], Xp[1], Xp[2], Y);
  const double a0 = Y[0] + Rt[9], a1 = Y[1] + Rt[10], a2 = Y[2] + Rt[11];
  const double q0 = (K[0] * a0 + K[1] * a1) + K[2] * a2;
  const double q1 = (K[3] * a0 + K[4] * a1) + K[5] * a2;
  const double q2 = (K[6] * a0 + K[7] * a1) + K[8] * a2;
  const double pu[2] = {q0 / q2, q1 / q2};
  r[0] = pu[0] - p.obs[2 * (int64_t)o];
  r[1] = pu[1] - p.obs[2 * (int64_t)o + 1];
  if (kJac) {
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      double g[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = (K[3 * a + k] - pu[a] * K[6 + k]) / q2;
      Jc[a][0] = Y[1] * g[2] - Y[2] * g[1];
      Jc[a][1] = Y[2] * g[0] - Y[0] * g[2];
      Jc[a][2] = Y[0] * g[1] - Y[1] * g[0];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        Jc[a][3 + k] = g[k];
        Jp[a][k] = (g[0] * R[k] + g[1] * R[3 + k]) + g[2] * R[6 + k];
      }
    }
  }
}

__global__ void __launch_bounds__(kBaThreads) k_ba_lin(BaProblem p) {
  if (p.st->done) return;
  const int o = blockIdx.x * kBaThreads + threadIdx.x;
  if (o >= p.M) return;
  double r[2], Jc[2][6], Jp[2][3];
  ba_observe<true>(p, o, p.st->cur, r, Jc, Jp);
  double* L = p.lin + (int64_t)o * kBaLin;
  L[0] = r[0], L[1] = r[1];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
#pragma unroll
    for (int k = 0; k < 6; ++k) L[2 + 6 * a + k] = Jc[a][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) L[14 + 3 * a + k] = Jp[a][k];
  }
}

// slot_xor: 0 the current state (the start cost), 1 the candidate
__global__ void __launch_bounds__(kBaThreads) k_ba_resid(BaProblem p, int slot_xor) {
  if (p.st->done) return;
  const int o = blockIdx.x * kBaThreads + threadIdx.x;
  if (o >= p.M) return;
  double r[2], Jc[2][6], Jp[2][3];
  ba_observe<false>(p, o, p.st->cur ^ slot_xor, r, Jc, Jp);
  p.e2[o] = r[0] * r[0] + r[1] * r[1];
}

__global__ void __launch_bounds__(kBaThreads) k_ba_point(BaProblem p) {
  if (p.st->done) return;
  const int j = blockIdx.x * kBaThreads + threadIdx.x;
  if (j >= p.n_pts) return;
  const int off = p.pt_off[j], k = p.pt_off[j + 1] - off;
  double* vinv = p.vinv + 6 * (int64_t)j;  // 00 01 02 11 12 22
  double* gp = p.gp + 3 * (int64_t)j;
  double* vg = p.vg + 3 * (int64_t)j;
  if (k == 0) {  // no observation: the identity block, no gradient
    vinv[0] = 1.0, vinv[1] = 0.0, vinv[2] = 0.0, vinv[3] = 1.0, vinv[4] = 0.0, vinv[5] = 1.0;
#pragma unroll
    for (int m = 0; m < 3; ++m) gp[m] = 0.0, vg[m] = 0.0;
    return;
  }
  const double lam = p.st->lam;
  double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
  for (int e = 0; e < k; ++e) {
    const double* L = p.lin + (int64_t)p.pt_list[off + e] * kBaLin;
    const double r0 = L[0], r1 = L[1];
    const double* A = L + 14;
    const double* B = L + 17;
    V[0] += A[0] * A[0] + B[0] * B[0];
    V[1] += A[0] * A[1] + B[0] * B[1];
    V[2] += A[0] * A[2] + B[0] * B[2];
    V[3] += A[1] * A[1] + B[1] * B[1];
    V[4] += A[1] * A[2] + B[1] * B[2];
    V[5] += A[2] * A[2] + B[2] * B[2];
#pragma unroll
    for (int m = 0; m < 3; ++m) g[m] += A[m] * r0 + B[m] * r1;
  }
  // V* = V + lam diag V = L L^T
  const double a00 = V[0] + lam * V[0], a11 = V[3] + lam * V[3], a22 = V[5] + lam * V[5];
  bool ok = a00 > 0.0 && finite_f64(a00);
  const double l00 = sqrt(a00), l10 = V[1] / l00, l20 = V[2] / l00;
  const double d1 = a11 - l10 * l10;
  ok = ok && d1 > 0.0 && finite_f64(d1);
  const double l11 = sqrt(d1), l21 = (V[4] - l20 * l10) / l11;
  const double d2 = (a22 - l20 * l20) - l21 * l21;
  ok = ok && d2 > 0.0 && finite_f64(d2);
  const double l22 = sqrt(d2);
  double Vi[6] = {0, 0, 0, 0, 0, 0};
  if (ok) {  // M = L^-1 (lower), V*^-1 = M^T M
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
    const double m10 = -(l10 * m00) / l11;
    const double m21 = -(l21 * m11) / l22;
    const double m20 = -(l20 * m00 + l21 * m10) / l22;
    Vi[0] = (m00 * m00 + m10 * m10) + m20 * m20;
    Vi[1] = m10 * m11 + m20 * m21;
    Vi[2] = m20 * m22;
    Vi[3] = m11 * m11 + m21 * m21;
    Vi[4] = m21 * m22;
    Vi[5] = m22 * m22;
  } else {
    p.st->fail = 1;  // (every writer stores the same word)
  }
#pragma unroll
  for (int m = 0; m < 6; ++m) vinv[m] = Vi[m];
  gp[0] = g[0], gp[1] = g[1], gp[2] = g[2];
  vg[0] = (Vi[0] * g[0] + Vi[1] * g[1]) + Vi[2] * g[2];
  vg[1] = (Vi[1] * g[0] + Vi[3] * g[1]) + Vi[4] * g[2];
  vg[2] = (Vi[2] * g[0] + Vi[4] * g[1]) + Vi[5] * g[2];
  // W_cj at the first observation of (c, j), summed over its duplicates in list order
  for (int e = 0; e < k; ++e) {
    const int c = clamp_index(p.cam_idx[p.pt_list[off + e]], p.n_cam);
    bool first = p.cam_active[c] != 0;
    for (int f = 0; f < e && first; ++f) first = clamp_index(p.cam_idx[p.pt_list[off + f]], p.n_cam) != c;
    p.lcam[off + e] = first ? c : -1;
    if (!first) continue;
    double W[6][3];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int m = 0; m < 3; ++m) W[a][m] = 0.0;
    for (int f = e; f < k; ++f) {
      const int of = p.pt_list[off + f];
      if (clamp_index(p.cam_idx[of], p.n_cam) != c) continue;
      const double* L = p.lin + (int64_t)of * kBaLin;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int m = 0; m < 3; ++m) W[a][m] += L[2 + a] * L[14 + m] + L[8 + a] * L[17 + m];
    }
    double* Wo = p.Wm + (int64_t)(off + e) * 18;
    double* Yo = p.Y + (int64_t)(off + e) * 18;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      Wo[3 * a] = W[a][0], Wo[3 * a + 1] = W[a][1], Wo[3 * a + 2] = W[a][2];
      Yo[3 * a] = (W[a][0] * Vi[0] + W[a][1] * Vi[1]) + W[a][2] * Vi[2];
      Yo[3 * a + 1] = (W[a][0] * Vi[1] + W[a][1] * Vi[3]) + W[a][2] * Vi[4];
      Yo[3 * a + 2] = (W[a][0] * Vi[2] + W[a][1] * Vi[4]) + W[a][2] * Vi[5];
    }
  }
}

// the entries of camera a's list that segment g of G walks: ceil(cnt / G) each, the last ones empty
SFM_DEV void ba_segment(int cnt, int g, int G, int& begin, int& end) {
  const int seg = (cnt + G - 1) / G;
  begin = min(g * seg, cnt);
  end = min(begin + seg, cnt);
}

// one wave per (camera a, segment g of its list): that segment's share of rows 6a .. 6a + 5 of S
// and of b (segment 0 also U*_a and -g_a), written to Spart [a][g].  LDS: [6][6 n_cam] + [6] doubles.
__global__ void __launch_bounds__(64) k_ba_schur(BaProblem p) {
  extern __shared__ __attribute__((aligned(16))) double s_row[];
  if (p.st->done) return;
  const int a = blockIdx.x, g = blockIdx.y, G = gridDim.y, lane = threadIdx.x;
  const int n6 = 6 * p.n_cam;
  double* s_b = s_row + 6 * n6;
  if (!p.cam_active[a]) return;  // fixed or unobserved: k_ba_schur_sum writes the identity block
  const int off = p.cam_off[a], cnt = p.cam_off[a + 1] - off;
  int e_begin, e_end;
  ba_segment(cnt, g, G, e_begin, e_end);
  if (e_begin >= e_end) return;  // an empty segment (never segment 0: an active camera has observations)
  for (int q = lane; q < 6 * n6 + 6; q += 64) s_row[q] = 0.0;
  const double lam = p.st->lam;
  if (g == 0) {  // U_a (upper triangle, row-major) and g_a over the whole list
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    for (int e = lane; e < cnt; e += 64) {
      const double* L = p.lin + (int64_t)p.cam_list[off + e] * kBaLin;
      double J0[6], J1[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) J0[k] = L[2 + k], J1[k] = L[8 + k];
      const double r0 = L[0], r1 = L[1];
      int k = 0;
#pragma unroll
      for (int x = 0; x < 6; ++x)
#pragma unroll
        for (int y = x; y < 6; ++y, ++k) acc[k] += J0[x] * J0[y] + J1[x] * J1[y];
#pragma unroll
      for (int x = 0; x < 6; ++x) acc[21 + x] += J0[x] * r0 + J1[x] * r1;
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = wave_sum_f64(acc[k]);
    __syncthreads();
    if (lane == 0) {
      int k = 0;
#pragma unroll
      for (int x = 0; x < 6; ++x)
#pragma unroll
        for (int y = x; y < 6; ++y, ++k) {
          s_row[x * n6 + 6 * a + y] = x == y ? acc[k] + lam * acc[k] : acc[k];
          s_row[y * n6 + 6 * a + x] = x == y ? acc[k] + lam * acc[k] : acc[k];
        }
#pragma unroll
      for (int x = 0; x < 6; ++x) s_b[x] = -acc[21 + x];
    }
  }
  __syncthreads();
  for (int e0 = e_begin; e0 < e_end; e0 += 64) {
    // each lane looks one entry up; the wave then takes them in order
    const int e = e0 + lane;
    int my_pos = -1, my_j = 0, my_base = 0, my_k = 0;
    if (e < e_end) {
      const int o = p.cam_list[off + e];
      const int ps = p.pos[o];
      if (p.lcam[ps] == a) {  // the first observation of (a, j): the merged block lives here
        my_pos = ps;
        my_j = clamp_index(p.pt_idx[o], p.n_pts);
        my_base = p.pt_off[my_j];
        my_k = p.pt_off[my_j + 1] - my_base;
      }
    }
    const int m = min(64, e_end - e0);
    for (int l = 0; l < m; ++l) {
      const int ps = __shfl(my_pos, l);
      if (ps < 0) continue;  // (the same for every lane)
      const int j = __shfl(my_j, l), base = __shfl(my_base, l), k = __shfl(my_k, l);
      const double* Yp = p.Y + (int64_t)ps * 18;
      for (int q = lane; q < k * 36; q += 64) {
        const int ep = base + q / 36, el = q % 36;
        const int b = p.lcam[ep];
        if (b < 0) continue;
        const int r = el / 6, s = el % 6;
        const double* Wp = p.Wm + (int64_t)ep * 18 + 3 * s;
        s_row[r * n6 + 6 * b + s] -= (Yp[3 * r] * Wp[0] + Yp[3 * r + 1] * Wp[1]) + Yp[3 * r + 2] * Wp[2];
      }
      if (lane < 6) {
        const double* g = p.gp + 3 * (int64_t)j;
        s_b[lane] += (Yp[3 * lane] * g[0] + Yp[3 * lane + 1] * g[1]) + Yp[3 * lane + 2] * g[2];
      }
      __syncthreads();
    }
  }
  __syncthreads();
  double* P = p.Spart + ((int64_t)a * G + g) * (6 * n6 + 6);
  for (int q = lane; q < 6 * n6 + 6; q += 64) P[q] = s_row[q];
}

// one workgroup per camera a: rows 6a .. 6a + 5 of S and of b, the segments summed in order
__global__ void __launch_bounds__(kBaThreads) k_ba_schur_sum(BaProblem p, int G) {
  if (p.st->done) return;
  const int a = blockIdx.x, tid = threadIdx.x;
  const int n6 = 6 * p.n_cam;
  double* Sg = p.S + (int64_t)6 * a * n6;
  if (!p.cam_active[a]) {
    for (int q = tid; q < 6 * n6; q += kBaThreads) Sg[q] = (q % n6 == 6 * a + q / n6) ? 1.0 : 0.0;
    if (tid < 6) p.b[6 * a + tid] = 0.0;
    return;
  }
  const int cnt = p.cam_off[a + 1] - p.cam_off[a];
  const int seg = (cnt + G - 1) / G, used = (cnt + seg - 1) / seg;  // the segments that are not empty
  const double* P = p.Spart + (int64_t)a * G * (6 * n6 + 6);
  for (int q = tid; q < 6 * n6 + 6; q += kBaThreads) {
    double v = P[q];
    for (int g = 1; g < used; ++g) v += P[(int64_t)g * (6 * n6 + 6) + q];
    if (q < 6 * n6) {
      Sg[q] = v;
    } else {
      p.b[6 * a + (q - 6 * n6)] = v;
    }
  }
}

// one workgroup: S = L L^T in place (lower triangle), L y = b, L^T d = y.  n6 <= 1536.
__global__ void __launch_bounds__(kBaSolveThreads) k_ba_solve(BaProblem p) {
  __shared__ double s_col[6 * 256], s_rhs[6 * 256];
  __shared__ int s_fail;
  if (p.st->done) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = 6 * p.n_cam;
  double* A = p.S;
  if (tid == 0) s_fail = 0;
  for (int i = tid; i < n; i += kBaSolveThreads) s_rhs[i] = p.b[i];
  for (int k = 0; k < n; ++k) {
    __syncthreads();  // the trailing update of column k - 1 is done
    if (tid == 0) {
      const double d = A[(int64_t)k * n + k];
      if (d > 0.0 && finite_f64(d)) {
        A[(int64_t)k * n + k] = s_col[k] = sqrt(d);
      } else {
        s_fail = 1;
      }
    }
    __syncthreads();
    if (s_fail) break;  // (uniform)
    const double lkk = s_col[k];
    for (int i = k + 1 + tid; i < n; i += kBaSolveThreads) {
      const double v = A[(int64_t)i * n + k] / lkk;
      A[(int64_t)i * n + k] = v;
      s_col[i] = v;
    }
    __syncthreads();
    for (int i = k + 1 + wave; i < n; i += kBaSolveThreads / 64) {
      const double li = s_col[i];
      double* Ai = A + (int64_t)i * n;
      for (int j = k + 1 + lane; j <= i; j += 64) Ai[j] -= li * s_col[j];
    }
  }
  __syncthreads();
  if (s_fail) {
    if (tid == 0) p.st->fail = 1;
    for (int i = tid; i < n; i += kBaSolveThreads) p.delta[i] = 0.0;
    return;
  }
  for (int k = 0; k < n; ++k) {  // forward, by columns
    __syncthreads();
    if (tid == 0) s_rhs[k] = s_rhs[k] / A[(int64_t)k * n + k];
    __syncthreads();
    const double yk = s_rhs[k];
    for (int i = k + 1 + tid; i < n; i += kBaSolveThreads) s_rhs[i] -= A[(int64_t)i * n + k] * yk;
  }
  for (int k = n - 1; k >= 0; --k) {  // backward, by rows of L
    __syncthreads();
    if (tid == 0) s_rhs[k] = s_rhs[k] / A[(int64_t)k * n + k];
    __syncthreads();
    const double xk = s_rhs[k];
    for (int i = tid; i < k; i += kBaSolveThreads) s_rhs[i] -= A[(int64_t)k * n + i] * xk;
  }
  __syncthreads();
  for (int i = tid; i < n; i += kBaSolveThreads) p.delta[i] = s_rhs[i];
}

// the candidate state in the other slot; nrm [n_pts + n_cam][2] = |d|^2, |params|^2 per row
__global__ void __launch_bounds__(kBaThreads) k_ba_update(BaProblem p) {
  if (p.st->done) return;
  const int64_t i = (int64_t)blockIdx.x * kBaThreads + threadIdx.x;
  const int cur = p.st->cur;
  if (i < p.n_pts) {
    const int off = p.pt_off[i], k = p.pt_off[i + 1] - off;
    double acc[3] = {0, 0, 0};
    for (int e = 0; e < k; ++e) {
      const int b = p.lcam[off + e];
      if (b < 0) continue;
      const double* W = p.Wm + (int64_t)(off + e) * 18;
      const double* d = p.delta + 6 * b;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        double s = W[m] * d[0];
#pragma unroll
        for (int a = 1; a < 6; ++a) s += W[3 * a + m] * d[a];
        acc[m] += s;
      }
    }
    const double* Vi = p.vinv + 6 * i;
    const double* vg = p.vg + 3 * i;
    const double dX[3] = {-(vg[0] + ((Vi[0] * acc[0] + Vi[1] * acc[1]) + Vi[2] * acc[2])),
                          -(vg[1] + ((Vi[1] * acc[0] + Vi[3] * acc[1]) + Vi[4] * acc[2])),
                          -(vg[2] + ((Vi[2] * acc[0] + Vi[4] * acc[1]) + Vi[5] * acc[2]))};
    const double* X = p.Xs + ((int64_t)cur * p.n_pts + i) * 3;
    double* Xn = p.Xs + ((int64_t)(cur ^ 1) * p.n_pts + i) * 3;
#pragma unroll
    for (int m = 0; m < 3; ++m) Xn[m] = k ? X[m] + dX[m] : X[m];
    p.nrm[2 * i] = k ? (dX[0] * dX[0] + dX[1] * dX[1]) + dX[2] * dX[2] : 0.0;
    p.nrm[2 * i + 1] = (X[0] * X[0] + X[1] * X[1]) + X[2] * X[2];
  } else if (i < (int64_t)p.n_pts + p.n_cam) {
    const int c = (int)(i - p.n_pts);
    const double* Rt = p.Rt + ((int64_t)cur * p.n_cam + c) * 12;
    double* Rn = p.Rt + ((int64_t)(cur ^ 1) * p.n_cam + c) * 12;
    const bool act = p.cam_active[c] != 0;
    double d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = act ? p.delta[6 * c + k] : 0.0;
    if (act) {
      double E[9];
      rodrigues(d[0], d[1], d[2], E);
      compose3(E, Rt, Rn);
#pragma unroll
      for (int k = 0; k < 3; ++k) Rn[9 + k] = Rt[9 + k] + d[3 + k];
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) Rn[k] = Rt[k];
    }
    double dd = d[0] * d[0];
#pragma unroll
    for (int k = 1; k < 6; ++k) dd += d[k] * d[k];
    p.nrm[2 * i] = dd;
    p.nrm[2 * i + 1] = (Rt[9] * Rt[9] + Rt[10] * Rt[10]) + Rt[11] * Rt[11];
  }
}

// first: the start cost (of the current state); otherwise the accept test of the candidate
__global__ void __launch_bounds__(kBaThreads) k_ba_decide(BaProblem p, int first) {
  __shared__ double s_red[kBaThreads];
  BaState* s = p.st;
  if (s->done) return;  // (uniform: nothing below has written it yet)
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < p.M; i += kBaThreads) acc += p.e2[i];
  const double cost_new = block_sum256_tree(acc, s_red);
  double d2 = 0.0, p2 = 0.0;
  if (!first) {
    const int64_t rows = (int64_t)p.n_pts + p.n_cam;
    double ad = 0.0, ap = 0.0;
    for (int64_t i = tid; i < rows; i += kBaThreads) {
      ad += p.nrm[2 * i];
      ap += p.nrm[2 * i + 1];
    }
    d2 = block_sum256_tree(ad, s_red);
    p2 = block_sum256_tree(ap, s_red);
  }
  if (tid != 0) return;
  if (first) {
    s->cost0 = s->cost = cost_new;
    if (!finite_f64(cost_new)) {
      s->status = kRefineNonFinite;
      s->done = 1;
    }
    return;
  }
  s->iters += 1;
  if (s->fail) s->rejected += 1;
  const double cost = s->cost;
  if (!s->fail && finite_f64(cost_new) && cost_new < cost) {
    const double rel = (cost - cost_new) / cost;
    s->accepted += 1;
    s->cost = cost_new;
    s->cur ^= 1;
    s->lam = fmax(s->lam / 10.0, 1e-12);
    if (rel <= p.ftol || sqrt(d2) <= 1e-14 * fmax(1.0, sqrt(p2))) {
      s->status = kRefineConverged;
      s->done = 1;
    }
  } else {
    s->lam *= 10.0;
    if (s->lam > 1e12) {
      s->status = kRefineLambda;
      s->done = 1;
    }
  }
  s->fail = 0;
}

__global__ void __launch_bounds__(kBaThreads) k_ba_finish(BaProblem p) {
  const int64_t i = (int64_t)blockIdx.x * kBaThreads + threadIdx.x;
  const BaState* s = p.st;
  const bool moved = s->accepted > 0;
  if (i == 0) {
    if (p.out_cost) p.out_cost[0] = s->cost0, p.out_cost[1] = s->cost;
    if (p.out_status) {
      p.out_status[0] = s->status;
      p.out_status[1] = s->accepted;
      p.out_status[2] = s->iters;
      p.out_status[3] = s->rejected;
    }
  }
  if (i < p.n_pts) {
    const double* X = moved ? p.Xs + ((int64_t)s->cur * p.n_pts + i) * 3 : p.X_in + 3 * i;
#pragma unroll
    for (int k = 0; k < 3; ++k) p.out_X[3 * i + k] = X[k];
  } else if (i < (int64_t)p.n_pts + p.n_cam) {
    const int c = (int)(i - p.n_pts);
    double o[6];
    if (moved && p.cam_active[c]) {
      const double* Rt = p.Rt + ((int64_t)s->cur * p.n_cam + c) * 12;
      double R[9], r[3];
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = Rt[k];
      rodrigues_inv(R, r);
#pragma unroll
      for (int k = 0; k < 3; ++k) o[k] = r[k], o[3 + k] = Rt[9 + k];
    } else {  // a row that never moved: its input bits
#pragma unroll
      for (int k = 0; k < 6; ++k) o[k] = p.cams_in[6 * c + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) p.out_cams[6 * c + k] = o[k];
  }
}

size_t ba_schur_lds_bytes(int n_cam) { return ((size_t)36 * n_cam + 6) * 8; }

// segments per camera list: as many as kBaSchurBudget bytes of partial rows allow, at most 64
int ba_schur_split(int n_cam) {
  const size_t per = (size_t)n_cam * ba_schur_lds_bytes(n_cam);
  return (int)std::min<size_t>(kBaMaxSplit, std::max<size_t>(1, kBaSchurBudget / per));
}

void launch_bundle_adjust(const BaProblem& p, hipStream_t st) {
  static const bool lds_attr = [] {  // 72 KiB + 48 B at 256 cameras
    return hipFuncSetAttribute((const void*)k_ba_schur, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)ba_schur_lds_bytes(kBaMaxCams)) == hipSuccess;
  }();
  (void)lds_attr;
  const dim3 tb(kBaThreads);
  const dim3 g_obs((unsigned)((p.M + kBaThreads - 1) / kBaThreads));
  const dim3 g_pts((unsigned)((p.n_pts + kBaThreads - 1) / kBaThreads));
  const dim3 g_rows((unsigned)(((int64_t)p.n_pts + p.n_cam + kBaThreads - 1) / kBaThreads));
  hipLaunchKernelGGL(k_ba_init, g_rows, tb, 0, st, p);
  hipLaunchKernelGGL(k_ba_count, g_obs, tb, 0, st, p);
  hipLaunchKernelGGL(k_ba_scan, dim3(1), tb, 0, st, p);
  hipLaunchKernelGGL(k_ba_fill_pt, g_obs, tb, 0, st, p);
  hipLaunchKernelGGL(k_ba_sort_pt, g_pts, tb, 0, st, p);
  hipLaunchKernelGGL(k_ba_fill_cam, dim3(p.n_cam), tb, 0, st, p);
  hipLaunchKernelGGL(k_ba_resid, g_obs, tb, 0, st, p, 0);
  hipLaunchKernelGGL(k_ba_decide, dim3(1), tb, 0, st, p, 1);
  for (int it = 0; it < p.max_iter; ++it) {
    hipLaunchKernelGGL(k_ba_lin, g_obs, tb, 0, st, p);
    hipLaunchKernelGGL(k_ba_point, g_pts, tb, 0, st, p);
    hipLaunchKernelGGL(k_ba_schur, dim3(p.n_cam, p.schur_split), dim3(64), ba_schur_lds_bytes(p.n_cam), st, p);
    hipLaunchKernelGGL(k_ba_schur_sum, dim3(p.n_cam), tb, 0, st, p, p.schur_split);
    hipLaunchKernelGGL(k_ba_solve, dim3(1), dim3(kBaSolveThreads), 0, st, p);
    hipLaunchKernelGGL(k_ba_update, g_rows, tb, 0, st, p);
    hipLaunchKernelGGL(k_ba_resid, g_obs, tb, 0, st, p, 1);
    hipLaunchKernelGGL(k_ba_decide, dim3(1), tb, 0, st, p, 0);
  }
  hipLaunchKernelGGL(k_ba_finish, g_rows, tb, 0, st, p);
}

}  // namespace sfm
