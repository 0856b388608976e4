// pnp.hip — the pose of every frame after the second (Runner.py:257-262, PoseEstimator.py):
// the library's own PnP rule (include/sfmfeat.h sfm_pnp_ransac_dev), in the
// spirit of cv2.solvePnPRansac(reprojectionError = 8, SOLVEPNP_ITERATIVE) — minimal-sample
// hypotheses, inliers under a reprojection threshold, iterative refinement of the winner on
// its inliers.  Parity with OpenCV is not pinned.
//
// * k_pnp_hyp, one thread per sample: the first 6 indices of the np.random.seed(5) stream
//   (ransac.hip), image points through K^-1, the six world points Hartley-normalised, the
//   first 11 rows of the 12 x 12 DLT system, its null vector with the last component 1 by
//   Gaussian elimination with partial pivoting (first row of the largest magnitude),
//   P -> (R, t) by the polar factor of P[:, :3].  The 11 x 12 system lives in LDS as
//   [entry][lane] (a wave's accesses are conflict-free and the pivot's runtime row index is an
//   address, not a register index): 66 KB per wave, one wave per workgroup.
// * k_pnp_count, one wave per sample, 8 samples per workgroup: the points staged in LDS as
//   float64 (structure of arrays) in chunks of kRansacChunk; lanes take points lane,
//   lane + 64, ..; the count is the sum of the rounds' ballots.  A NaN hypothesis counts 0.
// * k_pnp_select: the first strict maximum, its mask recomputed with the same test, the
//   inlier indices compacted in input order, the winner's (R, t) copied out.
// * k_pnp_refine, one 256-thread workgroup, the whole Levenberg-Marquardt in one launch: per
//   iteration one pass over the points at the trial pose accumulates J^T J (21), J^T r (6) and
//   the cost, which serve the accept test and, if accepted, the next solve.  Sums run per
//   thread in index order, then wave butterflies, then the four waves in order: no atomics,
//   the same bits every run.  Every thread solves the 6 x 6 system redundantly.
// * k_pnp_dlt_all (PnP without RANSAC): the same DLT over all points — A^T A from 40 sums
//   (its 78 distinct entries are those of sum W, sum u W, sum v W, sum (u^2 + v^2) W with
//   W = Yh Yh^T), the eigenvector of its smallest eigenvalue by cyclic Jacobi on the matrix
//   in LDS, the same P -> (R, t).
// Float64 throughout; -ffp-contract=off, fmas written where wanted.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "f64_dev.h"
#include "kernels.h"
#include "linalg3.h"

namespace sfm {

constexpr int kPnpWaves = 8;     // samples (waves) per workgroup of k_pnp_count
constexpr int kPnpThreads = 256; // k_pnp_select, k_pnp_refine, k_pnp_dlt_all

// K^-1 (u, v, 1) for upper-triangular K, by back substitution
SFM_DEV void normalised_pixel(const double* __restrict__ K, double u, double v, double& un, double& vn) {
  const double w = 1.0 / K[8];
  const double vh = (v - K[5] * w) / K[4];
  const double uh = ((u - K[1] * vh) - K[2] * w) / K[0];
  un = uh / w;
  vn = vh / w;
}

// p: a projection matrix (row-major 3 x 4, up to scale and sign) for world points normalised as
// Y = s (X - c) and normalised image points -> Rt = R (9, row-major), t (3) for the points
// themselves: R the polar factor of M = P[:, :3] (negated when det M < 0), M = sigma R with
// sigma the mean singular value, t = (P[:, 3] / sigma - s R c) / s.  All NaN unless all finite.
SFM_DEV void pose_from_p(const double (&p)[12], double s, const double (&c)[3], double (&Rt)[12]) {
  double M[3][3], p4[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) M[r][k] = p[4 * r + k];
    p4[r] = p[4 * r + 3];
  }
  const double sg = det3(M) < 0 ? -1.0 : 1.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) M[r][k] *= sg;
    p4[r] *= sg;
  }
  double S[3][3], V[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) S[r][k] = (M[0][r] * M[0][k] + M[1][r] * M[1][k]) + M[2][r] * M[2][k];
  jacobi_eig3(S, V);
  const double q0 = sqrt(S[0][0]), q1 = sqrt(S[1][1]), q2 = sqrt(S[2][2]);  // the singular values of M
  double B[3][3];  // (M^T M)^(-1/2)
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k)
      B[r][k] = (V[r][0] * V[k][0] / q0 + V[r][1] * V[k][1] / q1) + V[r][2] * V[k][2] / q2;
  const double sigma = ((q0 + q1) + q2) / 3.0;
  bool ok = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Rt[3 * r + k] = (M[r][0] * B[0][k] + M[r][1] * B[1][k]) + M[r][2] * B[2][k];
      ok = ok && finite_f64(Rt[3 * r + k]);
    }
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double Rc = (Rt[3 * r] * c[0] + Rt[3 * r + 1] * c[1]) + Rt[3 * r + 2] * c[2];
    Rt[9 + r] = (p4[r] / sigma - s * Rc) / s;
    ok = ok && finite_f64(Rt[9 + r]);
  }
  if (!ok) {
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = __builtin_nan("");
  }
}

// one thread per sample: hyp [iters][12] = R, t (NaN for a degenerate sample).  idx [iters][stride],
// the first 6 of each row used (entries are clamped to [0, n): the stream is the library's own).
__global__ void __launch_bounds__(64) k_pnp_hyp(const double* __restrict__ X, const double* __restrict__ x,
                                                const double* __restrict__ K, int n,
                                                const int32_t* __restrict__ idx, int stride, int iters,
                                                double* __restrict__ hyp) {
  extern __shared__ __attribute__((aligned(16))) double s_A[];  // [11 * 12][64]
  const int lane = threadIdx.x;
  const int it = blockIdx.x * 64 + lane;
  if (it >= iters) return;  // (the kernel has no barrier)
#define PNP_A(r, k) s_A[((r) * 12 + (k)) * 64 + lane]
  double Xs[6][3], un[6], vn[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int j = clamp_index(idx[(int64_t)it * stride + i], n);
#pragma unroll
    for (int k = 0; k < 3; ++k) Xs[i][k] = X[3 * (int64_t)j + k];
    normalised_pixel(K, x[2 * (int64_t)j], x[2 * (int64_t)j + 1], un[i], vn[i]);
  }
  double c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double a = Xs[0][k];
#pragma unroll
    for (int i = 1; i < 6; ++i) a += Xs[i][k];
    c[k] = a / 6.0;
  }
  double md = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) Xs[i][k] -= c[k];
    const double d = sqrt((Xs[i][0] * Xs[i][0] + Xs[i][1] * Xs[i][1]) + Xs[i][2] * Xs[i][2]);
    md = i ? md + d : d;
  }
  const double s = sqrt(3.0) / (md / 6.0);
  // rows 2i = [Yh, 0, -u Yh], 2i + 1 = [0, Yh, -v Yh]; the sixth point's second row is left out
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double Yh[4] = {s * Xs[i][0], s * Xs[i][1], s * Xs[i][2], 1.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      PNP_A(2 * i, k) = Yh[k];
      PNP_A(2 * i, 4 + k) = 0.0;
      PNP_A(2 * i, 8 + k) = -un[i] * Yh[k];
      if (i < 5) {
        PNP_A(2 * i + 1, k) = 0.0;
        PNP_A(2 * i + 1, 4 + k) = Yh[k];
        PNP_A(2 * i + 1, 8 + k) = -vn[i] * Yh[k];
      }
    }
  }
  // A[:, :11] z = -A[:, 11]: elimination with partial pivoting, then back substitution with
  // p[11] = 1; p[i] replaces A[i][11]
  bool ok = true;
  for (int col = 0; col < 11; ++col) {
    int best = col;
    double bv = fabs(PNP_A(col, col));
    for (int i = col + 1; i < 11; ++i) {
      const double v = fabs(PNP_A(i, col));
      if (v > bv) {
        bv = v;
        best = i;
      }
    }
    if (!(bv >= 1e-300)) {
      ok = false;
      break;
    }
    if (best != col)
      for (int k = col; k < 12; ++k) {
        const double a = PNP_A(col, k);
        PNP_A(col, k) = PNP_A(best, k);
        PNP_A(best, k) = a;
      }
    const double piv = PNP_A(col, col);
    for (int i = col + 1; i < 11; ++i) {
      const double f = PNP_A(i, col) / piv;
      for (int k = col; k < 12; ++k) PNP_A(i, k) = PNP_A(i, k) - f * PNP_A(col, k);
    }
  }
  double Rt[12];
  if (ok) {
    for (int i = 10; i >= 0; --i) {
      double acc = 0.0;
      for (int k = i + 1; k < 11; ++k) acc = acc + PNP_A(i, k) * PNP_A(k, 11);
      acc = acc + PNP_A(i, 11);  // p[11] = 1
      PNP_A(i, 11) = -acc / PNP_A(i, i);
    }
    double p[12];
#pragma unroll
    for (int k = 0; k < 11; ++k) p[k] = PNP_A(k, 11);
    p[11] = 1.0;
    pose_from_p(p, s, c, Rt);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = __builtin_nan("");
  }
#undef PNP_A
  double* o = hyp + (int64_t)it * 12;
#pragma unroll
  for (int k = 0; k < 12; ++k) o[k] = Rt[k];
}

// depth > 0 and |pi(K (R X + t)) - x| < thr; a NaN compares false
SFM_DEV bool pnp_inlier(const double (&Kc)[6], const double (&R)[9], const double (&t)[3], double X0, double X1,
                        double X2, double u, double v, double thr) {
  double Y[3];
  rotate3(R, X0, X1, X2, Y);
  const double a0 = Y[0] + t[0], a1 = Y[1] + t[1], a2 = Y[2] + t[2];
  const double q0 = (Kc[0] * a0 + Kc[1] * a1) + Kc[2] * a2;
  const double q1 = Kc[3] * a1 + Kc[4] * a2;
  const double q2 = Kc[5] * a2;
  const double dx = q0 / q2 - u, dy = q1 / q2 - v;
  return a2 > 0.0 && sqrt(dx * dx + dy * dy) < thr;
}

SFM_DEV void load_K6(const double* __restrict__ K, double (&Kc)[6]) {  // the upper triangle
  Kc[0] = K[0], Kc[1] = K[1], Kc[2] = K[2], Kc[3] = K[4], Kc[4] = K[5], Kc[5] = K[8];
}

__global__ void __launch_bounds__(64 * kPnpWaves) k_pnp_count(const double* __restrict__ X,
                                                              const double* __restrict__ x,
                                                              const double* __restrict__ K, int n,
                                                              const double* __restrict__ hyp, int iters, double thr,
                                                              int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) double s_p[];  // [5][cn]: X0, X1, X2, u, v
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int it = blockIdx.x * kPnpWaves + wave;
  const bool have = it < iters;
  const int cn = min(n, kRansacChunk);
  double Kc[6], R[9], t[3];
  load_K6(K, Kc);
  const double* H = hyp + (int64_t)(have ? it : 0) * 12;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = H[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = H[9 + k];
  const bool live = have && finite_f64(R[0]);  // (a NaN hypothesis is NaN throughout)
  uint32_t c = 0;
  for (int i0 = 0; i0 < n; i0 += kRansacChunk) {
    const int m = min(kRansacChunk, n - i0);
    if (i0) __syncthreads();  // every wave is done with the previous chunk
    for (int i = threadIdx.x; i < m; i += 64 * kPnpWaves) {
      const int64_t g = i0 + i;
      s_p[i] = X[3 * g];
      s_p[cn + i] = X[3 * g + 1];
      s_p[2 * cn + i] = X[3 * g + 2];
      s_p[3 * cn + i] = x[2 * g];
      s_p[4 * cn + i] = x[2 * g + 1];
    }
    __syncthreads();
    if (live)
      for (int r0 = 0; r0 < m; r0 += 64) {
        const int i = r0 + lane;
        bool in = false;
        if (i < m)
          in = pnp_inlier(Kc, R, t, s_p[i], s_p[cn + i], s_p[2 * cn + i], s_p[3 * cn + i], s_p[4 * cn + i], thr);
        c += (uint32_t)__popcll(__ballot(in));
      }
  }
  if (have && lane == 0) counts[it] = live ? (int32_t)c : 0;
}

// the first sample with the strictly largest count; out_n = -1 (n < 6) or 0 and out_iter = -1,
// Rt = NaN when there is no pose
__global__ void __launch_bounds__(kPnpThreads) k_pnp_select(const double* __restrict__ X,
                                                            const double* __restrict__ x,
                                                            const double* __restrict__ K, int n,
                                                            const double* __restrict__ hyp,
                                                            const int32_t* __restrict__ counts, int iters, double thr,
                                                            int32_t* __restrict__ out_inliers,
                                                            int32_t* __restrict__ out_n, int32_t* __restrict__ out_iter,
                                                            double* __restrict__ out_Rt) {
  __shared__ int s_bc[kPnpThreads], s_bi[kPnpThreads];
  __shared__ uint32_t s_scan[kPnpThreads / 64 + 1];
  const int tid = threadIdx.x;
  int bc = -1, bi = 0x7fffffff;
  if (n >= 6)
    for (int it = tid; it < iters; it += kPnpThreads) {
      const int c = counts[it];
      if (c > bc) {  // ascending it per thread: the first maximum is kept
        bc = c;
        bi = it;
      }
    }
  s_bc[tid] = bc;
  s_bi[tid] = bi;
  __syncthreads();
  for (int off = kPnpThreads / 2; off >= 1; off >>= 1) {
    if (tid < off) {
      const int oc = s_bc[tid + off], oi = s_bi[tid + off];
      if (oc > s_bc[tid] || (oc == s_bc[tid] && oi < s_bi[tid])) {
        s_bc[tid] = oc;
        s_bi[tid] = oi;
      }
    }
    __syncthreads();
  }
  const int best = s_bi[0];
  if (s_bc[0] <= 0) {  // n < 6, no iterations, or no sample with an inlier
    if (tid == 0) {
      *out_n = n < 6 ? -1 : 0;
      *out_iter = -1;
    }
    if (tid < 12) out_Rt[tid] = __builtin_nan("");
    return;
  }
  double Kc[6], R[9], t[3];
  load_K6(K, Kc);
  const double* H = hyp + (int64_t)best * 12;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = H[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = H[9 + k];
  uint32_t base = 0;
  for (int i0 = 0; i0 < n; i0 += kPnpThreads) {
    const int i = i0 + tid;
    bool in = false;
    if (i < n)  // the same test as k_pnp_count, so the mask has the count
      in = pnp_inlier(Kc, R, t, X[3 * (int64_t)i], X[3 * (int64_t)i + 1], X[3 * (int64_t)i + 2], x[2 * (int64_t)i],
                      x[2 * (int64_t)i + 1], thr);
    uint32_t total;
    const uint32_t pos = block_exclusive_scan(in ? 1u : 0u, s_scan, &total);
    if (in) out_inliers[base + pos] = i;
    base += total;
  }
  if (tid == 0) {
    *out_n = (int32_t)base;
    *out_iter = best;
  }
  if (tid < 12) out_Rt[tid] = H[tid];
}

// ---------------- refinement: a 6-parameter Levenberg-Marquardt in one workgroup ----------------

constexpr int kPnpSums = 28;  // J^T J upper triangle (21, row-major), J^T r (6), cost

// adds one point's terms at the pose (R, t): r = pi(K (R X + t)) - x, rows [Y x g_a, g_a] with
// Y = R X and g_a = d r_a / d X_c
SFM_DEV void pnp_accumulate(const double (&Kc)[6], const double (&R)[9], const double (&t)[3], double X0, double X1,
                            double X2, double u, double v, double (&acc)[kPnpSums]) {
  double Y[3];
  rotate3(R, X0, X1, X2, Y);
  const double a0 = Y[0] + t[0], a1 = Y[1] + t[1], a2 = Y[2] + t[2];
  const double q0 = (Kc[0] * a0 + Kc[1] * a1) + Kc[2] * a2;
  const double q1 = Kc[3] * a1 + Kc[4] * a2;
  const double q2 = Kc[5] * a2;
  const double pu = q0 / q2, pv = q1 / q2;
  const double r0 = pu - u, r1 = pv - v;
  const double g0[3] = {Kc[0] / q2, Kc[1] / q2, (Kc[2] - pu * Kc[5]) / q2};
  const double g1[3] = {0.0, Kc[3] / q2, (Kc[4] - pv * Kc[5]) / q2};
  const double J0[6] = {Y[1] * g0[2] - Y[2] * g0[1], Y[2] * g0[0] - Y[0] * g0[2], Y[0] * g0[1] - Y[1] * g0[0],
                        g0[0], g0[1], g0[2]};
  const double J1[6] = {Y[1] * g1[2] - Y[2] * g1[1], Y[2] * g1[0] - Y[0] * g1[2], Y[0] * g1[1] - Y[1] * g1[0],
                        g1[0], g1[1], g1[2]};
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b, ++k) acc[k] = fma(J1[a], J1[b], fma(J0[a], J0[b], acc[k]));
#pragma unroll
  for (int a = 0; a < 6; ++a) acc[21 + a] = fma(J1[a], r1, fma(J0[a], r0, acc[21 + a]));
  acc[27] = fma(r1, r1, fma(r0, r0, acc[27]));
}

// sums over the m points (inl: their indices, or nullptr for 0..m-1) at (R, t); every thread gets them
SFM_DEV void pnp_evaluate(const double* __restrict__ X, const double* __restrict__ x, const int32_t* __restrict__ inl,
                          int m, int n, const double (&Kc)[6], const double (&R)[9], const double (&t)[3],
                          double (*s_red)[kPnpSums], double (&out)[kPnpSums]) {
  const int tid = threadIdx.x;
  double acc[kPnpSums];
#pragma unroll
  for (int k = 0; k < kPnpSums; ++k) acc[k] = 0.0;
  for (int i = tid; i < m; i += kPnpThreads) {
    const int j = clamp_index(inl ? inl[i] : i, n);
    pnp_accumulate(Kc, R, t, X[3 * (int64_t)j], X[3 * (int64_t)j + 1], X[3 * (int64_t)j + 2], x[2 * (int64_t)j],
                   x[2 * (int64_t)j + 1], acc);
  }
  __syncthreads();  // the previous evaluation's reads of s_red are done
#pragma unroll
  for (int k = 0; k < kPnpSums; ++k) {
    const double w = wave_sum_f64(acc[k]);
    if ((tid & 63) == 0) s_red[tid >> 6][k] = w;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kPnpSums; ++k) out[k] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
}

// (H + lam diag H) d = -g by Cholesky; a pivot <= 0 gives NaN / inf, which the cost test rejects
SFM_DEV void pnp_solve6(const double (&s)[kPnpSums], double lam, double (&d)[6]) {
  double A[6][6], L[6][6];
  int k = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b, ++k) A[b][a] = a == b ? fma(lam, s[k], s[k]) : s[k];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double dj = A[j][j];
#pragma unroll
    for (int q = 0; q < j; ++q) dj = fma(-L[j][q], L[j][q], dj);
    L[j][j] = sqrt(dj);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int q = 0; q < j; ++q) v = fma(-L[i][q], L[j][q], v);
      L[i][j] = v / L[j][j];
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = -s[21 + i];
#pragma unroll
    for (int q = 0; q < i; ++q) v = fma(-L[i][q], y[q], v);
    y[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int q = i + 1; q < 6; ++q) v = fma(-L[q][i], d[q], v);
    d[i] = v / L[i][i];
  }
}

// Rt_in: the start pose (R, t).  count_p (with inl): the number of inliers on the device, <= 0
// for "no pose"; without inl the n points themselves.  out_status: found, LM status, accepted
// steps, iterations run; out_cost: the cost at the start and at the returned pose.
__global__ void __launch_bounds__(kPnpThreads) k_pnp_refine(const double* __restrict__ X,
                                                            const double* __restrict__ x,
                                                            const double* __restrict__ K, int n,
                                                            const int32_t* __restrict__ inl,
                                                            const int32_t* __restrict__ count_p,
                                                            const double* __restrict__ Rt_in, int max_iter,
                                                            double* __restrict__ out_R, double* __restrict__ out_t,
                                                            int32_t* __restrict__ out_status,
                                                            double* __restrict__ out_cost) {
  __shared__ double s_red[kPnpThreads / 64][kPnpSums];
  const int tid = threadIdx.x;
  int m = inl ? *count_p : n;
  m = m > n ? n : m;
  double R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = Rt_in[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = Rt_in[9 + k];
  if (m <= 0 || !finite_f64(R[0])) {  // no pose (uniform over the workgroup)
    if (tid < 9) out_R[tid] = __builtin_nan("");
    if (tid < 3) out_t[tid] = __builtin_nan("");
    if (tid < 2) out_cost[tid] = __builtin_nan("");
    if (tid < 4) out_status[tid] = tid == 1 ? -1 : 0;
    return;
  }
  double Kc[6];
  load_K6(K, Kc);
  double cur[kPnpSums];
  pnp_evaluate(X, x, inl, m, n, Kc, R, t, s_red, cur);
  const double cost0 = cur[27];
  int accepted = 0, ran = 0, status = kRefineMaxIter;
  if (!finite_f64(cost0)) {
    status = kRefineNonFinite;
  } else {
    double lam = 1e-3;
    for (int it = 0; it < max_iter; ++it) {
      ++ran;
      double d[6], E[9], Rn[9], tn[3], tr[kPnpSums];
      pnp_solve6(cur, lam, d);
      rodrigues(d[0], d[1], d[2], E);  // Rn = exp([d omega]x) R
      compose3(E, R, Rn);
#pragma unroll
      for (int k = 0; k < 3; ++k) tn[k] = t[k] + d[3 + k];
      pnp_evaluate(X, x, inl, m, n, Kc, Rn, tn, s_red, tr);
      if (tr[27] < cur[27]) {  // every thread holds the same bits: a uniform branch
        double nd = d[0] * d[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) nd = fma(d[k], d[k], nd);
        nd = sqrt(nd);
        const double nt = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = tn[k];
#pragma unroll
        for (int k = 0; k < kPnpSums; ++k) cur[k] = tr[k];
        lam = fmax(lam / 10.0, 1e-12);
        ++accepted;
        if (nd <= 1e-14 * fmax(1.0, nt)) {
          status = kRefineConverged;
          break;
        }
      } else {
        lam *= 10.0;
        if (lam > 1e12) {
          status = kRefineLambda;
          break;
        }
      }
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) out_R[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) out_t[k] = t[k];
    out_status[0] = 1;
    out_status[1] = status;
    out_status[2] = accepted;
    out_status[3] = ran;
    out_cost[0] = cost0;
    out_cost[1] = cur[27];
  }
}

// ---------------- PnP over all points: the DLT's start pose ----------------

constexpr int kPnpDltSums = 40;  // 10 each of sum W, sum u W, sum v W, sum (u^2 + v^2) W

// the sum over 256 threads as pnp_evaluate takes it: wave butterflies, then the four waves in
// order; every thread gets the sum.  (f64_dev.h's block_sum256_tree sums in another order: the
// two do not agree in the last bit.)
SFM_DEV double block_sum256_waves(double v, double* s4) {
  const int tid = threadIdx.x;
  const double w = wave_sum_f64(v);
  __syncthreads();
  if ((tid & 63) == 0) s4[tid >> 6] = w;
  __syncthreads();
  return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// out_Rt [12]: R, t (NaN when n < 6 or the result is not finite); out_n: n when found, else -1
__global__ void __launch_bounds__(kPnpThreads) k_pnp_dlt_all(const double* __restrict__ X,
                                                             const double* __restrict__ x,
                                                             const double* __restrict__ K, int n,
                                                             double* __restrict__ out_Rt) {
  __shared__ double s_red[kPnpThreads / 64][kPnpDltSums];
  __shared__ double s4[kPnpThreads / 64];
  __shared__ double s_M[144], s_V[144];
  const int tid = threadIdx.x;
  if (n < 6) {
    if (tid < 12) out_Rt[tid] = __builtin_nan("");
    return;
  }
  double c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double a = 0.0;
    for (int i = tid; i < n; i += kPnpThreads) a += X[3 * (int64_t)i + k];
    c[k] = block_sum256_waves(a, s4) / (double)n;
  }
  double sd = 0.0;
  for (int i = tid; i < n; i += kPnpThreads) {
    const double dx = X[3 * (int64_t)i] - c[0], dy = X[3 * (int64_t)i + 1] - c[1], dz = X[3 * (int64_t)i + 2] - c[2];
    sd += sqrt((dx * dx + dy * dy) + dz * dz);
  }
  const double s = sqrt(3.0) / (block_sum256_waves(sd, s4) / (double)n);
  double acc[kPnpDltSums];
#pragma unroll
  for (int k = 0; k < kPnpDltSums; ++k) acc[k] = 0.0;
  for (int i = tid; i < n; i += kPnpThreads) {
    double un, vn;
    normalised_pixel(K, x[2 * (int64_t)i], x[2 * (int64_t)i + 1], un, vn);
    const double Yh[4] = {s * (X[3 * (int64_t)i] - c[0]), s * (X[3 * (int64_t)i + 1] - c[1]),
                          s * (X[3 * (int64_t)i + 2] - c[2]), 1.0};
    const double uv = un * un + vn * vn;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = a; b < 4; ++b, ++k) {
        const double w = Yh[a] * Yh[b];
        acc[k] += w;
        acc[10 + k] = fma(un, w, acc[10 + k]);
        acc[20 + k] = fma(vn, w, acc[20 + k]);
        acc[30 + k] = fma(uv, w, acc[30 + k]);
      }
  }
#pragma unroll
  for (int k = 0; k < kPnpDltSums; ++k) {
    const double w = wave_sum_f64(acc[k]);
    if ((tid & 63) == 0) s_red[tid >> 6][k] = w;
  }
  __syncthreads();
  if (tid != 0) return;  // (no barrier below)
  // A^T A = [[W, 0, -uW], [0, W, -vW], [-uW, -vW, (u^2 + v^2) W]] in 4 x 4 blocks
  {
    int k = 0;
    for (int a = 0; a < 4; ++a)
      for (int b = a; b < 4; ++b, ++k) {
        double w[4];
        for (int g = 0; g < 4; ++g) w[g] = ((s_red[0][10 * g + k] + s_red[1][10 * g + k]) + s_red[2][10 * g + k]) + s_red[3][10 * g + k];
        for (int f = 0; f < 2; ++f) {  // (a, b) and (b, a)
          const int r = f ? b : a, q = f ? a : b;
          s_M[r * 12 + q] = w[0];
          s_M[(4 + r) * 12 + 4 + q] = w[0];
          s_M[r * 12 + 4 + q] = 0.0;
          s_M[(4 + r) * 12 + q] = 0.0;
          s_M[r * 12 + 8 + q] = -w[1];
          s_M[(8 + q) * 12 + r] = -w[1];
          s_M[(4 + r) * 12 + 8 + q] = -w[2];
          s_M[(8 + q) * 12 + 4 + r] = -w[2];
          s_M[(8 + r) * 12 + 8 + q] = w[3];
        }
      }
  }
  for (int r = 0; r < 12; ++r)
    for (int q = 0; q < 12; ++q) s_V[r * 12 + q] = r == q ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {  // cyclic Jacobi, the rotations of jacobi_eig3
    double off = 0.0, dia = 0.0;
    for (int p = 0; p < 12; ++p) {
      dia += fabs(s_M[p * 12 + p]);
      for (int q = p + 1; q < 12; ++q) off += fabs(s_M[p * 12 + q]);
    }
    if (!(off > 1e-18 * dia)) break;  // (or NaN)
    for (int p = 0; p < 11; ++p)
      for (int q = p + 1; q < 12; ++q) {
        const double apq = s_M[p * 12 + q];
        if (fabs(apq) < 1e-300) continue;
        const double theta = (s_M[q * 12 + q] - s_M[p * 12 + p]) / (2.0 * apq);
        const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(tt * tt + 1.0), sn = tt * cs;
        for (int k = 0; k < 12; ++k) {
          const double skp = s_M[k * 12 + p], skq = s_M[k * 12 + q];
          s_M[k * 12 + p] = cs * skp - sn * skq;
          s_M[k * 12 + q] = sn * skp + cs * skq;
        }
        for (int k = 0; k < 12; ++k) {
          const double spk = s_M[p * 12 + k], sqk = s_M[q * 12 + k];
          s_M[p * 12 + k] = cs * spk - sn * sqk;
          s_M[q * 12 + k] = sn * spk + cs * sqk;
        }
        for (int k = 0; k < 12; ++k) {
          const double vkp = s_V[k * 12 + p], vkq = s_V[k * 12 + q];
          s_V[k * 12 + p] = cs * vkp - sn * vkq;
          s_V[k * 12 + q] = sn * vkp + cs * vkq;
        }
      }
  }
  int mi = 0;
  double mv = s_M[0];
  for (int p = 1; p < 12; ++p)
    if (s_M[p * 12 + p] < mv) {
      mv = s_M[p * 12 + p];
      mi = p;
    }
  double p[12], Rt[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) p[k] = s_V[k * 12 + mi];
  pose_from_p(p, s, c, Rt);
#pragma unroll
  for (int k = 0; k < 12; ++k) out_Rt[k] = Rt[k];
}

// ---------------- launchers ----------------

size_t pnp_hyp_lds_bytes() { return (size_t)11 * 12 * 64 * 8; }

void launch_pnp_ransac(const double* X, const double* x, const double* K, int n, const int32_t* idx, int stride,
                       int iters, double thr, int max_refine_iter, double* hyp, int32_t* counts, double* Rt,
                       int32_t* out_inliers, int32_t* out_n, int32_t* out_iter, double* out_R, double* out_t,
                       int32_t* out_status, double* out_cost, hipStream_t st) {
  if (n >= 6 && iters > 0) {
    static const bool lds_attr = [] {  // 66 KB for k_pnp_hyp, up to kRansacChunk x 40 B of staged points
      return hipFuncSetAttribute((const void*)k_pnp_hyp, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)pnp_hyp_lds_bytes()) == hipSuccess &&
             hipFuncSetAttribute((const void*)k_pnp_count, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 kRansacChunk * 40) == hipSuccess;
    }();
    (void)lds_attr;
    hipLaunchKernelGGL(k_pnp_hyp, dim3((iters + 63) / 64), dim3(64), pnp_hyp_lds_bytes(), st, X, x, K, n, idx, stride,
                       iters, hyp);
    hipLaunchKernelGGL(k_pnp_count, dim3((iters + kPnpWaves - 1) / kPnpWaves), dim3(64 * kPnpWaves),
                       (size_t)std::min(n, kRansacChunk) * 40, st, X, x, K, n, (const double*)hyp, iters, thr, counts);
  }
  // always: without samples (or points) the selection writes "no pose" and the refinement its status
  hipLaunchKernelGGL(k_pnp_select, dim3(1), dim3(kPnpThreads), 0, st, X, x, K, n, (const double*)hyp,
                     (const int32_t*)counts, n >= 6 ? iters : 0, thr, out_inliers, out_n, out_iter, Rt);
  hipLaunchKernelGGL(k_pnp_refine, dim3(1), dim3(kPnpThreads), 0, st, X, x, K, n, (const int32_t*)out_inliers,
                     (const int32_t*)out_n, (const double*)Rt, max_refine_iter, out_R, out_t, out_status, out_cost);
}

void launch_pnp(const double* X, const double* x, const double* K, int n, int max_refine_iter, double* Rt,
                double* out_R, double* out_t, int32_t* out_status, double* out_cost, hipStream_t st) {
  hipLaunchKernelGGL(k_pnp_dlt_all, dim3(1), dim3(kPnpThreads), 0, st, X, x, K, n, Rt);
  hipLaunchKernelGGL(k_pnp_refine, dim3(1), dim3(kPnpThreads), 0, st, X, x, K, n, (const int32_t*)nullptr,
                     (const int32_t*)nullptr, (const double*)Rt, max_refine_iter, out_R, out_t, out_status, out_cost);
}

}  // namespace sfm
