// pnp_dev.h — the device functions the single-frame PnP kernels (pnp.hip) and the slot-batched
// resection kernels (resect.hip) share: the 6-point DLT hypothesis, the inlier test and count,
// and the Levenberg-Marquardt refinement.  One copy, so both calls run the same arithmetic in
// the same order and agree to the last bit on the same links.  The kernels around these bodies
// differ only in where a sample's indices come from and in which frame a workgroup serves.
// Float64 throughout; -ffp-contract=off, fmas written where wanted.
#pragma once
#include <math.h>
#include <stdint.h>

#include "f64_dev.h"
#include "kernels.h"
#include "linalg3.h"

namespace sfm {

constexpr int kPnpWaves = 8;     // samples (waves) per workgroup of the count kernels
constexpr int kPnpThreads = 256; // selection, refinement, k_pnp_dlt_all

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

constexpr size_t kPnpHypLdsBytes = (size_t)11 * 12 * 64 * 8;  // the 11 x 12 system of each lane of one wave

// One lane's hypothesis: Rt = R, t (NaN for a degenerate sample) from the six correspondences
// index_of(0..5) of X [n][3], x [n][2] (indices within [0, n) are the caller's).  s_A: the wave's
// [11 * 12][64] LDS block, this lane's column.  No barrier.
template <class IndexOf>
SFM_DEV void pnp_hypothesis(const double* __restrict__ X, const double* __restrict__ x,
                            const double* __restrict__ K, IndexOf index_of, double* s_A, int lane,
                            double (&Rt)[12]) {
#define PNP_A(r, k) s_A[((r) * 12 + (k)) * 64 + lane]
  double Xs[6][3], un[6], vn[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int j = index_of(i);
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

// A workgroup of kPnpWaves waves, one sample per wave: counts[it] for the samples
// blk * kPnpWaves .. of hyp [iters][12] over X [n][3], x [n][2].  s_p: [5][min(n, kRansacChunk)]
// doubles of LDS (X0, X1, X2, u, v).  Every thread of the workgroup must call it.
SFM_DEV void pnp_count_block(const double* __restrict__ X, const double* __restrict__ x,
                             const double* __restrict__ K, int n, const double* __restrict__ hyp, int iters,
                             double thr, int32_t* __restrict__ counts, int blk, double* s_p) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int it = blk * kPnpWaves + wave;
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

// The Levenberg-Marquardt of one frame in one workgroup of kPnpThreads threads, every one of
// which must call it, from the finite start pose (R, t) over the m >= 1 points (inl: their
// indices, or nullptr for 0..m-1).  out_status: found, LM status, accepted steps, iterations
// run; out_cost: the cost at the start and at the returned pose.  s_red: LDS.
SFM_DEV void pnp_lm_block(const double* __restrict__ X, const double* __restrict__ x, const double* __restrict__ K,
                          int n, const int32_t* __restrict__ inl, int m, double (&R)[9], double (&t)[3], int max_iter,
                          double* __restrict__ out_R, double* __restrict__ out_t, int32_t* __restrict__ out_status,
                          double* __restrict__ out_cost, double (*s_red)[kPnpSums]) {
  const int tid = threadIdx.x;
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

}  // namespace sfm
