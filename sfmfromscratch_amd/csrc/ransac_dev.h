// ransac_dev.h — the device functions of the 8-point fit and the epipolar inlier test, one copy
// for every kernel that fits or tests a fundamental matrix: k_ransac_F / k_ransac_count /
// k_ransac_select (ransac.hip) and the fused verification kernel (verify.hip).  float64, no
// contraction (the Makefile's -ffp-contract=off); the route is described at the top of ransac.hip.
#pragma once
#include <math.h>
#include <stdint.h>

#include "common.h"

namespace sfm {

// CameraPose.normalize_points (SFM.py:164-178) over the N points of a sample, sums in index order
template <int N>
SFM_DEV void normalise_sample(const double (&x)[N], const double (&y)[N], double (&nx)[N], double (&ny)[N], double& s,
                              double& cx, double& cy) {
  double mx = 0.0, my = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    mx += x[i];
    my += y[i];
  }
  mx /= (double)N;
  my /= (double)N;
  double md = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) md += sqrt((x[i] - mx) * (x[i] - mx) + (y[i] - my) * (y[i] - my));
  md /= (double)N;
  s = sqrt(2.0) / md;
  cx = mx;
  cy = my;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    nx[i] = s * x[i] + (-s * mx);
    ny[i] = s * y[i] + (-s * my);
  }
}

SFM_DEV void normalise8(const double (&x)[8], const double (&y)[8], double (&nx)[8], double (&ny)[8], double& s,
                        double& cx, double& cy) {
  normalise_sample<8>(x, y, nx, ny, s, cx, cy);
}

// A null vector of the 8 x 9 system (rows [x1x2, y1x2, x2, x1y2, y1y2, y2, x1, y1, 1]): the last
// column without a pivot is set to 1, every other free column to 0, and the pivots found are
// back-substituted.  Rank 8 has one free column and this is the null vector; below rank 8
// (columns that are exactly dependent: identical frames, one repeated correspondence, a
// constant coordinate) it is one finite member of the null space, where the reference's SVD
// returns another (LAPACK's choice inside a null space of more than one dimension is not
// reproduced).  An 8 x 9 system always has a null vector, so there is no failure to report.
SFM_DEV void null_vector_8x9(double (&A)[8][9], double (&f)[9]) {
  int piv_col[8];
  int r = 0;
  for (int c = 0; c < 9 && r < 8; ++c) {
    int best = r;
    double bv = fabs(A[r][c]);
    for (int i = r + 1; i < 8; ++i)
      if (fabs(A[i][c]) > bv) { bv = fabs(A[i][c]); best = i; }
    if (bv < 1e-300) continue;  // free column
    if (best != r)
      for (int k = 0; k < 9; ++k) { const double t = A[r][k]; A[r][k] = A[best][k]; A[best][k] = t; }
    for (int i = r + 1; i < 8; ++i) {
      const double fct = A[i][c] / A[r][c];
      for (int k = c; k < 9; ++k) A[i][k] -= fct * A[r][k];
    }
    piv_col[r++] = c;
  }
  int free_col = 8;  // the last column without a pivot (r < 8: rows r.. are zero and drop out)
  {
    bool used[9] = {false, false, false, false, false, false, false, false, false};
    for (int i = 0; i < r; ++i) used[piv_col[i]] = true;
    for (int c = 0; c < 9; ++c)
      if (!used[c]) free_col = c;
  }
  for (int k = 0; k < 9; ++k) f[k] = 0.0;
  f[free_col] = 1.0;
  for (int i = r - 1; i >= 0; --i) {
    const int c = piv_col[i];
    double acc = 0.0;
    for (int k = c + 1; k < 9; ++k) acc += A[i][k] * f[k];
    f[c] = -acc / A[i][c];
  }
}

// The same elimination when every column 0..7 has a pivot (the usual case), with every
// index compile-time: row exchanges are selects, so A stays in registers (the general
// routine's runtime row indices put it in scratch).  Returns false on a zero pivot; the
// caller then rebuilds A and takes the general routine, which handles free columns.
SFM_DEV bool null_vector_8x9_regs(double (&A)[8][9], double (&f)[9]) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
#pragma unroll
    for (int i = c + 1; i < 8; ++i) {  // the first row of largest |A[.][c]| ends in row c
      const bool sw = fabs(A[i][c]) > fabs(A[c][c]);
#pragma unroll
      for (int k = c; k < 9; ++k) {
        const double u = A[c][k], v = A[i][k];
        A[c][k] = sw ? v : u;
        A[i][k] = sw ? u : v;
      }
    }
    if (!(fabs(A[c][c]) >= 1e-300)) return false;
#pragma unroll
    for (int i = c + 1; i < 8; ++i) {
      const double fct = A[i][c] / A[c][c];
#pragma unroll
      for (int k = c; k < 9; ++k) A[i][k] -= fct * A[c][k];
    }
  }
  f[8] = 1.0;
#pragma unroll
  for (int i = 7; i >= 0; --i) {
    double acc = 0.0;
#pragma unroll
    for (int k = i + 1; k < 9; ++k) acc += A[i][k] * f[k];
    f[i] = -acc / A[i][i];
  }
  return true;
}

// smallest-eigenvalue eigenvector of a symmetric 3 x 3 (cyclic Jacobi)
SFM_DEV void smallest_eigvec3(double (&S)[3][3], double (&v)[3]) {
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = fabs(S[0][1]) + fabs(S[0][2]) + fabs(S[1][2]);
    const double dia = fabs(S[0][0]) + fabs(S[1][1]) + fabs(S[2][2]);
    if (off <= 1e-18 * dia) break;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        if (fabs(S[p][q]) < 1e-300) continue;
        const double theta = (S[q][q] - S[p][p]) / (2.0 * S[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {  // S = J^T S J
          const double skp = S[k][p], skq = S[k][q];
          S[k][p] = c * skp - s * skq;
          S[k][q] = s * skp + c * skq;
        }
        for (int k = 0; k < 3; ++k) {
          const double spk = S[p][k], sqk = S[q][k];
          S[p][k] = c * spk - s * sqk;
          S[q][k] = s * spk + c * sqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  const int mi = (S[1][1] < S[0][0]) ? ((S[2][2] < S[1][1]) ? 2 : 1) : ((S[2][2] < S[0][0]) ? 2 : 0);
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = mi == 0 ? V[k][0] : (mi == 1 ? V[k][1] : V[k][2]);  // no runtime index
}

// F (9 doubles, row-major) of eight correspondences (CameraPose._compute_fundamental_matrix,
// SFM.py:190-236).  No branch writes NaN: a rank-deficient system still has a null vector
// (null_vector_8x9).  NaN comes only out of the arithmetic, when the eight points of one image
// coincide (Hartley scale sqrt(2) / 0) — the reference's SVD raises there.
SFM_DEV void ransac_fit_F(const double (&x1)[8], const double (&y1)[8], const double (&x2)[8],
                          const double (&y2)[8], double (&F)[9]) {
  double a1[8], b1[8], a2[8], b2[8], s1, c1x, c1y, s2, c2x, c2y;
  normalise8(x1, y1, a1, b1, s1, c1x, c1y);
  normalise8(x2, y2, a2, b2, s2, c2x, c2y);
  double A[8][9];
  auto build = [&]() {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double u1 = a1[i], v1 = b1[i], u2 = a2[i], v2 = b2[i];
      A[i][0] = u1 * u2; A[i][1] = v1 * u2; A[i][2] = u2;
      A[i][3] = u1 * v2; A[i][4] = v1 * v2; A[i][5] = v2;
      A[i][6] = u1;      A[i][7] = v1;      A[i][8] = 1.0;
    }
  };
  build();
  double f[9];
  if (!null_vector_8x9_regs(A, f)) {  // a zero pivot: the general elimination (free columns) on a fresh system
    build();
    null_vector_8x9(A, f);
  }
  // scale to unit norm (the SVD's vector), then rank 2: F - (F v3) v3^T
  double nn = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) nn += f[k] * f[k];
  nn = 1.0 / sqrt(nn);
#pragma unroll
  for (int k = 0; k < 9; ++k) f[k] *= nn;
  double S[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) S[r][c] = f[0 + r] * f[0 + c] + f[3 + r] * f[3 + c] + f[6 + r] * f[6 + c];
  double v[3];
  smallest_eigvec3(S, v);
  double Fv[3];
  for (int r = 0; r < 3; ++r) Fv[r] = f[3 * r] * v[0] + f[3 * r + 1] * v[1] + f[3 * r + 2] * v[2];
  double F2[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) F2[r][c] = f[3 * r + c] - Fv[r] * v[c];
  // un-normalise: T2^T F2 T1 (SFM.py:181-182), T = [[s,0,-s cx],[0,s,-s cy],[0,0,1]]
  const double T1[3][3] = {{s1, 0, -s1 * c1x}, {0, s1, -s1 * c1y}, {0, 0, 1}};
  const double T2[3][3] = {{s2, 0, -s2 * c2x}, {0, s2, -s2 * c2y}, {0, 0, 1}};
  double M[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) M[r][c] = F2[r][0] * T1[0][c] + F2[r][1] * T1[1][c] + F2[r][2] * T1[2][c];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) F[3 * r + c] = T2[0][r] * M[0][c] + T2[1][r] * M[1][c] + T2[2][r] * M[2][c];
}

// d = |l . p2| / sqrt(l0^2 + l1^2) < thr (SFM.py:148-153).  Decided as num^2 vs thr^2 den2
// unless the two are within a relative 2^-40 of each other, where the reference's own
// expression decides: the squared comparison cannot flip a point farther than that from
// the threshold, and spares the float64 division and square root almost everywhere.
// lb = F p1 as fmas (numpy's F @ a_h goes through BLAS, whose order and fusing are its
// own; the bar is set by F's float64 rounding anyway).  thr2lo / thr2hi = thr^2 (1 -+ 2^-40).
// The test comes in two halves, so that a kernel whose occupancy hides no latency (verify.hip)
// can put the terms of several points ahead of their decisions; epi_inlier is the two in a row.
struct EpiTerms {
  double num, den2;  // |l . p2| and l0^2 + l1^2
};
SFM_DEV EpiTerms epi_terms(const double* F, double x1, double y1, double x2, double y2) {
  const double l0 = __builtin_fma(F[0], x1, __builtin_fma(F[1], y1, F[2]));
  const double l1 = __builtin_fma(F[3], x1, __builtin_fma(F[4], y1, F[5]));
  const double l2 = __builtin_fma(F[6], x1, __builtin_fma(F[7], y1, F[8]));
  const double num = fabs(__builtin_fma(l0, x2, __builtin_fma(l1, y2, l2)));
  const double den2 = __builtin_fma(l0, l0, l1 * l1);
  return {num, den2};
}
SFM_DEV bool epi_decide(const EpiTerms& e, double thr, double thr2lo, double thr2hi) {
  const double a = e.num * e.num;
  if (a < thr2lo * e.den2) return true;
  if (a > thr2hi * e.den2) return false;
  return e.num / sqrt(e.den2) < thr;  // near the threshold, or NaN (degenerate F) -> false
}
SFM_DEV bool epi_inlier(const double* F, double x1, double y1, double x2, double y2, double thr, double thr2lo,
                        double thr2hi) {
  return epi_decide(epi_terms(F, x1, y1, x2, y2), thr, thr2lo, thr2hi);
}

struct EpiThr {
  double thr, lo, hi;
};
SFM_DEV EpiThr epi_thr(double thr) {  // thr <= 0 (or NaN): nothing is an inlier (d >= 0)
  const double t2 = thr * thr;
  const bool on = thr > 0.0;
  return {thr, on ? t2 * (1.0 - 0x1p-40) : -1.0, on ? t2 * (1.0 + 0x1p-40) : -1.0};
}

}  // namespace sfm
