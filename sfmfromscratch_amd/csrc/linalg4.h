// linalg4.h — the 4 x 4 float64 null vector shared by pose.hip (two-view triangulation) and
// tracks.hip (N-view triangulation).  Every index is a compile-time constant, so the matrices
// stay in registers.  -ffp-contract=off; fmas only where written.
#pragma once

#include <math.h>

#include "common.h"

namespace sfm {

// the right singular vector of A's smallest singular value: one-sided Jacobi, columns p < q
// rotated until every pair is orthogonal to 2^-52 of their norms
SFM_DEV void null_vector_4x4(double (&A)[4][4], double (&v)[4]) {
  double V[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          al = __builtin_fma(A[k][p], A[k][p], al);
          be = __builtin_fma(A[k][q], A[k][q], be);
          ga = __builtin_fma(A[k][p], A[k][q], ga);
        }
        if (!(ga * ga > 0x1p-104 * (al * be))) continue;  // orthogonal already (or NaN)
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = c * t;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double ap = A[k][p], aq = A[k][q];
          A[k][p] = c * ap - s * aq;
          A[k][q] = s * ap + c * aq;
          const double vp = V[k][p], vq = V[k][q];
          V[k][p] = c * vp - s * vq;
          V[k][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  double nn[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
    nn[c] = A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c] + A[3][c] * A[3][c];
  int mi = 0;
  double mv = nn[0];
#pragma unroll
  for (int c = 1; c < 4; ++c)
    if (nn[c] < mv) { mv = nn[c]; mi = c; }
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = mi == 0 ? V[k][0] : (mi == 1 ? V[k][1] : (mi == 2 ? V[k][2] : V[k][3]));
}

}  // namespace sfm
