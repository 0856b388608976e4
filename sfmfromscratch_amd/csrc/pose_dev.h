// pose_dev.h — the device functions of the relative pose out of a fundamental matrix, one copy for
// the kernels that need them: k_pose_candidates / k_pose_cheirality / k_triangulate (pose.hip) and
// k_two_view_pose (twoview.hip).  The routes are described at the top of pose.hip.  float64, no
// contraction; each function's expression order is its contract.
#pragma once
#include <math.h>

#include "common.h"
#include "linalg3.h"  // jacobi_eig3, det3
#include "linalg4.h"  // null_vector_4x4

namespace sfm {

template <int A, int B>
SFM_DEV void order_desc(double (&l)[3], double (&V)[3][3]) {  // columns A < B: larger eigenvalue first
  const bool sw = l[A] < l[B];
  const double la = l[A], lb = l[B];
  l[A] = sw ? lb : la;
  l[B] = sw ? la : lb;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = V[k][A], b = V[k][B];
    V[k][A] = sw ? b : a;
    V[k][B] = sw ? a : b;
  }
}

// E = K2^T F K1 and its four (R, t): o [21] = R1, R2 (row-major) and T; the candidates are
// (R1, T), (R1, -T), (R2, T), (R2, -T) in this order.  NaN for a NaN F.
SFM_DEV void pose_candidates_dev(const double* F, const double* K1, const double* K2, double* o) {
  double M[3][3], E[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[r][c] = F[3 * r] * K1[c] + F[3 * r + 1] * K1[3 + c] + F[3 * r + 2] * K1[6 + c];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) E[r][c] = K2[r] * M[0][c] + K2[3 + r] * M[1][c] + K2[6 + r] * M[2][c];
  double S[3][3], V[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) S[r][c] = E[0][r] * E[0][c] + E[1][r] * E[1][c] + E[2][r] * E[2][c];
  jacobi_eig3(S, V);
  double l[3] = {S[0][0], S[1][1], S[2][2]};
  order_desc<0, 1>(l, V);
  order_desc<1, 2>(l, V);
  order_desc<0, 1>(l, V);
  double U[3][3];  // columns u1, u2, u3
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    double u[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) u[r] = E[r][0] * V[0][j] + E[r][1] * V[1][j] + E[r][2] * V[2][j];
    const double inv = 1.0 / sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);  // 1 / sigma_j
#pragma unroll
    for (int r = 0; r < 3; ++r) U[r][j] = u[r] * inv;
  }
  U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
  U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
  U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  // U W = [u2, -u1, u3], U W^T = [-u2, u1, u3]
  double R1[3][3], R2[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double a = U[r][1] * V[c][0] - U[r][0] * V[c][1], b = U[r][2] * V[c][2];
      R1[r][c] = a + b;
      R2[r][c] = b - a;
    }
  const double s1 = det3(R1) < 0 ? -1.0 : 1.0, s2 = det3(R2) < 0 ? -1.0 : 1.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      o[3 * r + c] = s1 * R1[r][c];
      o[9 + 3 * r + c] = s2 * R2[r][c];
    }
#pragma unroll
  for (int r = 0; r < 3; ++r) o[18 + r] = U[r][2];
}

// CameraPose.triangulate_point (SFM.py:239-253): P1, P2 row-major 3 x 4
SFM_DEV void triangulate_dlt(double x1, double y1, double x2, double y2, const double (&P1)[12],
                             const double (&P2)[12], double (&X)[3]) {
  double A[4][4], v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    A[0][k] = x1 * P1[8 + k] - P1[k];
    A[1][k] = y1 * P1[8 + k] - P1[4 + k];
    A[2][k] = x2 * P2[8 + k] - P2[k];
    A[3][k] = y2 * P2[8 + k] - P2[4 + k];
  }
  null_vector_4x4(A, v);
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = v[k] / v[3];
}

}  // namespace sfm
