// linalg3.h — 3 x 3 float64 helpers shared by the geometry kernels (pose, pnp, ba, registry).
// Every index is a compile-time constant, so the matrices stay in registers.  Rotations are
// row-major double[9].  -ffp-contract=off: each helper's expression order is its contract —
// kernels that call the same helper produce the same bits.
#pragma once

#include <math.h>

#include "common.h"

namespace sfm {

// eigen-decomposition of a symmetric 3 x 3 (cyclic Jacobi, the rotations of ransac.hip's
// smallest_eigvec3 with every column kept): S -> diagonal, V's columns the eigenvectors
SFM_DEV void jacobi_eig3(double (&S)[3][3], double (&V)[3][3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 16; ++sweep) {
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
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // S = J^T S J
          const double skp = S[k][p], skq = S[k][q];
          S[k][p] = c * skp - s * skq;
          S[k][q] = s * skp + c * skq;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double spk = S[p][k], sqk = S[q][k];
          S[p][k] = c * spk - s * sqk;
          S[q][k] = s * spk + c * sqk;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

SFM_DEV double det3(const double (&R)[3][3]) {
  return R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
         R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
}

// cv2.Rodrigues, vector -> matrix, in closed form: theta = sqrt((r0^2 + r1^2) + r2^2), the
// identity below DBL_EPSILON, else cs I + c1 k k^T + sn [k]x with each entry summed as written
SFM_DEV void rodrigues(double r0, double r1, double r2, double (&R)[9]) {
  const double th = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
  R[0] = 1.0, R[1] = 0.0, R[2] = 0.0, R[3] = 0.0, R[4] = 1.0, R[5] = 0.0, R[6] = 0.0, R[7] = 0.0, R[8] = 1.0;
  if (!(th < 2.220446049250313e-16)) {
    const double cs = cos(th), sn = sin(th), c1 = 1.0 - cs;
    const double kx = r0 / th, ky = r1 / th, kz = r2 / th;
    R[0] = cs + c1 * kx * kx;
    R[1] = c1 * kx * ky - sn * kz;
    R[2] = c1 * kx * kz + sn * ky;
    R[3] = c1 * kx * ky + sn * kz;
    R[4] = cs + c1 * ky * ky;
    R[5] = c1 * ky * kz - sn * kx;
    R[6] = c1 * kx * kz - sn * ky;
    R[7] = c1 * ky * kz + sn * kx;
    R[8] = cs + c1 * kz * kz;
  }
}

// matrix -> principal vector, as pose.rodrigues: the antisymmetric part up to theta = pi / 2,
// beyond it the axis from the symmetric part
SFM_DEV void rodrigues_inv(const double (&R)[9], double (&r)[3]) {
  const double v[3] = {(R[7] - R[5]) / 2.0, (R[2] - R[6]) / 2.0, (R[3] - R[1]) / 2.0};
  const double s = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const double c = (((R[0] + R[4]) + R[8]) - 1.0) / 2.0;
  const double th = atan2(s, c);
  if (c >= 0) {
    const double f = s == 0 ? 1.0 : th / s;
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = s == 0 ? v[k] : v[k] * f;
    return;
  }
  const double dg[3] = {R[0], R[4], R[8]};
  double k2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) k2[k] = fmax((dg[k] - c) / (1.0 - c), 0.0);
  const int best = k2[0] >= k2[1] ? (k2[0] >= k2[2] ? 0 : 2) : (k2[1] >= k2[2] ? 1 : 2);  // the first maximum
  double kk[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (i != best) continue;
    kk[i] = v[i] < 0 ? -sqrt(k2[i]) : sqrt(k2[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (j != i) kk[j] = (R[3 * i + j] + R[3 * j + i]) / 2.0 / ((1.0 - c) * kk[i]);
  }
  const double nk = sqrt((kk[0] * kk[0] + kk[1] * kk[1]) + kk[2] * kk[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = kk[k] / nk * th;
}

// Rn = E R, each entry (E[3r] R[k] + E[3r + 1] R[3 + k]) + E[3r + 2] R[6 + k].  Pointers: R and
// Rn may be rows of a global table (Rn must not overlap E or R).
SFM_DEV void compose3(const double* E, const double* R, double* Rn) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) Rn[3 * r + k] = (E[3 * r] * R[k] + E[3 * r + 1] * R[3 + k]) + E[3 * r + 2] * R[6 + k];
}

// Y = R (x, y, z), each entry (R[3r] x + R[3r + 1] y) + R[3r + 2] z
SFM_DEV void rotate3(const double (&R)[9], double x, double y, double z, double (&Y)[3]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) Y[r] = (R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z;
}

}  // namespace sfm
