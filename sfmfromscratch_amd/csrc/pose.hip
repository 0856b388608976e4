// pose.hip — the initial pair's consumer CameraPose.ransac_camera_motion (SFM.py:38-124)
// and the linear triangulation it is built from (triangulate_point, SFM.py:239-253;
// triangulate_points, :292-305).  The samples, fundamental matrices and inlier counts are
// ransac.hip's (the same np.random.seed(5) stream and the same distances); this file adds
//
// * k_pose_candidates, one thread per (pair, sample): E = K2^T F K1 (SFM.py:58), its SVD,
//   R1 = U W V^T, R2 = U W^T V^T (negated when det < 0, :68-75), T = U[:, 2] (:78).
//   V comes from a cyclic Jacobi eigen-decomposition of E^T E, u_i = E v_i / |E v_i|
//   (i = 1, 2), u3 = u1 x u2.  The signs of u3 and v3 are LAPACK's choice in the reference
//   and this construction's here; flipping either permutes the candidate list
//   {(R1, T), (R1, -T), (R2, T), (R2, -T)} and leaves it the same as a set.
// * k_pose_cheirality, one wave per (pair, sample): _check_valid_pose (SFM.py:105-124) for
//   the four candidates in turn.  Every lane triangulates the points lane, lane + 64, ..;
//   a point fails iff `depth < 1e-6` is true for either camera (a NaN depth does not fail,
//   as in numpy); a wave-wide vote ends a candidate at its first failing round, the first
//   candidate that survives every point ends the sample.  Samples without a valid
//   candidate get inlier count 0, so the unchanged k_ransac_select picks the reference's
//   winner: the first sample with the strictly largest count among those with a valid pose
//   (SFM.py:98).  Samples whose count is 0 already are skipped.
// * triangulation: the 4 x 4 system of SFM.py:241-246 on raw pixel coordinates, its
//   smallest right singular vector by a one-sided (Hestenes) Jacobi on the four columns
//   with V accumulated — accurate to eps cond(A) like LAPACK's SVD, where an
//   eigen-decomposition of A^T A would square the condition number of a matrix whose
//   entries span pixel x focal-length scales.  Every index is compile-time (selects), so A
//   and V stay in registers.
// Float64 throughout; -ffp-contract=off, fmas written where wanted.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "f64_dev.h"  // block_sum256_tree
#include "kernels.h"
#include "pose_dev.h"  // pose_candidates_dev, triangulate_dlt

namespace sfm {

// one thread per (pair, sample): R1, R2 (row-major) and T, 21 doubles (NaN for a NaN F)
__global__ void __launch_bounds__(128) k_pose_candidates(const double* __restrict__ Fs,
                                                         const int32_t* __restrict__ npts,
                                                         const double* __restrict__ Kc, int iters,
                                                         double* __restrict__ cand) {
  const int it = blockIdx.x * 128 + threadIdx.x;
  const int p = blockIdx.y;
  if (it >= iters || npts[p] < 8) return;  // (n < 8: no F was written, nothing reads cand)
  const double* F = Fs + ((int64_t)p * iters + it) * 9;
  const double* K1 = Kc + (int64_t)p * 18;
  const double* K2 = K1 + 9;
  pose_candidates_dev(F, K1, K2, cand + ((int64_t)p * iters + it) * 21);
}

constexpr int kPoseWaves = 8;  // samples (waves) per workgroup: they share the staged points

__global__ void __launch_bounds__(64 * kPoseWaves) k_pose_cheirality(
    const int32_t* __restrict__ pts, const int32_t* __restrict__ npts, int nmax, const double* __restrict__ Kc,
    const double* __restrict__ base, const double* __restrict__ cand, int iters, int32_t* __restrict__ counts,
    int32_t* __restrict__ cand_idx) {
  extern __shared__ __attribute__((aligned(16))) double s_pp[];  // [chunk][4]
  const int p = blockIdx.y;
  const int n = npts[p];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int it = blockIdx.x * kPoseWaves + wave;
  const bool have = it < iters;
  const int64_t slot = (int64_t)p * iters + (have ? it : 0);
  const bool live = have && n >= 8 && counts[slot] > 0;  // count 0 can never win (strict >, SFM.py:98)
  if (!__syncthreads_or(live ? 1 : 0)) {                 // (uniform over the workgroup)
    if (have && lane == 0) cand_idx[slot] = -1;
    return;
  }
  const int4* P = reinterpret_cast<const int4*>(pts + (int64_t)p * nmax * 4);
  const double* K1 = Kc + (int64_t)p * 18;
  const double* K2 = K1 + 9;
  const double* Rb = base + (int64_t)p * 12;
  const double* Tb = Rb + 9;
  const double* C = cand + slot * 21;
  double P1[12], K2R[2][9], K2T[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      P1[4 * r + c] = K1[3 * r] * Rb[c] + K1[3 * r + 1] * Rb[3 + c] + K1[3 * r + 2] * Rb[6 + c];
      K2R[0][3 * r + c] = K2[3 * r] * C[c] + K2[3 * r + 1] * C[3 + c] + K2[3 * r + 2] * C[6 + c];
      K2R[1][3 * r + c] = K2[3 * r] * C[9 + c] + K2[3 * r + 1] * C[12 + c] + K2[3 * r + 2] * C[15 + c];
    }
    P1[4 * r + 3] = K1[3 * r] * Tb[0] + K1[3 * r + 1] * Tb[1] + K1[3 * r + 2] * Tb[2];
    K2T[r] = K2[3 * r] * C[18] + K2[3 * r + 1] * C[19] + K2[3 * r + 2] * C[20];
  }
  const double rb0 = Rb[6], rb1 = Rb[7], rb2 = Rb[8], tb = Tb[2];
  uint32_t alive = live ? 0xfu : 0u;  // candidates that no point has failed yet (wave-uniform)
  int winner = -1;
  for (int i0 = 0; i0 < n; i0 += kRansacChunk) {
    const int m = min(kRansacChunk, n - i0);
    const bool last = i0 + m >= n;
    if (i0 && !__syncthreads_or(alive ? 1 : 0)) break;  // every lane is done with the previous chunk
    for (int i = threadIdx.x; i < m; i += 64 * kPoseWaves) {
      const int4 q = P[i0 + i];
      s_pp[4 * i + 0] = (double)q.x;
      s_pp[4 * i + 1] = (double)q.y;
      s_pp[4 * i + 2] = (double)q.z;
      s_pp[4 * i + 3] = (double)q.w;
    }
    __syncthreads();
    if (!alive) continue;
    for (int c = 0; c < 4; ++c) {
      if (!((alive >> c) & 1u)) continue;
      const bool second = c >= 2;
      const double sg = (c & 1) ? -1.0 : 1.0;
      double P2[12];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) P2[4 * r + k] = second ? K2R[1][3 * r + k] : K2R[0][3 * r + k];
        P2[4 * r + 3] = sg * K2T[r];
      }
      const double rc0 = second ? C[15] : C[6], rc1 = second ? C[16] : C[7], rc2 = second ? C[17] : C[8];
      const double tc = sg * C[20];
      bool ok = true;
      for (int r0 = 0; r0 < m; r0 += 64) {
        const int i = r0 + lane;
        bool fail = false;
        if (i < m) {
          const double4 q = reinterpret_cast<const double4*>(s_pp)[i];
          double X[3];
          triangulate_dlt(q.x, q.y, q.z, q.w, P1, P2, X);
          const double zb = (rb0 * X[0] + rb1 * X[1] + rb2 * X[2]) + tb;
          const double zc = (rc0 * X[0] + rc1 * X[1] + rc2 * X[2]) + tc;
          fail = (zb < 1e-6) || (zc < 1e-6);  // NaN: false, as numpy (SFM.py:121)
        }
        if (__ballot(fail) != 0ull) {
          ok = false;
          break;
        }
      }
      if (!ok) {
        alive &= ~(1u << c);
      } else if (last) {  // every earlier candidate has failed a point
        winner = c;
        break;
      }
    }
  }
  if (have && lane == 0) {
    cand_idx[slot] = winner;
    if (winner < 0) counts[slot] = 0;
  }
}

// per pair: the winner's (R, t) -> out [P][12]; untouched when no sample won
__global__ void k_pose_gather(const int32_t* __restrict__ out_iter, const double* __restrict__ cand,
                              const int32_t* __restrict__ cand_idx, int P, int iters, double* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int it = out_iter[p];
  if (it < 0 || it >= iters) return;
  const int c = cand_idx[(int64_t)p * iters + it];
  if (c < 0) return;
  const double* C = cand + ((int64_t)p * iters + it) * 21;
  const double* R = C + (c >= 2 ? 9 : 0);
  const double sg = (c & 1) ? -1.0 : 1.0;
  double* o = out + (int64_t)p * 12;
  for (int k = 0; k < 9; ++k) o[k] = R[k];
  for (int k = 0; k < 3; ++k) o[9 + k] = sg * C[18 + k];
}

void launch_pose_candidates(const double* Fs, const int32_t* npts, const double* Kc, int P, int iters,
                            double* cand, hipStream_t st) {
  hipLaunchKernelGGL(k_pose_candidates, dim3((iters + 127) / 128, P), dim3(128), 0, st, Fs, npts, Kc, iters, cand);
}

void launch_pose_cheirality(const int32_t* pts, const int32_t* npts, int nmax, int P, const double* Kc,
                            const double* base, const double* cand, int iters, int32_t* counts,
                            int32_t* cand_idx, hipStream_t st) {
  static const bool lds_attr = [] {  // up to kRansacChunk x 32 B of staged points
    return hipFuncSetAttribute((const void*)k_pose_cheirality, hipFuncAttributeMaxDynamicSharedMemorySize,
                               kRansacChunk * 32) == hipSuccess;
  }();
  (void)lds_attr;
  hipLaunchKernelGGL(k_pose_cheirality, dim3((iters + kPoseWaves - 1) / kPoseWaves, P), dim3(64 * kPoseWaves),
                     (size_t)std::min(nmax, kRansacChunk) * 32, st, pts, npts, nmax, Kc, base, cand, iters, counts,
                     cand_idx);
}

void launch_pose_gather(const int32_t* out_iter, const double* cand, const int32_t* cand_idx, int P, int iters,
                        double* out_Rt, hipStream_t st) {
  hipLaunchKernelGGL(k_pose_gather, dim3((P + 63) / 64), dim3(64), 0, st, out_iter, cand, cand_idx, P, iters,
                     out_Rt);
}

// ---------------- triangulation over N points ----------------

// CameraPose.normalize_points (SFM.py:163-178) of both point sets and T1 P1, T2 P2
// (:297-298): one workgroup; out = the two normalised matrices (24) then s, cu, cv of each set
__global__ void __launch_bounds__(256) k_hartley(const double* __restrict__ x1, const double* __restrict__ x2,
                                                 int64_t N, const double* __restrict__ P1,
                                                 const double* __restrict__ P2, double* __restrict__ out) {
  __shared__ double s_red[256];
  const int tid = threadIdx.x;
  for (int set = 0; set < 2; ++set) {
    const double* x = set ? x2 : x1;
    const double* Pm = set ? P2 : P1;
    double sx = 0.0, sy = 0.0;
    for (int64_t i = tid; i < N; i += 256) {
      sx += x[2 * i];
      sy += x[2 * i + 1];
    }
    const double cu = block_sum256_tree(sx, s_red) / (double)N;
    const double cv = block_sum256_tree(sy, s_red) / (double)N;
    double sd = 0.0;
    for (int64_t i = tid; i < N; i += 256) {
      const double dx = x[2 * i] - cu, dy = x[2 * i + 1] - cv;
      sd += sqrt(dx * dx + dy * dy);
    }
    const double sc = sqrt(2.0) / (block_sum256_tree(sd, s_red) / (double)N);
    if (tid < 4) {
      out[12 * set + tid] = sc * Pm[tid] + (-sc * cu) * Pm[8 + tid];
      out[12 * set + 4 + tid] = sc * Pm[4 + tid] + (-sc * cv) * Pm[8 + tid];
      out[12 * set + 8 + tid] = Pm[8 + tid];
    }
    if (tid == 0) {
      out[24 + 3 * set] = sc;
      out[24 + 3 * set + 1] = cu;
      out[24 + 3 * set + 2] = cv;
    }
  }
}

// one thread per point; tp (optional): s, cu, cv of both sets, applied as points @ T^T
__global__ void __launch_bounds__(128) k_triangulate(const double* __restrict__ x1, const double* __restrict__ x2,
                                                     int64_t N, const double* __restrict__ P1,
                                                     const double* __restrict__ P2, const double* __restrict__ tp,
                                                     double* __restrict__ X) {
  const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= N) return;
  double A1[12], A2[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    A1[k] = P1[k];
    A2[k] = P2[k];
  }
  double a = x1[2 * i], b = x1[2 * i + 1], c = x2[2 * i], d = x2[2 * i + 1];
  if (tp) {
    a = tp[0] * a + (-tp[0] * tp[1]);
    b = tp[0] * b + (-tp[0] * tp[2]);
    c = tp[3] * c + (-tp[3] * tp[4]);
    d = tp[3] * d + (-tp[3] * tp[5]);
  }
  double o[3];
  triangulate_dlt(a, b, c, d, A1, A2, o);
  X[3 * i] = o[0];
  X[3 * i + 1] = o[1];
  X[3 * i + 2] = o[2];
}

void launch_triangulate(const double* x1, const double* x2, int64_t N, const double* P1, const double* P2,
                        bool normalize, double* scratch30, double* X, hipStream_t st) {
  if (N < 1) return;
  const unsigned blocks = (unsigned)((N + 127) / 128);
  if (normalize) {
    hipLaunchKernelGGL(k_hartley, dim3(1), dim3(256), 0, st, x1, x2, N, P1, P2, scratch30);
    hipLaunchKernelGGL(k_triangulate, dim3(blocks), dim3(128), 0, st, x1, x2, N, (const double*)scratch30,
                       (const double*)(scratch30 + 12), (const double*)(scratch30 + 24), X);
  } else {
    hipLaunchKernelGGL(k_triangulate, dim3(blocks), dim3(128), 0, st, x1, x2, N, P1, P2, (const double*)nullptr, X);
  }
}

}  // namespace sfm
