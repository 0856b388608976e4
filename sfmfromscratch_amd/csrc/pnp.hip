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
// The hypothesis, the inlier count and the Levenberg-Marquardt are bodies of pnp_dev.h, which the
// slot-batched kernels of resect.hip call too.
// Float64 throughout; -ffp-contract=off, fmas written where wanted.
#include <algorithm>

#include "pnp_dev.h"

namespace sfm {

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
  double Rt[12];
  pnp_hypothesis(X, x, K, [&](int i) { return clamp_index(idx[(int64_t)it * stride + i], n); }, s_A, lane, Rt);
  double* o = hyp + (int64_t)it * 12;
#pragma unroll
  for (int k = 0; k < 12; ++k) o[k] = Rt[k];
}

__global__ void __launch_bounds__(64 * kPnpWaves) k_pnp_count(const double* __restrict__ X,
                                                              const double* __restrict__ x,
                                                              const double* __restrict__ K, int n,
                                                              const double* __restrict__ hyp, int iters, double thr,
                                                              int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) double s_p[];  // [5][cn]: X0, X1, X2, u, v
  pnp_count_block(X, x, K, n, hyp, iters, thr, counts, blockIdx.x, s_p);
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
  pnp_lm_block(X, x, K, n, inl, m, R, t, max_iter, out_R, out_t, out_status, out_cost, s_red);
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
