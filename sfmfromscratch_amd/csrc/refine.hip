// refine.hip — the "structure" stage: what SFMRunner.perform does with the triangulated
// points (Runner.py:209-211, :241-250, :279-282).
//
// * k_refine_points: CameraPose.non_linear_triangulation (SFM.py:255-289).  The reference
//   hands all 3n coordinates to one Levenberg-Marquardt solve; its cost is a sum over points
//   of each point's own four squared residuals, so the joint minimiser is the tuple of the
//   per-point minimisers: one thread per point runs a 3-unknown LM with the
//   analytic 4 x 3 Jacobian.  Per iteration (J^T J + lambda diag(J^T J)) d = -J^T r by a
//   3 x 3 Cholesky; X + d is accepted iff its cost is strictly smaller (a NaN cost compares
//   false), then lambda /= 10 (floor 1e-12), else lambda *= 10.  Stops: an accepted step
//   with |d| <= 1e-14 |X| (status 0), lambda > 1e12 (1), max_iter iterations (3); a point
//   whose initial cost is not finite is returned unchanged (2).  A failed factorisation gives
//   a non-finite d and so a rejected step.
// * k_reproj_error / k_reproj_mean: Util.print_reprojection_error (Util.py:65-82): the two
//   norms per point, and their mean by one workgroup's block_sum256_tree (no atomics).
// * k_link_points / k_link_compact: the 2D -> 3D association loop (Runner.py:241-250) on
//   integer pixels: per query the first target of the smallest squared distance (int64,
//   exact), kept iff sqrt((double)d2) < threshold; kept pairs compacted in query order.
// Float64 throughout; -ffp-contract=off, fmas written where wanted; every small-matrix index
// is a compile-time constant so the matrices stay in registers.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "f64_dev.h"
#include "kernels.h"

namespace sfm {

// one camera's two residuals p - pi(P X) (SFM.py:264-271) and their gradients
SFM_DEV void camera_residual(const double (&P)[12], const double (&X)[3], double px, double py, double& r0,
                             double& r1, double (&J0)[3], double (&J1)[3]) {
  const double h0 = fma(P[0], X[0], fma(P[1], X[1], fma(P[2], X[2], P[3])));
  const double h1 = fma(P[4], X[0], fma(P[5], X[1], fma(P[6], X[2], P[7])));
  const double h2 = fma(P[8], X[0], fma(P[9], X[1], fma(P[10], X[2], P[11])));
  const double u = h0 / h2, v = h1 / h2, iw = 1.0 / h2;
  r0 = px - u;
  r1 = py - v;
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // d(p - h_a / h_2) / dX_k = -(P[a][k] - (h_a / h_2) P[2][k]) / h_2
    J0[k] = -(fma(-u, P[8 + k], P[k]) * iw);
    J1[k] = -(fma(-v, P[8 + k], P[4 + k]) * iw);
  }
}

struct PointEval {
  double r[4];
  double J[4][3];
  double cost;
};

SFM_DEV void evaluate_point(const double (&P1)[12], const double (&P2)[12], const double (&X)[3], double a,
                            double b, double c, double d, PointEval& e) {
  camera_residual(P1, X, a, b, e.r[0], e.r[1], e.J[0], e.J[1]);
  camera_residual(P2, X, c, d, e.r[2], e.r[3], e.J[2], e.J[3]);
  e.cost = fma(e.r[3], e.r[3], fma(e.r[2], e.r[2], fma(e.r[1], e.r[1], e.r[0] * e.r[0])));
}

__global__ void __launch_bounds__(128) k_refine_points(const double* X0, const double* __restrict__ x1,
                                                       const double* __restrict__ x2, int64_t N,
                                                       const double* __restrict__ Pm, int S,
                                                       const int32_t* __restrict__ seg, int max_iter, double* X,
                                                       double* __restrict__ cost, int32_t* __restrict__ iters) {
  const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= N) return;
  const int s = clamp_index(seg ? seg[i] : 0, S);
  double P1[12], P2[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    P1[k] = Pm[(int64_t)s * 24 + k];
    P2[k] = Pm[(int64_t)s * 24 + 12 + k];
  }
  const double a = x1[2 * i], b = x1[2 * i + 1], c = x2[2 * i], d = x2[2 * i + 1];
  double Xc[3] = {X0[3 * i], X0[3 * i + 1], X0[3 * i + 2]};
  PointEval cur;
  evaluate_point(P1, P2, Xc, a, b, c, d, cur);
  int accepted = 0, status = kRefineMaxIter;
  if (!finite_f64(cur.cost)) {
    status = kRefineNonFinite;
  } else {
    double lam = 1e-3;
    for (int it = 0; it < max_iter; ++it) {
      // H = J^T J (upper triangle), g = J^T r
      double H00 = 0.0, H01 = 0.0, H02 = 0.0, H11 = 0.0, H12 = 0.0, H22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        H00 = fma(cur.J[q][0], cur.J[q][0], H00);
        H01 = fma(cur.J[q][0], cur.J[q][1], H01);
        H02 = fma(cur.J[q][0], cur.J[q][2], H02);
        H11 = fma(cur.J[q][1], cur.J[q][1], H11);
        H12 = fma(cur.J[q][1], cur.J[q][2], H12);
        H22 = fma(cur.J[q][2], cur.J[q][2], H22);
        g0 = fma(cur.J[q][0], cur.r[q], g0);
        g1 = fma(cur.J[q][1], cur.r[q], g1);
        g2 = fma(cur.J[q][2], cur.r[q], g2);
      }
      // Cholesky of H + lam diag(H); a pivot <= 0 gives NaN / inf, which the cost test rejects
      const double l00 = sqrt(fma(lam, H00, H00));
      const double l10 = H01 / l00, l20 = H02 / l00;
      const double l11 = sqrt(fma(-l10, l10, fma(lam, H11, H11)));
      const double l21 = fma(-l20, l10, H12) / l11;
      const double l22 = sqrt(fma(-l21, l21, fma(-l20, l20, fma(lam, H22, H22))));
      const double y0 = -g0 / l00;
      const double y1 = fma(-l10, y0, -g1) / l11;
      const double y2 = fma(-l21, y1, fma(-l20, y0, -g2)) / l22;
      const double d2 = y2 / l22;
      const double d1 = fma(-l21, d2, y1) / l11;
      const double d0 = fma(-l20, d2, fma(-l10, d1, y0)) / l00;
      const double Xt[3] = {Xc[0] + d0, Xc[1] + d1, Xc[2] + d2};
      PointEval tr;
      evaluate_point(P1, P2, Xt, a, b, c, d, tr);
      if (tr.cost < cur.cost) {
        const double nd = sqrt(fma(d2, d2, fma(d1, d1, d0 * d0)));
        const double nx = sqrt(fma(Xc[2], Xc[2], fma(Xc[1], Xc[1], Xc[0] * Xc[0])));
        Xc[0] = Xt[0], Xc[1] = Xt[1], Xc[2] = Xt[2];
        cur = tr;
        lam = fmax(lam / 10.0, 1e-12);
        ++accepted;
        if (nd <= 1e-14 * nx) {
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
  X[3 * i] = Xc[0];
  X[3 * i + 1] = Xc[1];
  X[3 * i + 2] = Xc[2];
  cost[i] = cur.cost;
  iters[i] = accepted | (status << kRefineStatusShift);
}

void launch_refine_points(const double* X0, const double* x1, const double* x2, int64_t N, const double* P, int S,
                          const int32_t* seg, int max_iter, double* X, double* cost, int32_t* iters,
                          hipStream_t st) {
  if (N < 1) return;
  hipLaunchKernelGGL(k_refine_points, dim3((unsigned)((N + 127) / 128)), dim3(128), 0, st, X0, x1, x2, N, P, S, seg,
                     max_iter, X, cost, iters);
}

// ---------------- reprojection error (Util.py:65-82) ----------------

__global__ void __launch_bounds__(128) k_reproj_error(const double* __restrict__ X, const double* __restrict__ x1,
                                                      const double* __restrict__ x2, int64_t N,
                                                      const double* __restrict__ P1g,
                                                      const double* __restrict__ P2g, double* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (i >= N) return;
  double P1[12], P2[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    P1[k] = P1g[k];
    P2[k] = P2g[k];
  }
  const double Xc[3] = {X[3 * i], X[3 * i + 1], X[3 * i + 2]};
  PointEval e;
  evaluate_point(P1, P2, Xc, x1[2 * i], x1[2 * i + 1], x2[2 * i], x2[2 * i + 1], e);
  err[2 * i] = sqrt(e.r[0] * e.r[0] + e.r[1] * e.r[1]);  // np.linalg.norm (Util.py:76-77)
  err[2 * i + 1] = sqrt(e.r[2] * e.r[2] + e.r[3] * e.r[3]);
}

// mean over points of (e1 + e2) / 2 (Util.py:81): strided partial sums in index order, then
// block_sum256_tree: the same bits every run.  N == 0 gives NaN, as np.mean([]).
__global__ void __launch_bounds__(256) k_reproj_mean(const double* __restrict__ err, int64_t N,
                                                     double* __restrict__ mean) {
  __shared__ double s_red[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t i = tid; i < N; i += 256) acc += (err[2 * i] + err[2 * i + 1]) / 2.0;
  const double sum = block_sum256_tree(acc, s_red);
  if (tid == 0) *mean = N > 0 ? sum / (double)N : __builtin_nan("");
}

void launch_reproj_error(const double* X, const double* x1, const double* x2, int64_t N, const double* P1,
                         const double* P2, double* err, double* mean, hipStream_t st) {
  if (N > 0)
    hipLaunchKernelGGL(k_reproj_error, dim3((unsigned)((N + 127) / 128)), dim3(128), 0, st, X, x1, x2, N, P1, P2,
                       err);
  hipLaunchKernelGGL(k_reproj_mean, dim3(1), dim3(256), 0, st, (const double*)err, N, mean);
}

// ---------------- 2D -> 3D association (Runner.py:241-250) ----------------

// one thread per query; the targets pass through LDS in chunks of kRansacChunk points.
// best [nq]: the kept query's target index, or -1; block_kept [blocks]: kept queries per workgroup
__global__ void __launch_bounds__(kLinkThreads) k_link_points(const int32_t* __restrict__ tgt, int m,
                                                              const int32_t* __restrict__ qry, int nq,
                                                              double threshold, int32_t* __restrict__ best,
                                                              int32_t* __restrict__ block_kept) {
  __shared__ int2 s_t[kRansacChunk];
  __shared__ int s_cnt[kLinkThreads / 64];
  const int tid = threadIdx.x;
  const int q = blockIdx.x * kLinkThreads + tid;
  const bool have = q < nq;
  const int64_t qx = have ? qry[2 * q] : 0, qy = have ? qry[2 * q + 1] : 0;
  int64_t bd = INT64_MAX;
  int bi = -1;
  for (int c0 = 0; c0 < m; c0 += kRansacChunk) {
    const int cn = min(kRansacChunk, m - c0);
    __syncthreads();
    for (int j = tid; j < cn; j += kLinkThreads)
      s_t[j] = make_int2(tgt[2 * (int64_t)(c0 + j)], tgt[2 * (int64_t)(c0 + j) + 1]);
    __syncthreads();
    if (have) {
      for (int j = 0; j < cn; ++j) {
        const int2 t = s_t[j];
        const int64_t dx = (int64_t)t.x - qx, dy = (int64_t)t.y - qy;
        const int64_t d2 = dx * dx + dy * dy;
        if (d2 < bd) {  // strict: the first index of the smallest distance (np.argmin)
          bd = d2;
          bi = c0 + j;
        }
      }
    }
  }
  const bool keep = have && bi >= 0 && sqrt((double)bd) < threshold;  // Runner.py:245
  if (have) best[q] = keep ? bi : -1;
  const unsigned long long bal = __ballot(keep);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = __popcll(bal);
  __syncthreads();
  if (tid == 0) {
    int n = 0;
#pragma unroll
    for (int w = 0; w < kLinkThreads / 64; ++w) n += s_cnt[w];
    block_kept[blockIdx.x] = n;
  }
}

// same grid: kept (target, query) pairs written in query order; the last workgroup writes the total
__global__ void __launch_bounds__(kLinkThreads) k_link_compact(const int32_t* __restrict__ best,
                                                               const int32_t* __restrict__ block_kept, int nq,
                                                               int32_t* __restrict__ out_tgt,
                                                               int32_t* __restrict__ out_qry,
                                                               int32_t* __restrict__ out_n) {
  __shared__ int s_red[kLinkThreads];
  __shared__ int s_cnt[kLinkThreads / 64];
  const int tid = threadIdx.x;
  int part = 0;  // kept queries of the workgroups before this one
  for (int b = tid; b < (int)blockIdx.x; b += kLinkThreads) part += block_kept[b];
  s_red[tid] = part;
  __syncthreads();
  for (int off = kLinkThreads / 2; off >= 1; off >>= 1) {
    if (tid < off) s_red[tid] += s_red[tid + off];
    __syncthreads();
  }
  const int base = s_red[0];
  const int q = blockIdx.x * kLinkThreads + tid;
  const int bi = q < nq ? best[q] : -1;
  const bool keep = bi >= 0;
  const unsigned long long bal = __ballot(keep);
  const int lane = tid & 63, wid = tid >> 6;
  if (lane == 0) s_cnt[wid] = __popcll(bal);
  __syncthreads();
  int before = __popcll(bal & ((1ull << lane) - 1ull));
  int total = 0;
#pragma unroll
  for (int w = 0; w < kLinkThreads / 64; ++w) {
    if (w < wid) before += s_cnt[w];
    total += s_cnt[w];
  }
  if (keep) {
    out_tgt[base + before] = bi;
    out_qry[base + before] = q;
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) *out_n = base + total;
}

int link_blocks(int nq) { return (nq + kLinkThreads - 1) / kLinkThreads; }

void launch_link_points(const int32_t* tgt, int m, const int32_t* qry, int nq, double threshold, int32_t* best,
                        int32_t* block_kept, int32_t* out_tgt, int32_t* out_qry, int32_t* out_n, hipStream_t st) {
  if (nq < 1 || m < 1) return;
  const int blocks = link_blocks(nq);
  hipLaunchKernelGGL(k_link_points, dim3(blocks), dim3(kLinkThreads), 0, st, tgt, m, qry, nq, threshold, best,
                     block_kept);
  hipLaunchKernelGGL(k_link_compact, dim3(blocks), dim3(kLinkThreads), 0, st, (const int32_t*)best,
                     (const int32_t*)block_kept, nq, out_tgt, out_qry, out_n);
}

}  // namespace sfm
