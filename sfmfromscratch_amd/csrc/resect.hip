// resect.hip — the pose of every unposed frame of a slot table from its feature tracks, all
// frames in one call (include/sfmfeat.h sfm_resect_tracks_dev has the rule).
// A row r of slot s is linked to the point X[node_track[s][r]]; the links need no gather on the
// host.  The hypothesis, the count and the refinement are pnp.hip's (pnp_dev.h: one copy of the
// arithmetic); the samples are the counter stream of verify_dev.h at sample size 6.
//
// Five launches, whatever nimg is; a workgroup's slot is blockIdx.x / (workgroups per slot):
// * k_resect_links, one 256-thread workgroup per slot: the slot's links compacted in ascending
//   row order by a block scan (no atomics) into the workspace as float64 (X, pixel) with their
//   rows; n_links; whether the slot is attempted.  A slot that is not gets its whole record here
//   ("not attempted", NaN pose, zero rkeep row, zero counts, NaN hypotheses), so the workgroups
//   of the later kernels that serve it leave at once.
// * k_resect_hyp, one thread per (slot, sample), one wave per workgroup (the 11 x 12 system in
//   LDS, 66 KB per wave: two workgroups per CU; four waves of it would not fit one, which is why
//   hypothesis and count are not one 256-thread kernel).
// * k_resect_count, one wave per (slot, sample), 8 samples per workgroup, the slot's links staged
//   in LDS in chunks of kRansacChunk.
// * k_resect_select, one workgroup per slot: the lowest sample with the largest count, posed iff
//   that count is > 0 and >= min_inliers, the winner's mask by the same test, its inliers in
//   link order, rkeep.
// * k_resect_refine, one workgroup per slot: pnp_lm_block over the winner's inliers.
// Float64 throughout; -ffp-contract=off, fmas written where wanted.
#include <algorithm>

#include "pnp_dev.h"
#include "verify_dev.h"

namespace sfm {

namespace {

SFM_DEV uint64_t resect_key(uint64_t seed, int s) {
  return mix64(mix64(seed ^ kResectSeedXor) + (uint64_t)(uint32_t)s);
}

// finite and upper triangular with a non-zero diagonal (pose._pnp_inputs' condition)
SFM_DEV bool resect_K_ok(const double* __restrict__ K) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) ok = ok && finite_f64(K[k]);
  return ok && K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[0] != 0.0 && K[4] != 0.0 && K[8] != 0.0;
}

__global__ void __launch_bounds__(kPnpThreads) k_resect_links(ResectProblem q) {
  __shared__ uint32_t s_scan[kPnpThreads / 64 + 1];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int cap = q.cap;
  const int c = min(max(q.count[s], 0), cap);
  const int32_t* nt = q.node_track + (int64_t)s * cap;
  const int2* px = reinterpret_cast<const int2*>(q.xy) + (int64_t)s * cap;
  double* Xl = q.Xl + (int64_t)s * cap * 3;
  double* xl = q.xl + (int64_t)s * cap * 2;
  int32_t* lrow = q.lrow + (int64_t)s * cap;
  uint32_t base = 0;
  for (int r0 = 0; r0 < c; r0 += kPnpThreads) {
    const int r = r0 + tid;
    bool link = false;
    double P0 = 0.0, P1 = 0.0, P2 = 0.0;
    if (r < c) {
      const int t = nt[r];
      if (t >= 0 && t < q.n_tracks) {
        P0 = q.X[3 * (int64_t)t], P1 = q.X[3 * (int64_t)t + 1], P2 = q.X[3 * (int64_t)t + 2];
        link = finite_f64(P0) && finite_f64(P1) && finite_f64(P2);
      }
    }
    uint32_t total;
    const uint32_t pos = base + block_exclusive_scan(link ? 1u : 0u, s_scan, &total);
    if (link) {
      const int2 p = px[r];
      Xl[3 * (int64_t)pos] = P0, Xl[3 * (int64_t)pos + 1] = P1, Xl[3 * (int64_t)pos + 2] = P2;
      xl[2 * (int64_t)pos] = (double)p.x, xl[2 * (int64_t)pos + 1] = (double)p.y;
      lrow[pos] = r;
    }
    base += total;
  }
  const int n = (int)base;
  const bool go = (!q.attempt || q.attempt[s] != 0) && n >= 6 && resect_K_ok(q.K + 9 * (int64_t)s);
  int32_t* st = q.rstat + 8 * (int64_t)s;
  if (tid == 0) {
    q.n_links[s] = n;
    q.go[s] = go ? 1 : 0;
    st[3] = n;
  }
  if (go) return;  // k_resect_select and k_resect_refine write the rest of the record
  if (tid < 8 && tid != 3) st[tid] = (tid == 0 || tid == 1 || tid == 5) ? -1 : 0;
  if (tid < 12) q.pose[12 * (int64_t)s + tid] = __builtin_nan("");
  if (tid < 2) q.rcost[2 * (int64_t)s + tid] = __builtin_nan("");
  if (q.rkeep)
    for (int r = tid; r < cap; r += kPnpThreads) q.rkeep[(int64_t)s * cap + r] = 0;
  if (q.out_counts)
    for (int it = tid; it < q.iters; it += kPnpThreads) q.out_counts[(int64_t)s * q.iters + it] = 0;
  if (q.out_hyp)
    for (int64_t k = tid; k < (int64_t)q.iters * 12; k += kPnpThreads)
      q.out_hyp[(int64_t)s * q.iters * 12 + k] = __builtin_nan("");
}

__global__ void __launch_bounds__(64) k_resect_hyp(ResectProblem q, int per_slot) {
  extern __shared__ __attribute__((aligned(16))) double s_A[];  // [11 * 12][64]
  const int s = blockIdx.x / per_slot;
  if (!q.go[s]) return;  // (the kernel has no barrier)
  const int lane = threadIdx.x;
  const int it = (blockIdx.x - s * per_slot) * 64 + lane;
  if (it >= q.iters) return;
  const int n = q.n_links[s];
  int idx[6];
  sample_indices<6>(resect_key(q.seed, s), it, n, idx);
  double Rt[12];
  pnp_hypothesis(q.Xl + (int64_t)s * q.cap * 3, q.xl + (int64_t)s * q.cap * 2, q.K + 9 * (int64_t)s,
                 [&](int i) { return idx[i]; }, s_A, lane, Rt);
  double* o = q.hyp + ((int64_t)s * q.iters + it) * 12;
#pragma unroll
  for (int k = 0; k < 12; ++k) o[k] = Rt[k];
}

__global__ void __launch_bounds__(64 * kPnpWaves) k_resect_count(ResectProblem q, int per_slot) {
  extern __shared__ __attribute__((aligned(16))) double s_p[];  // [5][min(n, kRansacChunk)]
  const int s = blockIdx.x / per_slot;
  if (!q.go[s]) return;  // uniform over the workgroup
  pnp_count_block(q.Xl + (int64_t)s * q.cap * 3, q.xl + (int64_t)s * q.cap * 2, q.K + 9 * (int64_t)s, q.n_links[s],
                  q.hyp + (int64_t)s * q.iters * 12, q.iters, q.thr, q.counts + (int64_t)s * q.iters,
                  blockIdx.x - s * per_slot, s_p);
}

__global__ void __launch_bounds__(kPnpThreads) k_resect_select(ResectProblem q) {
  __shared__ int s_bc[kPnpThreads], s_bi[kPnpThreads];
  __shared__ uint32_t s_scan[kPnpThreads / 64 + 1];
  const int s = blockIdx.x, tid = threadIdx.x;
  if (!q.go[s]) return;
  const int cap = q.cap, n = q.n_links[s], iters = q.iters;
  const int32_t* counts = q.counts + (int64_t)s * iters;
  int bc = -1, bi = 0x7fffffff;
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
  const int best = iters > 0 ? s_bi[0] : -1, best_count = iters > 0 ? s_bc[0] : 0;
  const bool posed = best_count > 0 && best_count >= q.min_inliers;
  int32_t* st = q.rstat + 8 * (int64_t)s;
  if (tid == 0) {
    st[0] = best_count;
    st[1] = best;
    st[2] = iters;
  }
  uint8_t* keep = q.rkeep ? q.rkeep + (int64_t)s * cap : nullptr;
  if (keep)
    for (int r = tid; r < cap; r += kPnpThreads) keep[r] = 0;
  if (!posed) {
    if (tid == 0) q.n_inl[s] = 0;
    if (tid >= 4 && tid < 8) st[tid] = tid == 5 ? -1 : 0;
    if (tid < 12) q.pose[12 * (int64_t)s + tid] = __builtin_nan("");
    if (tid < 2) q.rcost[2 * (int64_t)s + tid] = __builtin_nan("");
    return;
  }
  __syncthreads();  // the zeros of rkeep are written before any 1
  const double* X = q.Xl + (int64_t)s * cap * 3;
  const double* x = q.xl + (int64_t)s * cap * 2;
  const int32_t* lrow = q.lrow + (int64_t)s * cap;
  int32_t* inl = q.inl + (int64_t)s * cap;
  double Kc[6], R[9], t[3];
  load_K6(q.K + 9 * (int64_t)s, Kc);
  const double* H = q.hyp + ((int64_t)s * iters + best) * 12;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = H[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = H[9 + k];
  uint32_t base = 0;
  for (int i0 = 0; i0 < n; i0 += kPnpThreads) {
    const int i = i0 + tid;
    bool in = false;
    if (i < n)  // the same test as the count, so the mask has the count
      in = pnp_inlier(Kc, R, t, X[3 * (int64_t)i], X[3 * (int64_t)i + 1], X[3 * (int64_t)i + 2], x[2 * (int64_t)i],
                      x[2 * (int64_t)i + 1], q.thr);
    uint32_t total;
    const uint32_t pos = block_exclusive_scan(in ? 1u : 0u, s_scan, &total);
    if (in) {
      inl[base + pos] = i;
      if (keep) keep[lrow[i]] = 1;
    }
    base += total;
  }
  if (tid == 0) q.n_inl[s] = (int32_t)base;
  if (tid < 12) q.Rt0[12 * (int64_t)s + tid] = H[tid];
}

__global__ void __launch_bounds__(kPnpThreads) k_resect_refine(ResectProblem q) {
  __shared__ double s_red[kPnpThreads / 64][kPnpSums];
  const int s = blockIdx.x;
  if (!q.go[s]) return;
  const int n = q.n_links[s];
  const int m = min(q.n_inl[s], n);
  if (m <= 0) return;  // not posed: k_resect_select wrote the record (uniform over the workgroup)
  double R[9], t[3];
  const double* Rt_in = q.Rt0 + 12 * (int64_t)s;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = Rt_in[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = Rt_in[9 + k];
  // (a posed winner counted an inlier, so its hypothesis is finite)
  pnp_lm_block(q.Xl + (int64_t)s * q.cap * 3, q.xl + (int64_t)s * q.cap * 2, q.K + 9 * (int64_t)s, n,
               q.inl + (int64_t)s * q.cap, m, R, t, q.max_refine_iter, q.pose + 12 * (int64_t)s,
               q.pose + 12 * (int64_t)s + 9, q.rstat + 8 * (int64_t)s + 4, q.rcost + 2 * (int64_t)s, s_red);
}

}  // namespace

void launch_resect_tracks(const ResectProblem& q, hipStream_t st) {
  static const bool lds_attr = [] {  // 66 KB per hypothesis wave, up to kRansacChunk x 40 B of staged links
    return hipFuncSetAttribute((const void*)k_resect_hyp, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kPnpHypLdsBytes) == hipSuccess &&
           hipFuncSetAttribute((const void*)k_resect_count, hipFuncAttributeMaxDynamicSharedMemorySize,
                               kRansacChunk * 40) == hipSuccess;
  }();
  (void)lds_attr;
  hipLaunchKernelGGL(k_resect_links, dim3(q.nimg), dim3(kPnpThreads), 0, st, q);
  if (q.iters > 0) {
    const int hyp_per = (q.iters + 63) / 64, cnt_per = (q.iters + kPnpWaves - 1) / kPnpWaves;
    hipLaunchKernelGGL(k_resect_hyp, dim3((unsigned)(q.nimg * (int64_t)hyp_per)), dim3(64), kPnpHypLdsBytes, st, q,
                       hyp_per);
    hipLaunchKernelGGL(k_resect_count, dim3((unsigned)(q.nimg * (int64_t)cnt_per)), dim3(64 * kPnpWaves),
                       (size_t)std::min(q.cap, kRansacChunk) * 40, st, q, cnt_per);
  }
  hipLaunchKernelGGL(k_resect_select, dim3(q.nimg), dim3(kPnpThreads), 0, st, q);
  hipLaunchKernelGGL(k_resect_refine, dim3(q.nimg), dim3(kPnpThreads), 0, st, q);
}

}  // namespace sfm
