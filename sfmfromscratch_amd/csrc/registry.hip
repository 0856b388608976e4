// registry.hip — the global 3-D point registry and the bundle-adjustment input score: what
// SFMRunner.perform does with every batch of points after the structure stage
// (SFMRunner.add_points / is_new_point / find_existing_point, Runner.py:361-385, called at
// :217, :269, :280) and the figure it prints around bundle adjustment
// (total_reprojection_error, Runner.py:311-334).  DESIGN.md §13C.
//
// The reference walks the incoming points in order; point p is appended to the registry G
// when G is empty or min_j |G_j - p| >= threshold, otherwise it takes the first index of the
// smallest distance.  Points appended earlier in the same call count.  On the device:
//
// * k_reg_dist<false>: every point against the registry as it stood before the call.  The
//   registry is split across workgroups (grid.y); each workgroup stages its span in LDS in
//   chunks of kRegChunk entries and keeps, per point, the first-index minimum of the
//   distances below the threshold: one (distance, index) partial per (point, split).
//   The inner loop compares d^2 with a bound slightly above threshold^2; only survivors take
//   the (correctly rounded) square root and the exact `<`, so the result is the reference's.
// * k_reg_dist<true>: the same launch shape over the call's own points, restricted to the
//   earlier ones (k < i), whatever their status: the smallest such distance per point.
// * k_reg_reduce: both sets of partials reduced in registry order (strict `<`: the first
//   index wins ties).  A point is *contested* when an earlier point of the call is within
//   the threshold and strictly nearer than its hit in the old registry (a tie goes to the
//   old registry, whose indices are lower, so only a strictly nearer point of the call can
//   change the answer).  An uncontested point is new iff the old registry gave no hit.
// * k_reg_resolve (one workgroup): the contested points in index order — its threads scan
//   the earlier points of the call that are new (final by then), nearest wins, lower k on
//   ties; then an exclusive scan of the new flags gives the slots count + rank, the indices
//   and flags are written, the new coordinates appended and the device-resident count
//   updated.  The serial part is the walk over contested points only.
// * k_total_reproj / k_total_mean: per observation |pi(K (R X + t)) - obs| with R from the
//   Rodrigues vector (linalg3.h rodrigues), and the mean by one workgroup's block_sum256_tree.
// Float64 throughout; -ffp-contract=off (no fused multiply-add anywhere in this file: the
// distance is numpy's (dx*dx + dy*dy) + dz*dz).
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "f64_dev.h"
#include "kernels.h"
#include "linalg3.h"

namespace sfm {

constexpr int kRegWaves = kRegThreads / 64;
constexpr int kRegContested = -2;  // res[]: decided by the walk (>= 0 old index, -1 new, <= -3 point -(r + 3) of the call)

SFM_DEV int reg_count(const int32_t* count_p, int capacity) {
  const int c = *count_p;
  return c < 0 ? 0 : (c > capacity ? capacity : c);
}

// tab: the registry (kSelf: the call's own points), limit: entries that count for this
// workgroup; part_d / part_j [splits][n]
template <bool kSelf>
__global__ void __launch_bounds__(kRegThreads) k_reg_dist(const double* __restrict__ tab,
                                                          const int32_t* __restrict__ count_p, int capacity,
                                                          const double* __restrict__ pts, int n, int span, double thr,
                                                          double bound, double* __restrict__ part_d,
                                                          int32_t* __restrict__ part_j) {
  __shared__ double s_x[kRegChunk], s_y[kRegChunk], s_z[kRegChunk];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kRegThreads + tid;
  const int split = blockIdx.y;
  // self: point i sees entries k < i, so this workgroup needs none at or beyond its last point
  const int limit = kSelf ? min(n, (int)(blockIdx.x + 1) * kRegThreads) : reg_count(count_p, capacity);
  const int64_t begin64 = (int64_t)split * span;
  if (begin64 >= limit) return;  // (the whole workgroup: no barrier is skipped by a part of it)
  const int begin = (int)begin64;
  const int end = (int)min((int64_t)limit, begin64 + span);
  const bool have = i < n;
  // a thread without a point compares NaN: never below the bound
  const double px = have ? pts[3 * (int64_t)i] : __builtin_nan("");
  const double py = have ? pts[3 * (int64_t)i + 1] : 0.0;
  const double pz = have ? pts[3 * (int64_t)i + 2] : 0.0;
  double best = __builtin_inf();
  int bj = -1;
  for (int c0 = begin; c0 < end; c0 += kRegChunk) {
    const int cn = min(kRegChunk, end - c0);
    __syncthreads();
    for (int j = tid; j < cn; j += kRegThreads) {
      const int64_t o = 3 * (int64_t)(c0 + j);
      s_x[j] = tab[o];
      s_y[j] = tab[o + 1];
      s_z[j] = tab[o + 2];
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < cn; ++j) {
      const double dx = s_x[j] - px, dy = s_y[j] - py, dz = s_z[j] - pz;
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 <= bound && (!kSelf || c0 + j < i)) {  // rare: the exact test on the rounded distance
        const double d = sqrt(d2);
        if (d < thr && d < best) {  // strict: the first index of the smallest distance
          best = d;
          bj = c0 + j;
        }
      }
    }
  }
  if (have) {
    part_d[(int64_t)split * n + i] = best;
    if (!kSelf) part_j[(int64_t)split * n + i] = bj;
  }
}

// per point: (old_d, old_j) the hit in the old registry (inf, -1: none); res = old_j, or
// kRegContested when an earlier point of the call is strictly nearer than that hit
__global__ void __launch_bounds__(kRegThreads) k_reg_reduce(const int32_t* __restrict__ count_p, int capacity, int n,
                                                            int span_old, int span_self,
                                                            const double* __restrict__ part_d,
                                                            const int32_t* __restrict__ part_j,
                                                            const double* __restrict__ self_d,
                                                            double* __restrict__ old_d, int32_t* __restrict__ old_j,
                                                            int32_t* __restrict__ res) {
  const int i = blockIdx.x * kRegThreads + threadIdx.x;
  if (i >= n) return;
  const int count = reg_count(count_p, capacity);
  const int ns = count > 0 ? (count - 1) / span_old + 1 : 0;  // splits that begin below count
  double best = __builtin_inf();
  int bj = -1;
  for (int s = 0; s < ns; ++s) {
    const double d = part_d[(int64_t)s * n + i];
    if (d < best) {
      best = d;
      bj = part_j[(int64_t)s * n + i];
    }
  }
  const int nself = i > 0 ? (i - 1) / span_self + 1 : 0;  // splits that begin below i
  double sm = __builtin_inf();
  for (int s = 0; s < nself; ++s) sm = fmin(sm, self_d[(int64_t)s * n + i]);
  old_d[i] = best;
  old_j[i] = bj;
  res[i] = sm < best ? kRegContested : bj;
}

// flags of one 256-thread step -> this thread's rank among them and their number
SFM_DEV void reg_rank(bool f, int tid, int* s_cnt, int& before, int& total) {
  const unsigned long long bal = __ballot(f);
  const int lane = tid & 63, wid = tid >> 6;
  __syncthreads();  // (s_cnt of the previous step has been read)
  if (lane == 0) s_cnt[wid] = __popcll(bal);
  __syncthreads();
  before = __popcll(bal & ((1ull << lane) - 1ull));
  total = 0;
#pragma unroll
  for (int w = 0; w < kRegWaves; ++w) {
    if (w < wid) before += s_cnt[w];
    total += s_cnt[w];
  }
}

// one workgroup.  res is read and written across its threads between barriers (no __restrict__);
// tab may hold pts (rows below count), out_index is read back in the last pass.
__global__ void __launch_bounds__(kRegThreads) k_reg_resolve(double* tab, int32_t* count_p, int capacity,
                                                             const double* pts, int n, double thr, double bound,
                                                             const double* __restrict__ old_d,
                                                             const int32_t* __restrict__ old_j, int32_t* res,
                                                             int32_t* clist, int32_t* out_index,
                                                             int32_t* __restrict__ out_is_new) {
  __shared__ int s_cnt[kRegWaves];
  __shared__ double s_d[kRegWaves];
  __shared__ int s_k[kRegWaves];
  const int tid = threadIdx.x;
  const int count = reg_count(count_p, capacity);
  // the contested points, in index order
  int nc = 0;
  for (int c = 0; c < n; c += kRegThreads) {
    const int i = c + tid;
    const bool f = i < n && res[i] == kRegContested;
    int before, total;
    reg_rank(f, tid, s_cnt, before, total);
    if (f) clist[nc + before] = i;
    nc += total;
  }
  for (int q = 0; q < nc; ++q) {
    __syncthreads();  // clist, and the res of every earlier contested point, are visible
    const int i = clist[q];
    const double px = pts[3 * (int64_t)i], py = pts[3 * (int64_t)i + 1], pz = pts[3 * (int64_t)i + 2];
    double best = __builtin_inf();
    int bk = 0x7fffffff;
    // (the status and the coordinates are loaded side by side, several k at a time: this loop is
    // load latency, and it is the serial part of the call)
#pragma unroll 4
    for (int k = tid; k < i; k += kRegThreads) {
      const int rk = res[k];
      const double dx = pts[3 * (int64_t)k] - px, dy = pts[3 * (int64_t)k + 1] - py, dz = pts[3 * (int64_t)k + 2] - pz;
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      if (rk == -1 && d2 <= bound) {  // only the new points of the call are in the registry
        const double d = sqrt(d2);
        if (d < thr && d < best) {  // k ascends within a thread
          best = d;
          bk = k;
        }
      }
    }
    // the smallest (distance, k) of the workgroup
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const double od = __shfl_xor(best, off);
      const int ok = __shfl_xor(bk, off);
      if (od < best || (od == best && ok < bk)) {
        best = od;
        bk = ok;
      }
    }
    if ((tid & 63) == 0) {
      s_d[tid >> 6] = best;
      s_k[tid >> 6] = bk;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < kRegWaves; ++w)
        if (s_d[w] < best || (s_d[w] == best && s_k[w] < bk)) {
          best = s_d[w];
          bk = s_k[w];
        }
      // a tie goes to the old registry (lower indices)
      res[i] = best < old_d[i] ? -(bk + 3) : old_j[i];
    }
  }
  __syncthreads();
  // slots of the new points: count + rank; indices, flags, appended coordinates
  int added = 0;
  for (int c = 0; c < n; c += kRegThreads) {
    const int i = c + tid;
    const int r = i < n ? res[i] : 0;
    const bool f = i < n && r == -1;
    int before, total;
    reg_rank(f, tid, s_cnt, before, total);
    if (f) {
      const int slot = count + added + before;
      out_index[i] = slot;
      out_is_new[i] = 1;
      if (slot < capacity) {  // (capacity >= count + n is the caller's contract)
        tab[3 * (int64_t)slot] = pts[3 * (int64_t)i];
        tab[3 * (int64_t)slot + 1] = pts[3 * (int64_t)i + 1];
        tab[3 * (int64_t)slot + 2] = pts[3 * (int64_t)i + 2];
      }
    } else if (i < n) {
      out_is_new[i] = 0;
      if (r >= 0) out_index[i] = r;
    }
    added += total;
  }
  __syncthreads();
  for (int i = tid; i < n; i += kRegThreads) {
    const int r = res[i];
    if (r <= -3) out_index[i] = out_index[-(r + 3)];  // a new point of this call: its slot
  }
  if (tid == 0) *count_p = min(count + added, capacity);
}

int registry_span(int entries, int* splits) {
  const int chunks = std::max(1, (entries + kRegChunk - 1) / kRegChunk);
  const int per = (chunks + kRegMaxSplits - 1) / kRegMaxSplits;
  *splits = (chunks + per - 1) / per;
  return per * kRegChunk;
}

void launch_registry_add(double* reg_xyz, int32_t* reg_count, int capacity, const double* pts, int n, double thr,
                         double* part_d, int32_t* part_j, double* self_d, double* old_d, int32_t* old_j,
                         int32_t* res, int32_t* clist, int32_t* out_index, int32_t* out_is_new, hipStream_t st) {
  if (n < 1) return;
  // d < thr needs d^2 < thr^2 (1 + 2^-51); anything up to the bound takes the exact test.
  // (thr^2 may underflow or overflow: then everything tiny, or everything, takes it.)
  const double bound = std::max(thr * thr * 1.000001, 2.2250738585072014e-308);
  const int pblocks = (n + kRegThreads - 1) / kRegThreads;
  int splits_old, splits_self;
  const int span_old = registry_span(capacity, &splits_old);
  const int span_self = registry_span(n, &splits_self);
  hipLaunchKernelGGL(k_reg_dist<false>, dim3(pblocks, splits_old), dim3(kRegThreads), 0, st,
                     (const double*)reg_xyz, (const int32_t*)reg_count, capacity, pts, n, span_old, thr, bound,
                     part_d, part_j);
  hipLaunchKernelGGL(k_reg_dist<true>, dim3(pblocks, splits_self), dim3(kRegThreads), 0, st, pts,
                     (const int32_t*)nullptr, 0, pts, n, span_self, thr, bound, self_d, (int32_t*)nullptr);
  hipLaunchKernelGGL(k_reg_reduce, dim3(pblocks), dim3(kRegThreads), 0, st, (const int32_t*)reg_count, capacity, n,
                     span_old, span_self, (const double*)part_d, (const int32_t*)part_j, (const double*)self_d,
                     old_d, old_j, res);
  hipLaunchKernelGGL(k_reg_resolve, dim3(1), dim3(kRegThreads), 0, st, reg_xyz, reg_count, capacity, pts, n, thr,
                     bound, (const double*)old_d, (const int32_t*)old_j, res, clist, out_index, out_is_new);
}

// ---------------- total reprojection error (Runner.py:311-334) ----------------

__global__ void __launch_bounds__(128) k_total_reproj(const int32_t* __restrict__ cam_idx,
                                                      const int32_t* __restrict__ pt_idx,
                                                      const double* __restrict__ obs, int64_t M,
                                                      const double* __restrict__ cams, int n_cam,
                                                      const double* __restrict__ Kg, const double* __restrict__ X,
                                                      int n_pts, double* __restrict__ err) {
  const int64_t o = (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (o >= M) return;
  const int c = clamp_index(cam_idx[o], n_cam), p = clamp_index(pt_idx[o], n_pts);
  const double* cp = cams + 6 * (int64_t)c;
  double R[9], Y[3];
  rodrigues(cp[0], cp[1], cp[2], R);
  rotate3(R, X[3 * (int64_t)p], X[3 * (int64_t)p + 1], X[3 * (int64_t)p + 2], Y);
  const double a0 = Y[0] + cp[3], a1 = Y[1] + cp[4], a2 = Y[2] + cp[5];
  const double* K = Kg + 9 * (int64_t)c;
  const double q0 = K[0] * a0 + K[1] * a1 + K[2] * a2;
  const double q1 = K[3] * a0 + K[4] * a1 + K[5] * a2;
  const double q2 = K[6] * a0 + K[7] * a1 + K[8] * a2;
  const double ex = q0 / q2 - obs[2 * o], ey = q1 / q2 - obs[2 * o + 1];
  err[o] = sqrt(ex * ex + ey * ey);
}

// mean over the M observations: strided partial sums in index order, then block_sum256_tree:
// the same bits every run.  M == 0 gives NaN.
__global__ void __launch_bounds__(256) k_total_mean(const double* __restrict__ err, int64_t M,
                                                    double* __restrict__ mean) {
  __shared__ double s_red[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int64_t i = tid; i < M; i += 256) acc += err[i];
  const double sum = block_sum256_tree(acc, s_red);
  if (tid == 0) *mean = M > 0 ? sum / (double)M : __builtin_nan("");
}

void launch_total_reproj(const int32_t* cam_idx, const int32_t* pt_idx, const double* obs, int64_t M,
                         const double* cams, int n_cam, const double* K, const double* X, int n_pts, double* err,
                         double* mean, hipStream_t st) {
  if (M > 0)
    hipLaunchKernelGGL(k_total_reproj, dim3((unsigned)((M + 127) / 128)), dim3(128), 0, st, cam_idx, pt_idx, obs, M,
                       cams, n_cam, K, X, n_pts, err);
  hipLaunchKernelGGL(k_total_mean, dim3(1), dim3(256), 0, st, (const double*)err, M, mean);
}

}  // namespace sfm
