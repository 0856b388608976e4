// ransac.hip — the match consumer CameraPose.find_inliers (SFM.py:126-160, SURVEY.md §8f
// row 2): 8-point RANSAC over a pair's correspondences, max_iterations samples drawn by
// numpy's legacy RandomState after np.random.seed(5), the first sample with the most
// inliers (epipolar distance < threshold) wins.
//
// * Samples: `np.random.choice(n, 8, replace=False)` is permutation(n)[:8] — a full
//   Fisher-Yates shuffle of arange(n) whose j = random_interval(i) draws are MT19937
//   outputs masked to the next power of two, rejected above i (numpy legacy
//   _shuffle_raw / random_interval).  The stream depends only on (seed, n, iterations),
//   is inherently sequential, and is replayed on the host (ransac_sample_indices,
//   pinned bit-exactly against numpy by tests/test_ransac_cpu.py), cached per n.
// * Fundamental matrix per sample (CameraPose._compute_fundamental_matrix, SFM.py:
//   190-236), one thread per (pair, sample), float64: Hartley normalisation (mean,
//   mean distance, sqrt(2) scale), the 8 x 9 system's null vector by Gaussian
//   elimination with partial pivoting (the reference takes SVD's last right singular
//   vector: the same line, up to scale and sign, for a rank-8 system), rank 2 by
//   removing the smallest singular direction (F - (F v3) v3^T, v3 from a Jacobi
//   eigen-decomposition of F^T F: equal to U diag(d1, d2, 0) V^T), un-normalised.
//   Distances are invariant to F's scale and sign.
// * Inlier counts (SFM.py:147-156): one thread per sample, the pair's points staged in LDS
//   and read as broadcasts, d = |lb . p2| / sqrt(lb0^2 + lb1^2) with lb = F p1 in
//   float64, d < threshold (decided without the division away from the threshold).
// * Selection: the first sample with the largest count (strict > updates, SFM.py:156),
//   its mask recomputed and the inliers compacted in input order.
// Bar: on rank-8 samples every epipolar distance is within 1e-6 px of
// the reference's definition (measured 2.4e-7 px on a 4K frame, 1.4e-8 px at 960 x 540), so
// only a point that close to the threshold can change sides; the inlier sets equal the
// reference's on the golden pairs.  Degenerate motion (translations, identical frames,
// planes: numerical rank 6) leaves the choice inside the null space to rounding, in the
// reference too; there only what every null-space member guarantees is held.
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <vector>

#include "kernels.h"
#include "ransac_dev.h"

namespace sfm {

// ---------------- host: numpy legacy RandomState replay ----------------
namespace {
struct MT19937 {
  uint32_t mt[624];
  int pos = 624;
  explicit MT19937(uint32_t seed) {  // init_genrand (numpy legacy seeding of an int)
    mt[0] = seed;
    for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
  }
  void twist() {
    for (int i = 0; i < 624; ++i) {
      const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
      mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    pos = 0;
  }
  uint32_t next() {
    if (pos >= 624) twist();
    uint32_t y = mt[pos++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
};

// The tempered output stream of one seed, generated once per process in fixed chunks
// that never move: every pair restarts from np.random.seed(5) (SFM.py:133), so all
// pairs read the same raw words and differ only in how their n consumes them.
class RawStream {
 public:
  static constexpr size_t kChunk = size_t(1) << 20;
  explicit RawStream(uint32_t seed) : g_(seed) {}
  const uint32_t* chunk(size_t k) {
    std::lock_guard<std::mutex> lock(mu_);
    while (chunks_.size() <= k) {
      std::unique_ptr<uint32_t[]> c(new uint32_t[kChunk]);
      for (size_t i = 0; i < kChunk; ++i) c[i] = g_.next();
      chunks_.push_back(std::move(c));
    }
    return chunks_[k].get();
  }

 private:
  std::mutex mu_;
  MT19937 g_;
  std::vector<std::unique_ptr<uint32_t[]>> chunks_;
};

RawStream& raw_stream(uint32_t seed) {
  static std::mutex mu;
  static std::vector<std::pair<uint32_t, std::unique_ptr<RawStream>>> streams;
  std::lock_guard<std::mutex> lock(mu);
  for (auto& s : streams)
    if (s.first == seed) return *s.second;
  streams.emplace_back(seed, std::unique_ptr<RawStream>(new RawStream(seed)));
  return *streams.back().second;
}

struct Cursor {
  RawStream& s;
  size_t k = 0, i = 0;
  const uint32_t* c;
  explicit Cursor(RawStream& st) : s(st), c(st.chunk(0)) {}
  uint32_t next() {
    if (i == RawStream::kChunk) {
      c = s.chunk(++k);
      i = 0;
    }
    return c[i++];
  }
};
}  // namespace

void ransac_sample_indices(int n, int iters, uint32_t seed, int32_t* out) {
  ransac_sample_indices_k(n, iters, seed, 8, out);
}

// the same stream with `size` (<= n) indices kept per iteration: np.random.choice(n, size,
// replace=False) is permutation(n)[:size], a full shuffle whatever the size
void ransac_sample_indices_k(int n, int iters, uint32_t seed, int size, int32_t* out) {
  Cursor g(raw_stream(seed));
  std::vector<int32_t> a(std::max(n, 1));
  uint32_t top = 0;  // random_interval's mask for i = n - 1: the smallest 2^b - 1 >= i
  if (n > 1) {
    top = (uint32_t)(n - 1);
    top |= top >> 1;
    top |= top >> 2;
    top |= top >> 4;
    top |= top >> 8;
    top |= top >> 16;
  }
  for (int it = 0; it < iters; ++it) {
    for (int i = 0; i < n; ++i) a[i] = i;
    uint32_t mask = top;
    for (int i = n - 1; i >= 1; --i) {  // _shuffle_raw: j = random_interval(i)
      if ((uint32_t)i <= (mask >> 1)) mask >>= 1;  // i drops by one: one halving keeps it minimal
      uint32_t v;
      while ((v = (g.next() & mask)) > (uint32_t)i) {
      }
      const int32_t t = a[i];
      a[i] = a[v];
      a[v] = t;
    }
    for (int k = 0; k < size; ++k) out[(size_t)it * size + k] = a[k];
  }
}

// ---------------- device ----------------
struct Mat3 {
  double m[9];
};

// one thread per (pair, sample): F as 9 doubles (ransac_fit_F, ransac_dev.h, which also holds
// the inlier test epi_inlier: one copy, shared with verify.hip)
__global__ void __launch_bounds__(128) k_ransac_F(const int32_t* __restrict__ pts, const int32_t* __restrict__ npts,
                                                  int nmax, const int32_t* __restrict__ idx,
                                                  const int32_t* __restrict__ idx_off, int iters,
                                                  double* __restrict__ Fout) {
  const int it = blockIdx.x * 128 + threadIdx.x;
  const int p = blockIdx.y;
  if (it >= iters) return;
  double* F = Fout + ((int64_t)p * iters + it) * 9;
  const int n = npts[p];
  if (n < 8) return;
  const int32_t* id = idx + (int64_t)idx_off[p] + (int64_t)it * 8;
  const int32_t* P = pts + (int64_t)p * nmax * 4;
  double x1[8], y1[8], x2[8], y2[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int j = id[k];
    x1[k] = (double)P[4 * j + 0];
    y1[k] = (double)P[4 * j + 1];
    x2[k] = (double)P[4 * j + 2];
    y2[k] = (double)P[4 * j + 3];
  }
  double Fr[9];
  ransac_fit_F(x1, y1, x2, y2, Fr);
#pragma unroll
  for (int k = 0; k < 9; ++k) F[k] = Fr[k];
}

// inlier count per (pair, sample): one thread per sample, its F in registers for the whole
// sweep; the pair's points are staged in LDS as float64 (x1, y1, x2, y2) in chunks of
// kRansacChunk points and every lane reads the same point (a broadcast) — no per-sample
// reduction, F reload or conversion.  Any n: larger sets take several chunks.
__global__ void __launch_bounds__(256) k_ransac_count(const int32_t* __restrict__ pts,
                                                      const int32_t* __restrict__ npts, int nmax,
                                                      const double* __restrict__ Fs, int iters, double thr,
                                                      int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) double s_pd[];  // [chunk][4]
  const int p = blockIdx.y;
  const int n = npts[p];
  const int4* P = reinterpret_cast<const int4*>(pts + (int64_t)p * nmax * 4);
  const int it = blockIdx.x * 256 + threadIdx.x;
  const bool live = it < iters;
  double f[9];
  if (live) {
    const double* F = Fs + ((int64_t)p * iters + it) * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = F[k];
  }
  const EpiThr t = epi_thr(thr);
  uint32_t c = 0;
  for (int i0 = 0; i0 < n; i0 += kRansacChunk) {
    const int m = min(kRansacChunk, n - i0);
    if (i0) __syncthreads();  // every lane is done with the previous chunk
    for (int i = threadIdx.x; i < m; i += 256) {
      const int4 q = P[i0 + i];
      s_pd[4 * i + 0] = (double)q.x;
      s_pd[4 * i + 1] = (double)q.y;
      s_pd[4 * i + 2] = (double)q.z;
      s_pd[4 * i + 3] = (double)q.w;
    }
    __syncthreads();
    if (live)
      for (int i = 0; i < m; ++i) {
        const double4 q = reinterpret_cast<const double4*>(s_pd)[i];
        c += epi_inlier(f, q.x, q.y, q.z, q.w, t.thr, t.lo, t.hi) ? 1u : 0u;
      }
  }
  if (live) counts[(int64_t)p * iters + it] = n < 8 ? 0 : (int32_t)c;
}

// per pair: the first sample with the most inliers, its inliers compacted in order
__global__ void __launch_bounds__(256) k_ransac_select(const int32_t* __restrict__ pts,
                                                       const int32_t* __restrict__ npts, int nmax,
                                                       const double* __restrict__ Fs,
                                                       const int32_t* __restrict__ counts, int iters, double thr,
                                                       int32_t* __restrict__ out_pts, int32_t* __restrict__ out_n,
                                                       int32_t* __restrict__ out_iter) {
  __shared__ int s_bc[256], s_bi[256];
  __shared__ uint32_t s_scan[8];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = npts[p];
  int bc = -1, bi = 0x7fffffff;
  for (int it = tid; it < iters; it += 256) {
    const int c = counts[(int64_t)p * iters + it];
    if (c > bc) { bc = c; bi = it; }  // ascending it per thread: first max kept
  }
  s_bc[tid] = bc;
  s_bi[tid] = bi;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) {
      const int oc = s_bc[tid + off], oi = s_bi[tid + off];
      if (oc > s_bc[tid] || (oc == s_bc[tid] && oi < s_bi[tid])) { s_bc[tid] = oc; s_bi[tid] = oi; }
    }
    __syncthreads();
  }
  const int best = s_bi[0];
  if (n < 8 || s_bc[0] <= 0) {  // (< 8 points: the reference returns None; 0 inliers: empty)
    if (tid == 0) { out_n[p] = n < 8 ? -1 : 0; out_iter[p] = -1; }
    return;
  }
  const double* F = Fs + ((int64_t)p * iters + best) * 9;
  const int4* P = reinterpret_cast<const int4*>(pts + (int64_t)p * nmax * 4);
  int4* O = reinterpret_cast<int4*>(out_pts + (int64_t)p * nmax * 4);
  const EpiThr t = epi_thr(thr);  // the same test as k_ransac_count, so the mask has the count
  uint32_t base = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    bool in = false;
    int4 q = make_int4(0, 0, 0, 0);
    if (i < n) {
      q = P[i];
      in = epi_inlier(F, (double)q.x, (double)q.y, (double)q.z, (double)q.w, t.thr, t.lo, t.hi);
    }
    uint32_t total;
    const uint32_t pos = block_exclusive_scan(in ? 1u : 0u, s_scan, &total);
    if (in) O[base + pos] = q;
    base += total;
  }
  if (tid == 0) { out_n[p] = (int32_t)base; out_iter[p] = best; }
}

void launch_ransac(const int32_t* pts, const int32_t* npts, int nmax, int P, const int32_t* idx,
                   const int32_t* idx_off, int iters, double thr, double* Fs, int32_t* counts, int32_t* out_pts,
                   int32_t* out_n, int32_t* out_iter, hipStream_t st) {
  if (iters > 0) {
    hipLaunchKernelGGL(k_ransac_F, dim3((iters + 127) / 128, P), dim3(128), 0, st, pts, npts, nmax, idx, idx_off,
                       iters, Fs);
    static const bool lds_attr = [] {  // up to kRansacChunk x 32 B of staged points
      return hipFuncSetAttribute((const void*)k_ransac_count, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 kRansacChunk * 32) == hipSuccess;
    }();
    (void)lds_attr;
    hipLaunchKernelGGL(k_ransac_count, dim3((iters + 255) / 256, P), dim3(256),
                       (size_t)std::min(nmax, kRansacChunk) * 32, st, pts, npts, nmax, Fs, iters, thr, counts);
  }
  // always: with iters == 0 no sample exists and every pair gets the reference's empty
  // result (n >= 8) or None (n < 8), out_iter -1
  hipLaunchKernelGGL(k_ransac_select, dim3(P), dim3(256), 0, st, pts, npts, nmax, Fs, counts, iters, thr, out_pts,
                     out_n, out_iter);
}

// CameraPose.ransac_camera_motion (SFM.py:38-103): the same F and count launches, then the
// pose candidates and their cheirality check (pose.hip), which zeroes the count of every
// sample without a valid pose, then the same selection and the winner's (R, t).
void launch_ransac_pose(const int32_t* pts, const int32_t* npts, int nmax, int P, const int32_t* idx,
                        const int32_t* idx_off, int iters, double thr, const double* Kc, const double* base,
                        double* Fs, int32_t* counts, double* cand, int32_t* cand_idx, int32_t* out_pts,
                        int32_t* out_n, int32_t* out_iter, double* out_Rt, hipStream_t st) {
  if (iters > 0) {
    hipLaunchKernelGGL(k_ransac_F, dim3((iters + 127) / 128, P), dim3(128), 0, st, pts, npts, nmax, idx, idx_off,
                       iters, Fs);
    static const bool lds_attr = [] {
      return hipFuncSetAttribute((const void*)k_ransac_count, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 kRansacChunk * 32) == hipSuccess;
    }();
    (void)lds_attr;
    hipLaunchKernelGGL(k_ransac_count, dim3((iters + 255) / 256, P), dim3(256),
                       (size_t)std::min(nmax, kRansacChunk) * 32, st, pts, npts, nmax, Fs, iters, thr, counts);
    launch_pose_candidates(Fs, npts, Kc, P, iters, cand, st);
    launch_pose_cheirality(pts, npts, nmax, P, Kc, base, cand, iters, counts, cand_idx, st);
  }
  hipLaunchKernelGGL(k_ransac_select, dim3(P), dim3(256), 0, st, pts, npts, nmax, Fs, counts, iters, thr, out_pts,
                     out_n, out_iter);
  if (iters > 0) launch_pose_gather(out_iter, cand, cand_idx, P, iters, out_Rt, st);
}

}  // namespace sfm
