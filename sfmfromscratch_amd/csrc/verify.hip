// verify.hip — two-view geometric verification of a slot table's matches, the step between
// sfm_match_pairs_dev and sfm_build_tracks_dev (include/sfmfeat.h sfm_verify_matches_dev has the
// rule in full).  One fused kernel, one 256-thread workgroup per pair:
//
// * the pair's correspondences are gathered once through matches -> xy into LDS as float64
//   (x1, y1, x2, y2), an invalid match as NaN (epi_inlier's NaN rule rejects it); a pair of more
//   than kRansacChunk matches restages its chunks every round;
// * per round of 256 samples, thread t draws the eight indices of sample 256 (r - 1) + t from a
//   counter-based integer stream (no state, no host replay), fits its F in registers
//   (ransac_fit_F, the arithmetic of k_ransac_F) and sweeps the staged points as LDS broadcasts
//   (epi_inlier, as k_ransac_count);
// * a block reduction keeps (largest count, lowest sample); the thread that owns a new best
//   leaves its F in LDS (72 bytes), so no sample's F goes to memory and none is fitted twice.
//   This departs on purpose from the wording the call was specified with ("the winner's F is
//   recomputed from its sample index after the last round"): the stored F is the one that
//   produced the count, bit for bit what a second fit of the same sample would give, and it saves
//   one fit per pair.  The owner's store is followed by a __syncthreads before any read, and
//   only a strictly larger count replaces it;
// * the stop test after each round is uniform across the block; afterwards the block writes the
//   pair's keep row (the same test with the same F, so it holds exactly `count` ones), F, stat.
//
// Pairs that are not attempted (n < 8: most of an all-pairs schedule) leave after writing zeros.
// Nothing is allocated, nothing synchronises, no host memory is read by the device: the stop
// table travels in the kernel arguments.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "ransac_dev.h"
#include "verify_dev.h"  // mix64, pair_key, sample_indices, load_corr, stage

namespace sfm {

namespace {

constexpr int kVerifySweep = 4;  // points in flight per thread in the sweep

// The inliers of f among m staged points.  Two waves per SIMD hide little latency, so four points
// go through the test together: their LDS reads first, then their terms, then their decisions.
SFM_DEV uint32_t sweep(const double* s_pd, const double (&f)[9], int m, const EpiThr& t) {
  const double4* pd = reinterpret_cast<const double4*>(s_pd);
  uint32_t c = 0;
  int i = 0;
  for (; i + kVerifySweep <= m; i += kVerifySweep) {
    double4 q[kVerifySweep];
    EpiTerms e[kVerifySweep];
#pragma unroll
    for (int u = 0; u < kVerifySweep; ++u) q[u] = pd[i + u];
#pragma unroll
    for (int u = 0; u < kVerifySweep; ++u) e[u] = epi_terms(f, q[u].x, q[u].y, q[u].z, q[u].w);
#pragma unroll
    for (int u = 0; u < kVerifySweep; ++u) c += epi_decide(e[u], t.thr, t.lo, t.hi) ? 1u : 0u;
  }
  for (; i < m; ++i) {
    const double4 q = pd[i];
    c += epi_inlier(f, q.x, q.y, q.z, q.w, t.thr, t.lo, t.hi) ? 1u : 0u;
  }
  return c;
}

}  // namespace

// Two waves per SIMD (256 registers each; the fit then spills 106 of its registers to scratch):
// measured 181 ms against 325 ms at one wave per SIMD on the 32,640-pair job.
// Two workgroups share a CU while the staged points leave room: cap <= 2,556.
__global__ void __launch_bounds__(kVerifyThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_verify(const int32_t* __restrict__ xy, const int32_t* __restrict__ count, int nimg, int64_t cap,
         const int32_t* __restrict__ pairs, const int32_t* __restrict__ matches, const int32_t* __restrict__ nmatch,
         int iters, double thr, int min_inliers, uint64_t seed, VerifyStop stop, uint8_t* __restrict__ keep,
         double* __restrict__ Fout, int32_t* __restrict__ stat) {
  extern __shared__ __attribute__((aligned(16))) double s_pd[];  // [min(cap, kRansacChunk)][4]
  __shared__ int s_wc[kVerifyThreads / 64], s_wi[kVerifyThreads / 64];
  __shared__ double s_F[9];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int a = pairs[2 * (int64_t)p], b = pairs[2 * (int64_t)p + 1];
  const int64_t nm = nmatch[p];
  const int n = (int)(nm < 0 ? 0 : (nm > cap ? cap : nm));
  uint8_t* K = keep + (int64_t)p * cap;
  double* Fp = Fout + (int64_t)p * 9;
  int32_t* St = stat + (int64_t)p * 4;
  const double qnan = __builtin_nan("");
  const bool attempted = a >= 0 && a < nimg && b >= 0 && b < nimg && a != b && n >= 8;
  if (!attempted || iters == 0) {
    for (int64_t m = tid; m < cap; m += kVerifyThreads) K[m] = 0;
    if (tid < 9) Fp[tid] = qnan;
    if (tid < 4) St[tid] = attempted ? (tid == 1 ? -1 : 0) : (tid < 2 ? -1 : 0);
    return;
  }
  const int64_t cca = count[a], ccb = count[b];
  const int ca = (int)(cca < 0 ? 0 : (cca > cap ? cap : cca)), cb = (int)(ccb < 0 ? 0 : (ccb > cap ? cap : ccb));
  const int2* mt = reinterpret_cast<const int2*>(matches) + (int64_t)p * cap;
  const int2* xa = reinterpret_cast<const int2*>(xy) + (int64_t)a * cap;
  const int2* xb = reinterpret_cast<const int2*>(xy) + (int64_t)b * cap;
  const uint64_t key = pair_key(seed, a, b);
  const EpiThr t = epi_thr(thr);
  const bool multi = n > kRansacChunk;
  if (!multi) {
    stage(s_pd, mt, xa, xb, ca, cb, 0, n);
    __syncthreads();
  }
  const int rounds = (iters + kVerifyRound - 1) / kVerifyRound;
  int best_c = -1, best_it = -1, done = 0;  // uniform across the block
  for (int r = 1; r <= rounds; ++r) {
    const int it = kVerifyRound * (r - 1) + tid;
    const bool in_round = it < iters;
    bool live = in_round;
    double f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = qnan;
    if (in_round) {
      int idx[8];
      sample_indices<8>(key, it, n, idx);
      double x1[8], y1[8], x2[8], y2[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        Corr q;
        if (multi) {
          q = load_corr(mt, xa, xb, ca, cb, idx[k]);
        } else {
          const double4 d = reinterpret_cast<const double4*>(s_pd)[idx[k]];
          q = {d.x, d.y, d.z, d.w};
        }
        x1[k] = q.x1;
        y1[k] = q.y1;
        x2[k] = q.x2;
        y2[k] = q.y2;
        live = live && q.x1 == q.x1;  // a sample with an invalid match counts 0
      }
      if (live) ransac_fit_F(x1, y1, x2, y2, f);
    }
    uint32_t c = 0;
    if (!multi) {
      if (live) c = sweep(s_pd, f, n, t);
    } else {
      for (int i0 = 0; i0 < n; i0 += kRansacChunk) {
        const int m = min(kRansacChunk, n - i0);
        __syncthreads();  // every lane is done with the previous chunk
        stage(s_pd, mt, xa, xb, ca, cb, i0, m);
        __syncthreads();
        if (live) c += sweep(s_pd, f, m, t);
      }
    }
    // (largest count, lowest sample) of the round: within the wave, then over the four waves
    int rc = in_round ? (int)c : -1, ri = in_round ? it : 0x7fffffff;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int oc = __shfl_xor(rc, off, 64), oi = __shfl_xor(ri, off, 64);
      if (oc > rc || (oc == rc && oi < ri)) { rc = oc; ri = oi; }
    }
    if ((tid & 63) == 0) { s_wc[tid >> 6] = rc; s_wi[tid >> 6] = ri; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kVerifyThreads / 64; ++w) {
      const int oc = s_wc[w], oi = s_wi[w];
      if (oc > rc || (oc == rc && oi < ri)) { rc = oc; ri = oi; }
    }
    if (rc > best_c) {  // earlier rounds hold the lower samples: only a larger count replaces
      best_c = rc;
      best_it = ri;
      if (it == ri) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_F[k] = f[k];
      }
    }
    __syncthreads();  // s_wc / s_wi are free for the next round; s_F is visible
    done = r;
    if (r <= stop.n && (double)best_c >= stop.ratio[r - 1] * (double)n) break;
  }
  const int samples = min(iters, kVerifyRound * done);
  const bool verified = best_c > 0 && best_c >= min_inliers;
  double f[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) f[k] = best_c > 0 ? s_F[k] : qnan;
  for (int64_t m = tid; m < cap; m += kVerifyThreads) {
    bool in = false;
    if (verified && m < n) {
      const Corr q = load_corr(mt, xa, xb, ca, cb, (int)m);
      in = epi_inlier(f, q.x1, q.y1, q.x2, q.y2, t.thr, t.lo, t.hi);
    }
    K[m] = in ? 1 : 0;
  }
  if (tid < 9) Fp[tid] = best_c > 0 ? s_F[tid] : qnan;  // the winner's, verified or not
  if (tid == 0) {
    St[0] = best_c;
    St[1] = best_it;
    St[2] = samples;
    St[3] = verified ? 1 : 0;
  }
}

void launch_verify(const int32_t* xy, const int32_t* count, int nimg, int64_t cap, const int32_t* pairs, int P,
                   const int32_t* matches, const int32_t* nmatch, int iters, double thr, int min_inliers,
                   uint64_t seed, const VerifyStop& stop, uint8_t* keep, double* F, int32_t* stat, hipStream_t st) {
  if (P <= 0) return;
  static const bool lds_attr = [] {  // up to kRansacChunk x 32 B of staged points
    return hipFuncSetAttribute((const void*)k_verify, hipFuncAttributeMaxDynamicSharedMemorySize,
                               kRansacChunk * 32) == hipSuccess;
  }();
  (void)lds_attr;
  const size_t lds = (size_t)std::min<int64_t>(cap, kRansacChunk) * 32;
  hipLaunchKernelGGL(k_verify, dim3(P), dim3(kVerifyThreads), lds, st, xy, count, nimg, cap, pairs, matches, nmatch,
                     iters, thr, min_inliers, seed, stop, keep, F, stat);
}

}  // namespace sfm
