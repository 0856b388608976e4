// twoview.hip — the two-view geometry record of a verified pair, the step between
// sfm_verify_matches_dev and the choice of an initial pair (include/sfmfeat.h has both rules in
// full).
//
// k_homography: a homography RANSAC per pair, of the same build as k_verify (verify.hip).  One
// 256-thread workgroup per pair:
// * the pair's correspondences are gathered once into LDS as float64, an invalid match as NaN;
//   a pair of more than kRansacChunk matches restages its chunks every round;
// * per round of 256 samples, thread t draws the four indices of sample 256 (r - 1) + t from the
//   counter stream of verify_dev.h under the pair's H key, fits its H in registers (Hartley over
//   four points, the 8 x 9 DLT system, the null vector by ransac_dev.h's elimination) and sweeps
//   the staged points as LDS broadcasts.  The inlier test has no division and no square root: the
//   symmetric transfer error decided on the homogeneous quantities, forward with H, backward
//   with adj(H);
// * the block reduction, the owner's store of the winning H into LDS and the uniform stop test
//   are k_verify's.
//
// k_two_view_pose: no RANSAC.  One 256-thread workgroup per pair: thread 0 decomposes
// E = K2^T F K1 into the four candidates (pose_dev.h, the arithmetic of k_pose_candidates) and
// leaves them in LDS; every thread then triangulates the kept matches m = tid, tid + 256, ..
// under each candidate (triangulate_dlt) and counts, per candidate, the points in front of both
// cameras and those of them with enough parallax; the counts are integers, so their reduction
// has no order.  A pair that is not attempted leaves after writing NaN.
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "pose_dev.h"
#include "ransac_dev.h"
#include "verify_dev.h"

namespace sfm {

namespace {

constexpr int kHomographySweep = 4;  // points in flight per thread in the sweep
constexpr int kTwoViewThreads = 256;

// H (9 doubles, row-major) of four correspondences.  No degeneracy test: a collinear sample gives
// an H that maps few points and scores low; four coincident points of one image give NaN.
SFM_DEV void ransac_fit_H(const double (&x1)[4], const double (&y1)[4], const double (&x2)[4],
                          const double (&y2)[4], double (&H)[9]) {
  double a1[4], b1[4], a2[4], b2[4], s1, c1x, c1y, s2, c2x, c2y;
  normalise_sample<4>(x1, y1, a1, b1, s1, c1x, c1y);
  normalise_sample<4>(x2, y2, a2, b2, s2, c2x, c2y);
  double A[8][9];
  auto build = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double u1 = a1[i], v1 = b1[i], u2 = a2[i], v2 = b2[i];
      double* r0 = A[2 * i];
      double* r1 = A[2 * i + 1];
      r0[0] = -u1; r0[1] = -v1; r0[2] = -1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0;
      r0[6] = u2 * u1; r0[7] = u2 * v1; r0[8] = u2;
      r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = -u1; r1[4] = -v1; r1[5] = -1.0;
      r1[6] = v2 * u1; r1[7] = v2 * v1; r1[8] = v2;
    }
  };
  build();
  double h[9];
  if (!null_vector_8x9_regs(A, h)) {  // a zero pivot: the general elimination (free columns) on a fresh system
    build();
    null_vector_8x9(A, h);
  }
  // un-normalise: T2^-1 Hn T1, T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]], written out
  const double t1x = -s1 * c1x, t1y = -s1 * c1y, i2 = 1.0 / s2;
  double M[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    M[3 * r + 0] = h[3 * r + 0] * s1;
    M[3 * r + 1] = h[3 * r + 1] * s1;
    M[3 * r + 2] = (h[3 * r + 0] * t1x + h[3 * r + 1] * t1y) + h[3 * r + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    H[c] = M[c] * i2 + c2x * M[6 + c];
    H[3 + c] = M[3 + c] * i2 + c2y * M[6 + c];
    H[6 + c] = M[6 + c];
  }
}

// adj(H), the transposed cofactors: H adj(H) = det(H) I
SFM_DEV void adjugate3(const double (&H)[9], double (&G)[9]) {
  G[0] = H[4] * H[8] - H[5] * H[7];
  G[1] = H[2] * H[7] - H[1] * H[8];
  G[2] = H[1] * H[5] - H[2] * H[4];
  G[3] = H[5] * H[6] - H[3] * H[8];
  G[4] = H[0] * H[8] - H[2] * H[6];
  G[5] = H[2] * H[3] - H[0] * H[5];
  G[6] = H[3] * H[7] - H[4] * H[6];
  G[7] = H[1] * H[6] - H[0] * H[7];
  G[8] = H[0] * H[4] - H[1] * H[3];
}

// (u, v, w) = M (x, y, 1); ok iff (x' w - u)^2 + (y' w - v)^2 < thr2 w^2.  NaN anywhere and w == 0
// compare false; thr2 is -1 for a threshold that is <= 0 or NaN, inf w^2 is NaN at w == 0.
SFM_DEV bool transfer_ok(const double (&M)[9], double x, double y, double xp, double yp, double thr2) {
  const double u = (M[0] * x + M[1] * y) + M[2];
  const double v = (M[3] * x + M[4] * y) + M[5];
  const double w = (M[6] * x + M[7] * y) + M[8];
  const double du = xp * w - u, dv = yp * w - v;
  return du * du + dv * dv < thr2 * (w * w);
}

SFM_DEV bool homography_inlier(const double (&H)[9], const double (&G)[9], double x1, double y1, double x2, double y2,
                               double thr2) {
  const bool fwd = transfer_ok(H, x1, y1, x2, y2, thr2);
  const bool bwd = transfer_ok(G, x2, y2, x1, y1, thr2);
  return fwd && bwd;
}

// The inliers of (H, G) among m staged points, kHomographySweep points in flight: their LDS reads
// first, then their tests (two waves per SIMD hide little latency, as in k_verify's sweep).
SFM_DEV uint32_t sweep_H(const double* s_pd, const double (&H)[9], const double (&G)[9], int m, double thr2) {
  const double4* pd = reinterpret_cast<const double4*>(s_pd);
  uint32_t c = 0;
  int i = 0;
  for (; i + kHomographySweep <= m; i += kHomographySweep) {
    double4 q[kHomographySweep];
#pragma unroll
    for (int u = 0; u < kHomographySweep; ++u) q[u] = pd[i + u];
#pragma unroll
    for (int u = 0; u < kHomographySweep; ++u)
      c += homography_inlier(H, G, q[u].x, q[u].y, q[u].z, q[u].w, thr2) ? 1u : 0u;
  }
  for (; i < m; ++i) {
    const double4 q = pd[i];
    c += homography_inlier(H, G, q.x, q.y, q.z, q.w, thr2) ? 1u : 0u;
  }
  return c;
}

}  // namespace

// Two waves per SIMD, as k_verify: the fit holds the same 8 x 9 system (DESIGN.md §13I has the
// register figures).  Two workgroups share a CU while the staged points leave room.
__global__ void __launch_bounds__(kVerifyThreads) __attribute__((amdgpu_waves_per_eu(2, 2)))
k_homography(const int32_t* __restrict__ xy, const int32_t* __restrict__ count, int nimg, int64_t cap,
             const int32_t* __restrict__ pairs, const int32_t* __restrict__ matches,
             const int32_t* __restrict__ nmatch, const int32_t* __restrict__ attempt, int iters, double thr,
             uint64_t seed, VerifyStop stop, double* __restrict__ Hout, uint8_t* __restrict__ hkeep,
             int32_t* __restrict__ hstat) {
  extern __shared__ __attribute__((aligned(16))) double s_pd[];  // [min(cap, kRansacChunk)][4]
  __shared__ int s_wc[kVerifyThreads / 64], s_wi[kVerifyThreads / 64];
  __shared__ double s_H[9];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int a = pairs[2 * (int64_t)p], b = pairs[2 * (int64_t)p + 1];
  const int64_t nm = nmatch[p];
  const int n = (int)(nm < 0 ? 0 : (nm > cap ? cap : nm));
  uint8_t* K = hkeep ? hkeep + (int64_t)p * cap : nullptr;
  double* Hp = Hout + (int64_t)p * 9;
  int32_t* St = hstat + (int64_t)p * 4;
  const double qnan = __builtin_nan("");
  const bool attempted =
      a >= 0 && a < nimg && b >= 0 && b < nimg && a != b && n >= 4 && (attempt == nullptr || attempt[p] != 0);
  if (!attempted || iters == 0) {
    if (K)
      for (int64_t m = tid; m < cap; m += kVerifyThreads) K[m] = 0;
    if (tid < 9) Hp[tid] = qnan;
    if (tid < 4) St[tid] = attempted ? (tid == 1 ? -1 : 0) : (tid < 2 ? -1 : 0);
    return;
  }
  const int64_t cca = count[a], ccb = count[b];
  const int ca = (int)(cca < 0 ? 0 : (cca > cap ? cap : cca)), cb = (int)(ccb < 0 ? 0 : (ccb > cap ? cap : ccb));
  const int2* mt = reinterpret_cast<const int2*>(matches) + (int64_t)p * cap;
  const int2* xa = reinterpret_cast<const int2*>(xy) + (int64_t)a * cap;
  const int2* xb = reinterpret_cast<const int2*>(xy) + (int64_t)b * cap;
  const uint64_t key = pair_key(seed ^ kHomographySeedXor, a, b);
  const double thr2 = thr > 0.0 ? thr * thr : -1.0;
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
    double h[9], g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = qnan;
    if (in_round) {
      int idx[4];
      sample_indices<4>(key, it, n, idx);
      double x1[4], y1[4], x2[4], y2[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
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
      if (live) ransac_fit_H(x1, y1, x2, y2, h);
    }
    adjugate3(h, g);
    uint32_t c = 0;
    if (!multi) {
      if (live) c = sweep_H(s_pd, h, g, n, thr2);
    } else {
      for (int i0 = 0; i0 < n; i0 += kRansacChunk) {
        const int m = min(kRansacChunk, n - i0);
        __syncthreads();  // every lane is done with the previous chunk
        stage(s_pd, mt, xa, xb, ca, cb, i0, m);
        __syncthreads();
        if (live) c += sweep_H(s_pd, h, g, m, thr2);
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
        for (int k = 0; k < 9; ++k) s_H[k] = h[k];
      }
    }
    __syncthreads();  // s_wc / s_wi are free for the next round; s_H is visible
    done = r;
    if (r <= stop.n && (double)best_c >= stop.ratio[r - 1] * (double)n) break;
  }
  const int samples = min(iters, kVerifyRound * done);
  if (K) {
    double h[9], g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = best_c > 0 ? s_H[k] : qnan;
    adjugate3(h, g);
    for (int64_t m = tid; m < cap; m += kVerifyThreads) {
      bool in = false;
      if (best_c > 0 && m < n) {
        const Corr q = load_corr(mt, xa, xb, ca, cb, (int)m);
        in = homography_inlier(h, g, q.x1, q.y1, q.x2, q.y2, thr2);
      }
      K[m] = in ? 1 : 0;
    }
  }
  if (tid < 9) Hp[tid] = best_c > 0 ? s_H[tid] : qnan;
  if (tid == 0) {
    St[0] = best_c;
    St[1] = best_it;
    St[2] = samples;
    St[3] = 0;
  }
}

// One workgroup per pair (see the top of the file).  s_cand: R1, R2, T of pose_candidates_dev.
__global__ void __launch_bounds__(kTwoViewThreads)
k_two_view_pose(const int32_t* __restrict__ xy, const int32_t* __restrict__ count, int nimg, int64_t cap,
                const int32_t* __restrict__ pairs, const int32_t* __restrict__ matches,
                const int32_t* __restrict__ nmatch, const uint8_t* __restrict__ keep, const double* __restrict__ Fin,
                const double* __restrict__ Kin, const int32_t* __restrict__ attempt, double cos2_min,
                double* __restrict__ pose, int32_t* __restrict__ pstat) {
  __shared__ double s_cand[21];
  __shared__ int s_cnt[9];  // front [4], wide [4], points
  const int p = blockIdx.x, tid = threadIdx.x;
  const int a = pairs[2 * (int64_t)p], b = pairs[2 * (int64_t)p + 1];
  double* Po = pose + (int64_t)p * 12;
  int32_t* St = pstat + (int64_t)p * 4;
  const double qnan = __builtin_nan("");
  const double* F = Fin + (int64_t)p * 9;
  bool attempted = a >= 0 && a < nimg && b >= 0 && b < nimg && a != b && (attempt == nullptr || attempt[p] != 0);
  if (attempted) {
#pragma unroll
    for (int k = 0; k < 9; ++k) attempted = attempted && fabs(F[k]) < __builtin_inf();  // NaN compares false
  }
  if (!attempted) {
    if (tid < 12) Po[tid] = qnan;
    if (tid < 4) St[tid] = tid < 2 ? -1 : 0;
    return;
  }
  const double* K1 = Kin + (int64_t)a * 9;
  const double* K2 = Kin + (int64_t)b * 9;
  if (tid == 0) pose_candidates_dev(F, K1, K2, s_cand);
  if (tid < 9) s_cnt[tid] = 0;
  __syncthreads();
  const int64_t nm = nmatch[p];
  const int n = (int)(nm < 0 ? 0 : (nm > cap ? cap : nm));
  const int64_t cca = count[a], ccb = count[b];
  const int ca = (int)(cca < 0 ? 0 : (cca > cap ? cap : cca)), cb = (int)(ccb < 0 ? 0 : (ccb > cap ? cap : ccb));
  const int2* mt = reinterpret_cast<const int2*>(matches) + (int64_t)p * cap;
  const int2* xa = reinterpret_cast<const int2*>(xy) + (int64_t)a * cap;
  const int2* xb = reinterpret_cast<const int2*>(xy) + (int64_t)b * cap;
  const uint8_t* kp = keep + (int64_t)p * cap;
  // P1 = K1 [I | 0]; K2 R and K2 T of both rotations, as k_pose_cheirality forms them
  double P1[12], K2R[2][9], K2T[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      P1[4 * r + c] = K1[3 * r + c];
      K2R[0][3 * r + c] = K2[3 * r] * s_cand[c] + K2[3 * r + 1] * s_cand[3 + c] + K2[3 * r + 2] * s_cand[6 + c];
      K2R[1][3 * r + c] = K2[3 * r] * s_cand[9 + c] + K2[3 * r + 1] * s_cand[12 + c] + K2[3 * r + 2] * s_cand[15 + c];
    }
    P1[4 * r + 3] = 0.0;
    K2T[r] = K2[3 * r] * s_cand[18] + K2[3 * r + 1] * s_cand[19] + K2[3 * r + 2] * s_cand[20];
  }
  int front[4] = {0, 0, 0, 0}, wide[4] = {0, 0, 0, 0}, points = 0;
  for (int m = tid; m < n; m += kTwoViewThreads) {
    if (kp[m] == 0) continue;
    const Corr q = load_corr(mt, xa, xb, ca, cb, m);
    if (!(q.x1 == q.x1)) continue;
    ++points;
#pragma unroll 1  // one copy of the triangulation: four would take every register of the SIMD
    for (int c = 0; c < 4; ++c) {
      const bool second = c >= 2;
      const double* R = s_cand + (second ? 9 : 0);
      const double sg = (c & 1) ? -1.0 : 1.0;
      const double t0 = sg * s_cand[18], t1 = sg * s_cand[19], t2 = sg * s_cand[20];
      double P2[12];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) P2[4 * r + k] = second ? K2R[1][3 * r + k] : K2R[0][3 * r + k];
        P2[4 * r + 3] = sg * K2T[r];
      }
      double X[3];
      triangulate_dlt(q.x1, q.y1, q.x2, q.y2, P1, P2, X);
      const double z2 = (R[6] * X[0] + R[7] * X[1] + R[8] * X[2]) + t2;
      if (!(X[2] >= 1e-6 && z2 >= 1e-6)) continue;  // NaN: not in front
#pragma unroll
      for (int k = 0; k < 4; ++k) front[k] += k == c ? 1 : 0;  // (no runtime index: the counters stay in registers)
      // parallax at X between the rays to the two centres, 0 and C = -R^T t
      const double C0 = -((R[0] * t0 + R[3] * t1) + R[6] * t2);
      const double C1 = -((R[1] * t0 + R[4] * t1) + R[7] * t2);
      const double C2 = -((R[2] * t0 + R[5] * t1) + R[8] * t2);
      const double e0 = X[0] - C0, e1 = X[1] - C1, e2 = X[2] - C2;
      const double d = (X[0] * e0 + X[1] * e1) + X[2] * e2;
      const double nx = (X[0] * X[0] + X[1] * X[1]) + X[2] * X[2];
      const double ne = (e0 * e0 + e1 * e1) + e2 * e2;
      const bool is_wide = d <= 0.0 || d * d < (cos2_min * nx) * ne;
#pragma unroll
      for (int k = 0; k < 4; ++k) wide[k] += (k == c && is_wide) ? 1 : 0;
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (front[c]) atomicAdd(&s_cnt[c], front[c]);
    if (wide[c]) atomicAdd(&s_cnt[4 + c], wide[c]);
  }
  if (points) atomicAdd(&s_cnt[8], points);
  __syncthreads();
  int win = -1, best = 0;  // the largest count, the lowest candidate on a tie; 0 wins nothing
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (s_cnt[c] > best) { best = s_cnt[c]; win = c; }
  if (tid < 12) {
    double v = qnan;
    if (win >= 0) v = tid < 9 ? s_cand[(win >= 2 ? 9 : 0) + tid] : ((win & 1) ? -1.0 : 1.0) * s_cand[18 + tid - 9];
    Po[tid] = v;
  }
  if (tid == 0) {
    St[0] = best;
    St[1] = win;
    St[2] = win >= 0 ? s_cnt[4 + win] : 0;
    St[3] = s_cnt[8];
  }
}

void launch_homography(const int32_t* xy, const int32_t* count, int nimg, int64_t cap, const int32_t* pairs, int P,
                       const int32_t* matches, const int32_t* nmatch, const int32_t* attempt, int iters, double thr,
                       uint64_t seed, const VerifyStop& stop, double* H, uint8_t* hkeep, int32_t* hstat,
                       hipStream_t st) {
  if (P <= 0) return;
  static const bool lds_attr = [] {  // up to kRansacChunk x 32 B of staged points
    return hipFuncSetAttribute((const void*)k_homography, hipFuncAttributeMaxDynamicSharedMemorySize,
                               kRansacChunk * 32) == hipSuccess;
  }();
  (void)lds_attr;
  const size_t lds = (size_t)std::min<int64_t>(cap, kRansacChunk) * 32;
  hipLaunchKernelGGL(k_homography, dim3(P), dim3(kVerifyThreads), lds, st, xy, count, nimg, cap, pairs, matches,
                     nmatch, attempt, iters, thr, seed, stop, H, hkeep, hstat);
}

void launch_two_view_pose(const int32_t* xy, const int32_t* count, int nimg, int64_t cap, const int32_t* pairs, int P,
                          const int32_t* matches, const int32_t* nmatch, const uint8_t* keep, const double* F,
                          const double* K, const int32_t* attempt, double cos2_min, double* pose, int32_t* pstat,
                          hipStream_t st) {
  if (P <= 0) return;
  hipLaunchKernelGGL(k_two_view_pose, dim3(P), dim3(kTwoViewThreads), 0, st, xy, count, nimg, cap, pairs, matches,
                     nmatch, keep, F, K, attempt, cos2_min, pose, pstat);
}

}  // namespace sfm
