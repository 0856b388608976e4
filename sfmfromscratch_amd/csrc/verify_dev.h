// verify_dev.h — the device functions shared by the per-pair RANSAC kernels over a slot table's
// matches: the fused verification kernel (verify.hip) and the homography kernel (twoview.hip).
// The counter-based sampler, the gather of a correspondence through matches -> xy and the
// staging of a pair's correspondences into LDS: one copy, so both kernels draw from the same
// stream construction and agree on which match is valid.
#pragma once
#include <stdint.h>

#include "kernels.h"

namespace sfm {

constexpr int kVerifyThreads = kVerifyRound;  // one thread per sample of a round

SFM_DEV uint64_t mix64(uint64_t z) {  // the splitmix64 finaliser
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// the stream key of pair (a, b): a function of the seed and the two slots only
SFM_DEV uint64_t pair_key(uint64_t seed, int a, int b) {
  return mix64(mix64(seed) + (((uint64_t)(uint32_t)a << 32) | (uint64_t)(uint32_t)b));
}

// The S indices of sample `it`: a Fisher-Yates over a virtual arange(n) of which only the
// swapped positions are recorded (draw k writes position j_k; position k is never read again).
// Every index is compile-time, so the records stay in registers.
template <int S>
SFM_DEV void sample_indices(uint64_t key, int it, int n, int (&idx)[S]) {
  int pos[S], val[S];
#pragma unroll
  for (int k = 0; k < S; ++k) {
    const uint64_t r = mix64(key + (uint64_t)(S * (int64_t)it + k + 1) * 0x9E3779B97F4A7C15ull) >> 32;
    const int j = k + (int)((r * (uint64_t)(n - k)) >> 32);
    int vj = j, vk = k;  // the values now at positions j and k: the latest record of each
#pragma unroll
    for (int i = 0; i < k; ++i) {
      vj = pos[i] == j ? val[i] : vj;
      vk = pos[i] == k ? val[i] : vk;
    }
    idx[k] = vj;
    pos[k] = j;
    val[k] = vk;
  }
}

struct Corr {
  double x1, y1, x2, y2;
};

// correspondence m of the pair: NaN when a row lies outside [0, count) of its slot
SFM_DEV Corr load_corr(const int2* __restrict__ mt, const int2* __restrict__ xa, const int2* __restrict__ xb, int ca,
                       int cb, int m) {
  const int2 rr = mt[m];
  if (rr.x < 0 || rr.x >= ca || rr.y < 0 || rr.y >= cb) {
    const double q = __builtin_nan("");
    return {q, q, q, q};
  }
  const int2 u = xa[rr.x], v = xb[rr.y];
  return {(double)u.x, (double)u.y, (double)v.x, (double)v.y};
}

SFM_DEV void stage(double* s_pd, const int2* mt, const int2* xa, const int2* xb, int ca, int cb, int i0, int m) {
  for (int i = threadIdx.x; i < m; i += kVerifyThreads) {
    const Corr q = load_corr(mt, xa, xb, ca, cb, i0 + i);
    s_pd[4 * i + 0] = q.x1;
    s_pd[4 * i + 1] = q.y1;
    s_pd[4 * i + 2] = q.x2;
    s_pd[4 * i + 3] = q.y2;
  }
}

}  // namespace sfm
