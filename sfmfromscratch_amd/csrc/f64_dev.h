// f64_dev.h — the float64 device helpers the geometry kernels (pose, refine, registry, pnp, ba)
// share: guards and fixed-order sums.  Kernels that call the same helper produce the same bits
// (-ffp-contract=off; no atomics).  Not for common.h / kernels.h: the hot-path translation
// units do not see this file.
#pragma once

#include <math.h>

#include "common.h"

namespace sfm {

SFM_DEV bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }  // false for NaN

// v into [0, n) for n >= 1: the table indices a caller passes in are its contract, never an address
SFM_DEV int clamp_index(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// the sum over the wave's 64 lanes by an xor butterfly, offsets 32 .. 1: every lane ends with the
// same bits (a + b == b + a at every level)
SFM_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// the sum over a workgroup of exactly blockDim.x == 256 threads by a halving tree in LDS
// (s_red [256]; thread t adds s_red[t + off] for off = 128 .. 1): every thread gets the sum.
// The barrier in front lets calls follow each other on one s_red.  Every thread must call it.
// (pnp.hip's block_sum256_waves sums in another order: the two do not agree in the last bit.)
SFM_DEV double block_sum256_tree(double v, double* s_red) {
  const int tid = threadIdx.x;
  __syncthreads();  // the previous sum has been read
  s_red[tid] = v;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) s_red[tid] += s_red[tid + off];
    __syncthreads();
  }
  return s_red[0];
}

}  // namespace sfm
