// debug_geom.hip — sfm_debug_geom: a read-only probe of the float64 helpers the geometry kernels
// share (linalg3.h, linalg4.h, f64_dev.h).  Each op loads its row, calls the
// helper itself and stores what it returned, so a test can run a helper where no stage reaches
// (wide rotations, degenerate spectra, consecutive block sums).  Apart from debug.hip, which must
// not see f64_dev.h.  Not used by the pipeline.
#include "../../include/sfmfeat.h"
#include "common.h"
#include "f64_dev.h"
#include "linalg3.h"
#include "linalg4.h"

using namespace sfm;

namespace sfm {

constexpr int64_t kGeomMaxRows = 1 << 20;  // one workgroup per row at most: the grid stays small

// host tables: doubles per row in and out, indexed by op
constexpr int kGeomIn[SFM_GEOM_OPS] = {3, 9, 6, 16, 18, 12, 64, 512};
constexpr int kGeomOut[SFM_GEOM_OPS] = {9, 3, 12, 4, 9, 3, 64, 512};

// one thread per row
template <int OP>
__global__ void __launch_bounds__(64) k_geom_rows(const double* __restrict__ in, double* __restrict__ out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* a = in + i * kGeomIn[OP];
  double* o = out + i * kGeomOut[OP];
  if constexpr (OP == SFM_GEOM_RODRIGUES) {
    double R[9];
    rodrigues(a[0], a[1], a[2], R);
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = R[k];
  } else if constexpr (OP == SFM_GEOM_RODRIGUES_INV) {
    double R[9], r[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a[k];
    rodrigues_inv(R, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = r[k];
  } else if constexpr (OP == SFM_GEOM_EIG3) {
    double S[3][3] = {{a[0], a[1], a[2]}, {a[1], a[3], a[4]}, {a[2], a[4], a[5]}}, V[3][3];
    jacobi_eig3(S, V);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = S[k][k];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) o[3 + 3 * r + c] = V[r][c];
  } else if constexpr (OP == SFM_GEOM_NULL4) {
    double A[4][4], v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) A[r][c] = a[4 * r + c];
    null_vector_4x4(A, v);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = v[k];
  } else if constexpr (OP == SFM_GEOM_COMPOSE) {
    compose3(a, a + 9, o);  // rows of global tables, as k_ba_update passes them
  } else {
    static_assert(OP == SFM_GEOM_ROTATE, "one thread per row: ops 0 .. 5");
    double R[9], Y[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a[k];
    rotate3(R, a[9], a[10], a[11], Y);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = Y[k];
  }
}

// one wave of 64 lanes per row: each lane's own result
__global__ void __launch_bounds__(64) k_geom_wave_sum(const double* __restrict__ in, double* __restrict__ out) {
  const int64_t at = (int64_t)blockIdx.x * 64 + threadIdx.x;
  out[at] = wave_sum_f64(in[at]);
}

// one workgroup of 256 per row: two sums in a row on one s_red, what each thread got from each
__global__ void __launch_bounds__(256) k_geom_block_sum(const double* __restrict__ in, double* __restrict__ out) {
  __shared__ double s_red[256];
  const int64_t at = (int64_t)blockIdx.x * 512 + threadIdx.x;
  const double first = block_sum256_tree(in[at], s_red);
  const double second = block_sum256_tree(in[at + 256], s_red);
  out[at] = first;
  out[at + 256] = second;
}

template <int OP>
static void launch_geom_rows(const double* in, double* out, int64_t n) {
  hipLaunchKernelGGL(k_geom_rows<OP>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, in, out, n);
}

}  // namespace sfm

extern "C" {

int32_t sfm_debug_geom(int32_t device, int32_t op, const double* in, int64_t n, double* out) {
  if (!in || !out || n < 0 || n > kGeomMaxRows || op < 0 || op >= SFM_GEOM_OPS) return SFM_EINVAL;
  if (n == 0) return SFM_OK;
  if (hipSetDevice(device) != hipSuccess) return SFM_EDEVICE;
  const size_t bin = (size_t)n * kGeomIn[op] * 8, bout = (size_t)n * kGeomOut[op] * 8;
  double *din = nullptr, *dout = nullptr;
  int32_t rc = SFM_OK;
  if (hipMalloc(&din, bin) || hipMalloc(&dout, bout) || hipMemcpy(din, in, bin, hipMemcpyHostToDevice)) {
    rc = SFM_EDEVICE;
  } else {
    switch (op) {
      case SFM_GEOM_RODRIGUES: launch_geom_rows<SFM_GEOM_RODRIGUES>(din, dout, n); break;
      case SFM_GEOM_RODRIGUES_INV: launch_geom_rows<SFM_GEOM_RODRIGUES_INV>(din, dout, n); break;
      case SFM_GEOM_EIG3: launch_geom_rows<SFM_GEOM_EIG3>(din, dout, n); break;
      case SFM_GEOM_NULL4: launch_geom_rows<SFM_GEOM_NULL4>(din, dout, n); break;
      case SFM_GEOM_COMPOSE: launch_geom_rows<SFM_GEOM_COMPOSE>(din, dout, n); break;
      case SFM_GEOM_ROTATE: launch_geom_rows<SFM_GEOM_ROTATE>(din, dout, n); break;
      case SFM_GEOM_WAVE_SUM:
        hipLaunchKernelGGL(k_geom_wave_sum, dim3((unsigned)n), dim3(64), 0, 0, din, dout);
        break;
      default:  // SFM_GEOM_BLOCK_SUM
        hipLaunchKernelGGL(k_geom_block_sum, dim3((unsigned)n), dim3(256), 0, 0, din, dout);
        break;
    }
    if (hipGetLastError() || hipDeviceSynchronize() || hipMemcpy(out, dout, bout, hipMemcpyDeviceToHost))
      rc = SFM_EDEVICE;
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  return rc;
}

}  // extern "C"
