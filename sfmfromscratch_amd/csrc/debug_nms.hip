// debug_nms.hip — diagnostics of the block-driven certified NMS (nms.hip k_nms_blocks; include/
// sfmfeat.h under "diagnostics"): the kernel on host planes with block-maximum maps computed on
// the host, exact or inflated, beside the band kernel on the same planes; the size rule; and the
// tests' handle on the choice of kernel.  Not used by the pipeline.
#include <math.h>
#include <string.h>

#include <vector>

#include "ctx.h"

using namespace sfm;

extern "C" {

int64_t sfm_debug_bmax_stride(int32_t h, int32_t w) { return bmax_plane_stride(h, w); }

void sfm_debug_set_nms_blocks(int32_t mode) { extract_set_nms_blocks(mode); }

int32_t sfm_debug_nms_blocks_rule(int32_t h, int32_t w, int32_t kcap, int32_t ksize) {
  const LayoutSwitches sw;  // the defaults: exact_px, the size rule
  const bool exact = (int64_t)h * w < (int64_t)sw.exact_px * kcap;
  return nms_blocks_level(h, w, kcap, ksize, exact, -1) ? 1 : 0;
}

int32_t sfm_debug_nms_blocks(int32_t device, const float* R, int32_t B, int32_t H, int32_t W, const uint32_t* tnms,
                             const uint32_t* fallback, int32_t blocks, int32_t inflate, uint64_t* keys_out,
                             int64_t* counts_out) {
  if (!R || !tnms || !fallback || !keys_out || !counts_out || B < 1 || H < 1 || W < 4 || (W & 3)) return SFM_EINVAL;
  if (!nms_blocks_shape(W, 3, 0)) return SFM_EINVAL;  // (SFMFEAT_NMS_TILE=1 takes the tiled kernel)
  if (hipSetDevice(device) != hipSuccess) return SFM_EDEVICE;
  const int64_t n = (int64_t)H * W, tot = n * B;
  const int MH = (H + 3) / 4, MW = W / 4;
  const int64_t stride = bmax_plane_stride(H, W);
  // the maps: each block's maximum over its in-image pixels (fmaxf drops a NaN; an all-NaN
  // block keeps -inf), then raised; the floats between the planes' maps are NaN
  std::vector<float> M((size_t)B * stride, NAN);
  for (int b = 0; b < B; ++b)
    for (int by = 0; by < MH; ++by)
      for (int bx = 0; bx < MW; ++bx) {
        float m = -INFINITY;
        for (int i = 0; i < 4 && 4 * by + i < H; ++i)
          for (int e = 0; e < 4; ++e) m = fmaxf(m, R[(int64_t)b * n + (int64_t)(4 * by + i) * W + 4 * bx + e]);
        if (inflate) m = (by * MW + bx) % 3 == 0 ? INFINITY : nextafterf(m, INFINITY);
        M[(size_t)b * stride + (size_t)by * MW + bx] = m;
      }
  float *d_R = nullptr, *d_M = nullptr;
  MedianState* d_med = nullptr;
  unsigned long long* d_cnt = nullptr;
  uint64_t* d_cand = nullptr;
  int32_t rc = SFM_OK;
  if (hipMalloc(&d_R, tot * 4) || hipMalloc(&d_M, M.size() * 4) || hipMalloc(&d_med, sizeof(MedianState) * B) ||
      hipMalloc(&d_cnt, 8 * (size_t)B * kCounterStride) || hipMalloc(&d_cand, tot * 8)) {
    rc = SFM_EDEVICE;
  } else {
    std::vector<MedianState> ms(B);
    memset(ms.data(), 0, sizeof(MedianState) * B);
    for (int b = 0; b < B; ++b) {
      ms[b].tnms = tnms[b];
      ms[b].fallback = fallback[b] ? 1u : 0u;
    }
    if (hipMemcpy(d_R, R, tot * 4, hipMemcpyHostToDevice) || hipMemcpy(d_M, M.data(), M.size() * 4, hipMemcpyHostToDevice) ||
        hipMemcpy(d_med, ms.data(), sizeof(MedianState) * B, hipMemcpyHostToDevice) ||
        hipMemset(d_cnt, 0, 8 * (size_t)B * kCounterStride) || hipMemset(d_cand, 0xff, tot * 8)) {
      rc = SFM_EDEVICE;
    } else {
      launch_nms(d_R, d_med, d_cand, d_cnt, B, H, W, 3, 0, 0, 0, blocks ? d_M : nullptr);
      std::vector<unsigned long long> cnt((size_t)B * kCounterStride);
      if (hipGetLastError() || hipDeviceSynchronize() ||
          hipMemcpy(cnt.data(), d_cnt, 8 * cnt.size(), hipMemcpyDeviceToHost) ||
          hipMemcpy(keys_out, d_cand, tot * 8, hipMemcpyDeviceToHost)) {
        rc = SFM_EDEVICE;
      } else {
        for (int b = 0; b < B; ++b) counts_out[b] = (int64_t)cnt[(size_t)b * kCounterStride];
      }
    }
  }
  void* bufs[] = {d_R, d_M, d_med, d_cnt, d_cand};
  for (void* b : bufs) (void)hipFree(b);
  return rc;
}

}  // extern "C"
