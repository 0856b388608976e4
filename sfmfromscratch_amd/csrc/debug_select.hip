// debug_select.hip — sfm_debug_select: the keypoint selection an extraction runs (select scan,
// certified NMS, one k_select launch over the levels; api_extract.hip) on host R planes, so a test
// can hand k_select the planes that take each of its branches.  Launches only what
// extraction launches; the histogram Harris would have produced is computed on the host.  Not used
// by the pipeline.
#include <string.h>

#include <vector>

#include "../../include/sfmfeat.h"
#include "kernels.h"

using namespace sfm;

static_assert(sizeof(MedianState) == 4 * SFM_SELECT_STATE_WORDS, "sfmfeat.h: SFM_SELECT_STATE_WORDS");
static_assert(kSelectMaxLevels == 4, "sfmfeat.h: sfm_debug_select takes 1 .. 4 levels");

// common.h's fkey on the host
static uint32_t host_fkey(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

extern "C" int32_t sfm_debug_select(int32_t device, int32_t nlevels, int32_t B, const float* const* R,
                                    const int32_t* H, const int32_t* W, const int32_t* half_window, int32_t k,
                                    int32_t ksize, int64_t vmin, int32_t force_exact, int32_t* x, int32_t* y,
                                    float* conf, int32_t* count, uint32_t* state, int64_t* ncand, int32_t* consts) {
  if (!consts || k < 0 || k > kTopkLdsCap) return SFM_EINVAL;
  select_branch_sizes(k, consts);
  if (nlevels == 0) return SFM_OK;
  if (nlevels < 1 || nlevels > kSelectMaxLevels || B < 1 || !R || !H || !W || !half_window || !x || !y || !conf ||
      !count || !state || !ncand)
    return SFM_EINVAL;
  // vmin >= 3: the scan's ranks n - vmin, n - 3 vmin / 8 and n - vmin / 2 are pixels of the plane
  if (ksize < 1 || (ksize & 1) == 0 || vmin < 3) return SFM_EINVAL;
  if (!force_exact && ksize / 2 > SFM_NMS_MAX_HALF) return SFM_EINVAL;
  int64_t n[kSelectMaxLevels], off[kSelectMaxLevels], tot = 0;  // pixels per plane; the level's first pixel
  for (int l = 0; l < nlevels; ++l) {
    if (!R[l] || H[l] < 1 || W[l] < 1 || half_window[l] < 0) return SFM_EINVAL;
    n[l] = (int64_t)H[l] * W[l];
    if (n[l] >= ((int64_t)1 << 26)) return SFM_EINVAL;
    off[l] = tot;
    tot += n[l] * B;
  }
  if (hipSetDevice(device) != hipSuccess) return SFM_EDEVICE;
  const int kcap = k > 1 ? k : 1;
  const int64_t planes = (int64_t)nlevels * B;
  // Harris's digit-1 histogram of each plane
  std::vector<uint32_t> hist((size_t)planes * kMedBins1, 0u);
  for (int l = 0; l < nlevels; ++l)
    for (int b = 0; b < B; ++b) {
      uint32_t* h = hist.data() + ((size_t)l * B + b) * kMedBins1;
      const float* p = R[l] + (int64_t)b * n[l];
      for (int64_t i = 0; i < n[l]; ++i) ++h[host_fkey(p[i]) >> (32 - kMedBits1)];
    }
  float *d_R = nullptr, *d_conf = nullptr;
  uint32_t *d_hist = nullptr, *d_medlist = nullptr;
  uint64_t *d_cand = nullptr, *d_scratch = nullptr;
  MedianState* d_state = nullptr;
  unsigned long long* d_cnt = nullptr;  // two blocks of `planes` counters: median lists, certified NMS
  int32_t *d_x = nullptr, *d_y = nullptr, *d_count = nullptr;
  const size_t cnt_bytes = 2 * (size_t)planes * kCounterStride * 8, kp_bytes = (size_t)planes * kcap * 4;
  int32_t rc = SFM_OK;
  if (hipMalloc(&d_R, tot * 4) || hipMalloc(&d_hist, hist.size() * 4) || hipMalloc(&d_medlist, tot * 4) ||
      hipMalloc(&d_cand, tot * 8) || hipMalloc(&d_scratch, tot * 8) ||
      hipMalloc(&d_state, sizeof(MedianState) * planes) || hipMalloc(&d_cnt, cnt_bytes) ||
      hipMalloc(&d_x, kp_bytes) || hipMalloc(&d_y, kp_bytes) || hipMalloc(&d_conf, kp_bytes) ||
      hipMalloc(&d_count, planes * 4)) {
    rc = SFM_EDEVICE;
  } else {
    bool bad = false;
    for (int l = 0; l < nlevels; ++l)
      bad = bad || hipMemcpy(d_R + off[l], R[l], (size_t)n[l] * B * 4, hipMemcpyHostToDevice);
    bad = bad || hipMemcpy(d_hist, hist.data(), hist.size() * 4, hipMemcpyHostToDevice) ||
          hipMemset(d_state, 0, sizeof(MedianState) * planes) || hipMemset(d_cnt, 0, cnt_bytes) ||
          hipMemset(d_x, 0, kp_bytes) || hipMemset(d_y, 0, kp_bytes) || hipMemset(d_conf, 0, kp_bytes) ||
          hipMemset(d_count, 0, planes * 4);
    if (bad) {
      rc = SFM_EDEVICE;
    } else {
      init_topk_attributes();
      unsigned long long* medcnt = d_cnt;
      unsigned long long* candcnt = d_cnt + planes * kCounterStride;
      SelectLevels g{};
      g.n = nlevels;
      for (int l = 0; l < nlevels; ++l) {
        const int64_t p0 = (int64_t)l * B;  // the level's first plane
        launch_select_scan(d_hist + p0 * kMedBins1, d_state + p0, medcnt + p0 * kCounterStride, B, H[l], W[l], vmin,
                           force_exact ? 1 : 0, 0);
        if (!force_exact)
          launch_nms(d_R + off[l], d_state + p0, d_cand + off[l], candcnt + p0 * kCounterStride, B, H[l], W[l], ksize,
                     0, 0);
        g.l[l] = SelectLevels::Level{d_R + off[l],
                                     d_cand + off[l],
                                     candcnt + p0 * kCounterStride,
                                     d_medlist + off[l],
                                     d_scratch + off[l],
                                     KpList{d_x + p0 * kcap, d_y + p0 * kcap, d_conf + p0 * kcap, d_count + p0},
                                     d_state + p0,
                                     H[l],
                                     W[l],
                                     half_window[l]};
      }
      launch_select_levels(g, kcap, k, B, ksize, 0);
      std::vector<unsigned long long> cnt((size_t)planes * kCounterStride);
      if (hipGetLastError() || hipDeviceSynchronize() || hipMemcpy(x, d_x, kp_bytes, hipMemcpyDeviceToHost) ||
          hipMemcpy(y, d_y, kp_bytes, hipMemcpyDeviceToHost) ||
          hipMemcpy(conf, d_conf, kp_bytes, hipMemcpyDeviceToHost) ||
          hipMemcpy(count, d_count, planes * 4, hipMemcpyDeviceToHost) ||
          hipMemcpy(state, d_state, sizeof(MedianState) * planes, hipMemcpyDeviceToHost) ||
          hipMemcpy(cnt.data(), candcnt, cnt.size() * 8, hipMemcpyDeviceToHost)) {
        rc = SFM_EDEVICE;
      } else {
        for (int64_t p = 0; p < planes; ++p) ncand[p] = (int64_t)cnt[(size_t)p * kCounterStride];
      }
    }
  }
  void* bufs[] = {d_R, d_hist, d_medlist, d_cand, d_scratch, d_state, d_cnt, d_x, d_y, d_conf, d_count};
  for (void* b : bufs) (void)hipFree(b);
  return rc;
}
