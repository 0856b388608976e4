// api_profile.hip — stage profiling and Harris launch spans (workspace c->prof), and the two
// sfm_debug_* reads of the last extraction's workspace.
#include "ctx.h"

using namespace sfm;

namespace {

// every span slot back to {~0, 0} (the kernels fold their workgroups in with atomic min / max)
int spans_reset(sfm_ctx* c) {
  ProfilerWs& pr = c->prof;
  pr.span_n = 0;
  pr.span_dropped = 0;
  pr.span_level.clear();
  if (pr.span_cap == 0) return SFM_OK;
  std::vector<unsigned long long> init((size_t)2 * pr.span_cap, 0ull);
  for (int64_t i = 0; i < pr.span_cap; ++i) init[2 * i] = ~0ull;
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(pr.spans.p, init.data(), init.size() * 8, hipMemcpyHostToDevice));
  return SFM_OK;
}

}  // namespace

extern "C" {

int32_t sfm_profile_enable(sfm_ctx* c, int32_t on) {
  if (!c) return SFM_EINVAL;
  c->prof.on = on != 0;
  c->prof.mask = ~0u;
  return SFM_OK;
}

int32_t sfm_profile_stages(sfm_ctx* c, int32_t mask) {
  if (!c) return SFM_EINVAL;
  c->prof.on = mask != 0;
  c->prof.mask = (uint32_t)mask;
  return SFM_OK;
}

int32_t sfm_profile_read(sfm_ctx* c, double* ms, int64_t* launches, int32_t reset) {
  if (!c) return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  ProfilerWs& pr = c->prof;
  for (auto& e : pr.pending) {
    HIPCHK(c, hipEventSynchronize(e.second.second));
    float t = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&t, e.second.first, e.second.second));
    pr.ms[e.first] += t;
    pr.launches[e.first] += 1;
    pr.pool.push_back(e.second.first);
    pr.pool.push_back(e.second.second);
  }
  pr.pending.clear();
  for (int i = 0; i < SFM_PROF_STAGES; ++i) {
    if (ms) ms[i] = pr.ms[i];
    if (launches) launches[i] = pr.launches[i];
    if (reset) {
      pr.ms[i] = 0.0;
      pr.launches[i] = 0;
    }
  }
  return SFM_OK;
}

int32_t sfm_profile_spans(sfm_ctx* c, int64_t capacity) {
  if (!c || capacity < 0) return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if (capacity > 0 && (rc = ensure(c, c->prof.spans, (size_t)capacity * 16))) return rc;
  c->prof.span_cap = capacity;
  return spans_reset(c);
}

int32_t sfm_profile_spans_read(sfm_ctx* c, int64_t* spans_ns, int32_t* levels, int64_t cap, int64_t* n_out,
                               int64_t* dropped, int32_t reset) {
  if (!c || !n_out || cap < 0) return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  ProfilerWs& pr = c->prof;
  *n_out = pr.span_n;
  if (dropped) *dropped = pr.span_dropped;
  if (pr.span_n > 0 && spans_ns && cap > 0) {
    int khz = 0;
    HIPCHK(c, hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device));
    if (khz <= 0) return set_err(c, SFM_EDEVICE, "device reports no wall-clock rate");
    HIPCHK(c, hipDeviceSynchronize());
    const int64_t n = std::min(cap, pr.span_n);
    std::vector<unsigned long long> h((size_t)2 * n);
    HIPCHK(c, hipMemcpy(h.data(), pr.spans.p, h.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) {
      for (int k = 0; k < 2; ++k) {  // ticks -> ns; an untouched slot reads -1
        const unsigned long long t = h[2 * i + k];
        spans_ns[2 * i + k] = (t == ~0ull || (k == 1 && t == 0ull)) ? -1 : (int64_t)((long double)t * 1.0e6L / khz);
      }
      if (levels) levels[i] = pr.span_level[(size_t)i];
    }
  }
  return reset ? spans_reset(c) : SFM_OK;
}

// diagnostics: copy level `l`'s R maps (what = 0) or level images (what = 1) of the last
// extraction, all planes [B][h][w], to the device buffer `out` on `stream`
int32_t sfm_debug_copy_level(sfm_ctx* c, int32_t l, int32_t what, float* out, void* stream) {
  if (!c || !out || l < 0 || l >= c->L || !c->ex.last_B) return SFM_EINVAL;
  ExtractWs& x = c->ex;
  ExtractLayout y;
  if (extract_layout(&c->p, c->kcap, x.last_B, x.last_H, x.last_W, c->serial, extract_layout_switches(), &y) != SFM_OK)
    return SFM_EINVAL;
  if (what == 2) {  // the block-maximum maps, planes bmax_plane_stride apart
    if (!((x.last_mapped >> l) & 1u) || y.bmax[l] < 0) return set_err(c, SFM_EINVAL, "the level wrote no block-maximum map");
    HIPCHK(c, hipMemcpyAsync(out, as<float>(x.buf[kBufBmax]) + y.bmax[l],
                             (size_t)x.last_B * bmax_plane_stride(y.lv[l].h, y.lv[l].w) * 4, hipMemcpyDeviceToDevice,
                             (hipStream_t)stream));
    return SFM_OK;
  }
  const size_t bytes = (size_t)x.last_B * y.lv[l].h * y.lv[l].w * 4;
  const float* src = what == 0 ? as<float>(x.buf[kBufR]) + y.plane[l]
                               : (l == 0 ? as<float>(x.buf[kBufImg0]) : as<float>(x.buf[kBufLvl]) + y.lvl[l]);
  HIPCHK(c, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SFM_OK;
}

int32_t sfm_debug_select_stats(sfm_ctx* c, int32_t* fallback_planes, int32_t* total_planes) {
  if (!c || !fallback_planes || !total_planes) return SFM_EINVAL;
  *fallback_planes = 0;
  *total_planes = c->L * c->ex.last_B;
  if (*total_planes == 0) return SFM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  std::vector<MedianState> ms((size_t)*total_planes);
  HIPCHK(c, hipMemcpy(ms.data(), c->ex.buf[kBufMed].p, ms.size() * sizeof(MedianState), hipMemcpyDeviceToHost));
  for (const MedianState& m : ms) *fallback_planes += m.fallback ? 1 : 0;
  return SFM_OK;
}

}  // extern "C"
