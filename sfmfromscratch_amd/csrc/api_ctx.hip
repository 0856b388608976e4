// api_ctx.hip — the C-ABI (include/sfmfeat.h): parameters, context create / destroy and
// setters, the lane gate and the context stream.
#include <math.h>

#include "ctx.h"

using namespace sfm;

namespace {

// NaiveSIFT._generate_gaussian_kernel (NaiveSIFT.py:175-199) evaluated natively in double
// (numpy's linspace/exp/sum order); the Python wrapper passes numpy's own taps instead.
void gaussian_taps(int ks, double sigma, float* out) {
  double ax[SFM_MAX_GAUSS], k[SFM_MAX_GAUSS * SFM_MAX_GAUSS];
  int m = ks / 2;
  if (ks == 1) {
    ax[0] = (double)-m;
  } else {
    double step = ((double)m - (double)-m) / (double)(ks - 1);
    for (int i = 0; i < ks; ++i) ax[i] = (double)i * step + (double)-m;
    ax[ks - 1] = (double)m;
  }
  const double PI = 3.141592653589793;
  double c = 1.0 / (2.0 * PI * (sigma * sigma));
  double den = 2.0 * (sigma * sigma);
  for (int i = 0; i < ks; ++i)
    for (int j = 0; j < ks; ++j) k[i * ks + j] = c * exp(-((ax[i] * ax[i]) + (ax[j] * ax[j])) / den);
  int n = ks * ks;
  double total = 0.0;
  if (n < 8) {
    for (int i = 0; i < n; ++i) total += k[i];
  } else {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = k[j];
    int i;
    for (i = 8; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += k[i + j];
    total = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) total += k[i];
  }
  for (int i = 0; i < n; ++i) out[i] = (float)(k[i] / total);
}

bool gauss_size_supported(int ks) {
  return (ks >= 1 && ks <= 9) || ks == 11 || ks == 13 || ks == 15;
}

}  // namespace

extern "C" {

void sfm_params_default(sfm_params* p, int32_t mode) {
  memset(p, 0, sizeof(*p));
  p->mode = mode;
  p->num_interest_points = 2500;  // FeatureExtractor.py:11
  p->ksize = 7;                   // NaiveSIFT.py:35
  p->gaussian_size = 7;           // :36
  p->sigma = 5.0;                 // :37
  p->alpha = 0.05;                // :38
  p->feature_width = 16;          // :39
  p->pyramid_level = mode == SFM_MODE_NAIVE ? 1 : 4;  // ScaleRotInvSIFT.py:12
  p->pyramid_scale_factor = 2.0;                      // :13
  p->gauss_kernel_set = 0;
}

int32_t sfm_abi_version(void) { return 1; }

int32_t sfm_build_flags(void) {
#ifdef SFM_ABLATIONS
  return SFM_BUILD_ABLATIONS;
#else
  return 0;
#endif
}

int64_t sfm_keypoint_capacity(const sfm_params* p) {
  if (!p) return 0;
  if (p->mode == SFM_MODE_NAIVE) return p->num_interest_points > 0 ? p->num_interest_points : 0;
  int L = p->pyramid_level;
  if (L < 1) return 0;
  int64_t k = (int64_t)((double)p->num_interest_points / (double)L);
  return k > 0 ? (int64_t)L * k : 0;
}

int32_t sfm_pyramid_dims(const sfm_params* p, int32_t H, int32_t W, int32_t* dims) {
  if (!p || !dims) return SFM_EINVAL;
  Level lv[SFM_MAX_LEVELS];
  int L = 0;
  if (extract_levels(p, H, W, lv, &L) != SFM_OK) return SFM_EINVAL;
  for (int l = 0; l < L; ++l) {
    dims[2 * l] = lv[l].h;
    dims[2 * l + 1] = lv[l].w;
  }
  return SFM_OK;
}

int32_t sfm_ctx_create(int32_t device, const sfm_params* p, sfm_ctx** out) {
  if (!p || !out) return SFM_EINVAL;
  *out = nullptr;
  if (p->mode != SFM_MODE_SCALEROT && p->mode != SFM_MODE_NAIVE) return SFM_EINVAL;
  if (!gauss_size_supported(p->gaussian_size)) return SFM_EINVAL;
  if (p->ksize < 0 || p->ksize / 2 > SFM_NMS_MAX_HALF) return SFM_EINVAL;
  if (p->feature_width < 0 || p->feature_width > SFM_MAX_FW) return SFM_EINVAL;
  if (p->mode == SFM_MODE_SCALEROT && (p->pyramid_level < 1 || p->pyramid_level > SFM_MAX_LEVELS))
    return SFM_EINVAL;
  if (p->mode == SFM_MODE_SCALEROT && !(p->pyramid_scale_factor > 0.0)) return SFM_EINVAL;
  const int L = p->mode == SFM_MODE_NAIVE ? 1 : p->pyramid_level;
  int64_t k = p->mode == SFM_MODE_NAIVE ? p->num_interest_points
                                        : (int64_t)((double)p->num_interest_points / (double)L);
  if (k < 0) k = 0;
  if (k > kTopkLdsCap || (int64_t)L * k > kMaxMatchRows) return SFM_EINVAL;
  sfm_ctx* c = new sfm_ctx();
  c->device = device;
  c->p = *p;
  c->L = L;
  if (c->p.mode == SFM_MODE_NAIVE) c->p.pyramid_level = 1;
  c->kcap = (int)k;
  c->cap = (int64_t)L * k;
  c->match.direct = env_flag(getenv("SFMFEAT_MATCH_DIRECT"));
  const char* se = getenv("SFMFEAT_SELECT");
  c->exact_select = se && strcmp(se, "exact") == 0;
  c->serial = env_flag(getenv("SFMFEAT_SERIAL"));
  const int mb = env_int(getenv("SFMFEAT_MATCH_BUDGET_MB"), 0);
  if (mb > 0) c->match.budget = (size_t)mb << 20;
  int gs = p->gaussian_size;
  if (p->gauss_kernel_set) memcpy(c->gauss, p->gauss_kernel, sizeof(float) * gs * gs);
  else gaussian_taps(gs, p->sigma, c->gauss);
  // Both streams are created on first use: the context's own stream (host-pointer calls,
  // sfm_ctx_stream) and the aux stream (non-serial extractions).  The HIP runtime maps streams
  // onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and streams beyond that share one,
  // which serialises them; a context that only carries work on the streams it needs keeps
  // the caller's stream layout under the caller's control (pipeline.BatchPipeline).
  bool ok = hipSetDevice(device) == hipSuccess;
  // SFMFEAT_EAGER_HOST_STREAM=1 (A/B): the round-3 stream layout (both made here)
  if (ok && env_int(SFM_DIAG_ENV("SFMFEAT_EAGER_HOST_STREAM"), 0) == 1)
    ok = hipStreamCreateWithFlags(&c->s.stream, hipStreamNonBlocking) == hipSuccess &&
         hipStreamCreateWithFlags(&c->s.aux, hipStreamNonBlocking) == hipSuccess;
  for (hipEvent_t& e : c->s.ev) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
  std::vector<float> taps(harris_taps_floats(gs));
  harris_taps_build(c->gauss, gs, taps.data());
  ok = ok && ensure(c, c->ex.gauss, sizeof(float) * taps.size()) == SFM_OK &&
       hipMemcpy(c->ex.gauss.p, taps.data(), sizeof(float) * taps.size(), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    delete c;
    return SFM_EDEVICE;
  }
  init_topk_attributes();
  init_describe_attributes(describe_lds_bytes(SFM_MAX_FW, 1));
  init_describe_quad_tables();
  init_match_attributes(kMaxMatchRows);
  *out = c;
  return SFM_OK;
}

int32_t sfm_ctx_destroy(sfm_ctx* c) {
  delete c;
  return SFM_OK;
}

const char* sfm_last_error(const sfm_ctx* c) { return c ? c->err.c_str() : "null context"; }

int32_t sfm_ctx_set_fused_prep(sfm_ctx* c, int32_t on) {
  if (!c) return SFM_EINVAL;
  c->match.fused_prep = on != 0;
  operands_fused_clear(c);
  return SFM_OK;
}

int32_t sfm_ctx_set_serial(sfm_ctx* c, int32_t serial) {
  if (!c) return SFM_EINVAL;
  c->serial = serial != 0;
  return SFM_OK;
}

int32_t sfm_ctx_set_priority(sfm_ctx* c, int32_t priority) {
  if (!c) return SFM_EINVAL;
  if (c->s.stream || c->s.aux) return set_err(c, SFM_EINVAL, "stream priority after the context's streams exist");
  c->s.prio = priority;
  return SFM_OK;
}

int32_t sfm_ctx_stream(sfm_ctx* c, void** stream) {
  if (!c || !stream) return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st;
  int rc;
  if ((rc = host_stream(c, &st))) return rc;
  *stream = (void*)st;
  return SFM_OK;
}

int32_t sfm_gate_create(int32_t device, sfm_gate** out) {
  if (!out) return SFM_EINVAL;
  *out = nullptr;
  if (hipSetDevice(device) != hipSuccess) return SFM_EDEVICE;
  sfm_gate* g = new sfm_gate();
  g->device = device;
  if (hipEventCreateWithFlags(&g->ev, hipEventDisableTiming) != hipSuccess) {
    delete g;
    return SFM_EDEVICE;
  }
  *out = g;
  return SFM_OK;
}

int32_t sfm_gate_destroy(sfm_gate* g) {
  if (!g) return SFM_OK;
  (void)hipSetDevice(g->device);
  if (g->armed) (void)hipEventSynchronize(g->ev);
  (void)hipEventDestroy(g->ev);
  delete g;
  return SFM_OK;
}

int32_t sfm_ctx_set_gate(sfm_ctx* c, sfm_gate* g) {
  if (!c) return SFM_EINVAL;
  if (g && g->device != c->device) return set_err(c, SFM_EINVAL, "gate and context on different devices");
  c->gate = g;
  return SFM_OK;
}

}  // extern "C"
