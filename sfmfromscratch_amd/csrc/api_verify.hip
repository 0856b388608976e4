// api_verify.hip — geometric verification of a slot table's matches (verify.hip).  The call checks
// its arguments before touching the device, copies the host stop table into the kernel's
// arguments and enqueues one launch on the caller's stream: no workspace, no allocation, no
// synchronisation.
#include "ctx.h"

using namespace sfm;

extern "C" {

int32_t sfm_verify_matches_dev(sfm_ctx* c, const int32_t* xy, const int32_t* count, int32_t nimg, int64_t cap,
                               const int32_t* pairs, int32_t P, const int32_t* matches, const int32_t* nmatch,
                               int32_t iters, double threshold, int32_t min_inliers, int64_t seed,
                               const double* stop_ratio, int32_t n_stop, uint8_t* keep, double* F, int32_t* stat,
                               void* stream) {
  if (!c) return SFM_EINVAL;
  if (nimg < 1 || cap < 1 || P < 0) return set_err(c, SFM_EINVAL, "sfm_verify_matches_dev: nimg, cap >= 1 and P >= 0");
  if (iters < 0 || iters > kVerifyMaxIters)
    return set_err(c, SFM_EINVAL, "sfm_verify_matches_dev: iters must lie in [0, 2^20]");
  if (n_stop < 0 || n_stop > kVerifyMaxStop)
    return set_err(c, SFM_EINVAL, "sfm_verify_matches_dev: n_stop must lie in [0, 64]");
  if (n_stop > 0 && !stop_ratio) return set_err(c, SFM_EINVAL, "sfm_verify_matches_dev: stop_ratio is null");
  if (min_inliers < 0) return set_err(c, SFM_EINVAL, "sfm_verify_matches_dev: min_inliers must be >= 0");
  if (!xy || !count) return set_err(c, SFM_EINVAL, "sfm_verify_matches_dev: xy or count is null");
  if (P > 0 && (!pairs || !matches || !nmatch || !keep || !F || !stat))
    return set_err(c, SFM_EINVAL, "sfm_verify_matches_dev: pairs, matches, nmatch or an output pointer is null");
  if (P == 0) return SFM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  VerifyStop stop{};
  stop.n = n_stop;
  for (int i = 0; i < n_stop; ++i) stop.ratio[i] = stop_ratio[i];
  launch_verify(xy, count, nimg, cap, pairs, P, matches, nmatch, iters, threshold, min_inliers, (uint64_t)seed, stop,
                keep, F, stat, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

}  // extern "C"
