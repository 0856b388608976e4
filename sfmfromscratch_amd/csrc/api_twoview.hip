// api_twoview.hip — the two-view geometry record of a pair schedule (twoview.hip): the homography
// RANSAC and the relative pose out of verify's F.  Each call checks its arguments before touching
// the device and enqueues one launch on the caller's stream: no workspace, no allocation, no
// synchronisation.
#include "ctx.h"

using namespace sfm;

extern "C" {

int32_t sfm_homography_matches_dev(sfm_ctx* c, const int32_t* xy, const int32_t* count, int32_t nimg, int64_t cap,
                                   const int32_t* pairs, int32_t P, const int32_t* matches, const int32_t* nmatch,
                                   const int32_t* attempt, int32_t iters, double threshold, int64_t seed,
                                   const double* stop_ratio, int32_t n_stop, double* H, uint8_t* hkeep,
                                   int32_t* hstat, void* stream) {
  if (!c) return SFM_EINVAL;
  if (nimg < 1 || cap < 1 || P < 0)
    return set_err(c, SFM_EINVAL, "sfm_homography_matches_dev: nimg, cap >= 1 and P >= 0");
  if (iters < 0 || iters > kVerifyMaxIters)
    return set_err(c, SFM_EINVAL, "sfm_homography_matches_dev: iters must lie in [0, 2^20]");
  if (n_stop < 0 || n_stop > kVerifyMaxStop)
    return set_err(c, SFM_EINVAL, "sfm_homography_matches_dev: n_stop must lie in [0, 64]");
  if (n_stop > 0 && !stop_ratio) return set_err(c, SFM_EINVAL, "sfm_homography_matches_dev: stop_ratio is null");
  if (!xy || !count) return set_err(c, SFM_EINVAL, "sfm_homography_matches_dev: xy or count is null");
  if (P > 0 && (!pairs || !matches || !nmatch || !H || !hstat))
    return set_err(c, SFM_EINVAL, "sfm_homography_matches_dev: pairs, matches, nmatch, H or hstat is null");
  if (P == 0) return SFM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  VerifyStop stop{};
  stop.n = n_stop;
  for (int i = 0; i < n_stop; ++i) stop.ratio[i] = stop_ratio[i];
  launch_homography(xy, count, nimg, cap, pairs, P, matches, nmatch, attempt, iters, threshold, (uint64_t)seed, stop,
                    H, hkeep, hstat, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

int32_t sfm_two_view_pose_dev(sfm_ctx* c, const int32_t* xy, const int32_t* count, int32_t nimg, int64_t cap,
                              const int32_t* pairs, int32_t P, const int32_t* matches, const int32_t* nmatch,
                              const uint8_t* keep, const double* F, const double* K, const int32_t* attempt,
                              double cos2_min, double* pose, int32_t* pstat, void* stream) {
  if (!c) return SFM_EINVAL;
  if (nimg < 1 || cap < 1 || P < 0) return set_err(c, SFM_EINVAL, "sfm_two_view_pose_dev: nimg, cap >= 1 and P >= 0");
  if (!xy || !count || !K) return set_err(c, SFM_EINVAL, "sfm_two_view_pose_dev: xy, count or K is null");
  if (P > 0 && (!pairs || !matches || !nmatch || !keep || !F || !pose || !pstat))
    return set_err(c, SFM_EINVAL, "sfm_two_view_pose_dev: pairs, matches, nmatch, keep, F or an output pointer is null");
  if (P == 0) return SFM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  launch_two_view_pose(xy, count, nimg, cap, pairs, P, matches, nmatch, keep, F, K, attempt, cos2_min, pose, pstat,
                       (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

}  // extern "C"
