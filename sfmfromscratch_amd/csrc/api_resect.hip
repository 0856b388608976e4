// api_resect.hip — the poses of a slot table's unposed frames from its tracks (resect.hip;
// workspace c->resect).  The call checks its arguments before touching the device and enqueues
// five launches on the caller's stream; growing the workspace is its only allocation and nothing
// synchronises, so after a call of the same sizes it can be captured into a hipGraph.
#include "ctx.h"

using namespace sfm;

extern "C" {

int32_t sfm_resect_tracks_dev(sfm_ctx* c, const int32_t* xy, const int32_t* count, int32_t nimg, int64_t cap,
                              const int32_t* node_track, const double* X, int32_t n_tracks, const double* K,
                              const uint8_t* attempt, int32_t iters, double threshold, int32_t min_inliers,
                              int64_t seed, int32_t max_refine_iter, double* pose, int32_t* rstat, double* rcost,
                              uint8_t* rkeep, int32_t* out_counts, double* out_hyp, void* stream) {
  if (!c) return SFM_EINVAL;
  if (nimg < 1 || cap < 1) return set_err(c, SFM_EINVAL, "sfm_resect_tracks_dev: nimg, cap >= 1");
  if (n_tracks < 0) return set_err(c, SFM_EINVAL, "sfm_resect_tracks_dev: n_tracks is negative");
  if (iters < 0 || iters > kVerifyMaxIters)
    return set_err(c, SFM_EINVAL, "sfm_resect_tracks_dev: iters must lie in [0, 2^20]");
  if (!(threshold > 0.0)) return set_err(c, SFM_EINVAL, "sfm_resect_tracks_dev: threshold must be positive");
  if (min_inliers < 0) return set_err(c, SFM_EINVAL, "sfm_resect_tracks_dev: min_inliers is negative");
  if (max_refine_iter < 1 || max_refine_iter >= (1 << kRefineStatusShift))
    return set_err(c, SFM_EINVAL, "sfm_resect_tracks_dev: max_refine_iter must be in [1, 2^24)");
  if (!xy || !count || !node_track || !K || !pose || !rstat || !rcost)
    return set_err(c, SFM_EINVAL, "sfm_resect_tracks_dev: xy, count, node_track, K, pose, rstat or rcost is null");
  if (n_tracks > 0 && !X) return set_err(c, SFM_EINVAL, "sfm_resect_tracks_dev: X is null");
  if ((int64_t)nimg * cap > ((int64_t)1 << 30))
    return set_err(c, SFM_EINVAL, "sfm_resect_tracks_dev: at most 2^30 nodes (nimg * cap)");
  if ((int64_t)nimg * ((iters + 7) / 8) >= ((int64_t)1 << 31))
    return set_err(c, SFM_EINVAL, "sfm_resect_tracks_dev: nimg * iters / 8 must stay below 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  ResectWs& w = c->resect;
  const size_t N = (size_t)nimg * (size_t)cap, S = (size_t)nimg * (size_t)std::max(iters, 1);
  int rc;
  if ((rc = ensure(c, w.Xl, N * 24)) || (rc = ensure(c, w.xl, N * 16)) || (rc = ensure(c, w.lrow, N * 4)) ||
      (rc = ensure(c, w.inl, N * 4)) || (rc = ensure(c, w.n_links, (size_t)nimg * 4)) ||
      (rc = ensure(c, w.go, (size_t)nimg * 4)) || (rc = ensure(c, w.n_inl, (size_t)nimg * 4)) ||
      (rc = ensure(c, w.Rt0, (size_t)nimg * 96)))
    return rc;
  if (!out_hyp && (rc = ensure(c, w.hyp, S * 96))) return rc;
  if (!out_counts && (rc = ensure(c, w.counts, S * 4))) return rc;
  ResectProblem q{};
  q.xy = xy, q.count = count, q.node_track = node_track, q.X = X, q.K = K, q.attempt = attempt;
  q.nimg = nimg, q.cap = (int)cap, q.n_tracks = n_tracks, q.iters = iters, q.min_inliers = min_inliers;
  q.max_refine_iter = max_refine_iter, q.thr = threshold, q.seed = (uint64_t)seed;
  q.pose = pose, q.rstat = rstat, q.rcost = rcost, q.rkeep = rkeep, q.out_counts = out_counts, q.out_hyp = out_hyp;
  q.Xl = as<double>(w.Xl), q.xl = as<double>(w.xl), q.Rt0 = as<double>(w.Rt0);
  q.hyp = out_hyp ? out_hyp : as<double>(w.hyp);
  q.counts = out_counts ? out_counts : as<int32_t>(w.counts);
  q.lrow = as<int32_t>(w.lrow), q.inl = as<int32_t>(w.inl), q.n_links = as<int32_t>(w.n_links);
  q.go = as<int32_t>(w.go), q.n_inl = as<int32_t>(w.n_inl);
  launch_resect_tracks(q, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

}  // extern "C"
