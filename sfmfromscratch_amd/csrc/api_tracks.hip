// api_tracks.hip — feature tracks from a slot table's matches and their N-view triangulation
// (tracks.hip; workspace c->tracks).  Both calls check their arguments before touching the
// device and are enqueued on the caller's stream without synchronising (growing the workspace
// frees buffers).
#include "ctx.h"
#include "tracks.h"

using namespace sfm;

extern "C" {

int32_t sfm_build_tracks_dev(sfm_ctx* c, const int32_t* count, int32_t nimg, int64_t cap, const int32_t* pairs,
                             int32_t P, const int32_t* matches, const int32_t* nmatch, const uint8_t* keep,
                             int32_t min_len, int32_t* track_offsets, int32_t* obs_slot, int32_t* obs_row,
                             int32_t* node_track, int32_t* out_n, void* stream) {
  if (!c) return SFM_EINVAL;
  if (nimg < 1 || cap < 1 || P < 0) return set_err(c, SFM_EINVAL, "sfm_build_tracks_dev: nimg, cap >= 1 and P >= 0");
  if (cap > kTrkMaxNodes || (int64_t)nimg * cap > kTrkMaxNodes)
    return set_err(c, SFM_EINVAL, "sfm_build_tracks_dev: at most 2^30 nodes (nimg * cap)");
  if ((cap + kTrkThreads - 1) / kTrkThreads > 65535)
    return set_err(c, SFM_EINVAL, "sfm_build_tracks_dev: cap is at most 65535 * 256");
  if (min_len < 2) return set_err(c, SFM_EINVAL, "sfm_build_tracks_dev: min_len must be >= 2");
  if (!count || !track_offsets || !obs_slot || !obs_row || !node_track || !out_n)
    return set_err(c, SFM_EINVAL, "sfm_build_tracks_dev: count or an output pointer is null");
  if (P > 0 && (!pairs || !matches || !nmatch))
    return set_err(c, SFM_EINVAL, "sfm_build_tracks_dev: pairs, matches or nmatch is null");
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t N = (int64_t)nimg * cap;
  TracksWs& w = c->tracks;
  TracksProblem q{};
  q.hash_slots = tracks_hash_slots(N);
  const int nb = tracks_scan_blocks(N);
  int rc;
  if ((rc = ensure(c, w.parent, (size_t)N * 4)) || (rc = ensure(c, w.size, (size_t)N * 4)) ||
      (rc = ensure(c, w.state, (size_t)N * 4)) || (rc = ensure(c, w.tid, (size_t)N * 4)) ||
      (rc = ensure(c, w.tmp, (size_t)N * 4)) || (rc = ensure(c, w.hash, (size_t)q.hash_slots * 8)) ||
      (rc = ensure(c, w.bsum, (size_t)nb * 2 * 4)))
    return rc;
  q.count = count;
  q.nimg = nimg;
  q.cap = (int)cap;
  q.pairs = pairs;
  q.P = P;
  q.matches = matches;
  q.nmatch = nmatch;
  q.keep = keep;
  q.min_len = min_len;
  q.parent = as<int32_t>(w.parent);
  q.size = as<int32_t>(w.size);
  q.state = as<int32_t>(w.state);
  q.tid = as<int32_t>(w.tid);
  q.tmp = as<int32_t>(w.tmp);
  q.hash = as<unsigned long long>(w.hash);
  q.bsum = as<uint32_t>(w.bsum);
  q.track_offsets = track_offsets;
  q.obs_slot = obs_slot;
  q.obs_row = obs_row;
  q.node_track = node_track;
  q.out_n = out_n;
  launch_build_tracks(q, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

int32_t sfm_triangulate_tracks_dev(sfm_ctx* c, const int32_t* track_offsets, const int32_t* obs_slot,
                                   const int32_t* obs_row, int32_t n_tracks, int32_t n_obs, const int32_t* xy,
                                   int32_t nimg, int64_t cap, const double* P, const uint8_t* cam_valid,
                                   int32_t n_cam, double* X, int32_t* out_views, void* stream) {
  if (!c) return SFM_EINVAL;
  if (n_tracks < 0 || n_obs < 0 || nimg < 1 || cap < 1 || n_cam < 1)
    return set_err(c, SFM_EINVAL, "sfm_triangulate_tracks_dev: n_tracks, n_obs >= 0 and nimg, cap, n_cam >= 1");
  if (cap > kTrkMaxNodes || (int64_t)nimg * cap > kTrkMaxNodes)
    return set_err(c, SFM_EINVAL, "sfm_triangulate_tracks_dev: at most 2^30 nodes (nimg * cap)");
  if (!track_offsets || !xy || !P)
    return set_err(c, SFM_EINVAL, "sfm_triangulate_tracks_dev: track_offsets, xy or P is null");
  if (n_tracks > 0 && (!X || !out_views))
    return set_err(c, SFM_EINVAL, "sfm_triangulate_tracks_dev: X or out_views is null");
  if (n_obs > 0 && (!obs_slot || !obs_row))
    return set_err(c, SFM_EINVAL, "sfm_triangulate_tracks_dev: obs_slot or obs_row is null");
  HIPCHK(c, hipSetDevice(c->device));
  launch_triangulate_tracks(track_offsets, obs_slot, obs_row, n_tracks, n_obs, xy, nimg, (int)cap, P, cam_valid, n_cam,
                            X, out_views, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

}  // extern "C"
