// tracks.h — feature tracks (tracks.hip; include/sfmfeat.h sfm_build_tracks_dev,
// sfm_triangulate_tracks_dev): the workspace api_tracks.hip sizes and the two launch sequences.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sfm {

constexpr int kTrkThreads = 256;
constexpr int kTrkScanItems = 4;                             // nodes per thread of the scan kernels
constexpr int kTrkScanTile = kTrkThreads * kTrkScanItems;    // nodes per workgroup of the scan kernels
constexpr int64_t kTrkMaxNodes = (int64_t)1 << 30;           // nimg * cap

// component classes (state[] at a root)
constexpr int kTrkNone = 0;          // fewer than two nodes
constexpr int kTrkKept = 1;
constexpr int kTrkInconsistent = 2;  // node_track -2
constexpr int kTrkShort = 3;         // node_track -3

// the slots of the hash table of (root, slot) keys for N nodes: a power of two >= 2 N
inline int64_t tracks_hash_slots(int64_t N) {
  int64_t h = 64;
  while (h < 2 * N) h <<= 1;
  return h;
}
inline int tracks_scan_blocks(int64_t N) { return (int)((N + kTrkScanTile - 1) / kTrkScanTile); }

struct TracksProblem {
  const int32_t* count;    // [nimg]
  int nimg, cap;
  const int32_t* pairs;    // [P][2]
  int P;
  const int32_t* matches;  // [P][cap][2]
  const int32_t* nmatch;   // [P]
  const uint8_t* keep;     // [P][cap] or null
  int min_len;
  // workspace, N = nimg * cap nodes
  int32_t* parent;         // [N] union-find, parent[n] <= n
  int32_t* size;           // [N] at a root: the component's nodes (then its fill cursor)
  int32_t* state;          // [N] at a root: a duplicate (root, slot) was seen, then kTrk*
  int32_t* tid;            // [N] at a kept root: its track id
  int32_t* tmp;            // [N] each track's nodes in fill order
  unsigned long long* hash;  // [hash_slots] (root, slot) keys, ~0 where empty
  int64_t hash_slots;
  uint32_t* bsum;          // [2][scan_blocks]: kept components and their nodes per scan tile
  // outputs
  int32_t* track_offsets;  // [T + 1]
  int32_t* obs_slot;       // [n_obs]
  int32_t* obs_row;        // [n_obs]
  int32_t* node_track;     // [nimg][cap]
  int32_t* out_n;          // [6]
};
// P >= 0, nimg, cap >= 1, nimg * cap <= kTrkMaxNodes
void launch_build_tracks(const TracksProblem& p, hipStream_t st);

// one thread per track: the CSR of launch_build_tracks (T tracks, n_obs observations; offsets
// are clamped to [0, n_obs]), xy [nimg][cap][2], P [n_cam][12], cam_valid [n_cam] or null;
// X [T][3], out_views [T]
void launch_triangulate_tracks(const int32_t* track_offsets, const int32_t* obs_slot, const int32_t* obs_row, int T,
                               int n_obs, const int32_t* xy, int nimg, int cap, const double* P,
                               const uint8_t* cam_valid, int n_cam, double* X, int32_t* out_views, hipStream_t st);

}  // namespace sfm
