// tracks.hip — feature tracks: the connected components of the match graph, and the N-view
// linear triangulation of each track (include/sfmfeat.h sfm_build_tracks_dev,
// sfm_triangulate_tracks_dev).  The reference has no counterpart; the rule is the
// library's own (the COLMAP / OpenMVG track step) and is pinned to tests/tracks_ref.py.
//
// Part A, integers only (two runs, and any order of the pairs or of the matches within a pair,
// give the same bytes):
// * union-find over parent[node], node = slot * cap + row, with parent[n] <= n at all times.
//   uf_find walks strictly downward and halves its path with atomicMin, so a parent only ever
//   decreases and every loop ends by construction.  uf_union links the larger root under the
//   smaller with one compare-and-swap on the larger root's own word; it fails only when another
//   thread's hook on that word succeeded (lock-free), and the retry starts from what that hook
//   wrote, strictly below the failed root.  No workgroup waits on another: no flags, no tickets.
//   Reads of parent[] are relaxed atomic loads of wavefront scope: they may be served by the
//   CU's L1, which spreads the reads of a giant component's root over the CUs.  A stale word is
//   an older parent, still an ancestor; a stale "root" only makes the CAS, which acts in L2,
//   fail and report the true parent.  A kernel starts with a clean L1, and k_trk_flatten hooks
//   nothing, so the roots it reads are final.
// * k_trk_edges: workgroup (pair p, 256 match rows), coalesced int2 loads of the pair's rows;
//   workgroups past nmatch[p] return after one scalar load.  Contention: a successful hook
//   retires its root for good, so a root word takes at most one successful CAS, and the failed
//   ones are bounded by the threads that read it as a root at the same moment; edges inside an
//   already joined component only read.
// * k_trk_flatten: every node finds its root, points at it, and adds 1 to the root's size; the
//   lanes of a wave that share the first live lane's root add once (one giant component would
//   otherwise put every add of a wave on one word).
// * k_trk_dups: a component with more nodes than slots is inconsistent by counting; every other
//   component's nodes insert the 64-bit key root * nimg + slot into an open-addressing table
//   (CAS, linear probing, load <= 1/2): a key found already there flags the root.  The flag is a
//   property of the key set, not of the order.
// * k_trk_classify / k_trk_scan_blocks / k_trk_assign: exclusive scans over the node ids of
//   (root is a kept track) and of its size: track ids in ascending label order and CSR offsets.
// * k_trk_fill puts each kept node anywhere in its track's span (an atomic cursor);
//   k_trk_rank then writes every node at the rank of its id within the span (ids ascend with the
//   slot), one thread per observation, each reading its own track's span once.  A kept track
//   has at most nimg nodes (one per slot), so that is at most nimg loads per thread and
//   nimg^2 per track, spread over nimg / 64 waves.
//
// Part B, float64 with -ffp-contract=off: k_triangulate_tracks, one thread per track.  The two
// rows of every valid view (SFM.py:241-246 on raw pixels), in ascending slot order, are folded
// into an upper-triangular 4 x 4 R by Givens rotations (R^T R = A^T A without forming it:
// pose.hip's header says why), and R goes to the one-sided Jacobi of linalg4.h.  Every index is
// compile-time; the fixed row order makes the bits reproducible.
#include "tracks.h"

#include <math.h>

#include <algorithm>

#include "common.h"
#include "linalg4.h"

namespace sfm {

namespace {

constexpr unsigned long long kTrkEmpty = ~0ull;

SFM_DEV int32_t uf_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// the root of x's tree at some moment of the call; halves the path on the way down
SFM_DEV int32_t uf_find(int32_t* parent, int32_t x) {
  int32_t p = uf_load(parent + x);
  while (p != x) {                             // p < x
    const int32_t g = uf_load(parent + p);     // g <= p
    if (g != p) (void)atomicMin(parent + x, g);  // x is no root: only other halvings write its word
    x = p;
    p = g;
  }
  return x;
}

SFM_DEV void uf_union(int32_t* parent, int32_t a, int32_t b) {
  int32_t ra = uf_find(parent, a), rb = uf_find(parent, b);
  while (ra != rb) {
    const int32_t hi = max(ra, rb), lo = min(ra, rb);
    const int32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    // hi stopped being a root: another thread's hook put it under old < hi
    ra = uf_find(parent, old);
    rb = uf_find(parent, lo);
  }
}

SFM_DEV int clamp_count(const int32_t* count, int s, int cap) { return min(max(count[s], 0), cap); }

__global__ void __launch_bounds__(kTrkThreads) k_trk_init(TracksProblem q, int N) {
  const int n = blockIdx.x * kTrkThreads + threadIdx.x;
  if (n < 6) q.out_n[n] = 0;
  if (n >= N) return;
  q.parent[n] = n;
  q.size[n] = 0;
  q.state[n] = 0;
  q.node_track[n] = -1;
}

__global__ void __launch_bounds__(kTrkThreads) k_trk_edges(TracksProblem q) {
  const int p = blockIdx.x;
  const int m0 = blockIdx.y * kTrkThreads;
  const int nm = min(q.nmatch[p], q.cap);  // -1 (the matcher's IndexError pair): no edge
  if (m0 >= nm) return;
  const int m = m0 + threadIdx.x;
  const int s0 = q.pairs[2 * (int64_t)p], s1 = q.pairs[2 * (int64_t)p + 1];
  const bool pair_ok = (unsigned)s0 < (unsigned)q.nimg && (unsigned)s1 < (unsigned)q.nimg && s0 != s1;
  const int c0 = pair_ok ? clamp_count(q.count, s0, q.cap) : 0;
  const int c1 = pair_ok ? clamp_count(q.count, s1, q.cap) : 0;
  if (m >= nm) return;
  const int64_t e = (int64_t)p * q.cap + m;
  if (q.keep && q.keep[e] == 0) return;
  const int2 r = reinterpret_cast<const int2*>(q.matches)[e];
  if ((unsigned)r.x < (unsigned)c0 && (unsigned)r.y < (unsigned)c1)
    uf_union(q.parent, s0 * q.cap + r.x, s1 * q.cap + r.y);
  else
    atomicAdd(q.out_n + 4, 1);
}

__global__ void __launch_bounds__(kTrkThreads) k_trk_flatten(TracksProblem q, int N) {
  const int n = blockIdx.x * kTrkThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool live = false;
  int32_t r = -1;
  if (n < N) {
    const int s = n / q.cap;
    live = n - s * q.cap < clamp_count(q.count, s, q.cap);
    if (live) {
      r = uf_find(q.parent, n);
      if (r != n) (void)atomicMin(q.parent + n, r);
    }
  }
  const uint64_t lm = __ballot(live);
  if (lm == 0) return;
  const int leader = __ffsll((unsigned long long)lm) - 1;
  const int32_t lead = __shfl(r, leader);
  const bool same = live && r == lead;
  const uint64_t sm = __ballot(same);
  if (same) {
    if (lane == leader) atomicAdd(q.size + lead, (int)__popcll(sm));
  } else if (live) {
    atomicAdd(q.size + r, 1);
  }
}

SFM_DEV uint64_t mix64(uint64_t x) {  // splitmix64's finaliser
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

__global__ void __launch_bounds__(kTrkThreads) k_trk_dups(TracksProblem q, int N) {
  const int n = blockIdx.x * kTrkThreads + threadIdx.x;
  if (n >= N) return;
  const int s = n / q.cap;
  if (n - s * q.cap >= clamp_count(q.count, s, q.cap)) return;
  const int32_t r = q.parent[n];
  const int32_t sz = q.size[r];
  if (sz < 2) return;
  if (sz > q.nimg) {  // more nodes than slots
    q.state[r] = 1;
    return;
  }
  const unsigned long long key = (unsigned long long)r * (unsigned long long)q.nimg + (unsigned long long)s;
  const uint64_t mask = (uint64_t)q.hash_slots - 1;
  uint64_t h = mix64(key) & mask;
  for (int64_t probe = 0; probe < q.hash_slots; ++probe) {  // (load <= 1/2: an empty slot exists)
    const unsigned long long old = atomicCAS(q.hash + h, kTrkEmpty, key);
    if (old == kTrkEmpty) return;
    if (old == key) {
      q.state[r] = 1;
      return;
    }
    h = (h + 1) & mask;
  }
}

// the class of node n as a root, from its size and its duplicate flag
SFM_DEV int trk_class(const TracksProblem& q, int n, int32_t* sz_out) {
  const int32_t sz = q.size[n];
  *sz_out = sz;
  if (q.parent[n] != n || sz < 2) return kTrkNone;
  if (q.state[n] != 0) return kTrkInconsistent;
  return sz < q.min_len ? kTrkShort : kTrkKept;
}

// state[root] <- its class; per tile the kept components and their nodes; the counters
__global__ void __launch_bounds__(kTrkThreads) k_trk_classify(TracksProblem q, int N, int nb) {
  __shared__ uint32_t s_scan[kTrkThreads / 64 + 1];
  const int n0 = (blockIdx.x * kTrkThreads + threadIdx.x) * kTrkScanItems;
  uint32_t cnt = 0, len = 0;
  int bad = 0, shrt = 0, longest = 0;
#pragma unroll
  for (int i = 0; i < kTrkScanItems; ++i) {
    const int n = n0 + i;
    if (n >= N) continue;
    int32_t sz;
    const int cls = trk_class(q, n, &sz);
    q.state[n] = cls;
    if (cls == kTrkKept) {
      ++cnt;
      len += (uint32_t)sz;
      longest = max(longest, sz);
    }
    bad += cls == kTrkInconsistent;
    shrt += cls == kTrkShort;
  }
  if (bad) atomicAdd(q.out_n + 2, bad);
  if (shrt) atomicAdd(q.out_n + 3, shrt);
  if (longest) atomicMax(q.out_n + 5, longest);
  uint32_t tc, tl;
  (void)block_exclusive_scan(cnt, s_scan, &tc);
  (void)block_exclusive_scan(len, s_scan, &tl);
  if (threadIdx.x == 0) {
    q.bsum[blockIdx.x] = tc;
    q.bsum[nb + blockIdx.x] = tl;
  }
}

// one workgroup: both tile arrays to exclusive prefixes; T, n_obs and the CSR's last entry
__global__ void __launch_bounds__(1024) k_trk_scan_blocks(TracksProblem q, int nb) {
  __shared__ uint32_t s_scan[1024 / 64 + 1];
  uint32_t carry_c = 0, carry_l = 0;
  for (int b0 = 0; b0 < nb; b0 += 1024) {
    const int b = b0 + threadIdx.x;
    const uint32_t c = b < nb ? q.bsum[b] : 0u, l = b < nb ? q.bsum[nb + b] : 0u;
    uint32_t tc, tl;
    const uint32_t ec = block_exclusive_scan(c, s_scan, &tc);
    const uint32_t el = block_exclusive_scan(l, s_scan, &tl);
    if (b < nb) {
      q.bsum[b] = carry_c + ec;
      q.bsum[nb + b] = carry_l + el;
    }
    carry_c += tc;
    carry_l += tl;
  }
  if (threadIdx.x == 0) {
    q.out_n[0] = (int32_t)carry_c;
    q.out_n[1] = (int32_t)carry_l;
    q.track_offsets[carry_c] = (int32_t)carry_l;
  }
}

// kept root n: tid[n] = the kept roots before it, track_offsets[tid] = their nodes
__global__ void __launch_bounds__(kTrkThreads) k_trk_assign(TracksProblem q, int N, int nb) {
  __shared__ uint32_t s_scan[kTrkThreads / 64 + 1];
  const int n0 = (blockIdx.x * kTrkThreads + threadIdx.x) * kTrkScanItems;
  uint32_t cnt = 0, len = 0;
  int32_t sz[kTrkScanItems];
  bool kept[kTrkScanItems];
#pragma unroll
  for (int i = 0; i < kTrkScanItems; ++i) {
    const int n = n0 + i;
    kept[i] = n < N && q.state[n] == kTrkKept;
    sz[i] = kept[i] ? q.size[n] : 0;
    cnt += kept[i];
    len += (uint32_t)sz[i];
  }
  uint32_t tc, tl;
  uint32_t ec = q.bsum[blockIdx.x] + block_exclusive_scan(cnt, s_scan, &tc);
  uint32_t el = q.bsum[nb + blockIdx.x] + block_exclusive_scan(len, s_scan, &tl);
#pragma unroll
  for (int i = 0; i < kTrkScanItems; ++i) {
    if (!kept[i]) continue;
    q.tid[n0 + i] = (int32_t)ec;
    q.track_offsets[ec] = (int32_t)el;
    ec += 1;
    el += (uint32_t)sz[i];
  }
}

__global__ void __launch_bounds__(kTrkThreads) k_trk_fill(TracksProblem q, int N) {
  const int n = blockIdx.x * kTrkThreads + threadIdx.x;
  if (n >= N) return;
  const int s = n / q.cap;
  if (n - s * q.cap >= clamp_count(q.count, s, q.cap)) return;
  const int32_t r = q.parent[n];
  const int cls = q.state[r];
  if (cls == kTrkNone) return;
  if (cls != kTrkKept) {
    q.node_track[n] = cls == kTrkInconsistent ? -2 : -3;
    return;
  }
  const int32_t t = q.tid[r];
  q.node_track[n] = t;
  const int32_t pos = atomicSub(q.size + r, 1) - 1;  // the size counts down: any order, every place once
  q.tmp[q.track_offsets[t] + pos] = n;
}

__global__ void __launch_bounds__(kTrkThreads) k_trk_rank(TracksProblem q, int N) {
  const int i = blockIdx.x * kTrkThreads + threadIdx.x;
  if (i >= N || i >= q.out_n[1]) return;
  const int32_t node = q.tmp[i];
  const int32_t t = q.tid[q.parent[node]];
  const int32_t lo = q.track_offsets[t], hi = q.track_offsets[t + 1];
  int rank = 0;
  for (int32_t j = lo; j < hi; ++j) rank += q.tmp[j] < node;
  const int s = node / q.cap;
  q.obs_slot[lo + rank] = s;
  q.obs_row[lo + rank] = node - s * q.cap;
}

// one Givens rotation per column: (R[k][k..3], w[k..3]) -> w[k] = 0, so that R^T R gains w w^T
SFM_DEV void fold_row(double (&R)[4][4], double (&w)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = R[k][k], b = w[k];
    const double h = sqrt(__builtin_fma(a, a, b * b));
    const bool rot = b != 0.0 && h != 0.0;  // (a NaN rotates and spreads)
    const double c = rot ? a / h : 1.0, s = rot ? b / h : 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < k) continue;
      const double rj = R[k][j], wj = w[j];
      R[k][j] = c * rj + s * wj;
      w[j] = c * wj - s * rj;
    }
  }
}

__global__ void __launch_bounds__(128) k_triangulate_tracks(
    const int32_t* __restrict__ off, const int32_t* __restrict__ obs_slot, const int32_t* __restrict__ obs_row,
    int T, int n_obs, const int32_t* __restrict__ xy, int nimg, int cap, const double* __restrict__ Pm,
    const uint8_t* __restrict__ cam_valid, int n_cam, double* __restrict__ X, int32_t* __restrict__ out_views) {
  const int t = blockIdx.x * 128 + threadIdx.x;
  if (t >= T) return;
  double R[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) R[r][c] = 0.0;
  int views = 0;
  const int32_t lo = max(off[t], 0), hi = min(off[t + 1], n_obs);
  for (int32_t o = lo; o < hi; ++o) {
    const int s = obs_slot[o], row = obs_row[o];
    if ((unsigned)s >= (unsigned)min(nimg, n_cam) || (unsigned)row >= (unsigned)cap) continue;
    if (cam_valid && cam_valid[s] == 0) continue;
    const int2 px = reinterpret_cast<const int2*>(xy)[(int64_t)s * cap + row];
    const double x = (double)px.x, y = (double)px.y;
    const double* P = Pm + (int64_t)s * 12;
    double wx[4], wy[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      wx[k] = x * P[8 + k] - P[k];
      wy[k] = y * P[8 + k] - P[4 + k];
    }
    fold_row(R, wx);
    fold_row(R, wy);
    ++views;
  }
  out_views[t] = views;
  double v[4];
  null_vector_4x4(R, v);
  const double nan = __builtin_nan("");
#pragma unroll
  for (int k = 0; k < 3; ++k) X[(int64_t)t * 3 + k] = views >= 2 ? v[k] / v[3] : nan;
}

}  // namespace

void launch_build_tracks(const TracksProblem& q, hipStream_t st) {
  const int N = q.nimg * q.cap;
  const int gb = (N + kTrkThreads - 1) / kTrkThreads;
  const int nb = tracks_scan_blocks(N);
  (void)hipMemsetAsync(q.hash, 0xff, (size_t)q.hash_slots * 8, st);
  hipLaunchKernelGGL(k_trk_init, dim3(std::max(gb, 1)), dim3(kTrkThreads), 0, st, q, N);
  if (q.P > 0)
    hipLaunchKernelGGL(k_trk_edges, dim3(q.P, (q.cap + kTrkThreads - 1) / kTrkThreads), dim3(kTrkThreads), 0, st, q);
  hipLaunchKernelGGL(k_trk_flatten, dim3(gb), dim3(kTrkThreads), 0, st, q, N);
  hipLaunchKernelGGL(k_trk_dups, dim3(gb), dim3(kTrkThreads), 0, st, q, N);
  hipLaunchKernelGGL(k_trk_classify, dim3(nb), dim3(kTrkThreads), 0, st, q, N, nb);
  hipLaunchKernelGGL(k_trk_scan_blocks, dim3(1), dim3(1024), 0, st, q, nb);
  hipLaunchKernelGGL(k_trk_assign, dim3(nb), dim3(kTrkThreads), 0, st, q, N, nb);
  hipLaunchKernelGGL(k_trk_fill, dim3(gb), dim3(kTrkThreads), 0, st, q, N);
  hipLaunchKernelGGL(k_trk_rank, dim3(gb), dim3(kTrkThreads), 0, st, q, N);
}

void launch_triangulate_tracks(const int32_t* track_offsets, const int32_t* obs_slot, const int32_t* obs_row, int T,
                               int n_obs, const int32_t* xy, int nimg, int cap, const double* P,
                               const uint8_t* cam_valid, int n_cam, double* X, int32_t* out_views, hipStream_t st) {
  if (T <= 0) return;
  hipLaunchKernelGGL(k_triangulate_tracks, dim3((T + 127) / 128), dim3(128), 0, st, track_offsets, obs_slot, obs_row,
                     T, n_obs, xy, nimg, cap, P, cam_valid, n_cam, X, out_views);
}

}  // namespace sfm
