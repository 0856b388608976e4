// ctx.h — the C-ABI context (internal, not installed): one workspace per stage, each owned
// by its api_*.hip file, plus the small helpers those files share.
//
//   api_ctx.hip      params, create / destroy, setters, gate, stream
//   api_extract.hip  c->ex     (pyramid .. descriptors; layout in extract_layout.h)
//   api_match.hip    c->match  (operands + their owner record, per-pair buffers)
//   api_stage1.hip   c->ingest, c->ransac, c->pose
//   api_structure.hip c->structure (the link step's per-query and per-workgroup buffers),
//                    c->registry  (the point registry's partials and per-point state)
//   api_pnp.hip      c->pnp (sample stream on the device, hypotheses, counts; the host streams
//                    are c->ransac's cache)
//   api_ba.hip       c->ba (the plan's lists, the linearisation, the Schur system, the LM state)
//   api_tracks.hip   c->tracks (the union-find, the (root, slot) table, the scans' tile sums)
//   api_resect.hip   c->resect (each slot's compacted links, hypotheses, counts, the winners' inliers)
//   api_profile.hip  c->prof   (stage events, Harris spans, the sfm_debug_* reads)
#pragma once

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sfmfeat.h"
#include "extract_layout.h"
#include "kernels.h"

// A device allocation that frees itself (move-only).
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      std::swap(p, o.p);
      std::swap(bytes, o.bytes);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// Lane gate (sfm_gate_*): the contexts of batches in flight share one; each extraction's
// pyramid starts after the previous gated extraction's level-0 Harris launch has finished
// (SFMFEAT_GATE_LEVEL moves the release point), so the two batches' largest VALU launches
// alternate instead of competing for the CUs.
struct sfm_gate {
  int device = 0;
  hipEvent_t ev = nullptr;  // release point of the last gated extraction (timing disabled)
  bool armed = false;       // ev has been recorded
};

// The context's streams and fork/join events.  First member of sfm_ctx, so it is destroyed
// after every workspace has freed its buffers.
struct CtxStreams {
  hipStream_t stream = nullptr;  // host-pointer calls and sfm_ctx_stream, created on first use
  // extraction fork/join: keypoint selection + description of level l run on `aux` while
  // the caller's stream computes Harris + NMS of level l + 1 (events ev[0..SFM_MAX_LEVELS])
  hipStream_t aux = nullptr;
  hipEvent_t ev[SFM_MAX_LEVELS + 3] = {};
  int prio = 0;  // stream priority of both context streams (sfm_ctx_set_priority)
  CtxStreams() = default;
  CtxStreams(const CtxStreams&) = delete;
  CtxStreams& operator=(const CtxStreams&) = delete;
  ~CtxStreams() {
    if (stream) (void)hipStreamDestroy(stream);
    if (aux) (void)hipStreamDestroy(aux);
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// Stage profiling (sfm_profile_*): HIP events bracketing each stage's launches, and the
// kernel-active spans of the Harris launches (sfm_profile_spans): span_cap slots of {start,
// end} realtime ticks, the next free slot, each slot's first pyramid level.
struct ProfilerWs {
  bool on = false;
  uint32_t mask = ~0u;  // stages bracketed while profiling (sfm_profile_stages)
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> pending;
  std::vector<hipEvent_t> pool;
  double ms[SFM_PROF_STAGES] = {0};
  int64_t launches[SFM_PROF_STAGES] = {0};
  DevBuf spans;
  int64_t span_cap = 0, span_n = 0, span_dropped = 0;
  std::vector<int32_t> span_level;
  ~ProfilerWs() {  // (not copyable: DevBuf)
    spans.release();
    for (auto& e : pending) {
      (void)hipEventDestroy(e.second.first);
      (void)hipEventDestroy(e.second.second);
    }
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
  }
};

struct ExtractWs {
  DevBuf gauss;                     // the Harris launches' tap buffer (written at creation)
  DevBuf buf[sfm::kExtractBufs];    // sized and addressed by extract_layout()
  DevBuf xy, desc, conf, count;     // sfm_extract's one-slot table
  int64_t extractions = 0;          // extract_impl calls (SFMFEAT_SKIP leaves the first one whole)
  int last_B = 0, last_H = 0, last_W = 0;  // shape of the last extraction (sfm_debug_*)
  uint32_t last_mapped = 0;         // bit l: level l's Harris launch of that extraction wrote a block-maximum map
};

// The matcher's per-descriptor operands and the one record of what they hold.  Every write of
// these buffers goes through operands_claim (api_match.hip), so: a write for another table
// re-points the record at it, a reallocation does too, and after either nothing left over
// from the earlier table counts as valid.
struct MatchOperandsWs {
  DevBuf hi, lo, norm2, rnorm, imgmax;  // MFMA path (kernels.h MatchOperands)
  DevBuf descT;                         // SFMFEAT_MATCH_DIRECT: transposed descriptors
  // the table the buffers currently describe
  const float* desc = nullptr;
  const int32_t* count = nullptr;
  int64_t cap = -1;
  int fused_B = 0;     // leading slots the last extraction wrote itself (sfm_ctx_set_fused_prep)
  int prep_nimg = -1;  // table size of the preps since the record last moved; -1: none, a
                       // prepped match call is SFM_ESTATE
};

struct MatchWs {
  MatchOperandsWs ops;
  DevBuf rows, ovf, ovfc, cand, candn, candt, cands, work, units;   // per pair, bounded by `budget`
  DevBuf h_desc, h_count, h_pairs, h_matches, h_conf, h_nmatch;  // sfm_match's two-slot table
  bool fused_prep = false;
  bool direct = false;  // SFMFEAT_MATCH_DIRECT=1: all-pairs exact VALU kernel (A/B checks)
  // SFMFEAT_MATCH_BUDGET_MB: per-pair workspace bound (4 GiB: 1,575 pairs of 2,500 rows per
  // sub-launch at 256 admitted targets per row, configs[2]'s 4,096-pair calls in three)
  size_t budget = (size_t)4096 << 20;
  int64_t calls = 0;  // match sub-launches (SFMFEAT_SKIP leaves the first one whole)
  // the last match call: pairs, capacity and sub-launches (sfm_debug_match_windows)
  int last_P = 0, last_subs = 0;
  int64_t last_cap = 0;
};

// ingest (sfm_ingest_rgb*): resample tables for the cached (W -> W2, H -> H2) and the RGB temp
// of the horizontal pass; host staging for the host-pointer variant
struct IngestWs {
  DevBuf tab_h, tab_v, tmp, rgb, gray;
  DevBuf colmap, sets;  // row path (k_rows_h): column map + tap sets
  int w = -1, w2 = -1, h = -1, h2 = -1, ksh = 0, ksv = 0, nsets = 0;
  bool rows = false;
  std::vector<int32_t> th, tv;  // host copies of the tables
};

// RANSAC (sfm_ransac_*): sample-index streams cached per (n, iterations), device buffers
struct RansacWs {
  std::vector<std::pair<std::pair<int, int>, std::vector<int32_t>>> cache;
  DevBuf idx, off, F, counts, pts, npts, out, on, oit;
  int64_t last_entries = 0;  // P * iters of the last call (sfm_debug_ransac_fits)
};

// Pose (sfm_ransac_camera_motion*, sfm_triangulate_dev): per-pair intrinsics and base pose,
// per-sample candidates (R1, R2, T) and the valid candidate's index, the winners' (R, t);
// the sample streams, F and counts are RansacWs's
struct PoseWs {
  DevBuf K, base, cand, cand_idx, Rt, tri;
  int64_t last_entries = 0;  // P * iters of the last call (sfm_debug_pose_candidates)
};

// Structure (sfm_link_points_dev): each query's kept target or -1, kept queries per workgroup
struct StructWs {
  DevBuf best, block_kept;
};

// Registry (sfm_registry_add_dev): per-(point, split) partials against the old registry and
// against the call's own points, each point's old hit, its resolution and the contested list.
// The table and its count are the caller's.
struct RegistryWs {
  DevBuf part_d, part_j, self_d, old_d, old_j, res, clist;
};

// PnP (sfm_pnp_ransac_dev, sfm_pnp_dev): the device copy of one sample stream and the (n,
// iterations) it belongs to, per-sample hypotheses (R, t) and counts, the start pose of the
// refinement.  One call at a time per context, like StructWs.
struct PnpWs {
  DevBuf idx, hyp, counts, Rt;
  int idx_n = -1, idx_iters = -1, idx_stride = 0;
  // sfm_debug_pnp_fits: -1 before the first call, the samples that ran in the last
  // sfm_pnp_ransac_dev (its iters; 0 when n < 6), 0 after sfm_pnp_dev
  int64_t last_entries = -1;
};

// Bundle adjustment (sfm_bundle_adjust_dev): everything kernels.h BaProblem points at between
// its inputs and its outputs.  One call at a time per context.
struct BaWs {
  DevBuf st, Rt, Xs, cam_i, pt_cnt, pt_off, pt_list, pos, lin, e2, pts, lcam, Wm, Y, S, Spart, vec, nrm;
};

// Feature tracks (sfm_build_tracks_dev): per node parent, size, class and track id, the tracks'
// nodes in fill order, the (root, slot) hash table and the scans' per-tile sums (tracks.h
// TracksProblem).  One call at a time per context.
struct TracksWs {
  DevBuf parent, size, state, tid, tmp, hash, bsum;
};

// Resection from tracks (sfm_resect_tracks_dev): kernels.h ResectProblem's workspace members.
// Growing these is the call's only allocation.  One call at a time per context.
struct ResectWs {
  DevBuf Xl, xl, lrow, inl, n_links, go, n_inl, Rt0, hyp, counts;
};

struct sfm_ctx {
  CtxStreams s;  // (first: outlives the workspaces below)
  int device = 0;
  sfm_gate* gate = nullptr;
  sfm_params p;
  std::string err;
  int L = 1;
  int kcap = 0;     // per-level keypoint capacity = int(k / L) (ScaleRotInvSIFT.py:90)
  int64_t cap = 0;  // per-image capacity = L * kcap
  float gauss[SFM_MAX_GAUSS * SFM_MAX_GAUSS];
  bool exact_select = false;  // SFMFEAT_SELECT=exact
  bool serial = false;        // SFMFEAT_SERIAL=1: no aux-stream overlap (diagnostic timings)
  ProfilerWs prof;
  ExtractWs ex;
  MatchWs match;
  IngestWs ingest;
  RansacWs ransac;
  PoseWs pose;
  StructWs structure;
  RegistryWs registry;
  PnpWs pnp;
  BaWs ba;
  TracksWs tracks;
  ResectWs resect;
  // the workspaces free their buffers after this body, the streams and events go last
  ~sfm_ctx() {
    (void)hipSetDevice(device);
    if (s.stream) (void)hipStreamSynchronize(s.stream);
  }
};

inline int set_err(sfm_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

#define HIPCHK(ctx, expr)                                                              \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return set_err(ctx, SFM_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

inline int ensure(sfm_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (b.bytes >= bytes) return SFM_OK;
  b.release();
  HIPCHK(c, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return SFM_OK;
}

template <class T>
T* as(DevBuf& b) {
  return reinterpret_cast<T*>(b.p);
}

// the stream of the host-pointer calls, created on first use
inline int host_stream(sfm_ctx* c, hipStream_t* out) {
  if (!c->s.stream) HIPCHK(c, hipStreamCreateWithPriority(&c->s.stream, hipStreamNonBlocking, c->s.prio));
  *out = c->s.stream;
  return SFM_OK;
}

// RAII bracket: records a start event now and a stop event at scope exit (when enabled).
struct StageScope {
  ProfilerWs& pr;
  int stage;
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  static hipEvent_t event(ProfilerWs& pr) {
    hipEvent_t e = nullptr;
    if (pr.pool.empty()) {
      (void)hipEventCreate(&e);
    } else {
      e = pr.pool.back();
      pr.pool.pop_back();
    }
    return e;
  }
  StageScope(sfm_ctx* c, int stage_, hipStream_t st_) : pr(c->prof), stage(stage_), st(st_) {
    if (pr.on && ((pr.mask >> stage) & 1u)) {
      a = event(pr);
      b = event(pr);
      (void)hipEventRecord(a, st);
    }
  }
  ~StageScope() {
    if (a) {
      (void)hipEventRecord(b, st);
      pr.pending.push_back({stage, {a, b}});
    }
  }
};

// Per-process switches of the extraction, read once at the first use.
struct ExtractSwitches {
  sfm::LayoutSwitches layout;  // SFMFEAT_PYR_FUSED, SFMFEAT_EXACT_PX, SFMFEAT_SELECT_MERGE
  bool fill_launches;          // SFMFEAT_FILL_LAUNCHES=1: separate fills (A/B)
  int harris_group;            // SFMFEAT_HARRIS_GROUP=g: levels >= g share Harris launches
  int gate_level;              // SFMFEAT_GATE_LEVEL: the lane gate's release point
  bool select_caller;          // SFMFEAT_SELECT_CALLER=1: aux levels select on the caller's stream
  int skip;                    // SFMFEAT_SKIP=mask (timing bounds only, results wrong by design)
};
const ExtractSwitches& extract_switches();  // api_extract.hip
// the layout switches with the tests' override of SFMFEAT_NMS_BLOCKS applied (-1: the size rule,
// 0 / 1 / n >= 2 as the switch; below -1: no override)
sfm::LayoutSwitches extract_layout_switches();
void extract_set_nms_blocks(int mode);

// api_extract.hip
int extract_reserve(sfm_ctx* c, int B, int H, int W);
int extract_impl(sfm_ctx* c, const float* imgs, int B, int H, int W, int32_t* xy, float* desc, float* conf,
                 int32_t* count, int64_t cap, hipStream_t st);

// api_stage1.hip: the cached [iters][8] sample stream of (n >= 8, iters) (RansacWs::cache; valid
// until the next call that touches the cache)
const std::vector<int32_t>& ransac_stream(sfm_ctx* c, int n, int iters);

// api_match.hip: the extraction's side of the operand owner record (MatchOperandsWs).
// begin: with fused prep on, an extraction is about to write the operands of slots [0, B) of
// the table (desc, count, cap): buffers for them plus spare slots, the record on that table
// with nothing valid yet, *mo filled in (left as it is, "not written", with fused prep off).
// commit: every level's descriptor launch wrote its operands.  clear: no slot is fused.
int operands_fused_begin(sfm_ctx* c, const float* desc, const int32_t* count, int64_t cap, int B,
                         sfm::MatchOperands* mo);
void operands_fused_commit(sfm_ctx* c, int B);
void operands_fused_clear(sfm_ctx* c);
