// kernels.h — launcher declarations and the per-plane bookkeeping shared between the
// host orchestration (api_*.hip) and the gfx950 kernels.
//
// A "plane" is one pyramid level of one image.  All B planes of a level are stored
// contiguously ([B][h][w]) and are processed by one launch per stage.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "common.h"

namespace sfm {

#define SFM_NMS_MAX_HALF 15                 // ksize <= 31

constexpr int kHistBits = 12;               // first radix digit of the median select
constexpr int kHistBins = 1 << kHistBits;   // 4096: generic LDS histogram for <= 12-bit digits
constexpr int kMedBits1 = 11;               // median digit 1 (histogrammed inside Harris)
constexpr int kMedBins1 = 1 << kMedBits1;   // 2048 (digits 2 / 3 are 11 / 10 bits)
constexpr int kTopkLdsCap = 8192;           // max keys sorted in LDS by the top-k kernel
constexpr int kMaxMatchRows = 16384;        // max keypoints per image for the matcher sort
constexpr int kMatchCandCap = 256;          // admitted targets per query row (MFMA matcher lists)
constexpr int kCounterStride = 32;          // u64 per per-plane atomic counter (own 256-B line)
// the sweep's work units (k_match_units) encode pair | block << kMatchUnitPairBits: one
// matcher sub-launch takes at most 2^kMatchUnitPairBits pairs (match_impl clamps)
constexpr int kMatchUnitPairBits = 20;

// The matcher's per-descriptor operands (match_mfma.hip): split-f16 copies hi = f16(v * 2^8),
// lo = f16((v * 2^8 - hi) * 2^11), the squared norm float(sum v^2 in double) and the norm,
// [img][capP] rows (capP = cap rounded up to 128; padding rows: norm2 = +inf, hi = lo = 0),
// and per 16-row block the maxima of (norm2, norm) over the valid rows.  k_match_prep writes
// them from a slot table; an extraction with fused operands (sfm_ctx_set_fused_prep) has the
// descriptor kernel write them for every row it produces.
constexpr float kMatchScale = 256.0f;   // operand pre-scale (2^8)
constexpr float kMatchLoScale = 2048.0f;  // lo part scale (2^11)
constexpr int kPrepRows = 16;           // rows per (norm2, norm) maxima block
struct MatchOperands {
  _Float16* hi;    // nullptr: not written
  _Float16* lo;
  float* norm2;
  float* rnorm;
  float2* pmax;    // [img][capP / kPrepRows], zeroed by the extraction before its levels
  int64_t capP;
};

// Per-plane state of the keypoint selection (NaiveSIFT.py:90-120).
//
// Certified select (default): the reference keeps R == window max && R >= median, then the
// k largest.  NMS collects the window maxima with key >= tnms (a volume threshold: about
// vmin pixels lie above it).  If at least k were found and the k-th largest has key >=
// tcert (the first key above the median's digit-1 bucket), all of the top k are >= the
// median and every reference candidate outranking the k-th was found: the top k equal
// the reference's whatever the exact median is — so the median is only bounded, from the
// Harris histogram.  Other planes (and forced exact mode) set `fallback` and run the
// exact path: np.median by radix select, then the full NMS predicate.
struct MedianState {
  uint32_t bucket[2];   // digit-1 (top 11 bits) bucket holding rank k1 / k2
  uint32_t rank[2];     // residual rank inside that bucket
  uint32_t odd;         // H*W odd -> median is element k1 alone
  float median;         // exact median (fallback planes only)
  uint32_t tnms;        // certified select: candidate threshold key
  uint32_t tcert;       // certified select: the k-th key must reach this
  uint32_t fallback;    // 1: this plane takes the exact path
  // higher candidate thresholds (>= tnms): the buckets holding the 3 vmin / 8-th and
  // vmin / 2-th largest values.  k_select first tries the candidates at or above them (a
  // subset of about 2k-4k at vmin = 128 k, sorted whole), the full list when they are too few.
  uint32_t tsub[2];
};

// Buckets from 2^126 up (and inf / NaN) never certify: (lo + hi) / 2 could overflow.
constexpr uint32_t kHugeBucket = 0x7F4u;

// Per-plane select scan (median.hip k_med_scan; fused into the Harris kernel's last
// workgroup of each plane): from the digit-1 histogram, the buckets holding the two
// middle ranks (exact-median state) and the certified-select thresholds.  Needs 256 or
// 512 threads (8 bins each for the first 256, one prefix pass for all five ranks); s_red
// holds 10 u32.
// `hist` is read with agent-scope atomic loads so a fused caller sees every workgroup's
// flush (L2 is per XCD); the 8 loads per thread are issued together.
SFM_DEV void select_scan_plane(const uint32_t* hist, MedianState* st, unsigned long long* list_count,
                               int64_t n, int64_t vmin, int force_exact, uint32_t* s_red) {
  static_assert(kMedBins1 == 256 * 8, "select scan: 8 bins per thread");
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool act = tid < 256;  // a 512-thread caller: the upper half holds no bins
  uint32_t v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    v[j] = act ? __hip_atomic_load(hist + 8 * tid + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
  uint32_t local = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) local += v[j];
  uint32_t x = local;  // inclusive scan within the wave
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(x, off);
    if (lane >= off) x += y;
  }
  if (lane == 63) s_red[wid] = x;
  __syncthreads();
  uint32_t wbase = 0;
  for (int w = 0; w < wid; ++w) wbase += s_red[w];
  const uint32_t excl = wbase + x - local;  // values in bins below this thread's first bin
  __syncthreads();
  const uint32_t k1 = (n % 2 == 1) ? (uint32_t)(n / 2) : (uint32_t)(n / 2 - 1);
  const uint32_t k2 = (uint32_t)(n / 2);
  const uint32_t kv = n > vmin ? (uint32_t)(n - vmin) : 0u;  // vmin-th largest value
  const int64_t vs0 = 3 * vmin / 8, vs1 = vmin / 2;          // the subset thresholds' ranks
  const uint32_t ks0 = n > vs0 ? (uint32_t)(n - vs0) : 0u, ks1 = n > vs1 ? (uint32_t)(n - vs1) : 0u;
  const uint32_t ranks[5] = {k1, k2, kv, ks0, ks1};
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const uint32_t r = ranks[q];
    if (r >= excl && r < excl + local) {  // exactly one thread owns each rank
      uint32_t c = excl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (r >= c && r < c + v[j]) {
          s_red[2 * q] = (uint32_t)(8 * tid + j);
          s_red[2 * q + 1] = r - c;  // residual rank inside the bucket
        }
        c += v[j];
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    const uint32_t b1 = s_red[0], r1 = s_red[1], b2 = s_red[2], r2 = s_red[3];
    // candidate threshold: the bucket holding the vmin-th largest value (so >= vmin values
    // lie at or above it), at least the median's lower bucket b1 (nothing below certifies)
    const uint32_t tb = max(n > vmin ? s_red[4] : 0u, b1);
    const bool certifiable = !force_exact && b2 < kHugeBucket;
    st->tnms = tb << (32 - kMedBits1);
    st->tsub[0] = max(n > vs0 ? s_red[6] : 0u, tb) << (32 - kMedBits1);
    st->tsub[1] = max(n > vs1 ? s_red[8] : 0u, tb) << (32 - kMedBits1);
    st->tcert = certifiable ? (b2 + 1) << (32 - kMedBits1) : 0xffffffffu;
    st->fallback = certifiable ? 0u : 1u;
    st->bucket[0] = b1;
    st->bucket[1] = b2;
    st->rank[0] = r1;
    st->rank[1] = r2;
    st->odd = (uint32_t)(n % 2);
    *list_count = 0ull;
  }
}

// Resolve one rank within bucket `bk` (the key's top 11 bits) from a collected list of keys
// (exact median, digits 2 and 3; every thread of the block calls it).
SFM_DEV uint32_t select_in_list(const uint32_t* lp, int64_t m, uint32_t bk, uint32_t rank,
                                uint32_t* s_h, uint32_t* s_scan, uint32_t* s_out) {
  const int tid = threadIdx.x, nt = blockDim.x;
  // digit 2: bits [20:10]
  for (int i = tid; i < kHistBins; i += nt) s_h[i] = 0u;
  __syncthreads();
  for (int64_t i = tid; i < m; i += nt) {
    uint32_t k = lp[i];
    if ((k >> 21) == bk) atomicAdd(&s_h[(k >> 10) & 0x7ffu], 1u);
  }
  __syncthreads();
  find_bin(s_h, kHistBins, rank, s_scan, s_out);
  uint32_t d2 = s_out[0];
  rank -= s_out[1];
  uint32_t pre = (bk << 11) | d2;  // top 22 bits
  __syncthreads();
  // digit 3: bits [9:0] (histogram padded to 4096 bins for find_bin)
  for (int i = tid; i < kHistBins; i += nt) s_h[i] = 0u;
  __syncthreads();
  for (int64_t i = tid; i < m; i += nt) {
    uint32_t k = lp[i];
    if ((k >> 10) == pre) atomicAdd(&s_h[k & 0x3ffu], 1u);
  }
  __syncthreads();
  find_bin(s_h, kHistBins, rank, s_scan, s_out);
  uint32_t d3 = s_out[0];
  __syncthreads();
  return (pre << 10) | d3;
}

// Arguments of the select scan fused into the Harris launch (state == nullptr: not fused).
struct SelectScan {
  MedianState* state;                  // [B]
  unsigned long long* list_count;      // [B], stride kCounterStride
  unsigned long long* done;            // [B], stride kCounterStride: workgroup arrivals (zeroed)
  int64_t vmin;
  int force_exact;
};

// Per-plane keypoint list produced by the top-k kernel (level coordinates).
struct KpList {
  int32_t* x;      // [planes][kcap]
  int32_t* y;
  float* conf;
  int32_t* count;  // [planes]
};

// pyramid.hip
void launch_u8_to_f32(const uint8_t* src, float* dst, int64_t n, hipStream_t st);

// ransac.hip: CameraPose.find_inliers (SFM.py:126-160) for P correspondence sets
// pts [P][nmax][4] int32 (x1, y1, x2, y2), sample indices idx (+ idx_off[p]) [iters][8].
void ransac_sample_indices(int n, int iters, uint32_t seed, int32_t* out);
void ransac_sample_indices_k(int n, int iters, uint32_t seed, int size, int32_t* out);  // [iters][size]
void launch_ransac(const int32_t* pts, const int32_t* npts, int nmax, int P, const int32_t* idx,
                   const int32_t* idx_off, int iters, double thr, double* Fs, int32_t* counts, int32_t* out_pts,
                   int32_t* out_n, int32_t* out_iter, hipStream_t st);
constexpr int kRansacChunk = 2560;  // points staged in LDS at a time (32 B each)

// verify.hip: sfm_verify_matches_dev (include/sfmfeat.h has the rule).  The stop table goes to
// the kernel by value, so the call reads no host memory after it returns.
constexpr int kVerifyRound = 256;   // samples per round: part of the rule
constexpr int kVerifyMaxStop = 64;  // rounds that can carry a stop ratio
constexpr int kVerifyMaxIters = 1 << 20;
struct VerifyStop {
  double ratio[kVerifyMaxStop];
  int n;
};
void launch_verify(const int32_t* xy, const int32_t* count, int nimg, int64_t cap, const int32_t* pairs, int P,
                   const int32_t* matches, const int32_t* nmatch, int iters, double thr, int min_inliers,
                   uint64_t seed, const VerifyStop& stop, uint8_t* keep, double* F, int32_t* stat, hipStream_t st);

// twoview.hip: sfm_homography_matches_dev and sfm_two_view_pose_dev (include/sfmfeat.h has the
// rules).  The homography RANSAC shares verify's rounds and stop table; its sample stream is
// verify's with this constant xor-ed into the seed ("Homograp" in ASCII), so the two never draw
// the same numbers for one (seed, a, b).
constexpr uint64_t kHomographySeedXor = 0x486F6D6F67726170ull;
void launch_homography(const int32_t* xy, const int32_t* count, int nimg, int64_t cap, const int32_t* pairs, int P,
                       const int32_t* matches, const int32_t* nmatch, const int32_t* attempt, int iters, double thr,
                       uint64_t seed, const VerifyStop& stop, double* H, uint8_t* hkeep, int32_t* hstat,
                       hipStream_t st);
void launch_two_view_pose(const int32_t* xy, const int32_t* count, int nimg, int64_t cap, const int32_t* pairs, int P,
                          const int32_t* matches, const int32_t* nmatch, const uint8_t* keep, const double* F,
                          const double* K, const int32_t* attempt, double cos2_min, double* pose, int32_t* pstat,
                          hipStream_t st);

// resect.hip: sfm_resect_tracks_dev (include/sfmfeat.h has the rule).  The sample stream is
// verify's construction at sample size 6 with this constant xor-ed into the seed ("Resectio" in
// ASCII) and the slot alone in the key.  Inputs and outputs as the C call names them; the rest is
// workspace (api_resect.hip sizes it): Xl [nimg][cap][3], xl [nimg][cap][2] and lrow [nimg][cap]
// the links of each slot in ascending row order, inl [nimg][cap] the winner's inliers as link
// numbers, n_links, go (attempted), n_inl [nimg], Rt0 [nimg][12] the winning hypothesis,
// hyp [nimg][iters][12] and counts [nimg][iters] (the caller's tables when it passes them).
constexpr uint64_t kResectSeedXor = 0x526573656374696Full;
struct ResectProblem {
  const int32_t* xy;
  const int32_t* count;
  const int32_t* node_track;
  const double* X;
  const double* K;
  const uint8_t* attempt;
  int nimg, cap, n_tracks, iters, min_inliers, max_refine_iter;
  double thr;
  uint64_t seed;
  double* pose;
  int32_t* rstat;
  double* rcost;
  uint8_t* rkeep;
  int32_t* out_counts;
  double* out_hyp;
  double *Xl, *xl, *hyp, *Rt0;
  int32_t *lrow, *inl, *n_links, *go, *n_inl, *counts;
};
void launch_resect_tracks(const ResectProblem& q, hipStream_t st);

// pose.hip: CameraPose.ransac_camera_motion (SFM.py:38-124) on top of the RANSAC launches, and
// triangulate_point / triangulate_points (SFM.py:239-253, 292-305).  Kc [P][2][9] (K1, K2),
// base [P][12] (R_base, T_base), cand [P][iters][21] (R1, R2, T), cand_idx [P][iters] (the
// valid candidate of each sample or -1), out_Rt [P][12]; all device, row-major float64.
void launch_ransac_pose(const int32_t* pts, const int32_t* npts, int nmax, int P, const int32_t* idx,
                        const int32_t* idx_off, int iters, double thr, const double* Kc, const double* base,
                        double* Fs, int32_t* counts, double* cand, int32_t* cand_idx, int32_t* out_pts,
                        int32_t* out_n, int32_t* out_iter, double* out_Rt, hipStream_t st);  // ransac.hip
void launch_pose_candidates(const double* Fs, const int32_t* npts, const double* Kc, int P, int iters,
                            double* cand, hipStream_t st);
void launch_pose_cheirality(const int32_t* pts, const int32_t* npts, int nmax, int P, const double* Kc,
                            const double* base, const double* cand, int iters, int32_t* counts,
                            int32_t* cand_idx, hipStream_t st);
void launch_pose_gather(const int32_t* out_iter, const double* cand, const int32_t* cand_idx, int P, int iters,
                        double* out_Rt, hipStream_t st);
// x1, x2 [N][2], P1, P2 [12], X [N][3]; normalize: Hartley transforms computed on the device
// (scratch30: 30 doubles of workspace)
void launch_triangulate(const double* x1, const double* x2, int64_t N, const double* P1, const double* P2,
                        bool normalize, double* scratch30, double* X, hipStream_t st);

// refine.hip: the structure stage.  launch_refine_points:
// CameraPose.non_linear_triangulation (SFM.py:255-289) as one Levenberg-Marquardt per point;
// X0, X [N][3], x1, x2 [N][2], P [S][2][12] camera pairs, seg [N] (nullptr: pair 0; clamped to
// [0, S)), cost [N] the final sum of squared residuals, iters [N] accepted steps | status <<
// kRefineStatusShift.  X may be X0.
constexpr int kRefineStatusShift = 24;
constexpr int kRefineConverged = 0;  // an accepted step with |d| <= 1e-14 |X|
constexpr int kRefineLambda = 1;     // lambda grew beyond 1e12
constexpr int kRefineNonFinite = 2;  // initial cost not finite: the point is returned unchanged
constexpr int kRefineMaxIter = 3;    // max_iter iterations ran
void launch_refine_points(const double* X0, const double* x1, const double* x2, int64_t N, const double* P, int S,
                          const int32_t* seg, int max_iter, double* X, double* cost, int32_t* iters,
                          hipStream_t st);
// Util.print_reprojection_error (Util.py:65-82): err [N][2] and the mean of (e1 + e2) / 2 (NaN
// for N == 0), the same bits every run
void launch_reproj_error(const double* X, const double* x1, const double* x2, int64_t N, const double* P1,
                         const double* P2, double* err, double* mean, hipStream_t st);
// the 2D -> 3D association of Runner.py:241-250: tgt [m][2], qry [nq][2] int32 (|coordinate| <=
// 2^30); out_tgt / out_qry [nq]: the kept (first nearest target, query) pairs in query order,
// out_n their number; best [nq] and block_kept [link_blocks(nq)] are workspace
constexpr int kLinkThreads = 256;
int link_blocks(int nq);
void launch_link_points(const int32_t* tgt, int m, const int32_t* qry, int nq, double threshold, int32_t* best,
                        int32_t* block_kept, int32_t* out_tgt, int32_t* out_qry, int32_t* out_n, hipStream_t st);

// pnp.hip: the pose of a frame from its 2D-3D links.  X [n][3], x [n][2], K [9]
// (upper triangular), idx [iters][stride] sample indices (the first 6 of a row are used).
// launch_pnp_ransac: hypotheses, counts, selection and refinement; hyp [iters][12], counts
// [iters], Rt [12] are workspace (counts may be the caller's table), out_status [4] = found,
// LM status (kRefine*), accepted steps, iterations run; out_cost [2] = cost at the winning
// hypothesis and at the returned pose.  launch_pnp: the DLT over all points, then the same
// refinement.
void launch_pnp_ransac(const double* X, const double* x, const double* K, int n, const int32_t* idx, int stride,
                       int iters, double thr, int max_refine_iter, double* hyp, int32_t* counts, double* Rt,
                       int32_t* out_inliers, int32_t* out_n, int32_t* out_iter, double* out_R, double* out_t,
                       int32_t* out_status, double* out_cost, hipStream_t st);
void launch_pnp(const double* X, const double* x, const double* K, int n, int max_refine_iter, double* Rt,
                double* out_R, double* out_t, int32_t* out_status, double* out_cost, hipStream_t st);

// registry.hip: the global 3-D point registry (SFMRunner.add_points, Runner.py:361-385;
// DESIGN.md §13C).  reg_xyz [capacity][3] and *reg_count are the caller's device memory,
// pts [n][3]; out_index [n] each point's registry index, out_is_new [n] 1 where it was appended.
// Workspace: part_d / part_j [splits_old][n], self_d [splits_self][n] (registry_span gives the
// splits of `capacity` and of n entries), old_d, old_j, res, clist [n].
constexpr int kRegThreads = 256;     // points per workgroup (one each)
constexpr int kRegChunk = 256;       // registry entries staged in LDS at a time (24 B each); short, so that a
                                     // small registry still spreads over many workgroups
constexpr int kRegMaxSplits = 1024;  // workgroups across the registry (grid.y); longer tables: longer spans
int registry_span(int entries, int* splits);
void launch_registry_add(double* reg_xyz, int32_t* reg_count, int capacity, const double* pts, int n, double thr,
                         double* part_d, int32_t* part_j, double* self_d, double* old_d, int32_t* old_j,
                         int32_t* res, int32_t* clist, int32_t* out_index, int32_t* out_is_new, hipStream_t st);
// SFMRunner.total_reprojection_error (Runner.py:311-334): cam_idx, pt_idx [M] int32 (clamped to
// their tables), obs [M][2], cams [n_cam][6] (Rodrigues vector, t), K [n_cam][9], X [n_pts][3];
// err [M] and their mean (NaN for M == 0), the same bits every run
void launch_total_reproj(const int32_t* cam_idx, const int32_t* pt_idx, const double* obs, int64_t M,
                         const double* cams, int n_cam, const double* K, const double* X, int n_pts, double* err,
                         double* mean, hipStream_t st);

// ba.hip: bundle adjustment (Runner.py:294-306), the library's own Schur-complement
// Levenberg-Marquardt (include/sfmfeat.h sfm_bundle_adjust_dev).  BaState is the
// device-resident LM state; BaProblem the call's inputs, workspace (api_ba.hip sizes it) and
// outputs, passed to every kernel by value.  Status values are kRefine*.
// (include/sfmfeat.h SFM_BA_MAX_*; api_ba.hip asserts they agree)
constexpr int kBaMaxCams = 256;       // the S row of one camera fits in LDS (72 KiB)
constexpr int kBaMaxPoints = 1 << 24;
constexpr int kBaMaxObs = 1 << 26;
constexpr int kBaMaxSplit = 64;                      // segments a camera's list is cut into for the Schur rows
constexpr size_t kBaSchurBudget = (size_t)64 << 20;  // bytes of partial rows (3 segments at 256 cameras)
struct BaState {
  double lam, cost, cost0;
  int32_t cur;       // the slot of Rt / Xs that holds the accepted state
  int32_t done;      // set by k_ba_decide: every later launch of the call returns at once
  int32_t status, accepted, iters, rejected;
  int32_t fail;      // a pivot of V*_j or of S was not positive and finite this iteration
};
struct BaProblem {
  const int32_t* cam_idx;  // [M]
  const int32_t* pt_idx;   // [M]
  const double* obs;       // [M][2]
  int M;
  const double* cams_in;   // [n_cam][6]
  int n_cam;
  const double* K;         // [n_cam][9]
  const double* X_in;      // [n_pts][3]
  int n_pts;
  const uint8_t* cam_fixed;  // [n_cam] or null
  double ftol;
  int max_iter;
  BaState* st;
  double* Rt;              // [2][n_cam][12]: R row-major, t
  double* Xs;              // [2][n_pts][3]
  int32_t *cam_cnt, *cam_off, *cam_list, *cam_active;  // [n_cam], [n_cam + 1], [M], [n_cam]
  int32_t *pt_cnt, *pt_off, *pt_list, *pos;            // [n_pts], [n_pts + 1], [M], [M]
  double* lin;             // [M][20]: r, J_c rows, J_p rows
  double* e2;              // [M] squared residuals of the state being scored
  double *vinv, *gp, *vg;  // [n_pts][6], [n_pts][3], [n_pts][3]
  int32_t* lcam;           // [M] by list position: the camera of a merged W block, or -1
  double *Wm, *Y;          // [M][18] by list position: W_cj and W_cj V*_j^-1 (6 x 3 row-major)
  double *S, *b, *delta;   // [6 n_cam][6 n_cam], [6 n_cam], [6 n_cam]
  double* Spart;           // [n_cam][schur_split][36 n_cam + 6]: each list segment's share of S's rows and of b
  int schur_split;         // ba_schur_split(n_cam)
  double* nrm;             // [n_pts + n_cam][2]
  double* out_cams;        // [n_cam][6]
  double* out_X;           // [n_pts][3]
  double* out_cost;        // [2] or null
  int32_t* out_status;     // [4] or null
};
// M >= 1, 1 <= n_cam <= kBaMaxCams, n_pts >= 1; cam_cnt and pt_cnt zeroed on the stream before
int ba_schur_split(int n_cam);
size_t ba_schur_lds_bytes(int n_cam);
void launch_bundle_adjust(const BaProblem& p, hipStream_t st);

// ingest.hip: PIL BICUBIC resize of [B][H][W][3] u8 RGB to H2 x W2 + /255 + _rgb2gray
// (Runner.py:33-46) -> [B][H2][W2] float32; tmp holds [B][H][W2][3] u8.  Tables from
// build_resample_table (host, Pillow's double-precision taps in 22-bit fixed point).
int build_resample_table(int in, int out, std::vector<int32_t>& tab);
bool ingest_rows_tables(const std::vector<int32_t>& tab_h, int ks_h, int W, int W2, int ks,
                        std::vector<int32_t>& colmap, std::vector<int32_t>& sets);
int ingest_rows_ks(int ks_h, int ks_v);
void launch_ingest_rgb(const uint8_t* rgb, uint8_t* tmp, float* gray, const int32_t* tab_h, int ks_h,
                       const int32_t* tab_v, int ks_v, const int32_t* colmap, const int32_t* sets, int nsets,
                       int B, int H, int W, int H2, int W2, hipStream_t st);
// levels l+1..l+3 of exact 2x steps in one pass; false (nothing launched) when the sizes or
// alignments do not allow it
// z0 / z1 (optional, 16-B aligned, multiples of 16 B): buffers the launch zeroes on the side
bool launch_down2x3(const float* src, int sh, int sw, float* d1, float* d2, float* d3, int B, hipStream_t st,
                    void* z0 = nullptr, size_t z0_bytes = 0, void* z1 = nullptr, size_t z1_bytes = 0);
void launch_resize(const float* src, int sh, int sw, float* dst, int dh, int dw, int B,
                   hipStream_t st);

// harris.hip: R map + first median digit histogram (hist zeroed by the caller); with
// scan.state set, the last workgroup of each plane also runs select_scan_plane.
void launch_harris(const float* lvl, float* R, uint32_t* hist, int B, int H, int W,
                   const float* d_gauss, int ks, float alpha, SelectScan scan, hipStream_t st);
// Several pyramid levels of a batch in one Harris launch (workgroups partitioned by
// level; tiles_x / ntiles / wg0 / nwg are filled in by the launcher)
constexpr int kHarrisMaxLevels = 4;
struct HarrisLevels {
  struct Level {
    const float* lvl;
    float* R;
    uint32_t* hist;
    int H, W, tiles_x, ntiles, wg0, nwg;
    SelectScan scan;
    // fused pyramid (64 x 64 tiles, H and W multiples of 8): the three exact 2x levels below
    // this one, written from the image tile in LDS (nullptr: none)
    float* down[3];
    // block-maximum map (64 x 64 tiles, W % 4 == 0): [B][ceil(H / 4)][W / 4], an upper bound of
    // the maximum of R over each 4 x 4 block, for nms.hip's k_nms_blocks (nullptr: not written)
    // Planes bmax_plane_stride(H, W) floats apart; R must be 16-B aligned.
    float* bmax;
    // filled in by the launcher: plane b's map lies at (address of plane b's R >> bmax_shift) +
    // bmax_rel bytes (0: no map) — the kernel's tile loop holds the plane's R pointer and has no
    // SGPRs left for another
    int64_t bmax_rel;
    int bmax_shift;
  } l[kHarrisMaxLevels];
  int n;
  int prio;  // 1: waves raise their issue priority with the tiles they have left (A/B)
  int stagger;  // n > 0: odd workgroups sleep n x 8k cycles before their first tile (A/B)
  // kernel-active span of this launch (sfm_profile_spans; nullptr: off): {earliest workgroup
  // start, latest workgroup end} on the device's constant-rate realtime clock, folded in with
  // one atomic min / max per workgroup (the slot starts at {~0, 0})
  unsigned long long* span;
};
// floats between the block-maximum maps of consecutive planes (each ceil(H / 4) x (W / 4),
// W % 4 == 0): the planes' R lie H W floats apart and the kernel shifts R's address, so the maps
// are packed where H % 4 == 0 and H W / 4 apart otherwise
constexpr int64_t bmax_plane_stride(int H, int W) { return H % 4 == 0 ? (int64_t)H * W / 16 : (int64_t)H * W / 4; }
void launch_harris_levels(const HarrisLevels& g, int B, const float* d_gauss, int ks, float alpha,
                          hipStream_t st);
// true: the launch of these levels takes the 64 x 64 form whether or not a level carries a
// block-maximum map (a map makes it take that form; this asks what it takes without one)
bool harris_tiles_64(const HarrisLevels& g, int B, int ks);
// The Harris launches' tap buffer (d_gauss above): the ks x ks Gaussian taps (row-major) at 0,
// then from float kHarrisPairOff the window's tap pairs (g[d][j], g[d-1][j]) for d = 0..ks,
// j < ks (a missing tap row is 0), which the kernel reads as wave-uniform scalar loads.
constexpr int kHarrisPairOff = 256;
size_t harris_taps_floats(int ks);
void harris_taps_build(const float* g, int ks, float* out);

int64_t match_stamps_copy(uint64_t* out, int64_t cap);
// words of the sweep's work-unit list (k_match_units) for P pairs of up to max_rows rows
size_t match_units_words(int P, int max_rows);
float time_harris_ablation(int abl, const float* lvl, float* R, uint32_t* hist, int B, int H, int W,
                           const float* gk, float alpha, int iters, uint64_t* stamps = nullptr,
                           int64_t stamps_cap = 0);

// median.hip.  launch_select_scan: median buckets + certified threshold per plane
// (vmin = pixels required at or above the threshold).  launch_median_exact: the exact
// median of the planes flagged `fallback`.
void launch_select_scan(const uint32_t* hist, MedianState* state, unsigned long long* list_count, int B,
                        int H, int W, int64_t vmin, int force_exact, hipStream_t st);
void launch_median_exact(const float* R, MedianState* state, uint32_t* list, unsigned long long* list_count,
                         int B, int H, int W, hipStream_t st);

// nms.hip: candidates as 64-bit keys (~fkey(conf) << 32 | raster index), appended per
// plane.  mode 0 (certified planes): R == window max && key(R) >= tnms; mode 1 (fallback
// planes): the exact predicate (R == window max, or R == 0 below the median).
// force_tile: the tiled kernel for the certified 3x3 case too (parity test of both forms)
// bmax: the level's block-maximum map (HarrisLevels::Level::bmax; any upper bound of each 4 x 4
// block's maximum): the certified 3x3 case with W % 4 == 0 then reads only the blocks that can
// hold a candidate (k_nms_blocks); nullptr: every pixel (k_nms_band)
void launch_nms(const float* R, const MedianState* state, uint64_t* cand,
                unsigned long long* cand_count, int B, int H, int W, int ksize, int mode, hipStream_t st,
                int force_tile = 0, const float* bmax = nullptr);
// whether launch_nms takes k_nms_blocks for this call when given a map
bool nms_blocks_shape(int W, int ksize, int mode);

// select.hip: keypoint selection of one level, one workgroup per plane: top-k by (conf
// desc, index asc) of the certified NMS candidates + edge filter (NaiveSIFT.py:99-120);
// planes that do not certify (or are flagged fallback already) run the exact path in the
// same workgroup: exact median into state.median (medlist: n u32 per plane), the full NMS
// predicate into cand (n u64 per plane), then the same top-k.  scratch: n u64 per plane.
void init_topk_attributes();
void init_describe_attributes(size_t max_lds);
// the quad describe kernel's bin-edge key tables on the current device (once per device)
void init_describe_quad_tables();
size_t describe_lds_bytes(int fw, int rotate);
void launch_select(const float* R, uint64_t* cand, const unsigned long long* cand_count, uint32_t* medlist,
                   uint64_t* scratch, KpList kp, int kcap, int k, int B, int H, int W, int ksize, int half_window,
                   MedianState* state, hipStream_t st);
// Several levels' selections in one launch (B workgroups per level, level-major); each
// level brings its own medlist / scratch regions (they must not overlap).
constexpr int kSelectMaxLevels = 4;
struct SelectLevels {
  struct Level {
    const float* R;
    uint64_t* cand;
    const unsigned long long* cand_count;
    uint32_t* medlist;
    uint64_t* scratch;
    KpList kp;
    MedianState* state;
    int H, W, hw;
  } l[kSelectMaxLevels];
  int n;
};
void launch_select_levels(const SelectLevels& g, int kcap, int k, int B, int ksize, hipStream_t st);
// the sizes the selection's branches turn on at this k: keys sorted whole (sel_cap), its floor,
// confidence ties sorted in LDS, keys selected in registers, median-list keys held in LDS
void select_branch_sizes(int k, int32_t out[5]);

// describe_q.hip: four keypoints per wavefront for window widths 2..22 (false: not handled)
// out_count (the last level's launch): also write each slot's keypoint count
bool launch_describe_quad(const float* lvl, int B, int H, int W, int fw, int rotate, KpList kp, int kcap,
                          const int32_t* level_counts_all, int level, double scale, int32_t* out_xy,
                          float* out_desc, float* out_conf, int64_t out_cap, int32_t* out_count, int L,
                          const MatchOperands& mo, hipStream_t st);
// describe.hip: descriptors of one level written into the output slot table; returns true when
// the launch also wrote the slot counts (out_count set and the quad kernel took the level),
// otherwise the caller runs launch_finalize_counts
// mo.hi set: the quad kernel also writes the matcher operands of every row (and, in the last
// level's launch, the padding rows); *operands_written reports whether it did (the
// one-wavefront kernel of widths above 22 does not)
bool launch_describe(const float* lvl, int B, int H, int W, int fw, int rotate, KpList kp,
                     int kcap, const int32_t* level_counts_all, int level, int L, double scale,
                     int32_t* out_xy, float* out_desc, float* out_conf, int64_t out_cap,
                     int32_t* out_count, const MatchOperands& mo, bool* operands_written, hipStream_t st);
void launch_finalize_counts(const int32_t* level_counts_all, int B, int L, int32_t* out_count,
                            hipStream_t st);

// match.hip
struct RowBest {
  int32_t col;   // -1: rejected
  float nndr;
};
// The matcher's arithmetic contract with the reference (match.hip's file head), once for every
// exact kernel.  A row's state is its nearest two squared distances e1 <= e2 and the nearest's
// index j1, ordered by (distance, index); it starts at (INFINITY, 0x7fffffff, INFINITY).
// Candidate (d, j) into the state:
SFM_DEV void top2_update(float d, int j, float& e1, int& j1, float& e2) {
  if (d < e1 || (d == e1 && j < j1)) {
    e2 = e1;
    e1 = d;
    j1 = j;
  } else if (d < e2) {
    e2 = d;
  }
}
// another lane's state (o1, oj, o2) over disjoint candidates into this one's (the step of the
// kernels' xor-shuffle merges)
SFM_DEV void top2_merge(float& e1, int& j1, float& e2, float o1, int oj, float o2) {
  if (o1 < e1 || (o1 == e1 && oj < j1)) {
    e2 = fminf(e1, o2);
    e1 = o1;
    j1 = oj;
  } else {
    e2 = fminf(e2, o1);
  }
}
// the row's result: the roots (sqrt is monotone, so the state is kept on squared distances),
// nndr = d1 / d2 and the ratio test
SFM_DEV RowBest top2_finish(float e1, int j1, float e2, float ratio) {
  RowBest rb;
  rb.col = -1;
  rb.nndr = 0.0f;
  const float d1 = sqrtf(e1), d2 = sqrtf(e2);
  if (d2 > 0.0f) {
    const float nndr = d1 / d2;
    if (nndr <= ratio) { rb.col = j1; rb.nndr = nndr; }
  }
  return rb;
}
void launch_transpose_desc(const float* desc, const int32_t* count, int nimg, int64_t cap,
                           int64_t capP, float* descT, hipStream_t st);
void launch_match_rows(const float* descT, const int32_t* count, int64_t capP, const int32_t* pairs,
                       int P, float ratio, RowBest* rows, int max_rows, hipStream_t st);
void launch_match_compact(const RowBest* rows, const int32_t* count, const int32_t* pairs, int P,
                          int max_rows, int64_t cap, int32_t* matches, float* conf, int32_t* nmatch,
                          int* reset_counter, hipStream_t st);
void init_match_attributes(int max_rows);
// match_mfma.hip: exact matching with the split-fp16 MFMA prefilter
// pmax: per-16-row-block maxima of (norm2, norm) per image, match_pmax_bytes(capP) per image
size_t match_pmax_bytes(int64_t capP);
void launch_match_prep(const float* desc, const int32_t* count, int nimg, int64_t cap, int64_t capP,
                       _Float16* hi, _Float16* lo, float* norm2, float* rnorm, void* pmax, hipStream_t st);
void launch_match_mfma(const float* desc, const int32_t* count, int64_t cap, int64_t capP,
                       const _Float16* hi, const _Float16* lo, const float* norm2, const float* rnorm,
                       const void* pmax, const int32_t* pairs, int P, float ratio,
                       RowBest* rows, int max_rows, uint32_t* cand, int32_t* cand_n, float* cand_thr,
                       uint8_t* cand_skip, uint32_t* work_list, int* ovf_count, int2* ovf_list, int32_t* units,
                       hipStream_t st);

}  // namespace sfm
