/*
 * sfmfeat.h — C-ABI of the MI355X-native feature stage (detect + describe + match)
 * of reesque/SfmFromScratch.
 *
 * This is the drop-in boundary.  Every entry point replaces one reference interface;
 * the citation after each declaration is the reference file:line it stands in for
 * (paths relative to the reference repository root).  Plain C types only: pointers,
 * sizes and a POD parameter struct; no torch / HIP types cross this boundary (HIP
 * streams are passed as opaque `void*`).
 *
 * Error model: every function returns an int status and never aborts.
 *   SFM_OK      0  success
 *   SFM_EINVAL  1  bad argument          -> Python ValueError / AssertionError
 *                                          (Runner.py:29-30, ScaleRotInvSIFT.py:38)
 *   SFM_ESTATE  2  call out of order     -> RuntimeError (NaiveSIFT.py:49-50)
 *   SFM_EDEVICE 3  HIP runtime failure   -> RuntimeError, text via sfm_last_error()
 *   SFM_ERANGE  4  output capacity too small (n_out holds the required size)
 *   SFM_EINDEX  5  matcher with fewer than 2 target descriptors -> IndexError
 *                                          (NNRatioFeatureMatcher.py:41-43)
 *
 * Threading: the reference drives extractor and matcher from 8 Python threads
 * (Runner.py:183-191).  A context is NOT shared between threads; create one context
 * per thread (the Python wrapper keeps a thread-local context).  The library keeps no
 * global mutable state, so distinct contexts are fully re-entrant.
 */
#ifndef SFMFEAT_H_
#define SFMFEAT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFM_OK 0
#define SFM_EINVAL 1
#define SFM_ESTATE 2
#define SFM_EDEVICE 3
#define SFM_ERANGE 4
#define SFM_EINDEX 5

/* Extractor plugin classes (FeatureExtractor/SIFT/NaiveSIFT.py, ScaleRotInvSIFT.py). */
#define SFM_MODE_SCALEROT 0 /* ScaleRotInvSIFT: pyramid + dominant orientation */
#define SFM_MODE_NAIVE 1    /* NaiveSIFT: one level, un-rotated descriptors */

#define SFM_DESC_DIM 128
#define SFM_MAX_GAUSS 15 /* largest gaussian_size accepted */
#define SFM_MAX_KSIZE 31 /* largest NMS ksize accepted */
#define SFM_MAX_FW 64    /* largest feature_width accepted */
#define SFM_MAX_LEVELS 12
#define SFM_BA_MAX_CAMERAS 256              /* sfm_bundle_adjust_dev: n_cam */
#define SFM_BA_MAX_POINTS (1 << 24)          /* n_pts */
#define SFM_BA_MAX_OBSERVATIONS (1 << 26)    /* M */

/*
 * POD mirror of the reference's `extractor_params` dict keys.  Defaults are the
 * reference's `.get(key, default)` values:
 *   num_interest_points 2500  FeatureExtractor.py:11
 *   ksize 7, gaussian_size 7, sigma 5, alpha 0.05, feature_width 16  NaiveSIFT.py:35-39
 *   pyramid_level 4, pyramid_scale_factor 2                          ScaleRotInvSIFT.py:12-13
 * `gauss_kernel` optionally carries the float32 values of
 * NaiveSIFT._generate_gaussian_kernel (NaiveSIFT.py:175-199) computed by the caller
 * (the Python wrapper computes them with numpy exactly as the reference does); when
 * `gauss_kernel_set` is 0 the library computes them itself in double precision.
 */
typedef struct sfm_params {
  int32_t mode;
  int32_t num_interest_points;
  int32_t ksize;
  int32_t gaussian_size;
  int32_t feature_width;
  int32_t pyramid_level;
  double sigma;
  double alpha;
  double pyramid_scale_factor;
  int32_t gauss_kernel_set;
  int32_t reserved0;
  float gauss_kernel[SFM_MAX_GAUSS * SFM_MAX_GAUSS];
} sfm_params;

/* Fill `p` with the reference defaults for `mode`. */
void sfm_params_default(sfm_params* p, int32_t mode);

/* ABI version, bumped on any signature change. */
int32_t sfm_abi_version(void);

/* Build flags of this library: SFM_BUILD_ABLATIONS set only in the diagnostic build
 * (make ABLATIONS=1), whose timing switches (SFMFEAT_SKIP, SFMFEAT_*_ABL, SFMFEAT_NMS_DRY) skip
 * or hollow out work by design; the shipped build reads none of them.  (No reference
 * counterpart: build provenance for bench lines.) */
#define SFM_BUILD_ABLATIONS 1
int32_t sfm_build_flags(void);

/* Maximum number of keypoints one image can produce:
 * ScaleRot: pyramid_level * int(k / pyramid_level)  (ScaleRotInvSIFT.py:90 scaled_k)
 * Naive:    k                                       (NaiveSIFT.py:100-103) */
int64_t sfm_keypoint_capacity(const sfm_params* p);

/* Pyramid level sizes for an H x W image, chained int(w/s), int(h/s)
 * (ScaleRotInvSIFT.py:109-115).  dims receives 2*L ints (h0,w0,h1,w1,...). */
int32_t sfm_pyramid_dims(const sfm_params* p, int32_t H, int32_t W, int32_t* dims);

typedef struct sfm_ctx sfm_ctx;

/* Create a context bound to HIP device `device` with fixed extractor parameters. */
int32_t sfm_ctx_create(int32_t device, const sfm_params* p, sfm_ctx** out);
int32_t sfm_ctx_destroy(sfm_ctx* ctx);
/* Last error text for this context (never NULL). */
const char* sfm_last_error(const sfm_ctx* ctx);

/*
 * Per-image extraction from host memory — replaces the ScaleRotInvSIFT constructor
 * (ScaleRotInvSIFT.py:9-16, all work eager) and NaiveSIFT.detect_keypoints +
 * extract_descriptors (NaiveSIFT.py:42-52), chosen by params.mode.
 *   img: H x W float32 grayscale, row stride `row_stride` elements (>= W)
 *   X, Y: int64 column / row of each keypoint in level-0 pixels
 *         (ScaleRotInvSIFT.py:101-102: (x * s^l).astype(int))
 *   desc: n x 128 float32 RootSIFT descriptors (ScaleRotInvSIFT.py:79-85)
 *   conf: optional, n float32 Harris responses (NaiveSIFT.py:44 `self.confidences`)
 *   cap: capacity of X/Y/desc in keypoints; n_out: keypoints written
 *   level_counts: optional, pyramid_level ints — keypoints contributed per level
 *                 (the Python wrapper uses it to mirror ScaleRotInvSIFT.py:103's
 *                 ragged extend when a level yields exactly one keypoint)
 * Output order is the reference's: level by level, confidence descending.
 */
int32_t sfm_extract(sfm_ctx* ctx, const float* img, int32_t H, int32_t W, int64_t row_stride,
                    int64_t* X, int64_t* Y, float* desc, float* conf, int64_t cap,
                    int64_t* n_out, int32_t* level_counts);

/*
 * Brute-force L2 nearest neighbour with Lowe ratio test — replaces
 * NNRatioFeatureMatcher.match_features_ratio_test (NNRatioFeatureMatcher.py:8-60).
 *   d1: n1 x 128, d2: n2 x 128 float32 (row-major, contiguous)
 *   ratio: threshold, compared in float32 (`nndr <= float32(ratio)`, :49)
 *   matches: k x 2 int64 [row in d1, row in d2]; conf: k float32 nndr
 *   sorted by (conf ascending, row ascending).  cap >= n1 always suffices.
 * Returns SFM_EINDEX when n2 < 2 (the reference raises IndexError at :42).
 *
 * Domain (this call, sfm_match_pairs_dev and sfm_match_pairs_prepped_dev): any finite float32
 * tables whose reference distances sqrt(sum((a - b)^2)) in float32 are all finite — not only
 * unit-norm descriptors.  Results equal the reference on all of them.  The MFMA prefilter
 * covers elements with |x| * 2^8 finite in float16 (|x| < 255.9375); a row holding a larger
 * element, and every query row matched against an image that holds such a row, is computed
 * exactly over all targets instead (slower, same results).  Tables with non-finite elements
 * are unspecified: the reference's own result then depends on its unstable sort.
 */
int32_t sfm_match(sfm_ctx* ctx, const float* d1, int64_t n1, const float* d2, int64_t n2,
                  float ratio, int64_t* matches, float* conf, int64_t cap, int64_t* k_out);

/*
 * Frame ingest of FeatureRunner (Runner.py:33-46): a decoded RGB frame ([H][W][3] uint8,
 * what _load_image reads, Runner.py:551-563) -> PIL BICUBIC resize to W2 x H2
 * (_PIL_resize, Runner.py:37-42,481-493; Pillow's 8-bit fixed-point resampler, bit
 * exact) -> /255 -> _rgb2gray (Runner.py:467-478) -> [H2][W2] float32, the image the
 * extractor classes take.  Host pointers; synchronous.
 */
int32_t sfm_ingest_rgb(sfm_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t H2, int32_t W2,
                       float* gray);

/* (int(H * scale), int(W * scale)) — the PIL target size of Runner.py:37-42. */
int32_t sfm_resize_dims(int32_t H, int32_t W, double scale, int32_t* H2, int32_t* W2);

/*
 * RANSAC inlier filter — replaces CameraPose.find_inliers (SFM.py:126-160), the match
 * consumer of SFMRunner stage 1 (Runner.py:349-351).  p1, p2: n x 2 int64 pixel
 * coordinates (the pairs of _convert_matches_to_coords, Runner.py:423-434); iters =
 * max_iterations; samples replay numpy's legacy RandomState after np.random.seed(5).
 * in1 / in2 (capacity n x 2) receive the winning sample's inliers in input order,
 * n_out their count; n_out = -1 when n < 8 (the reference returns four Nones), 0 when
 * iters == 0 (the reference's empty arrays).  No limit on n.
 * best_iter (optional): the winning sample's index.
 * Each sample's F is the null vector of its normalised 8 x 9 system by Gaussian elimination
 * with partial pivoting: for a rank-8 system the line of the reference's smallest right
 * singular vector (epipolar distances within 1e-6 px of the reference's definition, DESIGN.md
 * section 13).  A sample whose system is exactly rank-deficient (identical frames, a repeated
 * correspondence, a constant coordinate) gets one finite member of its null space: the last
 * column without a pivot set to 1, the other free columns to 0, the pivots back-substituted.
 * The reference's SVD returns another member (LAPACK's choice, not reproduced), so the two may
 * keep different points of such a pair beyond those that every member keeps.  F is NaN, and
 * the sample counts no inlier, only when its eight points coincide in one image (the
 * reference raises there).
 */
int32_t sfm_ransac_find_inliers(sfm_ctx* ctx, const int64_t* p1, const int64_t* p2, int64_t n, int32_t iters,
                                double threshold, int64_t* in1, int64_t* in2, int64_t* n_out,
                                int32_t* best_iter);

/* The sample indices np.random.choice(n, 8, replace=False) draws on each of `iters`
 * iterations after np.random.seed(seed) (numpy legacy MT19937 + Fisher-Yates):
 * out [iters][8] int32.  Host-only. */
int32_t sfm_ransac_sample_indices(int32_t n, int32_t iters, uint32_t seed, int32_t* out);
/* The same stream with `size` indices kept per iteration, np.random.choice(n, size,
 * replace=False): out [iters][size] int32; size 8 is sfm_ransac_sample_indices.  numpy's legacy
 * choice without replacement is permutation(n)[:size], so the draws consumed per iteration do
 * not depend on size.  SFM_EINVAL: size < 1, n < size, iters < 0, out null.  Host-only. */
int32_t sfm_ransac_sample_indices_k(int32_t n, int32_t iters, uint32_t seed, int32_t size, int32_t* out);

/* ---------------- device-resident batch API (throughput path) ----------------
 * All pointers are device pointers on the context's device; `stream` is the
 * hipStream_t the work is enqueued on, exactly as given (NULL = HIP's null stream, as
 * in the HIP API — so a caller on PyTorch's default stream passes its handle, 0, and
 * stays ordered with its own work).  The calls are asynchronous with respect to the
 * host: results are valid once the stream has been synchronised.
 * Workspace is owned by the context; call sfm_reserve() once with the largest batch
 * so that the batch calls perform no device allocation (hipGraph-capturable).
 *
 * Slot table layout (also the RCCL all-gather unit):
 *   xy    [B][cap][2] int32   (X, Y) level-0 pixel coordinates
 *   desc  [B][cap][128] float32
 *   count [B] int32
 */
int32_t sfm_reserve(sfm_ctx* ctx, int32_t B, int32_t H, int32_t W);

/* sfm_ransac_find_inliers for P pairs at once: pts [P][nmax][4] int32 (x1, y1, x2, y2),
 * npts [P] on the device and npts_host [P] on the host (the sample streams depend on n);
 * out_pts [P][nmax][4] inliers in order, out_n [P] (-1 for n < 8, 0 when iters == 0),
 * out_iter [P] (-1 when no sample won).  Any nmax (the points are staged through LDS in
 * chunks).  Synchronises the stream before returning. */
int32_t sfm_ransac_find_inliers_dev(sfm_ctx* ctx, const int32_t* pts, const int32_t* npts,
                                    const int32_t* npts_host, int32_t P, int32_t nmax, int32_t iters,
                                    double threshold, int32_t* out_pts, int32_t* out_n, int32_t* out_iter,
                                    void* stream);

/* CameraPose.ransac_camera_motion (SFM.py:38-103), the initial pair's own RANSAC
 * (Runner.py:202-208, :349-351), for P correspondence sets at once.
 * pts/npts/npts_host/nmax/iters/threshold/out_pts/out_n/out_iter as sfm_ransac_find_inliers_dev;
 * K [P][2][9] (K1, K2 row-major), base [P][12] (R_base row-major, then T_base), host doubles;
 * out_R [P][9], out_t [P][3] host doubles (untouched where out_iter = -1).
 * out_n: -1 for n < 8 (four Nones), 0 when no sample had both a valid pose
 * (_check_valid_pose, SFM.py:105-124) and an inlier.  Synchronises the stream. */
int32_t sfm_ransac_camera_motion_dev(sfm_ctx* ctx, const int32_t* pts, const int32_t* npts,
                                     const int32_t* npts_host, int32_t P, int32_t nmax, int32_t iters,
                                     double threshold, const double* K, const double* base, int32_t* out_pts,
                                     int32_t* out_n, int32_t* out_iter, double* out_R, double* out_t,
                                     void* stream);

/* The same for one pair through host pointers: p1, p2 n x 2 int64, K1, K2, R_base [9]
 * row-major, T_base [3]; R [9], t [3] written when *n_out > 0; in1, in2, n_out, best_iter as
 * sfm_ransac_find_inliers (n_out -1 for n < 8, 0 when nothing won). */
int32_t sfm_ransac_camera_motion(sfm_ctx* ctx, const int64_t* p1, const int64_t* p2, int64_t n,
                                 const double* K1, const double* K2, const double* R_base,
                                 const double* T_base, int32_t iters, double threshold, double* R, double* t,
                                 int64_t* in1, int64_t* in2, int64_t* n_out, int32_t* best_iter);

/* CameraPose.triangulate_point (SFM.py:239-253) over N points (Runner.py:208, :278), or
 * CameraPose.triangulate_points (SFM.py:292-305) with normalize = 1 (the Hartley transforms of
 * both sets computed on the device).  Device pointers: x1, x2 [N][2], P1, P2 [12] row-major
 * 3 x 4, X [N][3], all float64.  Enqueued on `stream`, not synchronised. */
int32_t sfm_triangulate_dev(sfm_ctx* ctx, const double* x1, const double* x2, int64_t N, const double* P1,
                            const double* P2, int32_t normalize, double* X, void* stream);

/* ---- the structure stage: what SFMRunner.perform does with the triangulated points ----
 * Device pointers, float64 unless said otherwise; enqueued on `stream`, not synchronised.
 * Argument errors (null pointers, negative sizes, S < 1, max_iter < 1) return SFM_EINVAL with a
 * message in sfm_last_error. */

/* CameraPose.non_linear_triangulation (SFM.py:255-289; Runner.py:209, :279).  The reference's
 * joint least-squares problem over all 3N coordinates is a sum of per-point terms, so each
 * point is refined on its own: Levenberg-Marquardt on the four residuals of SFM.py:262-273
 * with the analytic Jacobian, lambda from 1e-3, / 10 (floor 1e-12) after an accepted step
 * (strictly smaller cost), * 10 after a rejected one; stops at an accepted step with
 * |d| <= 1e-14 |X|, at lambda > 1e12, or after max_iter iterations (the bindings pass 50).
 * X0, X [N][3] (X may be X0), x1, x2 [N][2], P [S][2][12]: S pairs of row-major 3 x 4
 * projection matrices (P1, P2); seg [N] int32 picks each point's pair (values are clamped to
 * [0, S); NULL: every point uses pair 0).  cost [N]: the final sum of squared residuals;
 * iters [N] int32: accepted steps in bits 0-23, status in bits 24-31 (0 converged by step
 * size, 1 lambda > 1e12, 2 the initial cost was not finite and the point is returned
 * unchanged, 3 max_iter ran). */
int32_t sfm_refine_points_dev(sfm_ctx* ctx, const double* X0, const double* x1, const double* x2, int64_t N,
                              const double* P, int32_t S, const int32_t* seg, int32_t max_iter, double* X,
                              double* cost, int32_t* iters, void* stream);

/* Util.print_reprojection_error (Util.py:65-82; Runner.py:211, :282): err [N][2] the two
 * norms of Util.py:76-77 per point, *mean (device) the mean over points of (e1 + e2) / 2
 * (Util.py:81), summed in a fixed order (the same bits every run).  P1, P2 [12].  N == 0
 * writes NaN to *mean, numpy's mean of an empty list. */
int32_t sfm_reprojection_error_dev(sfm_ctx* ctx, const double* X, const double* x1, const double* x2, int64_t N,
                                   const double* P1, const double* P2, double* err, double* mean, void* stream);

/* The 2D -> 3D association loop of Runner.py:241-250: for each query qry[q] (prev_frame_2d,
 * [nq][2] int32) the first nearest target (points_2D_from_prev_frame, tgt [m][2] int32) by the
 * exact int64 squared distance — np.argmin of the float64 norms — kept iff
 * sqrt((double)d2) < threshold (Runner.py:245).  The kept (target index, query index) pairs go
 * to out_tgt / out_qry ([nq] int32 each) in query order, their number to *out_n (device).
 * Coordinates within +-2^30.  m == 0 returns SFM_EINVAL: the reference fails there too
 * (np.argmin of an empty sequence). */
int32_t sfm_link_points_dev(sfm_ctx* ctx, const int32_t* tgt, int32_t m, const int32_t* qry, int32_t nq,
                            double threshold, int32_t* out_tgt, int32_t* out_qry, int32_t* out_n, void* stream);

/* SFMRunner.add_points with is_new_point / find_existing_point (Runner.py:361-385; called at
 * :217, :269, :280): the global registry of 3-D points.  reg_xyz [reg_capacity][3] float64 and
 * *reg_count (int32) are caller-owned device memory holding the registry and its size; the
 * caller guarantees reg_capacity >= *reg_count + n (the sum of the n of all calls so far bounds
 * the count without reading the device).  pts [n][3] are processed in order, as the
 * reference's loop: with d_j = sqrt((dx*dx + dy*dy) + dz*dz) (float64, no fused multiply-add,
 * correctly rounded sqrt) against every registered point, including those appended earlier
 * in this call, a point with no registered point or min_j d_j >= threshold is appended and
 * takes the new last index; otherwise it takes the first index of the smallest distance.
 * out_index [n] int32 receives that index, out_is_new [n] int32 1 where the point was
 * appended; reg_xyz gains the new coordinates (copied bit for bit) and *reg_count their
 * number.  The reference's threshold is 1e-6.  Finite coordinates are the caller's contract
 * (a NaN compares false everywhere the reference's min / argmin would propagate it).
 * SFM_EINVAL: a negative size, a null pointer, threshold <= 0 (or NaN), reg_capacity < n,
 * reg_capacity > 2^30 or n > 2^24; n == 0 does nothing.  Calls on one registry must be ordered
 * (one stream, or events); the context's workspace serves one call at a time. */
int32_t sfm_registry_add_dev(sfm_ctx* ctx, double* reg_xyz, int32_t* reg_count, int32_t reg_capacity,
                             const double* pts, int32_t n, double threshold, int32_t* out_index,
                             int32_t* out_is_new, void* stream);

/* SFMRunner.total_reprojection_error (Runner.py:311-334, printed before and after bundle
 * adjustment) over the M observations of prepare_for_ba (Runner.py:387-401): for observation o,
 * R = Rodrigues(camera_params[cam_idx[o]][0:3]) (theta = |r|; identity for theta < DBL_EPSILON,
 * else cos(theta) I + (1 - cos(theta)) k k^T + sin(theta) [k]x with k = r / theta),
 * q = K[cam_idx[o]] (R X[pt_idx[o]] + camera_params[cam_idx[o]][3:6]) and
 * err[o] = |q[:2] / q[2] - obs[o]|; *mean (device) is their mean, summed in a fixed order (the
 * same bits every run; NaN for M == 0, where the reference divides by zero).  cam_idx, pt_idx
 * [M] int32, obs [M][2], camera_params [n_cam][6], K [n_cam][9] row-major, X [n_pts][3].
 * Indices within their tables are the caller's contract (values are clamped, like seg in
 * sfm_refine_points_dev).  SFM_EINVAL: M < 0, a null pointer, M > 0 with n_cam or n_pts < 1. */
int32_t sfm_total_reprojection_error_dev(sfm_ctx* ctx, const int32_t* cam_idx, const int32_t* pt_idx,
                                         const double* obs, int64_t M, const double* camera_params, int32_t n_cam,
                                         const double* K, const double* X, int32_t n_pts, double* err, double* mean,
                                         void* stream);

/* The pose of a frame from its 2D-3D links (Runner.py:257-262, PoseEstimator.PnPRansac): the
 * library's own rule in the spirit of cv2.solvePnPRansac(reprojectionError = 8,
 * iterationsCount = iters, flags = SOLVEPNP_ITERATIVE).  Parity with OpenCV is NOT pinned
 * (DESIGN.md §13D); the rule is pinned to a numpy restatement, planted poses and scipy.
 * X [n][3] world points, x [n][2] pixels, K [9] row-major upper triangular (skew allowed); all
 * float64 on the device.
 *  1. Sample s = the first 6 indices of sfm_ransac_sample_indices(n, iters, 5)[s] (for n < 8:
 *     sfm_ransac_sample_indices_k with size 6).  n < 6: no pose.
 *  2. Hypothesis: image points through K^-1; the six world points as Y = s (X - c), c their
 *     centroid, s = sqrt(3) / mean |X - c|; DLT rows [Yh, 0, -u Yh], [0, Yh, -v Yh] per point,
 *     the first 11 of the 12; the null vector with last component 1 by Gaussian elimination
 *     with partial pivoting; P negated when det P[:, :3] < 0; R = the polar factor of
 *     M = P[:, :3], sigma = M's mean singular value, t = (P[:, 3] / sigma - s R c) / s.  A
 *     zero pivot or a non-finite result gives a NaN hypothesis.
 *  3. Count: points with depth (R X + t)[2] > 0 and |pi(K (R X + t)) - x| < threshold.
 *  4. The first sample with the strictly largest count wins; all counts 0 (or iters == 0): no
 *     pose.  out_inliers [n] receives the winner's inlier indices in ascending order, *out_n
 *     their number (0: no pose; -1: n < 6), *out_iter the winner (-1: none).
 *  5. Levenberg-Marquardt over the winner's inliers on (d omega, d t), R <- exp([d omega]x) R,
 *     t <- t + d t: residuals pi(K (R X + t)) - x, (J^T J + lambda diag J^T J) d = -J^T r by
 *     Cholesky, lambda from 1e-3; a step is accepted iff the cost is strictly smaller, then
 *     lambda <- max(lambda / 10, 1e-12), else lambda <- 10 lambda.  Status as
 *     sfm_refine_points_dev: 0 an accepted step with |d| <= 1e-14 max(1, |t|), 1 lambda > 1e12,
 *     3 max_refine_iter iterations, 2 non-finite start cost (pose unchanged).  The inliers
 *     are not re-scored.
 * Outputs (device): R [9] row-major, t [3] (NaN without a pose), out_status [4] = found (0 / 1),
 * LM status (-1 without a pose), accepted steps, iterations run; out_cost [2] = the sum of
 * squared residuals at the winning hypothesis and at the returned pose; out_counts [iters]
 * (optional) every sample's count.  Sums run in a fixed order: the same bits every run.
 * Enqueued on `stream`; the call synchronises only when the context first uploads the sample
 * stream of (n, iters).  One call at a time per context.  SFM_EINVAL: a null pointer,
 * n < 0, iters < 0, threshold not positive, max_refine_iter outside [1, 2^24). */
int32_t sfm_pnp_ransac_dev(sfm_ctx* ctx, const double* X, const double* x, const double* K, int32_t n,
                           int32_t iters, double threshold, int32_t max_refine_iter, double* R, double* t,
                           int32_t* out_inliers, int32_t* out_n, int32_t* out_iter, int32_t* out_status,
                           double* out_cost, int32_t* out_counts, void* stream);
/* PoseEstimator.PnP (no RANSAC): the DLT of step 2 over all n >= 6 points (normalised over all
 * of them; the eigenvector of the smallest eigenvalue of the 12 x 12 A^T A by cyclic Jacobi),
 * the same P -> (R, t), then step 5 over all points.  Outputs as above (found 0 for n < 6 or a
 * non-finite DLT pose). */
int32_t sfm_pnp_dev(sfm_ctx* ctx, const double* X, const double* x, const double* K, int32_t n,
                    int32_t max_refine_iter, double* R, double* t, int32_t* out_status, double* out_cost,
                    void* stream);

/* Bundle adjustment over the registry (Runner.py:294-306, SFM.py:405-464): the library's own
 * Levenberg-Marquardt rule with the Schur complement, in place of scipy's
 * least_squares(method='trf', jac='2-point', ftol=1e-2).  Which iterate scipy's TRF path stops
 * at is NOT pinned; the minimum is (a numpy restatement, scipy's tight-tolerance
 * minimum and the reference's own recorded run).  Float64 without contraction.
 * cam_idx, pt_idx [M] int32, obs [M][2], camera_params [n_cam][6] (Rodrigues vector, t),
 * K [n_cam][9] row-major, X [n_pts][3], cam_fixed [n_cam] uint8 (optional; non-zero: the camera
 * does not move); all on the device.  All M observations count (compute_residuals zips them
 * all; the first-num_points bound belongs to total_reprojection_error alone).
 *  Unknowns: per camera R_c = Rodrigues(camera_params[c][0:3]) (the closed form of
 *   sfm_total_reprojection_error_dev) and t_c; per point X_j.
 *  Residual: r_o = pi(K_c (R_c X_j + t_c)) - obs[o]; cost = the sum of their squares.
 *  Update: R_c <- exp([d omega_c]x) R_c, t_c <- t_c + d t_c, X_j <- X_j + d X_j.
 *  Jacobian rows, a in {0, 1}: Y = R_c X_j, q = K_c (Y + t_c), g_a = (K_c[a] - (q_a / q_2) K_c[2]) / q_2;
 *   camera block [Y x g_a, g_a], point block g_a^T R_c.
 *  Blocks: U_c = sum J_c^T J_c, V_j = sum J_p^T J_p, W_cj = sum J_c^T J_p (over the duplicate
 *   observations of one (c, j) too), g_c, g_j.  Damping U*_c = U_c + lambda diag U_c,
 *   V*_j = V_j + lambda diag V_j.  A camera flagged in cam_fixed, a camera without an
 *   observation and a point without an observation do not move: their block is the identity,
 *   their gradient and W are zero.
 *  Step: S = U* - sum_j W_j V*_j^-1 W_j^T, b = -g_c + sum_j W_j V*_j^-1 g_j, S d_c = b by a dense
 *   Cholesky, d X_j = -V*_j^-1 (g_j + W_j^T d_c).  A pivot of V*_j or of S that is not positive
 *   and finite, or a candidate cost that is not finite, rejects the step.
 *  lambda starts at 1e-3; a step is accepted iff the cost is strictly smaller, then
 *   lambda <- max(lambda / 10, 1e-12), else lambda <- 10 lambda.
 *  Status: 0 an accepted step with (cost - cost_new) / cost <= ftol, or with
 *   |d| <= 1e-14 max(1, |params|) (params: every t_c and X_j); 1 lambda > 1e12; 3 max_iter
 *   iterations ran; 2 the start cost is not finite (everything returned unchanged).
 * Outputs (device): out_camera_params [n_cam][6], out_X [n_pts][3],
 * out_cost [2] (optional) = start and final cost, out_status [4] (optional) = status, accepted
 * steps, iterations run, iterations with a rejected factorisation.  The rotation goes back to
 * its principal Rodrigues vector on the device (the closed form of the Python rodrigues): a
 * vector that came in with theta > pi comes out as its equivalent with theta <= pi.  A camera
 * that does not move, and every row when no step was accepted, returns its input bits.
 * M == 0 returns the inputs, cost 0 and status 0.
 * Every sum runs in a fixed order — ascending observation index within a point; U_c and g_c
 * ascending per lane over the camera's list (lane = position mod 64), then a butterfly over the
 * 64 lanes; the rows of S over the camera's points in list order within each of the equal
 * segments its list is cut into (a number fixed by n_cam), then the segments in order; the
 * cost over 256 strided partial sums and a fixed tree — so two runs give the same bits.
 * Enqueued on `stream`: max_iter rounds of ordinary launches, each of which returns at once
 * when the device-resident stop word is set; no synchronisation (growing the workspace frees
 * buffers).  One call at a time per context.  Indices within their tables are the caller's
 * contract (values are clamped).  SFM_EINVAL: n_cam outside [1, 256], n_pts outside [0, 2^24],
 * M outside [0, 2^26], M > 0 with n_pts < 1, a null pointer (but cam_fixed, out_cost,
 * out_status), ftol < 0 or NaN, max_iter outside [1, 2^24). */
int32_t sfm_bundle_adjust_dev(sfm_ctx* ctx, const int32_t* cam_idx, const int32_t* pt_idx, const double* obs,
                              int64_t M, const double* camera_params, int32_t n_cam, const double* K,
                              const double* X, int32_t n_pts, const uint8_t* cam_fixed, double ftol,
                              int32_t max_iter, double* out_camera_params, double* out_X, double* out_cost,
                              int32_t* out_status, void* stream);

/* Feature tracks: the connected components of the match graph of a slot table, the step between
 * pairwise matches and reconstruction in COLMAP / OpenMVG / openMVS.  The reference has none; the
 * rule is the library's own, pinned to a numpy restatement and scipy's connected_components
 * (DESIGN.md §13F).  `keep` carries the geometric verification: sfm_verify_matches_dev (below)
 * writes it on the device in exactly this layout, and a caller may pass a mask of its own.
 * Inputs (device), in the layouts of sfm_match_pairs_dev: count [nimg], pairs [P][2],
 * matches [P][cap][2], nmatch [P]; keep [P][cap] uint8 (optional; NULL: every match counts).
 *  Nodes: (slot s, row r) with r < count[s] (count clamped to [0, cap]); id = s * cap + r.
 *  Edges: for each pair p and each m < nmatch[p] (nmatch = -1 counts as 0, values above cap as
 *   cap) with keep[p][m] != 0, an edge between (pairs[p][0], matches[p][m][0]) and
 *   (pairs[p][1], matches[p][m][1]).  Such an edge is skipped and counted when a slot is outside
 *   [0, nimg), when the two slots are equal, or when a row is outside [0, count) of its slot.
 *   Duplicate edges are harmless.
 *  Components: the connected sets of two or more nodes; a component's label is its smallest id.
 *  Tracks: a component with two nodes of one slot is inconsistent and dropped whole; a
 *   consistent one with fewer than min_len nodes is dropped as short; the others are the tracks,
 *   numbered in ascending label order.
 * Outputs (device, caller-allocated for the worst case): track_offsets [nimg * cap / 2 + 1] (T + 1
 * written: a CSR by track), obs_slot and obs_row [nimg * cap] (n_obs written; ascending slot
 * within a track), node_track [nimg][cap] (the node's track id; -1: in no component, or beyond
 * count; -2: its component is inconsistent; -3: short), out_n [6] = T, n_obs, inconsistent
 * components, short components, skipped edges, the longest track.
 * Integers only: two runs, and any order of the pairs or of the matches within a pair, write the
 * same bytes.  Enqueued on `stream`, no synchronisation (growing the workspace, 36 to 52 bytes
 * per node, frees buffers); one call at a time per context.  SFM_EINVAL: nimg or cap < 1,
 * P < 0, nimg * cap > 2^30, min_len < 2, a null pointer (but keep; pairs, matches, nmatch when
 * P == 0). */
int32_t sfm_build_tracks_dev(sfm_ctx* ctx, const int32_t* count, int32_t nimg, int64_t cap, const int32_t* pairs,
                             int32_t P, const int32_t* matches, const int32_t* nmatch, const uint8_t* keep,
                             int32_t min_len, int32_t* track_offsets, int32_t* obs_slot, int32_t* obs_row,
                             int32_t* node_track, int32_t* out_n, void* stream);

/* Two-view geometric verification of the matches of a pair schedule, the step COLMAP and OpenMVG
 * put between matching and tracks: an 8-point RANSAC per pair whose inlier mask is the `keep` of
 * sfm_build_tracks_dev.  The reference has none; the rule is the library's own, pinned to a numpy
 * restatement (tests/verify_ref.py).
 * Inputs (device), exactly as sfm_match_pairs_dev leaves them: xy [nimg][cap][2] int32 and
 * count [nimg] of the slot table, pairs [P][2], matches [P][cap][2], nmatch [P].
 * For pair p with slots (a, b) = pairs[p] and n = clamp(nmatch[p], 0, cap) (nmatch = -1 counts as 0):
 *  Candidates: match m < n is valid when both rows lie in [0, count) of their slots (count
 *   clamped to [0, cap]); its correspondence is (xy[a][matches[p][m][0]], xy[b][matches[p][m][1]]).
 *   An invalid match is never an inlier and never kept; a sample that contains one counts 0.  The
 *   pair is not attempted when a slot is outside [0, nimg), when a == b or when n < 8: then
 *   stat = {-1, -1, 0, 0}, keep all 0, F all NaN.
 *  Samples: counter-based, integers only, a function of (seed, a, b, it) and nothing else (not of
 *   P, of the pair's position in the call or of the other pairs).  mix64 is the splitmix64
 *   finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 *   z ^= z >> 31), G = 0x9E3779B97F4A7C15, all in uint64: key = mix64(mix64(seed) + ((a << 32) | b));
 *   draw k = 0..7 of sample it is r = mix64(key + (8 it + k + 1) G) >> 32.  The eight indices come
 *   from a Fisher-Yates over a virtual arange(n): j = k + ((r (n - k)) >> 32), the sample's k-th
 *   index is the value now at position j, then positions k and j are swapped.  The indices are
 *   distinct and in [0, n) for every n >= 8.
 *  Fit and test: F per sample by the route of sfm_ransac_find_inliers (Hartley normalisation,
 *   elimination with partial pivoting, the last free column set to 1, rank 2 by Jacobi,
 *   un-normalisation) and that call's inlier test d = |l . p2| / sqrt(l0^2 + l1^2) < threshold,
 *   l = F p1, float64.  A threshold that is <= 0 or NaN admits nothing.
 *  Rounds and early stop: samples are evaluated in rounds of 256 (the round size is part of the
 *   rule): round r = 1, 2, ... holds samples 256 (r - 1) .. min(iters, 256 r) - 1.  After round r,
 *   with `best` the largest count so far, the pair stops when r <= n_stop and
 *   (double)best >= stop_ratio[r - 1] * (double)n (one IEEE multiply, one compare); otherwise
 *   after the last round.  stop_ratio is a HOST array of n_stop <= 64 doubles, copied into the
 *   kernel's arguments before the call returns; n_stop = 0 means fixed iterations.
 *  Winner: the lowest it among the evaluated samples with the largest count.  The pair is
 *   verified when that count is > 0 and >= min_inliers.  For a verified pair keep[p][m] = 1
 *   exactly for the valid matches that are inliers of the winner's F (the same test and the same F
 *   that produced the count, so the row holds exactly `count` ones); otherwise the row is all 0.
 *   Every one of the cap bytes of keep[p] is written, 0 at and beyond n.
 * Outputs (device): keep [P][cap] uint8; F [P][9] float64, the winner's whether or not the pair
 * is verified (scale and sign unspecified; NaN when no sample had an inlier); stat [P][4] int32 =
 * best count, winning sample, samples evaluated, verified (0/1).  iters == 0: every attempted pair
 * gets {0, -1, 0, 0}.
 * Two runs write the same bytes; permuting the pairs, or splitting a schedule over several calls,
 * gives each pair the same bytes.  The order of the matches WITHIN a pair does matter: the sample
 * indices address it.  No refit on the inliers, no guided matching; the homography test that
 * tells a planar or rotation-only pair apart is sfm_homography_matches_dev (below).  One launch enqueued on `stream`: no workspace, no allocation, no
 * synchronisation, no device read of host memory, so the call can be captured into a hipGraph.
 * SFM_EINVAL: nimg or cap < 1, P < 0, iters outside [0, 2^20], n_stop outside [0, 64], stop_ratio
 * null with n_stop > 0, min_inliers < 0, a null pointer (but every array indexed by p when
 * P == 0). */
int32_t sfm_verify_matches_dev(sfm_ctx* ctx, const int32_t* xy, const int32_t* count, int32_t nimg, int64_t cap,
                               const int32_t* pairs, int32_t P, const int32_t* matches, const int32_t* nmatch,
                               int32_t iters, double threshold, int32_t min_inliers, int64_t seed,
                               const double* stop_ratio, int32_t n_stop, uint8_t* keep, double* F, int32_t* stat,
                               void* stream);

/* The two-view geometry record of a verified pair, first half: a homography RANSAC per pair, whose
 * inlier count set against verify's tells a planar scene or a pure rotation (both pass the F test
 * with a high count) from a general one.  COLMAP and OpenMVG keep such a record per verified pair;
 * the reference has none.  The rule is the library's own, pinned to a numpy restatement
 * (tests/two_view_ref.py).
 * Inputs (device): xy, count, nimg, cap, pairs, P, matches, nmatch exactly as
 * sfm_verify_matches_dev reads them; attempt [P] int32 (optional; NULL: every pair may be
 * attempted), a pair with attempt[p] == 0 is skipped (pass a contiguous copy of column 3 of verify's stat).
 * For pair p with slots (a, b) = pairs[p] and n = clamp(nmatch[p], 0, cap):
 *  Attempted iff both slots lie in [0, nimg), a != b, n >= 4 and attempt allows it.  A pair that
 *   is not attempted gets hstat = {-1, -1, 0, 0}, H all NaN, hkeep all 0.
 *  Candidates: valid matches as in sfm_verify_matches_dev.  An invalid match is never an inlier; a
 *   sample that contains one counts 0.
 *  Samples: verify's counter stream generalised to sample size 4, under a key of its own.  With
 *   mix64 and G as there, keyH = mix64(mix64(seed ^ 0x486F6D6F67726170) + ((a << 32) | b)); draw
 *   k = 0..3 of sample it is r = mix64(keyH + (4 it + k + 1) G) >> 32, and the four indices are the
 *   first four steps of the same Fisher-Yates over a virtual arange(n): j = k + ((r (n - k)) >> 32),
 *   the k-th index is the value now at position j, then positions k and j are swapped.
 *  Fit, float64 without contraction: Hartley normalisation over the four points of each image
 *   (mean, mean distance, s = sqrt(2) / mean distance; the arithmetic of the 8-point fit over four
 *   points); the 8 x 9 DLT system whose rows for point i = 0..3, in point order, are
 *   [-x -y -1 0 0 0 x'x x'y x'] and [0 0 0 -x -y -1 y'x y'y y'] on the normalised (x, y) -> (x', y');
 *   its null vector by the elimination of the 8-point fit (partial pivoting, the last free column
 *   set to 1); H = T2^-1 Hn T1 with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]], written out as
 *   M = Hn T1 (M[r][0] = Hn[r][0] s1, M[r][1] = Hn[r][1] s1,
 *   M[r][2] = (Hn[r][0] (-s1 c1x) + Hn[r][1] (-s1 c1y)) + Hn[r][2]), then H[0] = M[0] (1 / s2) + c2x M[2],
 *   H[1] = M[1] (1 / s2) + c2y M[2], H[2] = M[2] by rows.  No unit norm, no degeneracy test of the
 *   sample: a collinear sample simply scores low.
 *  Inlier test, no division and no square root: with (u, v, w) = H (x1, y1, 1), each as
 *   (H[3r] x1 + H[3r+1] y1) + H[3r+2], the forward transfer is ok iff
 *   (x2 w - u)^2 + (y2 w - v)^2 < thr2 (w w), thr2 = threshold^2.  The backward transfer is the
 *   same test with adj(H) (the transposed cofactors, each entry one difference of two products)
 *   on (x2, y2, 1) against (x1, y1).  A match is an inlier iff both hold.  Any NaN compares false,
 *   w == 0 admits nothing (also at threshold = inf), and a threshold that is <= 0 or NaN admits
 *   nothing.
 *  Rounds of 256, early stop against the caller's stop_ratio (a HOST array, copied into the
 *   kernel's arguments; for this sample size pose.ransac_stop_ratios(c, r, 4)), winner (largest
 *   count, lowest sample): as sfm_verify_matches_dev.
 * Outputs (device): H [P][9] float64 row-major, the winner's — the one that produced the count;
 * NaN when no sample had an inlier (scale and sign unspecified); hkeep [P][cap] uint8 (optional):
 * the winner's inlier mask when its count is > 0, else 0, every one of the cap bytes written;
 * hstat [P][4] int32 = best count, winning sample, samples evaluated, 0.  iters == 0: every
 * attempted pair gets {0, -1, 0, 0}.
 * Two runs write the same bytes; permuting the pairs or splitting the schedule gives each pair
 * the same bytes.  One launch enqueued on `stream`: no workspace, no allocation, no
 * synchronisation, no device read of host memory, so the call can be captured into a hipGraph.
 * SFM_EINVAL: nimg or cap < 1, P < 0, iters outside [0, 2^20], n_stop outside [0, 64], stop_ratio
 * null with n_stop > 0, a null pointer (but attempt and hkeep; every array indexed by p when
 * P == 0). */
int32_t sfm_homography_matches_dev(sfm_ctx* ctx, const int32_t* xy, const int32_t* count, int32_t nimg, int64_t cap,
                                   const int32_t* pairs, int32_t P, const int32_t* matches, const int32_t* nmatch,
                                   const int32_t* attempt, int32_t iters, double threshold, int64_t seed,
                                   const double* stop_ratio, int32_t n_stop, double* H, uint8_t* hkeep,
                                   int32_t* hstat, void* stream);

/* The two-view geometry record, second half: the relative pose (R, t) of each verified pair out
 * of verify's F and the intrinsics, chosen by a cheirality count, and the number of its points
 * with enough parallax.  No RANSAC.  The rule is the library's own (tests/two_view_ref.py).
 * Inputs (device): the slot table, pairs, matches, nmatch as above; keep [P][cap] uint8 and
 * F [P][9] as sfm_verify_matches_dev wrote them; K [nimg][9] float64 row-major, one intrinsic
 * matrix per slot; attempt [P] int32 (optional, as above); cos2_min, the squared cosine of the
 * minimum parallax angle, a host value.
 * For pair p with slots (a, b):
 *  Attempted iff both slots lie in [0, nimg), a != b, attempt allows it and all nine entries of
 *   F[p] are finite.  Otherwise pstat = {-1, -1, 0, 0} and pose is all NaN.
 *  Points: the matches m < n with keep[p][m] != 0 and both rows valid; n_points is their number.
 *  Candidates: E = K[b]^T F K[a] and the four poses (R1, T), (R1, -T), (R2, T), (R2, -T) of
 *   sfm_ransac_camera_motion_dev, the same arithmetic, numbered 0..3 in this order.
 *  Cheirality count: P1 = K[a] [I | 0], P2 = K[b] [R | t]; X by the linear triangulation of
 *   sfm_triangulate_dev on raw pixels.  A point is in front iff X_z >= 1e-6 and
 *   (R X + t)_z >= 1e-6, the latter as (R[6] X_x + R[7] X_y + R[8] X_z) + t_z; a NaN is not in
 *   front.  The winner is the candidate with the largest count, the lowest number on a tie; a
 *   largest count of 0 gives pose NaN, candidate -1 and n_front 0.
 *  Parallax, over the winner's front points: C = -R^T t, e = X - C, d = X . e (each dot product
 *   summed left to right).  The point is wide iff d <= 0 or d^2 < (cos2_min |X|^2) |e|^2: the angle
 *   at X between the rays to the two centres is at least the minimum.  No sqrt, no acos.
 * Outputs (device): pose [P][12] float64, R row-major then t (|t| = 1); pstat [P][4] int32 =
 * n_front, candidate, n_wide, n_points.
 * Counts are integers: two runs, any order of the pairs and any split of the schedule write the
 * same bytes.  One launch enqueued on `stream`, nothing allocated, nothing synchronised,
 * capturable into a hipGraph.  SFM_EINVAL: nimg or cap < 1, P < 0, a null pointer (but attempt;
 * every array indexed by p when P == 0). */
int32_t sfm_two_view_pose_dev(sfm_ctx* ctx, const int32_t* xy, const int32_t* count, int32_t nimg, int64_t cap,
                              const int32_t* pairs, int32_t P, const int32_t* matches, const int32_t* nmatch,
                              const uint8_t* keep, const double* F, const double* K, const int32_t* attempt,
                              double cos2_min, double* pose, int32_t* pstat, void* stream);

/* Each track's 3-D point from all its views: CameraPose.triangulate_point (SFM.py:241-246)
 * extended from 2 to V views.  track_offsets / obs_slot / obs_row: the CSR of
 * sfm_build_tracks_dev with n_tracks tracks and n_obs observations (host values; offsets are
 * clamped to [0, n_obs]); xy [nimg][cap][2] int32 the slot table's pixels; P [n_cam][12] row-major
 * 3 x 4, one projection matrix per slot; cam_valid [n_cam] uint8 (optional; 0: the slot has no
 * pose).  A view is valid when its slot is below min(nimg, n_cam), its row below cap and its
 * camera valid.  Every valid view adds the rows x P[2] - P[0] and y P[2] - P[1] on raw pixel
 * coordinates, in ascending slot order; X [n_tracks][3] (float64) is the right singular vector of
 * the smallest singular value of the stacked rows divided by its fourth component, NaN with
 * fewer than 2 valid views; out_views [n_tracks] the valid views.  The rows are folded one at a
 * time into a 4 x 4 triangular factor by Givens rotations (A^T A is never formed), whose null
 * vector comes from sfm_triangulate_dev's one-sided Jacobi; float64 without contraction, the
 * same bits every run.  Enqueued on `stream`, not synchronised.  SFM_EINVAL: a negative count,
 * nimg, cap or n_cam < 1, a null pointer (but cam_valid; outputs of an empty call). */
int32_t sfm_triangulate_tracks_dev(sfm_ctx* ctx, const int32_t* track_offsets, const int32_t* obs_slot,
                                   const int32_t* obs_row, int32_t n_tracks, int32_t n_obs, const int32_t* xy,
                                   int32_t nimg, int64_t cap, const double* P, const uint8_t* cam_valid,
                                   int32_t n_cam, double* X, int32_t* out_views, void* stream);

/* Resection from tracks: the pose of every frame of a slot table that has none yet, from the
 * 2D-3D links its feature tracks give it, all frames in one call.  The step between the initial
 * pair (sfm_two_view_pose_dev) and the triangulation of the model (sfm_triangulate_tracks_dev);
 * the rule is the library's own (tests/resect_ref.py).
 * Inputs (device): xy [nimg][cap][2] int32 and count [nimg] of the slot table; node_track
 * [nimg][cap] int32 as sfm_build_tracks_dev wrote it; X [n_tracks][3] float64 as
 * sfm_triangulate_tracks_dev wrote it (NaN: no point; may be null when n_tracks == 0); K [nimg][9]
 * float64 row-major, one intrinsic matrix per slot; attempt [nimg] uint8 (optional; null: every
 * slot, else only the slots with a non-zero entry).  Host values: n_tracks, iters, threshold,
 * min_inliers, seed, max_refine_iter.
 * For slot s:
 *  Links: c = clamp(count[s], 0, cap); row r < c is a link iff t = node_track[s][r] lies in
 *   [0, n_tracks) and all three of X[t] are finite.  The links are taken in ascending r; link i is
 *   the correspondence (X[t_i], (double)xy[s][r_i]).  n_links is written for every slot.
 *  Attempted iff attempt allows it, n_links >= 6 and K[s] is finite and upper triangular with a
 *   non-zero diagonal.  Otherwise rstat = {-1, -1, 0, n_links, 0, -1, 0, 0}, pose and rcost are NaN,
 *   the rkeep row is 0, the out_counts row 0 and the out_hyp row NaN.
 *  Samples: the counter stream of sfm_verify_matches_dev at sample size 6 under a key of its own,
 *   keyR = mix64(mix64(seed ^ 0x526573656374696F) + (uint64)(uint32)s); draw k = 0..5 of sample it
 *   is mix64(keyR + (6 it + k + 1) G) >> 32 with G = 0x9E3779B97F4A7C15, and the indices are the
 *   first six steps of the Fisher-Yates shuffle of arange(n_links) those draws give.  The indices
 *   address the link list, not the rows.  The stream is a function of (seed, s, it) only.
 *  Hypothesis, count, refinement: steps 2, 3 and 5 of sfm_pnp_ransac_dev over the links, the same
 *   arithmetic in the same order.  Fixed iters: no rounds, no early stop.
 *  Winner: the lowest sample with the largest count (sample -1 and count 0 when iters == 0).  The
 *   slot is posed iff that count is > 0 and >= min_inliers; otherwise pose and rcost are NaN, the
 *   rkeep row is 0 and rstat[4..7] = {0, -1, 0, 0}.  The refinement runs over the winner's inliers
 *   in link order; the inliers are not re-scored.
 * Outputs (device): pose [nimg][12] float64, R row-major then t; rstat [nimg][8] int32 = best
 * count, winning sample, samples evaluated, n_links, posed (0 / 1), LM status, accepted steps, LM
 * iterations; rcost [nimg][2] the sum of squared residuals over the inliers at the winning
 * hypothesis and at the returned pose; rkeep [nimg][cap] uint8 (optional), 1 exactly at the rows
 * that are links and inliers of a posed winner, every byte written; out_counts [nimg][iters] int32
 * and out_hyp [nimg][iters][12] float64 (optional) every sample's count and (R, t).
 * Two runs write the same bytes, and a slot gets the same bytes (those of its pose included)
 * whatever attempt says about the other slots and however the table's slots are split over calls
 * by attempt.  Five launches enqueued on `stream` whatever nimg is, nothing synchronised, no host
 * memory read by the device.  The workspace (48 B per node of the table, 100 B per (slot, sample)
 * where the caller passes no out_hyp / out_counts) grows on demand and is the only allocation:
 * after a call of the same sizes the call can be captured into a hipGraph.  One call at a time
 * per context.  SFM_EINVAL: nimg or cap < 1, n_tracks < 0, iters outside [0, 2^20], threshold not
 * positive, min_inliers < 0, max_refine_iter outside [1, 2^24), a null pointer (but attempt,
 * rkeep, out_counts, out_hyp, and X when n_tracks == 0), more than 2^30 nodes. */
int32_t sfm_resect_tracks_dev(sfm_ctx* ctx, const int32_t* xy, const int32_t* count, int32_t nimg, int64_t cap,
                              const int32_t* node_track, const double* X, int32_t n_tracks, const double* K,
                              const uint8_t* attempt, int32_t iters, double threshold, int32_t min_inliers,
                              int64_t seed, int32_t max_refine_iter, double* pose, int32_t* rstat, double* rcost,
                              uint8_t* rkeep, int32_t* out_counts, double* out_hyp, void* stream);

/* sfm_ingest_rgb for B frames: rgb [B][H][W][3] uint8 -> gray [B][H2][W2] float32 (device
 * pointers).  Enqueued on `stream`, not synchronised.  The tap tables and the temp image belong
 * to the context: one ingest call at a time per context, on one stream.  A call whose shape
 * (H, W, H2, W2) differs from the context's last one, or whose temp is larger, first waits for
 * the work already enqueued on `stream` and uploads its tables there; a call on another stream
 * needs the caller to have synchronised the previous one. */
int32_t sfm_ingest_rgb_dev(sfm_ctx* ctx, const uint8_t* rgb, int32_t B, int32_t H, int32_t W,
                           int32_t H2, int32_t W2, float* gray, void* stream);

/* Extract B images of identical size H x W stored contiguously ([B][H][W] float32). */
int32_t sfm_extract_batch_dev(sfm_ctx* ctx, const float* imgs, int32_t B, int32_t H, int32_t W,
                              int32_t* xy, float* desc, int32_t* count, int64_t cap,
                              void* stream);

/* Same, from 8-bit grayscale frames ([B][H][W] uint8, value/255 as float32 —
 * the conversion of Runner.py:507-509,521 done on the device). */
int32_t sfm_extract_batch_u8_dev(sfm_ctx* ctx, const uint8_t* imgs, int32_t B, int32_t H,
                                 int32_t W, int32_t* xy, float* desc, int32_t* count,
                                 int64_t cap, void* stream);

/*
 * Match P image pairs out of a slot table of `nimg` images (the consecutive / all-pairs
 * schedule of Runner.py:183-191).  pairs: [P][2] int32 image indices into the table.
 * Output per pair p: matches [p][cap][2] int32 (row in first, row in second),
 * conf [p][cap] float32, nmatch [p] int32; sorted as sfm_match.  A pair whose second
 * image has fewer than 2 keypoints yields nmatch = -1 (the reference's IndexError).
 */
int32_t sfm_match_pairs_dev(sfm_ctx* ctx, const float* desc, const int32_t* count, int32_t nimg,
                            int64_t cap, const int32_t* pairs, int32_t P, float ratio,
                            int32_t* matches, float* conf, int32_t* nmatch, void* stream);

/*
 * The same matcher split in two for large resident tables (BASELINE configs[3]'s gathered
 * table of thousands of slots, matched a chunk of pairs at a time):
 *  - sfm_match_prep_dev builds the matcher's per-descriptor operands (split-f16 copies,
 *    norms, per-slot maxima) for slots [slot_lo, slot_lo + slot_n) of a table of `nimg`
 *    slots into ctx-owned buffers sized for the whole table;
 *  - sfm_match_pairs_prepped_dev matches pairs whose slots were all prepped by earlier
 *    calls on this ctx (same table, descriptors unchanged since) — sfm_match_pairs_dev
 *    without its prep of every slot.
 * Results are identical to sfm_match_pairs_dev.  Same pairs / outputs / status rules.
 * A prepped call whose table (desc, count, nimg, cap) is not the one last prepped on this
 * ctx returns SFM_ESTATE.  That every slot the device-resident pairs touch was prepped,
 * and that its descriptors did not change since, is the caller's (unchecked) contract.
 *
 * Matcher workspace (both calls): operands 520 B per slot (x capP = cap rounded up to
 * 128) for the table, plus per pair cap x 532 B (row results, overflow list and 128
 * admitted-target words per query row).  The per-pair part is bounded: a call with more
 * pairs than fit the budget (default 4 GiB, env SFMFEAT_MATCH_BUDGET_MB read at context
 * creation) runs as consecutive sub-launches over the same buffers.
 */
int32_t sfm_match_prep_dev(sfm_ctx* ctx, const float* desc, const int32_t* count, int32_t nimg,
                           int64_t cap, int32_t slot_lo, int32_t slot_n, void* stream);
int32_t sfm_match_pairs_prepped_dev(sfm_ctx* ctx, const float* desc, const int32_t* count,
                                    int32_t nimg, int64_t cap, const int32_t* pairs, int32_t P,
                                    float ratio, int32_t* matches, float* conf, int32_t* nmatch,
                                    void* stream);

/* ---------------- stream layout of a context ----------------
 * Replaces no reference interface (the reference has no device streams).
 * sfm_ctx_stream: the context's own HIP stream (created on first use; the host-pointer calls
 * run on it) for callers that enqueue the batch calls on it instead of a stream of their own.
 * sfm_ctx_set_serial: 1 = extractions run every stage on the caller's stream (no internal
 * aux stream, no fork/join); 0 = the two largest levels' selection and descriptors overlap
 * the later levels' Harris on the context's aux stream (default; SFMFEAT_SERIAL=1 flips the
 * default).  Each stream maps onto one of the HIP runtime's hardware queues, and streams
 * beyond GPU_MAX_HW_QUEUES share one, so a batch pipeline chooses how many it uses.
 * sfm_ctx_set_priority: HIP stream priority of the context's two streams (lower = higher
 * priority, hipDeviceGetStreamPriorityRange; default 0); only before either stream exists
 * (SFM_EINVAL after).  BatchPipeline's SFMFEAT_LANE_PRIO=1 gives its first lane the higher
 * priority (an A/B setting; DESIGN_LOG.md §B). */
int32_t sfm_ctx_stream(sfm_ctx* ctx, void** stream);
/* sfm_ctx_set_fused_prep: 1 = each batch extraction on this context also writes the matcher's
 * per-descriptor operands (split-f16 copies, norms, block maxima; sfm_match_prep_dev's work)
 * from its descriptor kernel, and the next sfm_match_pairs_dev on this context over the same
 * table (desc, count, cap) preps only the slots beyond the extraction's batch — one launch
 * fewer per batch (BatchPipeline turns it on for its own tables).  Contract: the
 * descriptors an extraction wrote are not modified before that match (or
 * sfm_match_prep_dev is called over them first); 0 (default) = off.  A fused extraction
 * invalidates earlier sfm_match_prep_dev preps on that context (a prepped match is then
 * SFM_ESTATE until the table is prepped again). */
int32_t sfm_ctx_set_fused_prep(sfm_ctx* ctx, int32_t on);
int32_t sfm_ctx_set_serial(sfm_ctx* ctx, int32_t serial);
int32_t sfm_ctx_set_priority(sfm_ctx* ctx, int32_t priority);

/* ---------------- batches in flight: the lane gate ----------------
 * Replaces no reference interface: the reference runs one pair per host thread
 * (Runner.py:183-191); this orders the device-resident batch path's lanes.  Contexts that
 * share a gate (set with sfm_ctx_set_gate) order their extractions in submission order:
 * each batched extraction's pyramid waits, on its stream, until the previous gated
 * extraction's level-0 Harris launch has finished, so the two batches' largest VALU
 * launches never compete, and one batch's level-0 Harris overlaps the other's level-0 NMS,
 * selection and descriptors.  The gated contexts must be driven from one host thread; a
 * gate must outlive the contexts that use it (or be unset with NULL first). */
typedef struct sfm_gate sfm_gate;
int32_t sfm_gate_create(int32_t device, sfm_gate** out);
int32_t sfm_gate_destroy(sfm_gate* gate);
int32_t sfm_ctx_set_gate(sfm_ctx* ctx, sfm_gate* gate);

/* ---------------- multi-GPU exchange over RCCL (SURVEY.md §8b "sfm_dist_*", §8e) ----------
 * The reference fans the extractor and matcher out over 8 threads of one process
 * (Runner.py:183-191, 336-355); sharded over GPUs (one process per GPU, frames in contiguous
 * shards), the only data exchanged is the slot table the match schedule needs: the halo slot
 * of the consecutive schedule and, for configs[3], each chunk's slots on every rank.  These
 * calls move exactly that over RCCL without torch: a host in any language creates one
 * communicator per rank (the 128-byte id made by one rank and handed to the others over any
 * channel), then enqueues the exchange on its stream next to sfm_extract_batch_dev /
 * sfm_match_pairs_dev.  RCCL is loaded at run time (the copy already in the process, e.g.
 * PyTorch's, else librccl.so.1 from the library path): without it every call returns
 * SFM_EDEVICE and the rest of the library is unaffected.  One device per rank (RCCL does not
 * allow two ranks of one communicator on the same GPU).  Slot-table layout as
 * sfm_extract_batch_dev writes it: xy [slot][cap][2] int32, desc [slot][cap][128] float32,
 * count [slot] int32.  Errors: SFM_EINVAL (arguments), SFM_EDEVICE (RCCL / HIP; text via
 * sfm_dist_last_error, which takes NULL for failures before a communicator exists). */
#define SFM_DIST_ID_BYTES 128
typedef struct sfm_dist sfm_dist;
int32_t sfm_dist_unique_id(uint8_t* id /* [SFM_DIST_ID_BYTES] */);
/* Collective over the `world` ranks: every rank calls it with the same id (blocks until all
 * have joined). */
int32_t sfm_dist_create(int32_t device, int32_t rank, int32_t world, const uint8_t* id, sfm_dist** out);
int32_t sfm_dist_destroy(sfm_dist* d);
const char* sfm_dist_last_error(const sfm_dist* d);
int32_t sfm_dist_rank(const sfm_dist* d, int32_t* rank, int32_t* world);
/* configs[3]'s chunk gather (distributed.py allgather_chunk): every rank's bc slots
 * (src_*) land at table slots [base + r * bc, base + (r + 1) * bc) of every rank r, all three
 * fields in one grouped RCCL launch on `stream`.  In place (no copy of the own slots) when
 * src_* point at the table's own slots base + rank * bc. */
int32_t sfm_dist_allgather_slots_dev(sfm_dist* d, int32_t bc, int32_t cap, const int32_t* src_xy,
                                     const float* src_desc, const int32_t* src_count, int32_t* tab_xy,
                                     float* tab_desc, int32_t* tab_count, int64_t base, void* stream);
/* The consecutive schedule's halo (distributed.py halo_exchange): rank r sends its slot
 * (src_*, one slot) to rank r - 1 and receives rank r + 1's into dst_* (one slot); the first
 * rank only receives, the last only sends, a single rank does nothing. */
int32_t sfm_dist_halo_dev(sfm_dist* d, int32_t cap, const int32_t* src_xy, const float* src_desc,
                          const int32_t* src_count, int32_t* dst_xy, float* dst_desc, int32_t* dst_count,
                          void* stream);

/* ---------------- stage profiling (bench.py's live roofline numbers) ----------------
 * When enabled, every stage's launches are bracketed by HIP events on the launch
 * stream; sfm_profile_read synchronises them and returns the accumulated device time
 * (ms) and bracket count per stage, indexed by SFM_PROF_*. */
#define SFM_PROF_PYRAMID 0
#define SFM_PROF_HARRIS 1
#define SFM_PROF_MEDIAN 2
#define SFM_PROF_NMS 3
#define SFM_PROF_TOPK 4
#define SFM_PROF_DESCRIBE 5
#define SFM_PROF_MATCH_PREP 6
#define SFM_PROF_MATCH 7
#define SFM_PROF_MATCH_POST 8
#define SFM_PROF_STAGES 9
int32_t sfm_profile_enable(sfm_ctx* ctx, int32_t on);
/* Bracket only the stages whose bit (1 << SFM_PROF_*) is set in `mask` (0 = off): the
 * bench times its headline run with the dominant stage's events alone. */
int32_t sfm_profile_stages(sfm_ctx* ctx, int32_t mask);
int32_t sfm_profile_read(sfm_ctx* ctx, double* ms, int64_t* launches, int32_t reset);
/* Kernel-active spans of the Harris launches (the dominant kernel of the headline step):
 * with capacity > 0, each of the context's next `capacity` Harris launches records
 * {earliest workgroup start, latest workgroup end} on the device's constant-rate realtime
 * clock (one atomic per workgroup, so it can stay on inside a timed region; unlike a pair of
 * stream events it excludes the time a launch waits on its stream for CUs another stream
 * holds).  capacity 0 turns it off.  Both calls reset the slots (and synchronise the device).
 * sfm_profile_spans_read: spans_ns [n][2] in ns on that clock (comparable across the contexts
 * of one device), levels [n] the first pyramid level of each launch, n_out the launches
 * recorded (at most `capacity`), dropped the launches beyond it.
 * (No reference counterpart: bench.py's roofline) */
int32_t sfm_profile_spans(sfm_ctx* ctx, int64_t capacity);
int32_t sfm_profile_spans_read(sfm_ctx* ctx, int64_t* spans_ns, int32_t* levels, int64_t cap, int64_t* n_out,
                               int64_t* dropped, int32_t reset);

/* ---------------- diagnostics (used by the parity tests) ----------------
 * Run individual stages of the same device code on host data. */
/* numpy-SVML-exact float32 atan2 on the device (np.arctan2, ScaleRotInvSIFT.py:42). */
int32_t sfm_debug_atan2(int32_t device, const float* y, const float* x, float* out, int64_t n);
/* Harris R map, exact median and candidate count of one plane (NaiveSIFT.py:59-97). */
int32_t sfm_debug_harris(int32_t device, const float* gauss, int32_t gs, double alpha,
                         int32_t ksize, const float* img, int32_t H, int32_t W, float* R_out,
                         float* median_out, int64_t* ncand_out);

/* The float64 helpers the geometry kernels share (csrc/linalg3.h, linalg4.h, f64_dev.h), each
 * run by itself on n rows of host data (synchronises; only reads `in`), so that a helper can be
 * tested where no stage reaches.  Doubles per row, in -> out:
 *   RODRIGUES      r[3] -> R[9]                       RODRIGUES_INV  R[9] -> r[3]
 *   EIG3           s00 s01 s02 s11 s12 s22 -> the 3 diagonal entries after, then V[9] row-major
 *   NULL4          A[16] row-major -> v[4]            COMPOSE        E[9], R[9] -> E R [9]
 *   ROTATE         R[9], x, y, z -> Y[3]              (one thread per row up to here)
 *   WAVE_SUM       64 values -> each lane's own result of wave_sum_f64 (one wave per row)
 *   BLOCK_SUM      2 x 256 values -> what each of the 256 threads got from block_sum256_tree of
 *                  the first 256 and then, on the same LDS array, of the second (2 x 256)
 * SFM_EINVAL: a null pointer, n < 0 or n > 2^20, an unknown op; n == 0 launches nothing. */
#define SFM_GEOM_RODRIGUES 0
#define SFM_GEOM_RODRIGUES_INV 1
#define SFM_GEOM_EIG3 2
#define SFM_GEOM_NULL4 3
#define SFM_GEOM_COMPOSE 4
#define SFM_GEOM_ROTATE 5
#define SFM_GEOM_WAVE_SUM 6
#define SFM_GEOM_BLOCK_SUM 7
#define SFM_GEOM_OPS 8
int32_t sfm_debug_geom(int32_t device, int32_t op, const double* in, int64_t n, double* out);

/* Certified-mode NMS candidates (NaiveSIFT.py:77-95 with keys >= tnms[b]) of B planes:
 * unordered u64 keys ~fkey(R) << 32 | raster index in keys_out[b*H*W ...], counts_out[b] of
 * them.  tile = 1 forces the tiled kernel where the streaming one runs by default. */
int32_t sfm_debug_nms(int32_t device, const float* R, int32_t B, int32_t H, int32_t W, int32_t ksize,
                      const uint32_t* tnms, int32_t tile, uint64_t* keys_out, int64_t* counts_out);

/* The keypoint selection an extraction runs (NaiveSIFT.py:90-120), on host R planes instead of
 * Harris's: per level the digit-1 histogram of the planes' order keys (host), the select scan,
 * the certified NMS (not with force_exact) and then ONE selection launch over all the levels,
 * on the null stream, with buffers sized as an extraction sizes them (kcap = max(k, 1); the
 * levels' planes packed one after another, so a later level's planes need not be 16-B aligned).
 *   R[l]           host [B][H[l]][W[l]] float32, l < nlevels (1 .. 4 levels)
 *   x, y, conf     [nlevels][B][max(k, 1)] (slots past count[l][b] are 0), count [nlevels][B]
 *   state          [nlevels][B][SFM_SELECT_STATE_WORDS] u32: the plane's final selection state -
 *                  bucket[2], rank[2], odd, median (float bits; exact-path planes only), tnms,
 *                  tcert, fallback (1: took the exact path, by the scan or at run time), tsub[2]
 *   ncand          [nlevels][B] candidates of the certified NMS (0 with force_exact)
 *   consts         [SFM_SELECT_CONSTS] the sizes the selection's branches turn on, for this k:
 *                  keys sorted whole (sel_cap), its floor (kTopkDirect), confidence ties sorted in
 *                  LDS (kTieLdsCap), keys selected in registers, median-list keys held in LDS
 * consts is written before anything else is looked at except k; nlevels == 0 returns after that
 * without a device call.  SFM_EINVAL: what a context rejects (k < 0 or above 8192, an even ksize,
 * ksize / 2 > 15 when the certified NMS runs), B < 1, a level without pixels or of 2^26 and
 * more, a negative half_window, vmin < 3 (an extraction passes max(65536, 128 k); below 3 the
 * scan's ranks n - 3 vmin / 8 and n - vmin / 2 are not pixels), a null pointer. */
#define SFM_SELECT_STATE_WORDS 11
#define SFM_SELECT_CONSTS 5
int32_t sfm_debug_select(int32_t device, int32_t nlevels, int32_t B, const float* const* R, const int32_t* H,
                         const int32_t* W, const int32_t* half_window, int32_t k, int32_t ksize, int64_t vmin,
                         int32_t force_exact, int32_t* x, int32_t* y, float* conf, int32_t* count,
                         uint32_t* state, int64_t* ncand, int32_t* consts);

/* Mean time (ms) of one fused Harris launch on synthetic planes, ablation variant abl
 * (0 full, 1 no digit histogram, 2 window sums over the first tap row only). */
float sfm_debug_time_harris(int32_t device, int32_t abl, int32_t B, int32_t H, int32_t W,
                            int32_t iters);
/* As sfm_debug_time_harris; abl = 3 (full kernel + timestamps) also copies the last launch's
   per-workgroup records into out[cap] (48 u64 per workgroup: start, end, CU id, tiles, then
   the end of each tile; s_memrealtime ticks of 10 ns). */
float sfm_debug_harris_stamps(int32_t device, int32_t abl, int32_t B, int32_t H, int32_t W,
                              int32_t iters, uint64_t* out, int64_t cap);

/* Diagnostic build only (make ABLATIONS=1; -1 in the shipped library): the matcher sweep's
 * per-wave shader-clock stamps of its last launch under SFMFEAT_MATCH_ABL=32, u64
 * [16 workgroups][8 waves][41][4] (stages 0..39: after the stage barrier, after each sub-tile
 * region, after the DMA issue; row 40: start clock, start / end realtime, pair | stages << 32),
 * then u64 [1024 workgroups][4]: start / end realtime, __smid(), pair | row0 << 32. */
int64_t sfm_debug_match_stamps(uint64_t* out, int64_t cap);

/* The matcher's intermediate state, copied out of the context's workspaces (both calls
 * synchronise the device; host outputs; SFM_ESTATE on a SFMFEAT_MATCH_DIRECT context).
 *
 * sfm_debug_match_operands: the operands of slot `slot` of the table last prepped
 * (sfm_match_prep_dev, or the prep inside sfm_match / sfm_match_pairs_dev) or written by a fused
 * extraction on this context.  rows must be that table's capP (cap rounded up to 128, else
 * SFM_EINVAL).  hi, lo [rows][128]: the float16 bit patterns of f16(x * 2^8) and
 * f16((x * 2^8 - hi) * 2^11); norm2, rnorm [rows]: float32 of the squared norm summed in
 * double, and of its square root (rows at or beyond the slot's count: norm2 = +inf); pmax
 * [rows / 16][2]: the (norm2, rnorm) maxima of each block of 16 rows.  A row with an element
 * outside the float16 range has hi = lo = 0 and rnorm = +inf.  SFM_ESTATE when the context
 * holds no operands for that slot (no prep or fused extraction yet, or the slot is outside
 * the prepped table / the extraction's batch).
 *
 * sfm_debug_match_windows: the prefilter's windows of pair `pair` of the last sfm_match /
 * sfm_match_pairs*_dev call on this context, for its first `rows` query rows (1 <= rows <= that
 * call's cap).  cand_n [rows]: the two half-list counts (low / high 16 bits; the appends a
 * half-list saw, which may exceed its 128 entries: then, or when the count word is 0x7fff — the
 * row's error bound (2E, as the sweep carries it) was not finite —, the row was computed exactly
 * over all targets);
 * cand_thr [rows]: the row's final threshold b2~ + 2E; cand [rows][256]: the list words, half
 * h at [128 h ...): target index in the low 16 bits, d~ rounded down to bfloat16 in the high
 * 16.  Rows at or beyond the pair's first count, and every row of a pair whose second image is
 * empty, are not written.  SFM_ESTATE when that call ran as more than one sub-launch (the
 * workspaces then hold the last one only) or no call was made; SFM_EINVAL for pair outside it.
 *
 * sfm_debug_match_skips: of the same pair and rows, with the same argument and state rules,
 * skip [rows]: 1 for a row the sweep proved to fail the ratio test from its two smallest d~ and
 * E alone (the sweep wrote its "no match"; the exact re-rank never saw the row), else 0.
 * A row handed to the exact kernel is never flagged.  The rows sfm_debug_match_windows leaves
 * unwritten are unwritten here too. */
int32_t sfm_debug_match_operands(sfm_ctx* ctx, int32_t slot, int64_t rows, uint16_t* hi, uint16_t* lo,
                                 float* norm2, float* rnorm, float* pmax);
int32_t sfm_debug_match_windows(sfm_ctx* ctx, int32_t pair, int64_t rows, int32_t* cand_n, float* cand_thr,
                                uint32_t* cand);
int32_t sfm_debug_match_skips(sfm_ctx* ctx, int32_t pair, int64_t rows, uint8_t* skip);

/* Exchange emulation for a single-GPU rehearsal of the multi-GPU job (bench.py
 * --emulate-exchange): copy `bytes` from src to dst (device pointers, 16-B aligned) on
 * `stream` with exactly `workgroups` persistent 256-thread workgroups — the launch shape of a
 * collective kernel (one workgroup per channel) receiving the same bytes. */
int32_t sfm_copy_wg(void* dst, const void* src, int64_t bytes, int32_t workgroups, void* stream);

/* Keypoint selection of the context's last extraction (synchronises the device): planes
 * (image x level) that took the exact-median path, and planes in total.  The default
 * certified select decides the others from the Harris histogram alone. */
int32_t sfm_debug_select_stats(sfm_ctx* ctx, int32_t* fallback_planes, int32_t* total_planes);
/* The last sfm_ransac_camera_motion* call's per-sample result -> cand_idx [P][iters] (host):
 * the index of the sample's valid candidate in this library's order (R1, T), (R1, -T),
 * (R2, T), (R2, -T), or -1 (none valid, or the sample had no inlier and was skipped).
 * entries must be that call's P * iters (else SFM_ESTATE). */
int32_t sfm_debug_pose_candidates(sfm_ctx* ctx, int32_t* cand_idx, int64_t entries);
/* The per-sample fits of the last sfm_ransac_find_inliers* or sfm_ransac_camera_motion* call on
 * this context (host outputs; synchronises the device): F [P][iters][9], each sample's
 * fundamental matrix row-major as the count and selection kernels read it, and counts
 * [P][iters], its inlier count — after a pose call the count that the cheirality check has
 * zeroed for a sample without a valid candidate.  A copy of the workspaces; nothing is
 * recomputed.  Entries of a pair with n < 8 are unspecified (no kernel writes its F).  entries
 * must be that call's P * iters (else SFM_ESTATE; a single-pair host call with n < 8 runs
 * nothing and counts as 0 entries); SFM_EINVAL for a null pointer or entries < 0. */
int32_t sfm_debug_ransac_fits(sfm_ctx* ctx, double* F, int32_t* counts, int64_t entries);
/* The per-sample fits of the last sfm_pnp_ransac_dev call on this context and the start pose of
 * the last PnP call's refinement (host outputs; synchronises the device): hyp [iters][12], each
 * sample's hypothesis (R row-major, then t) as the count and selection kernels read it, all 12
 * NaN for a degenerate sample; counts [iters], its inlier count (0 for a NaN hypothesis);
 * start_Rt [12], the pose the refinement started from: the winning hypothesis (NaN without a
 * pose) or, after sfm_pnp_dev, the DLT's pose over all points.  A copy of the workspaces;
 * nothing is recomputed.  entries must be that call's iters, or 0 when it ran no sample (n < 6,
 * iters == 0) and after sfm_pnp_dev: then only start_Rt is written and hyp, counts may be null.
 * SFM_EINVAL with a message for any other entries, when the context has made no PnP call (or
 * its last one failed), for a null start_Rt, or for null hyp or counts with entries > 0. */
int32_t sfm_debug_pnp_fits(sfm_ctx* ctx, double* hyp, int32_t* counts, double* start_Rt, int64_t entries);
/* Level l's R maps (what 0) or level images (what 1) of the last extraction -> out [B][h][w]
 * (device, on `stream`; diagnostics).  what 2: the level's block-maximum maps as its Harris
 * launch wrote them -> out [B][sfm_debug_bmax_stride(h, w)], each plane's ceil(h / 4) x (w / 4)
 * map at its start; SFM_EINVAL when the level wrote none. */
int32_t sfm_debug_copy_level(sfm_ctx* ctx, int32_t l, int32_t what, float* out, void* stream);
/* Floats between the block-maximum maps of consecutive h x w planes (w % 4 == 0). */
int64_t sfm_debug_bmax_stride(int32_t h, int32_t w);
/* The certified 3x3 NMS's choice of kernel for every later extraction of this process: 1 = the
 * block-driven kernel wherever the shape allows it (W % 4 == 0, ksize 3), 0 = the band kernel
 * everywhere, -1 = by the size rule, n >= 2 = the size rule with the constant n, below -1 = as
 * the library was started (the diagnostic build's SFMFEAT_NMS_BLOCKS, else the size rule).  For the tests: the shipped library does not
 * read the switch. */
void sfm_debug_set_nms_blocks(int32_t mode);
/* Which kernel the size rule picks for a certified h x w level at per-level keypoint capacity
 * kcap and NMS window ksize: 1 = the block-driven kernel, 0 = the band kernel. */
int32_t sfm_debug_nms_blocks_rule(int32_t h, int32_t w, int32_t kcap, int32_t ksize);
/* The certified 3x3 NMS on B host planes R [B][H][W] (W % 4 == 0) with per-plane thresholds
 * tnms [B] and fallback flags [B] (a flagged plane yields nothing), as sfm_debug_nms: blocks = 0
 * runs the band kernel, 1 the block-driven kernel on maps computed on the host: each 4 x 4
 * block's maximum over its in-image pixels (NaN dropped) when inflate = 0, that maximum raised
 * (+inf on every third block, the next float up elsewhere) when inflate = 1 - any upper bound
 * must give the same candidates. */
int32_t sfm_debug_nms_blocks(int32_t device, const float* R, int32_t B, int32_t H, int32_t W, const uint32_t* tnms,
                             const uint32_t* fallback, int32_t blocks, int32_t inflate, uint64_t* keys_out,
                             int64_t* counts_out);


#ifdef __cplusplus
}
#endif

#endif /* SFMFEAT_H_ */
