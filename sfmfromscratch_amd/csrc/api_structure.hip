// api_structure.hip — the structure stage (refine.hip): refinement, reprojection error and the
// 2D -> 3D association of the triangulated points (workspace c->structure).  Every call is
// enqueued on the caller's stream and checks its arguments before touching the device.
#include "ctx.h"

using namespace sfm;

extern "C" {

int32_t sfm_refine_points_dev(sfm_ctx* c, const double* X0, const double* x1, const double* x2, int64_t N,
                              const double* P, int32_t S, const int32_t* seg, int32_t max_iter, double* X,
                              double* cost, int32_t* iters, void* stream) {
  if (!c) return SFM_EINVAL;
  if (N < 0) return set_err(c, SFM_EINVAL, "sfm_refine_points_dev: N is negative");
  if (S < 1) return set_err(c, SFM_EINVAL, "sfm_refine_points_dev: S < 1 (at least one camera pair)");
  if (max_iter < 1 || max_iter >= (1 << kRefineStatusShift))
    return set_err(c, SFM_EINVAL, "sfm_refine_points_dev: max_iter must be in [1, 2^24)");
  if (!P) return set_err(c, SFM_EINVAL, "sfm_refine_points_dev: P is null");
  if (N > 0 && (!X0 || !x1 || !x2 || !X || !cost || !iters))
    return set_err(c, SFM_EINVAL, "sfm_refine_points_dev: a point or output pointer is null");
  if (N > ((int64_t)1 << 37)) return set_err(c, SFM_EINVAL, "sfm_refine_points_dev: too many points");
  if (N == 0) return SFM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  launch_refine_points(X0, x1, x2, N, P, S, seg, max_iter, X, cost, iters, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

int32_t sfm_reprojection_error_dev(sfm_ctx* c, const double* X, const double* x1, const double* x2, int64_t N,
                                   const double* P1, const double* P2, double* err, double* mean, void* stream) {
  if (!c) return SFM_EINVAL;
  if (N < 0) return set_err(c, SFM_EINVAL, "sfm_reprojection_error_dev: N is negative");
  if (!P1 || !P2 || !mean) return set_err(c, SFM_EINVAL, "sfm_reprojection_error_dev: P1, P2 or mean is null");
  if (N > 0 && (!X || !x1 || !x2 || !err))
    return set_err(c, SFM_EINVAL, "sfm_reprojection_error_dev: a point or output pointer is null");
  if (N > ((int64_t)1 << 37)) return set_err(c, SFM_EINVAL, "sfm_reprojection_error_dev: too many points");
  HIPCHK(c, hipSetDevice(c->device));
  launch_reproj_error(X, x1, x2, N, P1, P2, err, mean, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

int32_t sfm_link_points_dev(sfm_ctx* c, const int32_t* tgt, int32_t m, const int32_t* qry, int32_t nq,
                            double threshold, int32_t* out_tgt, int32_t* out_qry, int32_t* out_n, void* stream) {
  if (!c) return SFM_EINVAL;
  if (m < 0 || nq < 0) return set_err(c, SFM_EINVAL, "sfm_link_points_dev: a size is negative");
  if (m == 0)
    return set_err(c, SFM_EINVAL,
                   "sfm_link_points_dev: no target points (the reference fails here: np.argmin of an empty "
                   "sequence, Runner.py:243)");
  if (!tgt || !out_n || (nq > 0 && (!qry || !out_tgt || !out_qry)))
    return set_err(c, SFM_EINVAL, "sfm_link_points_dev: a point or output pointer is null");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  if (nq == 0) {
    HIPCHK(c, hipMemsetAsync(out_n, 0, 4, st));
    return SFM_OK;
  }
  int rc;
  StructWs& w = c->structure;
  if ((rc = ensure(c, w.best, (size_t)nq * 4))) return rc;
  if ((rc = ensure(c, w.block_kept, (size_t)link_blocks(nq) * 4))) return rc;
  launch_link_points(tgt, m, qry, nq, threshold, as<int32_t>(w.best), as<int32_t>(w.block_kept), out_tgt, out_qry,
                     out_n, st);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

}  // extern "C"
