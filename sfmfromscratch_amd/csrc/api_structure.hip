// api_structure.hip — the structure stage (refine.hip): refinement, reprojection error and the
// 2D -> 3D association of the triangulated points (workspace c->structure), then what follows
// them (registry.hip): the global point registry and the total reprojection error (workspace
// c->registry, the table itself being the caller's).  Every call is
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

int32_t sfm_registry_add_dev(sfm_ctx* c, double* reg_xyz, int32_t* reg_count, int32_t reg_capacity,
                             const double* pts, int32_t n, double threshold, int32_t* out_index,
                             int32_t* out_is_new, void* stream) {
  if (!c) return SFM_EINVAL;
  if (n < 0 || reg_capacity < 0) return set_err(c, SFM_EINVAL, "sfm_registry_add_dev: a size is negative");
  if (!(threshold > 0.0)) return set_err(c, SFM_EINVAL, "sfm_registry_add_dev: threshold must be positive");
  if (!reg_xyz || !reg_count) return set_err(c, SFM_EINVAL, "sfm_registry_add_dev: reg_xyz or reg_count is null");
  if (n > 0 && (!pts || !out_index || !out_is_new))
    return set_err(c, SFM_EINVAL, "sfm_registry_add_dev: pts, out_index or out_is_new is null");
  if (reg_capacity < n)
    return set_err(c, SFM_EINVAL, "sfm_registry_add_dev: reg_capacity < n (capacity >= count + n is required)");
  if (reg_capacity > (1 << 30) || n > (1 << 24))
    return set_err(c, SFM_EINVAL, "sfm_registry_add_dev: at most 2^30 registered and 2^24 incoming points");
  if (n == 0) return SFM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc, splits_old, splits_self;
  (void)registry_span(reg_capacity, &splits_old);
  (void)registry_span(n, &splits_self);
  RegistryWs& w = c->registry;
  if ((rc = ensure(c, w.part_d, (size_t)splits_old * n * 8))) return rc;
  if ((rc = ensure(c, w.part_j, (size_t)splits_old * n * 4))) return rc;
  if ((rc = ensure(c, w.self_d, (size_t)splits_self * n * 8))) return rc;
  if ((rc = ensure(c, w.old_d, (size_t)n * 8))) return rc;
  if ((rc = ensure(c, w.old_j, (size_t)n * 4))) return rc;
  if ((rc = ensure(c, w.res, (size_t)n * 4))) return rc;
  if ((rc = ensure(c, w.clist, (size_t)n * 4))) return rc;
  launch_registry_add(reg_xyz, reg_count, reg_capacity, pts, n, threshold, as<double>(w.part_d),
                      as<int32_t>(w.part_j), as<double>(w.self_d), as<double>(w.old_d), as<int32_t>(w.old_j),
                      as<int32_t>(w.res), as<int32_t>(w.clist), out_index, out_is_new, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

int32_t sfm_total_reprojection_error_dev(sfm_ctx* c, const int32_t* cam_idx, const int32_t* pt_idx,
                                         const double* obs, int64_t M, const double* camera_params, int32_t n_cam,
                                         const double* K, const double* X, int32_t n_pts, double* err, double* mean,
                                         void* stream) {
  if (!c) return SFM_EINVAL;
  if (M < 0) return set_err(c, SFM_EINVAL, "sfm_total_reprojection_error_dev: M is negative");
  if (!mean) return set_err(c, SFM_EINVAL, "sfm_total_reprojection_error_dev: mean is null");
  if (M > 0 && (!cam_idx || !pt_idx || !obs || !camera_params || !K || !X || !err))
    return set_err(c, SFM_EINVAL, "sfm_total_reprojection_error_dev: an input or output pointer is null");
  if (M > 0 && (n_cam < 1 || n_pts < 1))
    return set_err(c, SFM_EINVAL, "sfm_total_reprojection_error_dev: observations without cameras or points");
  if (M > ((int64_t)1 << 37)) return set_err(c, SFM_EINVAL, "sfm_total_reprojection_error_dev: too many observations");
  HIPCHK(c, hipSetDevice(c->device));
  launch_total_reproj(cam_idx, pt_idx, obs, M, camera_params, n_cam, K, X, n_pts, err, mean, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

}  // extern "C"
