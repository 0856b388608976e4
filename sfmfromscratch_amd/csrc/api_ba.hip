// api_ba.hip — bundle adjustment over the registry (ba.hip; workspace c->ba).  The call checks
// its arguments before touching the device, sizes the workspace and enqueues every launch on the
// caller's stream; it never synchronises (growing the workspace frees the old buffers, which
// waits for the device as every hipFree does).
#include <math.h>

#include "ctx.h"

using namespace sfm;

static_assert(kBaMaxCams == SFM_BA_MAX_CAMERAS && kBaMaxPoints == SFM_BA_MAX_POINTS &&
                  kBaMaxObs == SFM_BA_MAX_OBSERVATIONS,
              "kernels.h and include/sfmfeat.h disagree on the bundle-adjustment limits");

extern "C" {

int32_t sfm_bundle_adjust_dev(sfm_ctx* c, const int32_t* cam_idx, const int32_t* pt_idx, const double* obs,
                              int64_t M, const double* camera_params, int32_t n_cam, const double* K,
                              const double* X, int32_t n_pts, const uint8_t* cam_fixed, double ftol,
                              int32_t max_iter, double* out_camera_params, double* out_X, double* out_cost,
                              int32_t* out_status, void* stream) {
  if (!c) return SFM_EINVAL;
  if (n_cam < 1 || n_cam > kBaMaxCams)
    return set_err(c, SFM_EINVAL, "sfm_bundle_adjust_dev: n_cam must be in [1, 256]");
  if (n_pts < 0 || n_pts > kBaMaxPoints)
    return set_err(c, SFM_EINVAL, "sfm_bundle_adjust_dev: n_pts must be in [0, 2^24]");
  if (M < 0 || M > kBaMaxObs) return set_err(c, SFM_EINVAL, "sfm_bundle_adjust_dev: M must be in [0, 2^26]");
  if (!(ftol >= 0.0)) return set_err(c, SFM_EINVAL, "sfm_bundle_adjust_dev: ftol must be >= 0 (and not NaN)");
  if (max_iter < 1 || max_iter >= (1 << kRefineStatusShift))
    return set_err(c, SFM_EINVAL, "sfm_bundle_adjust_dev: max_iter must be in [1, 2^24)");
  if (!camera_params || !K || !out_camera_params)
    return set_err(c, SFM_EINVAL, "sfm_bundle_adjust_dev: camera_params, K or out_camera_params is null");
  if (n_pts > 0 && (!X || !out_X)) return set_err(c, SFM_EINVAL, "sfm_bundle_adjust_dev: X or out_X is null");
  if (M > 0 && (!cam_idx || !pt_idx || !obs))
    return set_err(c, SFM_EINVAL, "sfm_bundle_adjust_dev: cam_idx, pt_idx or obs is null");
  if (M > 0 && n_pts < 1) return set_err(c, SFM_EINVAL, "sfm_bundle_adjust_dev: observations without points");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) {  // nothing to fit: the inputs, cost 0, status 0
    if (out_camera_params != camera_params)
      HIPCHK(c, hipMemcpyAsync(out_camera_params, camera_params, (size_t)n_cam * 48, hipMemcpyDeviceToDevice, st));
    if (n_pts > 0 && out_X != X)
      HIPCHK(c, hipMemcpyAsync(out_X, X, (size_t)n_pts * 24, hipMemcpyDeviceToDevice, st));
    if (out_cost) HIPCHK(c, hipMemsetAsync(out_cost, 0, 16, st));
    if (out_status) HIPCHK(c, hipMemsetAsync(out_status, 0, 16, st));
    return SFM_OK;
  }
  BaWs& w = c->ba;
  const size_t m = (size_t)M, nc = (size_t)n_cam, np = (size_t)n_pts, n6 = 6 * nc;
  int rc;
  if ((rc = ensure(c, w.st, sizeof(BaState)))) return rc;
  if ((rc = ensure(c, w.Rt, 2 * nc * 12 * 8))) return rc;
  if ((rc = ensure(c, w.Xs, 2 * np * 3 * 8))) return rc;
  if ((rc = ensure(c, w.cam_i, (3 * nc + 1) * 4 + m * 4))) return rc;  // cnt, off, active, list
  if ((rc = ensure(c, w.pt_cnt, np * 4))) return rc;
  if ((rc = ensure(c, w.pt_off, (np + 1) * 4))) return rc;
  if ((rc = ensure(c, w.pt_list, m * 4))) return rc;
  if ((rc = ensure(c, w.pos, m * 4))) return rc;
  if ((rc = ensure(c, w.lin, m * 20 * 8))) return rc;
  if ((rc = ensure(c, w.e2, m * 8))) return rc;
  if ((rc = ensure(c, w.pts, np * 12 * 8))) return rc;  // vinv, gp, vg
  if ((rc = ensure(c, w.lcam, m * 4))) return rc;
  if ((rc = ensure(c, w.Wm, m * 18 * 8))) return rc;
  if ((rc = ensure(c, w.Y, m * 18 * 8))) return rc;
  if ((rc = ensure(c, w.S, n6 * n6 * 8))) return rc;
  const int split = ba_schur_split(n_cam);
  if ((rc = ensure(c, w.Spart, nc * split * ba_schur_lds_bytes(n_cam)))) return rc;
  if ((rc = ensure(c, w.vec, 2 * n6 * 8))) return rc;  // b, delta
  if ((rc = ensure(c, w.nrm, (np + nc) * 2 * 8))) return rc;
  BaProblem p;
  p.cam_idx = cam_idx, p.pt_idx = pt_idx, p.obs = obs, p.M = (int)M;
  p.cams_in = camera_params, p.n_cam = n_cam, p.K = K, p.X_in = X, p.n_pts = n_pts, p.cam_fixed = cam_fixed;
  p.ftol = ftol, p.max_iter = max_iter;
  p.st = as<BaState>(w.st), p.Rt = as<double>(w.Rt), p.Xs = as<double>(w.Xs);
  p.cam_cnt = as<int32_t>(w.cam_i);
  p.cam_off = p.cam_cnt + nc;
  p.cam_active = p.cam_off + nc + 1;
  p.cam_list = p.cam_active + nc;
  p.pt_cnt = as<int32_t>(w.pt_cnt), p.pt_off = as<int32_t>(w.pt_off), p.pt_list = as<int32_t>(w.pt_list);
  p.pos = as<int32_t>(w.pos), p.lin = as<double>(w.lin), p.e2 = as<double>(w.e2);
  p.vinv = as<double>(w.pts), p.gp = p.vinv + 6 * np, p.vg = p.gp + 3 * np;
  p.lcam = as<int32_t>(w.lcam), p.Wm = as<double>(w.Wm), p.Y = as<double>(w.Y);
  p.Spart = as<double>(w.Spart), p.schur_split = split;
  p.S = as<double>(w.S), p.b = as<double>(w.vec), p.delta = p.b + n6, p.nrm = as<double>(w.nrm);
  p.out_cams = out_camera_params, p.out_X = out_X, p.out_cost = out_cost, p.out_status = out_status;
  HIPCHK(c, hipMemsetAsync(p.cam_cnt, 0, nc * 4, st));
  HIPCHK(c, hipMemsetAsync(p.pt_cnt, 0, np * 4, st));
  launch_bundle_adjust(p, st);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

}  // extern "C"
