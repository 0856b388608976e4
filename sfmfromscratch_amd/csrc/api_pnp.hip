// api_pnp.hip — the pose of a frame from its 2D-3D links (pnp.hip; workspace c->pnp).  Both
// calls check their arguments before touching the device and are enqueued on the caller's
// stream; the only synchronisation is the upload of a sample stream the context has not yet
// got on the device.
#include "ctx.h"

using namespace sfm;

namespace {

// the [iters][stride] sample stream of (n, iters) on the device: c->ransac's cached host
// stream (n >= 8, stride 8) or the size-6 draw (6 <= n < 8, stride 6)
int pnp_stream(sfm_ctx* c, int n, int iters, hipStream_t st) {
  PnpWs& w = c->pnp;
  if (w.idx_n == n && w.idx_iters == iters) return SFM_OK;
  int rc;
  std::vector<int32_t> small;
  const std::vector<int32_t>* h;
  int stride;
  if (n >= 8) {
    h = &ransac_stream(c, n, iters);  // np.random.seed(5), as every RANSAC of the reference
    stride = 8;
  } else {
    small.resize((size_t)iters * 6);
    ransac_sample_indices_k(n, iters, 5u, 6, small.data());
    h = &small;
    stride = 6;
  }
  w.idx_n = w.idx_iters = -1;
  if ((rc = ensure(c, w.idx, h->size() * 4))) return rc;
  HIPCHK(c, hipMemcpyAsync(w.idx.p, h->data(), h->size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));  // the host stream may move or go before the copy runs
  w.idx_n = n;
  w.idx_iters = iters;
  w.idx_stride = stride;
  return SFM_OK;
}

}  // namespace

extern "C" {

int32_t sfm_pnp_ransac_dev(sfm_ctx* c, const double* X, const double* x, const double* K, int32_t n, int32_t iters,
                           double threshold, int32_t max_refine_iter, double* R, double* t, int32_t* out_inliers,
                           int32_t* out_n, int32_t* out_iter, int32_t* out_status, double* out_cost,
                           int32_t* out_counts, void* stream) {
  if (!c) return SFM_EINVAL;
  if (n < 0 || iters < 0) return set_err(c, SFM_EINVAL, "sfm_pnp_ransac_dev: n or iters is negative");
  if (!(threshold > 0.0)) return set_err(c, SFM_EINVAL, "sfm_pnp_ransac_dev: threshold must be positive");
  if (max_refine_iter < 1 || max_refine_iter >= (1 << kRefineStatusShift))
    return set_err(c, SFM_EINVAL, "sfm_pnp_ransac_dev: max_refine_iter must be in [1, 2^24)");
  if (!K || !R || !t || !out_n || !out_iter || !out_status || !out_cost)
    return set_err(c, SFM_EINVAL, "sfm_pnp_ransac_dev: K or an output pointer is null");
  if (n > 0 && (!X || !x || !out_inliers))
    return set_err(c, SFM_EINVAL, "sfm_pnp_ransac_dev: X, x or out_inliers is null");
  if (n > (1 << 28)) return set_err(c, SFM_EINVAL, "sfm_pnp_ransac_dev: at most 2^28 points");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  int rc;
  PnpWs& w = c->pnp;
  const bool sampled = n >= 6 && iters > 0;
  if (sampled && (rc = pnp_stream(c, n, iters, st))) return rc;
  if ((rc = ensure(c, w.idx, 16))) return rc;
  if ((rc = ensure(c, w.hyp, (size_t)std::max(iters, 1) * 12 * 8))) return rc;
  if ((rc = ensure(c, w.Rt, 12 * 8))) return rc;
  // the kernels count into the caller's table when there is one; the workspace's gets a copy
  // below (sfm_debug_pnp_fits reads the workspace: the caller's table may be gone by then)
  if ((rc = ensure(c, w.counts, (size_t)std::max(iters, 1) * 4))) return rc;
  int32_t* counts = out_counts ? out_counts : as<int32_t>(w.counts);
  if (out_counts && !sampled && iters > 0)
    HIPCHK(c, hipMemsetAsync(out_counts, 0, (size_t)iters * 4, st));  // n < 6: no sample counts anything
  w.last_entries = -1;
  launch_pnp_ransac(X, x, K, n, as<int32_t>(w.idx), w.idx_stride, iters, threshold, max_refine_iter,
                    as<double>(w.hyp), counts, as<double>(w.Rt), out_inliers, out_n, out_iter, R, t, out_status,
                    out_cost, st);
  HIPCHK(c, hipGetLastError());
  if (out_counts && sampled)
    HIPCHK(c, hipMemcpyAsync(w.counts.p, out_counts, (size_t)iters * 4, hipMemcpyDeviceToDevice, st));
  w.last_entries = sampled ? iters : 0;
  return SFM_OK;
}

int32_t sfm_pnp_dev(sfm_ctx* c, const double* X, const double* x, const double* K, int32_t n,
                    int32_t max_refine_iter, double* R, double* t, int32_t* out_status, double* out_cost,
                    void* stream) {
  if (!c) return SFM_EINVAL;
  if (n < 0) return set_err(c, SFM_EINVAL, "sfm_pnp_dev: n is negative");
  if (max_refine_iter < 1 || max_refine_iter >= (1 << kRefineStatusShift))
    return set_err(c, SFM_EINVAL, "sfm_pnp_dev: max_refine_iter must be in [1, 2^24)");
  if (!K || !R || !t || !out_status || !out_cost)
    return set_err(c, SFM_EINVAL, "sfm_pnp_dev: K or an output pointer is null");
  if (n > 0 && (!X || !x)) return set_err(c, SFM_EINVAL, "sfm_pnp_dev: X or x is null");
  if (n > (1 << 28)) return set_err(c, SFM_EINVAL, "sfm_pnp_dev: at most 2^28 points");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure(c, c->pnp.Rt, 12 * 8))) return rc;
  c->pnp.last_entries = -1;
  launch_pnp(X, x, K, n, max_refine_iter, as<double>(c->pnp.Rt), R, t, out_status, out_cost, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  c->pnp.last_entries = 0;
  return SFM_OK;
}

int32_t sfm_debug_pnp_fits(sfm_ctx* c, double* hyp, int32_t* counts, double* start_Rt, int64_t entries) {
  if (!c) return SFM_EINVAL;
  if (!start_Rt || entries < 0 || (entries > 0 && (!hyp || !counts)))
    return set_err(c, SFM_EINVAL, "sfm_debug_pnp_fits: a null pointer or entries < 0");
  if (c->pnp.last_entries < 0) return set_err(c, SFM_EINVAL, "sfm_debug_pnp_fits: no PnP call on this context");
  if (entries != c->pnp.last_entries)
    return set_err(c, SFM_EINVAL, "sfm_debug_pnp_fits: not the last PnP call's samples");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());  // the call ran on the caller's stream
  HIPCHK(c, hipMemcpy(start_Rt, c->pnp.Rt.p, 12 * 8, hipMemcpyDeviceToHost));
  if (entries == 0) return SFM_OK;
  HIPCHK(c, hipMemcpy(hyp, c->pnp.hyp.p, (size_t)entries * 12 * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(counts, c->pnp.counts.p, (size_t)entries * 4, hipMemcpyDeviceToHost));
  return SFM_OK;
}

}  // extern "C"
