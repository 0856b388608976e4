// api_stage1.hip — the stages around detect + describe + match: frame ingest (workspace
// c->ingest), RANSAC inlier search (workspace c->ransac) and the initial pair's pose RANSAC
// with triangulation (workspace c->pose, on top of c->ransac's samples, F and counts).
#include <atomic>
#include <thread>

#include "ctx.h"

using namespace sfm;

namespace {

int ingest_impl(sfm_ctx* c, const uint8_t* rgb, int B, int H, int W, int H2, int W2, float* gray,
                hipStream_t st) {
  int rc;
  IngestWs& g = c->ingest;
  const bool newh = g.w != W || g.w2 != W2, newv = g.h != H || g.h2 != H2;
  const size_t tmp_bytes = (size_t)B * H * W2 * 3 + 16;
  // The tables and the temp are the context's, and the previous call's kernels may still read
  // them on `st` (the call is not synchronised): a new shape, or a larger temp, first waits for
  // that work, then uploads on `st` itself.  A blocking hipMemcpy would be ordered against the
  // null stream only, which a non-blocking stream such as torch's side streams never joins.
  if (newh || newv || g.tmp.bytes < tmp_bytes) HIPCHK(c, hipStreamSynchronize(st));
  if (newh) {
    g.w = g.w2 = -1;
    g.ksh = build_resample_table(W, W2, g.th);
    if ((rc = ensure(c, g.tab_h, g.th.size() * 4))) return rc;
    HIPCHK(c, hipMemcpyAsync(g.tab_h.p, g.th.data(), g.th.size() * 4, hipMemcpyHostToDevice, st));
  }
  if (newv) {
    g.h = g.h2 = -1;
    g.ksv = build_resample_table(H, H2, g.tv);
    if ((rc = ensure(c, g.tab_v, g.tv.size() * 4))) return rc;
    HIPCHK(c, hipMemcpyAsync(g.tab_v.p, g.tv.data(), g.tv.size() * 4, hipMemcpyHostToDevice, st));
  }
  if (newh || newv) {
    std::vector<int32_t> cm, sets;
    const int ks = ingest_rows_ks(g.ksh, g.ksv);
    g.rows = ks && ingest_rows_tables(g.th, g.ksh, W, W2, ks, cm, sets);
    if (g.rows) {
      if ((rc = ensure(c, g.colmap, cm.size() * 4))) return rc;
      if ((rc = ensure(c, g.sets, sets.size() * 4))) return rc;
      HIPCHK(c, hipMemcpyAsync(g.colmap.p, cm.data(), cm.size() * 4, hipMemcpyHostToDevice, st));
      HIPCHK(c, hipMemcpyAsync(g.sets.p, sets.data(), sets.size() * 4, hipMemcpyHostToDevice, st));
      g.nsets = (int)(sets.size() / ks);
    }
    HIPCHK(c, hipStreamSynchronize(st));  // cm and sets are locals; as PnpWs's sample stream
    g.w = W, g.w2 = W2, g.h = H, g.h2 = H2;  // only now: a failed upload is redone by the next call
  }
  if ((rc = ensure(c, g.tmp, tmp_bytes))) return rc;
  launch_ingest_rgb(rgb, as<uint8_t>(g.tmp), gray, as<int32_t>(g.tab_h), g.ksh, as<int32_t>(g.tab_v), g.ksv,
                    g.rows ? as<int32_t>(g.colmap) : nullptr, as<int32_t>(g.sets), g.nsets, B, H, W, H2, W2, st);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

constexpr size_t kRansacCacheCap = 256;  // cached (n, iterations) streams per context (~190 KB each)

const std::vector<int32_t>* ransac_cached(sfm_ctx* c, int n, int iters) {
  for (auto& e : c->ransac.cache)
    if (e.first.first == n && e.first.second == iters) return &e.second;
  return nullptr;
}

// Replays the sample streams of every size in `ns` not cached yet, the sizes spread over
// host threads (each walks the shared raw MT19937 words on its own), and caches them.
void ransac_prefetch_streams(sfm_ctx* c, const std::vector<int>& ns, int iters) {
  std::vector<int> todo;
  for (int n : ns)
    if (!ransac_cached(c, n, iters)) todo.push_back(n);
  if (todo.empty()) return;
  std::vector<std::vector<int32_t>> out(todo.size());
  std::atomic<size_t> next{0};
  auto work = [&]() {
    for (size_t i; (i = next.fetch_add(1)) < todo.size();) {
      out[i].resize((size_t)iters * 8);
      ransac_sample_indices(todo[i], iters, 5u, out[i].data());  // np.random.seed(5), SFM.py:133
    }
  };
  const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const size_t nt = std::min<size_t>(todo.size(), hw);
  std::vector<std::thread> pool;
  for (size_t t = 1; t < nt; ++t) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
  auto& cache = c->ransac.cache;
  for (size_t i = 0; i < todo.size(); ++i) cache.push_back({{todo[i], iters}, std::move(out[i])});
  // trim: the oldest streams this call does not use go first
  for (auto it = cache.begin(); cache.size() > kRansacCacheCap && it != cache.end();) {
    if (it->first.second != iters || std::find(ns.begin(), ns.end(), it->first.first) == ns.end())
      it = cache.erase(it);
    else
      ++it;
  }
}

// host K [P][18] and base [P][12] of a pose call, its host outputs
struct PoseJob {
  const double* K;
  const double* base;
  double* out_R;
  double* out_t;
};

// pose == nullptr: find_inliers; else ransac_camera_motion (the cheirality check between the
// count and the selection, the winners' (R, t) copied to the job's host outputs)
int ransac_impl(sfm_ctx* c, const int32_t* pts, const int32_t* npts_dev, const int32_t* npts_host, int P, int nmax,
                int iters, double thr, int32_t* out_pts, int32_t* out_n, int32_t* out_iter, hipStream_t st,
                const PoseJob* pose = nullptr) {
  // sample streams (host replay of numpy's RandomState; identical for equal n)
  {
    std::vector<int> ns;
    for (int p = 0; p < P; ++p) {
      const int n = npts_host[p];
      if (n > nmax) return set_err(c, SFM_EINVAL, "correspondence count above nmax");
      if (n >= 8 && std::find(ns.begin(), ns.end(), n) == ns.end()) ns.push_back(n);
    }
    ransac_prefetch_streams(c, ns, iters);
  }
  std::vector<int32_t> all, off(P, 0);
  std::vector<int> seen_n;
  std::vector<int32_t> seen_off;
  for (int p = 0; p < P; ++p) {
    const int n = npts_host[p];
    if (n < 8 || n > nmax) {
      if (n > nmax) return set_err(c, SFM_EINVAL, "correspondence count above nmax");
      continue;
    }
    int k = -1;
    for (size_t i = 0; i < seen_n.size(); ++i)
      if (seen_n[i] == n) k = (int)i;
    if (k < 0) {
      const std::vector<int32_t>& s = *ransac_cached(c, n, iters);
      seen_n.push_back(n);
      seen_off.push_back((int32_t)all.size());
      all.insert(all.end(), s.begin(), s.end());
      k = (int)seen_n.size() - 1;
    }
    off[p] = seen_off[k];
  }
  if (all.empty()) all.assign(8, 0);
  int rc;
  RansacWs& r = c->ransac;
  if ((rc = ensure(c, r.idx, all.size() * 4))) return rc;
  if ((rc = ensure(c, r.off, (size_t)P * 4))) return rc;
  if ((rc = ensure(c, r.F, (size_t)P * std::max(iters, 1) * 9 * 8))) return rc;
  if ((rc = ensure(c, r.counts, (size_t)P * std::max(iters, 1) * 4))) return rc;
  HIPCHK(c, hipMemcpyAsync(r.idx.p, all.data(), all.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(r.off.p, off.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
  r.last_entries = (int64_t)P * iters;
  if (pose) {
    PoseWs& w = c->pose;
    const size_t slots = (size_t)P * std::max(iters, 1);
    if ((rc = ensure(c, w.K, (size_t)P * 18 * 8))) return rc;
    if ((rc = ensure(c, w.base, (size_t)P * 12 * 8))) return rc;
    if ((rc = ensure(c, w.cand, slots * 21 * 8))) return rc;
    if ((rc = ensure(c, w.cand_idx, slots * 4))) return rc;
    if ((rc = ensure(c, w.Rt, (size_t)P * 12 * 8))) return rc;
    HIPCHK(c, hipMemcpyAsync(w.K.p, pose->K, (size_t)P * 18 * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(w.base.p, pose->base, (size_t)P * 12 * 8, hipMemcpyHostToDevice, st));
    launch_ransac_pose(pts, npts_dev, nmax, P, as<int32_t>(r.idx), as<int32_t>(r.off), iters, thr, as<double>(w.K),
                       as<double>(w.base), as<double>(r.F), as<int32_t>(r.counts), as<double>(w.cand),
                       as<int32_t>(w.cand_idx), out_pts, out_n, out_iter, as<double>(w.Rt), st);
    HIPCHK(c, hipGetLastError());
    w.last_entries = (int64_t)P * iters;
    std::vector<int32_t> oit(P);
    std::vector<double> rt((size_t)P * 12);
    HIPCHK(c, hipMemcpyAsync(oit.data(), out_iter, (size_t)P * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(rt.data(), w.Rt.p, rt.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int p = 0; p < P; ++p) {
      if (oit[p] < 0) continue;  // no pose: the caller's R, t stay as they are
      std::copy(rt.begin() + 12 * p, rt.begin() + 12 * p + 9, pose->out_R + 9 * p);
      std::copy(rt.begin() + 12 * p + 9, rt.begin() + 12 * p + 12, pose->out_t + 3 * p);
    }
    return SFM_OK;
  }
  // iters == 0 still launches the select kernel: it writes every pair's empty / None result
  launch_ransac(pts, npts_dev, nmax, P, as<int32_t>(r.idx), as<int32_t>(r.off), iters, thr, as<double>(r.F),
                as<int32_t>(r.counts), out_pts, out_n, out_iter, st);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(st));  // the host index buffers above are stack-owned
  return SFM_OK;
}

// one pair through host pointers (int64 points): staging, ransac_impl, the inliers copied back
int ransac_host_pair(sfm_ctx* c, const int64_t* p1, const int64_t* p2, int64_t n, int iters, double threshold,
                     int64_t* in1, int64_t* in2, int64_t* n_out, int32_t* best_iter, const PoseJob* pose) {
  if (n > INT32_MAX / 4) return set_err(c, SFM_EINVAL, "too many correspondences");
  HIPCHK(c, hipSetDevice(c->device));
  *n_out = -1;
  if (n < 8) {  // the reference returns (None, None, None, None); nothing ran: no fits to read back
    c->ransac.last_entries = 0;
    return SFM_OK;
  }
  const int nmax = (int)n;
  std::vector<int32_t> h((size_t)nmax * 4);
  for (int64_t i = 0; i < n; ++i) {
    h[4 * i + 0] = (int32_t)p1[2 * i];
    h[4 * i + 1] = (int32_t)p1[2 * i + 1];
    h[4 * i + 2] = (int32_t)p2[2 * i];
    h[4 * i + 3] = (int32_t)p2[2 * i + 1];
  }
  int rc;
  RansacWs& r = c->ransac;
  if ((rc = ensure(c, r.pts, h.size() * 4))) return rc;
  if ((rc = ensure(c, r.npts, 16))) return rc;
  if ((rc = ensure(c, r.out, h.size() * 4))) return rc;
  if ((rc = ensure(c, r.on, 16))) return rc;
  if ((rc = ensure(c, r.oit, 16))) return rc;
  hipStream_t st;
  if ((rc = host_stream(c, &st))) return rc;
  const int32_t nn = (int32_t)n;
  HIPCHK(c, hipMemcpyAsync(r.pts.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(r.npts.p, &nn, 4, hipMemcpyHostToDevice, st));
  if ((rc = ransac_impl(c, as<int32_t>(r.pts), as<int32_t>(r.npts), &nn, 1, nmax, iters, threshold,
                        as<int32_t>(r.out), as<int32_t>(r.on), as<int32_t>(r.oit), st, pose)))
    return rc;
  int32_t k = 0, bi = -1;
  HIPCHK(c, hipMemcpyAsync(&k, r.on.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(&bi, r.oit.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (k > n) return set_err(c, SFM_EDEVICE, "inlier count above the correspondence count");
  if (k > 0) {
    std::vector<int32_t> o((size_t)k * 4);
    HIPCHK(c, hipMemcpy(o.data(), r.out.p, o.size() * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < k; ++i) {
      if (in1) { in1[2 * i] = o[4 * i]; in1[2 * i + 1] = o[4 * i + 1]; }
      if (in2) { in2[2 * i] = o[4 * i + 2]; in2[2 * i + 1] = o[4 * i + 3]; }
    }
  }
  *n_out = k;
  if (best_iter) *best_iter = bi;
  return SFM_OK;
}

}  // namespace

const std::vector<int32_t>& ransac_stream(sfm_ctx* c, int n, int iters) {
  ransac_prefetch_streams(c, {n}, iters);
  return *ransac_cached(c, n, iters);
}

extern "C" {

int32_t sfm_resize_dims(int32_t H, int32_t W, double scale, int32_t* H2, int32_t* W2) {
  if (!H2 || !W2 || H < 1 || W < 1 || !(scale > 0.0)) return SFM_EINVAL;
  const double h = (double)H * scale, w = (double)W * scale;  // int(shape * scale_factor)
  if (h < 1.0 || w < 1.0 || h > 65535.0 || w > 65535.0) return SFM_EINVAL;
  *H2 = (int32_t)h;
  *W2 = (int32_t)w;
  return SFM_OK;
}

int32_t sfm_ingest_rgb_dev(sfm_ctx* c, const uint8_t* rgb, int32_t B, int32_t H, int32_t W, int32_t H2,
                           int32_t W2, float* gray, void* stream) {
  if (!c || !rgb || !gray || B < 1 || H < 1 || W < 1 || H2 < 1 || W2 < 1 || H2 > 65535 || W2 > 65535)
    return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  return ingest_impl(c, rgb, B, H, W, H2, W2, gray, (hipStream_t)stream);
}

int32_t sfm_ingest_rgb(sfm_ctx* c, const uint8_t* rgb, int32_t H, int32_t W, int32_t H2, int32_t W2,
                       float* gray) {
  if (!c || !rgb || !gray || H < 1 || W < 1 || H2 < 1 || W2 < 1 || H2 > 65535 || W2 > 65535)
    return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  IngestWs& g = c->ingest;
  if ((rc = ensure(c, g.rgb, (size_t)H * W * 3))) return rc;
  if ((rc = ensure(c, g.gray, (size_t)H2 * W2 * 4))) return rc;
  hipStream_t st;
  if ((rc = host_stream(c, &st))) return rc;
  HIPCHK(c, hipMemcpyAsync(g.rgb.p, rgb, (size_t)H * W * 3, hipMemcpyHostToDevice, st));
  if ((rc = ingest_impl(c, as<uint8_t>(g.rgb), 1, H, W, H2, W2, as<float>(g.gray), st))) return rc;
  HIPCHK(c, hipMemcpyAsync(gray, g.gray.p, (size_t)H2 * W2 * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return SFM_OK;
}

int32_t sfm_ransac_sample_indices(int32_t n, int32_t iters, uint32_t seed, int32_t* out) {
  if (n < 8 || iters < 0 || !out) return SFM_EINVAL;
  ransac_sample_indices(n, iters, seed, out);
  return SFM_OK;
}

int32_t sfm_ransac_sample_indices_k(int32_t n, int32_t iters, uint32_t seed, int32_t size, int32_t* out) {
  if (size < 1 || n < size || iters < 0 || !out) return SFM_EINVAL;
  ransac_sample_indices_k(n, iters, seed, size, out);
  return SFM_OK;
}

int32_t sfm_ransac_find_inliers_dev(sfm_ctx* c, const int32_t* pts, const int32_t* npts, const int32_t* npts_host,
                                    int32_t P, int32_t nmax, int32_t iters, double threshold, int32_t* out_pts,
                                    int32_t* out_n, int32_t* out_iter, void* stream) {
  if (!c || !pts || !npts || !npts_host || !out_pts || !out_n || !out_iter || P < 1 || nmax < 1 || iters < 0)
    return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  return ransac_impl(c, pts, npts, npts_host, P, nmax, iters, threshold, out_pts, out_n, out_iter,
                     (hipStream_t)stream);
}

int32_t sfm_ransac_find_inliers(sfm_ctx* c, const int64_t* p1, const int64_t* p2, int64_t n, int32_t iters,
                                double threshold, int64_t* in1, int64_t* in2, int64_t* n_out, int32_t* best_iter) {
  if (!c || !n_out || n < 0 || iters < 0 || (n > 0 && (!p1 || !p2))) return SFM_EINVAL;
  return ransac_host_pair(c, p1, p2, n, iters, threshold, in1, in2, n_out, best_iter, nullptr);
}

int32_t sfm_ransac_camera_motion_dev(sfm_ctx* c, const int32_t* pts, const int32_t* npts, const int32_t* npts_host,
                                     int32_t P, int32_t nmax, int32_t iters, double threshold, const double* K,
                                     const double* base, int32_t* out_pts, int32_t* out_n, int32_t* out_iter,
                                     double* out_R, double* out_t, void* stream) {
  if (!c || !pts || !npts || !npts_host || !K || !base || !out_pts || !out_n || !out_iter || !out_R || !out_t ||
      P < 1 || nmax < 1 || iters < 0)
    return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  const PoseJob job{K, base, out_R, out_t};
  return ransac_impl(c, pts, npts, npts_host, P, nmax, iters, threshold, out_pts, out_n, out_iter,
                     (hipStream_t)stream, &job);
}

int32_t sfm_ransac_camera_motion(sfm_ctx* c, const int64_t* p1, const int64_t* p2, int64_t n, const double* K1,
                                 const double* K2, const double* R_base, const double* T_base, int32_t iters,
                                 double threshold, double* R, double* t, int64_t* in1, int64_t* in2,
                                 int64_t* n_out, int32_t* best_iter) {
  if (!c || !n_out || !K1 || !K2 || !R_base || !T_base || !R || !t || n < 0 || iters < 0 ||
      (n > 0 && (!p1 || !p2)))
    return SFM_EINVAL;
  double Kc[18], base[12];
  std::copy(K1, K1 + 9, Kc);
  std::copy(K2, K2 + 9, Kc + 9);
  std::copy(R_base, R_base + 9, base);
  std::copy(T_base, T_base + 3, base + 9);
  const PoseJob job{Kc, base, R, t};
  return ransac_host_pair(c, p1, p2, n, iters, threshold, in1, in2, n_out, best_iter, &job);
}

int32_t sfm_debug_pose_candidates(sfm_ctx* c, int32_t* cand_idx, int64_t entries) {
  if (!c || !cand_idx || entries < 0) return SFM_EINVAL;
  if (entries != c->pose.last_entries) return set_err(c, SFM_ESTATE, "not the last pose call's P * iters");
  if (entries == 0) return SFM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpy(cand_idx, c->pose.cand_idx.p, (size_t)entries * 4, hipMemcpyDeviceToHost));
  return SFM_OK;
}

int32_t sfm_debug_ransac_fits(sfm_ctx* c, double* F, int32_t* counts, int64_t entries) {
  if (!c || !F || !counts || entries < 0) return SFM_EINVAL;
  if (entries != c->ransac.last_entries) return set_err(c, SFM_ESTATE, "not the last RANSAC call's P * iters");
  if (entries == 0) return SFM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpy(F, c->ransac.F.p, (size_t)entries * 9 * 8, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(counts, c->ransac.counts.p, (size_t)entries * 4, hipMemcpyDeviceToHost));
  return SFM_OK;
}

int32_t sfm_triangulate_dev(sfm_ctx* c, const double* x1, const double* x2, int64_t N, const double* P1,
                            const double* P2, int32_t normalize, double* X, void* stream) {
  if (!c || N < 0 || !P1 || !P2 || (normalize != 0 && normalize != 1) || (N > 0 && (!x1 || !x2 || !X)))
    return SFM_EINVAL;
  if (N > ((int64_t)1 << 37)) return set_err(c, SFM_EINVAL, "too many points");
  if (N == 0) return SFM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure(c, c->pose.tri, 30 * 8))) return rc;
  launch_triangulate(x1, x2, N, P1, P2, normalize != 0, as<double>(c->pose.tri), X, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

}  // extern "C"
