// api_extract.hip — the per-batch launch sequence of detect + describe (workspace c->ex).
//
// Launch sequence for a batch of B same-size images (no host sync inside):
//   pyramid (L-1 resize launches, or fused into the level-0 Harris launch)
//   per level: harris(+digit histogram, select scan) -> nms/candidates -> top-k + edge filter
//   per level: descriptors into the caller's slot table; finalize counts
// Buffer sizes and every per-level offset come from extract_layout() (extract_layout.h).
#include "ctx.h"

using namespace sfm;

static_assert(kLayoutMedBins == kMedBins1 && kLayoutCounterStride == kCounterStride &&
                  kLayoutMedianStateBytes == sizeof(MedianState) && kLayoutSelectMaxLevels == kSelectMaxLevels,
              "extract_layout.h mirrors kernels.h");
static_assert(layout_bmax_stride(1080, 1920) == bmax_plane_stride(1080, 1920) &&
                  layout_bmax_stride(270, 480) == bmax_plane_stride(270, 480) &&
                  layout_bmax_stride(70, 132) == bmax_plane_stride(70, 132),
              "extract_layout.h mirrors kernels.h");

// sfm_debug_set_nms_blocks (debug_nms.hip): the tests' override of SFMFEAT_NMS_BLOCKS, which
// the shipped library does not read (-2: none)
static int g_nms_blocks_override = -2;
void extract_set_nms_blocks(int mode) { g_nms_blocks_override = mode < -1 ? -2 : mode; }

LayoutSwitches extract_layout_switches() {
  LayoutSwitches s = extract_switches().layout;
  if (g_nms_blocks_override != -2) s.nms_blocks = g_nms_blocks_override;
  return s;
}

const ExtractSwitches& extract_switches() {
  static const ExtractSwitches sw = [] {
    ExtractSwitches s;
    // SFMFEAT_PYR_FUSED=0: the pyramid by k_down2x3 / resize launches (A/B)
    s.layout.pyr_fused = env_int(getenv("SFMFEAT_PYR_FUSED"), 1) != 0;
    // levels of fewer than 128 x kcap pixels (the certified select's vmin) skip certification:
    // they hardly ever certify (4K level 3 never did), and the attempt costs a certified NMS
    // pass and a top-k before the exact path (configs[4] 8.85k -> 9.02k img/s with 128 against
    // 64; 1080p takes the same levels either way).  SFMFEAT_EXACT_PX=n: n x kcap (A/B)
    s.layout.exact_px = env_int(getenv("SFMFEAT_EXACT_PX"), 128);
    // SFMFEAT_SELECT_MERGE=0: one selection launch per caller-stream level
    s.layout.select_merge = env_int(SFM_DIAG_ENV("SFMFEAT_SELECT_MERGE"), 1) != 0;
    // SFMFEAT_NMS_BLOCKS=0: the band kernel at every level; =1: the block-driven certified NMS
    // (and Harris's block-maximum map) wherever the shape allows it; =n (n >= 2): the size rule
    // with the constant n; default: the size rule (extract_layout.h nms_blocks_level)
    s.layout.nms_blocks = env_int(SFM_DIAG_ENV("SFMFEAT_NMS_BLOCKS"), -1);
    s.fill_launches = env_int(SFM_DIAG_ENV("SFMFEAT_FILL_LAUNCHES"), 0) != 0;
    // Harris launches: one per level, unless SFMFEAT_HARRIS_GROUP=g (g >= 1): levels >= g then
    // share launches (up to kHarrisMaxLevels each).  Off by default: grouping L1-L3 or L2-L3 cut
    // the Harris stage time by ~2% but the pipeline lost more overlap than that (DESIGN_LOG.md §B).
    s.harris_group = env_int(SFM_DIAG_ENV("SFMFEAT_HARRIS_GROUP"), 0);
    // the lane gate's release point: after the Harris launch of level gate_level (default 0:
    // the next gated extraction's pyramid and level-0 Harris follow this one's level-0 Harris;
    // SFMFEAT_GATE_LEVEL=-1: after every level's Harris and NMS)
    s.gate_level = env_int(SFM_DIAG_ENV("SFMFEAT_GATE_LEVEL"), 0);
    // SFMFEAT_SELECT_CALLER=1 (A/B): an aux level's selection on the caller's stream ahead of
    // the next level's Harris, only its descriptors on aux
    s.select_caller = env_int(SFM_DIAG_ENV("SFMFEAT_SELECT_CALLER"), 0) == 1;
    // SFMFEAT_SKIP=mask: stages whose launches are left out from a context's second extraction
    // on (the first fills every buffer the skipped stages' consumers read) — 1 keypoint
    // selection, 2 descriptors, 8 match sweep + re-rank, 16 Harris of the levels above 0
    s.skip = env_int(SFM_ABLATION_ENV("SFMFEAT_SKIP"), 0);
    return s;
  }();
  return sw;
}

namespace {

int layout_of(sfm_ctx* c, int B, int H, int W, ExtractLayout* y) {
  if (extract_layout(&c->p, c->kcap, B, H, W, c->serial, extract_layout_switches(), y) != SFM_OK)
    return set_err(c, SFM_EINVAL, "image too small for the pyramid");
  return SFM_OK;
}

int reserve(sfm_ctx* c, const ExtractLayout& y) {
  for (int i = 0; i < kExtractBufs; ++i)
    if (int rc = ensure(c, c->ex.buf[i], y.bytes[i])) return rc;
  return SFM_OK;
}

// One extraction in flight: the layout resolved to pointers, and the launches of one level.
struct Extraction {
  sfm_ctx* c;
  const ExtractSwitches& sw;
  const ExtractLayout& y;
  int B, skip;
  hipStream_t st;  // the caller's stream
  // outputs: the caller's slot table and (fused) the matcher operands
  int32_t* xy;
  float* desc;
  float* conf;
  int32_t* count;
  int64_t cap;
  MatchOperands mo;
  const float* lvl[SFM_MAX_LEVELS];
  unsigned long long *medcnt, *candcnt, *donecnt;
  bool zeroed;           // histograms and append counters are zeroed (or a launch will)
  bool fused_ok;         // every describe launch so far wrote its operands
  bool counted = false;  // the last level's describe launch wrote the slot counts
  bool gate_released = false;
  bool mapped[SFM_MAX_LEVELS] = {};  // the level's Harris launch wrote its block-maximum map

  template <class T>
  T* at(ExtractBuf b, int64_t off) const {
    return as<T>(c->ex.buf[b]) + off;
  }
  float* R(int l) const { return at<float>(kBufR, y.plane[l]); }
  uint64_t* cand(int l) const { return at<uint64_t>(kBufCand, y.plane[l]); }
  float* bmax(int l) const { return at<float>(kBufBmax, y.bmax[l]); }
  MedianState* med(int l) const { return at<MedianState>(kBufMed, y.state[l]); }
  bool exact(int l) const { return c->exact_select || y.exact[l]; }
  KpList kp(int l) const {
    return KpList{at<int32_t>(kBufKpx, y.kp[l]), at<int32_t>(kBufKpy, y.kp[l]), at<float>(kBufKpc, y.kp[l]),
                  at<int32_t>(kBufLc, y.state[l])};
  }

  // levels [from, L) from their predecessors: three exact 2x levels from one read of their
  // source where the sizes allow (the first such pass also zeroes the histograms and append
  // counters), else one resize per level
  void pyramid_from(int from) {
    const Level* lv = y.lv;
    for (int l = from; l < y.L;) {
      const Level& s = lv[l - 1];
      const bool x2 = l + 2 < y.L && lv[l].h * 2 == s.h && lv[l].w * 2 == s.w && lv[l + 1].h * 4 == s.h &&
                      lv[l + 1].w * 4 == s.w && lv[l + 2].h * 8 == s.h && lv[l + 2].w * 8 == s.w;
      if (x2 && launch_down2x3(lvl[l - 1], s.h, s.w, const_cast<float*>(lvl[l]), const_cast<float*>(lvl[l + 1]),
                               const_cast<float*>(lvl[l + 2]), B, st, zeroed ? nullptr : c->ex.buf[kBufHist].p,
                               y.bytes[kBufHist], zeroed ? nullptr : c->ex.buf[kBufCounts].p, y.bytes[kBufCounts])) {
        zeroed = true;
        l += 3;
        continue;
      }
      launch_resize(lvl[l - 1], s.h, s.w, const_cast<float*>(lvl[l]), lv[l].h, lv[l].w, B, st);
      ++l;
    }
  }

  void harris(int l0, int l1) {
    StageScope sc(c, SFM_PROF_HARRIS, st);
    // certified select: at least max(65536, 128 k) pixels at or above the threshold
    const int64_t vmin = std::max<int64_t>(65536, (int64_t)128 * c->kcap);
    HarrisLevels g{};
    g.n = l1 - l0;
    for (int l = l0; l < l1; ++l) {
      HarrisLevels::Level& q = g.l[l - l0];
      q.lvl = lvl[l];
      q.R = R(l);
      q.hist = at<uint32_t>(kBufHist, y.hist[l]);
      q.H = y.lv[l].h;
      q.W = y.lv[l].w;
      q.scan = SelectScan{med(l), medcnt + y.counter[l], donecnt + y.counter[l], vmin, exact(l) ? 1 : 0};
      q.down[0] = q.down[1] = q.down[2] = nullptr;
      if (y.pyr_fused && l == 0)
        for (int k = 0; k < 3; ++k) q.down[k] = const_cast<float*>(lvl[1 + k]);
    }
    // The block-maximum map of a level the layout gave one: written by the 64 x 64 form of a
    // launch of its own, from 16-B aligned planes of R, and only where launch_nms will read it.
    // By the size rule a level keeps the Harris form it would take without a map; the forced
    // switch (a diagnostic) makes it take the 64 x 64 form.
    if (l1 - l0 == 1 && y.bmax[l0] >= 0 && ((uintptr_t)R(l0) & 15) == 0 &&
        nms_blocks_shape(y.lv[l0].w, c->p.ksize, 0) &&
        (extract_layout_switches().nms_blocks == 1 || harris_tiles_64(g, B, c->p.gaussian_size))) {
      g.l[0].bmax = bmax(l0);
      mapped[l0] = true;
      c->ex.last_mapped |= 1u << l0;
    }
    ProfilerWs& pr = c->prof;
    if (pr.span_cap > 0) {
      if (pr.span_n < pr.span_cap) {
        g.span = as<unsigned long long>(pr.spans) + 2 * pr.span_n++;
        pr.span_level.push_back(l0);
      } else {
        ++pr.span_dropped;
      }
    }
    const float alpha = (float)c->p.alpha;  // NEP 50: the python float becomes float32
    if (!(l0 > 0 && (skip & 16))) launch_harris_levels(g, B, as<float>(c->ex.gauss), c->p.gaussian_size, alpha, st);
  }

  void select_level(int l, hipStream_t s) {  // top-k, exact path in the same launch
    StageScope sc(c, SFM_PROF_TOPK, s);
    if (skip & 1) return;
    launch_select(R(l), cand(l), candcnt + y.counter[l], at<uint32_t>(kBufMedlist, y.sel[l]),
                  at<uint64_t>(kBufScratch, y.sel[l]), kp(l), std::max(c->kcap, 1), c->kcap, B, y.lv[l].h, y.lv[l].w,
                  c->p.ksize, y.lv[l].fw / 2, med(l), s);
  }

  // the caller stream's levels in one launch (each level its own scratch regions)
  void select_merged() {
    StageScope sc(c, SFM_PROF_TOPK, st);
    SelectLevels g{};
    g.n = y.L - y.L_aux;
    for (int l = y.L_aux; l < y.L; ++l)
      g.l[l - y.L_aux] = SelectLevels::Level{R(l), cand(l), candcnt + y.counter[l], at<uint32_t>(kBufMedlist, y.sel[l]),
                                             at<uint64_t>(kBufScratch, y.sel[l]), kp(l), med(l), y.lv[l].h, y.lv[l].w,
                                             y.lv[l].fw / 2};
    if (!(skip & 1)) launch_select_levels(g, std::max(c->kcap, 1), c->kcap, B, c->p.ksize, st);
  }

  void describe_level(int l, hipStream_t s) {
    StageScope sc(c, SFM_PROF_DESCRIBE, s);
    const int L = y.L;
    if ((skip & 2) && l != L - 1) {
      fused_ok = false;
      return;
    }
    bool ow = false;
    const bool r = launch_describe(lvl[l], B, y.lv[l].h, y.lv[l].w, y.lv[l].fw, c->p.mode == SFM_MODE_NAIVE ? 0 : 1,
                                   kp(l), c->kcap, as<int32_t>(c->ex.buf[kBufLc]), l, L, y.lv[l].scale, xy, desc, conf,
                                   cap, l == L - 1 ? count : nullptr, mo, &ow, s);
    if (l == L - 1) counted = r;
    fused_ok = fused_ok && ow;
  }

  int release_gate() {
    if (c->gate && !gate_released) {
      HIPCHK(c, hipEventRecord(c->gate->ev, st));
      c->gate->armed = true;
      gate_released = true;
    }
    return SFM_OK;
  }

  int run(const float* imgs);
};

int Extraction::run(const float* imgs) {
  const int L = y.L, L_aux = y.L_aux;
  CtxStreams& cs = c->s;
  int rc;
  lvl[0] = imgs;
  for (int l = 1; l < L; ++l) lvl[l] = at<float>(kBufLvl, y.lvl[l]);
  zeroed = sw.fill_launches;
  // Fused pyramid (y.pyr_fused; round 4: 35.6k -> 37.3k img/s at configs[1]): level 0 is read
  // from HBM once, levels >= 4 follow the level-0 Harris launch, and the histograms / counters
  // take the fill launches instead of k_down2x3's side job.
  {
    StageScope sc(c, SFM_PROF_PYRAMID, st);
    if (!y.pyr_fused) pyramid_from(1);
  }
  // fused matcher operands: buffers for the B slots (plus spare slots, so a match of the table
  // with a few extra slots, e.g. BatchPipeline's halo slot, does not reallocate them), their
  // per-block maxima zeroed ahead of the descriptor launches' atomic maxima
  if ((rc = operands_fused_begin(c, desc, count, cap, B, &mo))) return rc;
  if (mo.hi) HIPCHK(c, hipMemsetAsync(mo.pmax, 0, (size_t)B * match_pmax_bytes(mo.capP), st));
  fused_ok = mo.hi != nullptr;
  if (!zeroed || sw.fill_launches) {
    HIPCHK(c, hipMemsetAsync(c->ex.buf[kBufHist].p, 0, y.bytes[kBufHist], st));
    HIPCHK(c, hipMemsetAsync(c->ex.buf[kBufCounts].p, 0, y.bytes[kBufCounts], st));
    // the fused pyramid's later k_down2x3 (pyramid_from(4), after level 0's Harris) must not
    // zero them again: level 0's histogram and counters are live by then
    zeroed = true;
  }
  medcnt = as<unsigned long long>(c->ex.buf[kBufCounts]);
  candcnt = medcnt + y.counter_block;      // certified NMS (block 2: the fallback NMS's)
  donecnt = medcnt + 3 * y.counter_block;  // Harris arrivals
  // Fork/join over two streams.  The caller's stream runs Harris (+ fused select scan) and
  // the certified NMS of every level; the keypoint selection (top-k, the exact path for
  // the planes flagged `fallback`) and the descriptors of the two largest levels run on
  // `aux`, overlapping the later levels' Harris; the small levels' selection and
  // descriptors run on the caller's stream once its Harris work is done.  Descriptors of
  // level l need the keypoint counts of levels < l (slot offsets): ev[L + 2 + l].
  // serial (SFMFEAT_SERIAL=1 or sfm_ctx_set_serial): one stream, no fork/join at all
  hipStream_t ax = nullptr;
  if (L_aux > 0) {
    if (!cs.aux) HIPCHK(c, hipStreamCreateWithPriority(&cs.aux, hipStreamNonBlocking, cs.prio));  // on first use
    ax = cs.aux;
    HIPCHK(c, hipEventRecord(cs.ev[L], st));
    HIPCHK(c, hipStreamWaitEvent(ax, cs.ev[L], 0));
  }
  for (int l0 = 0; l0 < L;) {
    int l1 = l0 + 1;
    if (sw.harris_group > 0 && l0 >= sw.harris_group) l1 = std::min(L, l0 + kHarrisMaxLevels);
    harris(l0, l1);
    if (y.pyr_fused && l0 == 0 && L > 4) {
      StageScope sc(c, SFM_PROF_PYRAMID, st);
      pyramid_from(4);
    }
    if (sw.gate_level >= l0 && sw.gate_level < l1 && (rc = release_gate())) return rc;
    for (int l = l0; l < l1; ++l) {
      if (!exact(l)) {
        StageScope sc(c, SFM_PROF_NMS, st);
        launch_nms(R(l), med(l), cand(l), candcnt + y.counter[l], B, y.lv[l].h, y.lv[l].w, c->p.ksize, 0, st, 0,
                   mapped[l] ? bmax(l) : nullptr);
      }
      if (l < L_aux) {
        if (sw.select_caller) select_level(l, st);
        HIPCHK(c, hipEventRecord(cs.ev[l], st));
        HIPCHK(c, hipStreamWaitEvent(ax, cs.ev[l], 0));
        if (!sw.select_caller) select_level(l, ax);
        if (l == L_aux - 1) HIPCHK(c, hipEventRecord(cs.ev[L + 2], ax));  // counts of the aux levels known
        describe_level(l, ax);
      }
    }
    l0 = l1;
  }
  if ((rc = release_gate())) return rc;  // (SFMFEAT_GATE_LEVEL=-1, or fewer levels)
  if (y.select_merged) {
    select_merged();
  } else {
    for (int l = L_aux; l < L; ++l) select_level(l, st);
  }
  if (L_aux > 0 && L > L_aux) HIPCHK(c, hipStreamWaitEvent(st, cs.ev[L + 2], 0));
  for (int l = L_aux; l < L; ++l) describe_level(l, st);
  if (L_aux > 0) {  // join: the caller's stream waits for the aux work
    HIPCHK(c, hipEventRecord(cs.ev[L + 1], ax));
    HIPCHK(c, hipStreamWaitEvent(st, cs.ev[L + 1], 0));
  }
  if (!counted) launch_finalize_counts(as<int32_t>(c->ex.buf[kBufLc]), B, L, count, st);
  HIPCHK(c, hipGetLastError());
  // every level's descriptors (and the padding rows) carry operands
  if (fused_ok && counted) operands_fused_commit(c, B);
  return SFM_OK;
}

}  // namespace

int extract_reserve(sfm_ctx* c, int B, int H, int W) {
  ExtractLayout y;
  if (int rc = layout_of(c, B, H, W, &y)) return rc;
  return reserve(c, y);
}

int extract_impl(sfm_ctx* c, const float* imgs, int B, int H, int W, int32_t* xy, float* desc, float* conf,
                 int32_t* count, int64_t cap, hipStream_t st) {
  if (B < 1 || H < 1 || W < 1) return set_err(c, SFM_EINVAL, "empty batch or image");
  if (cap < c->cap) return set_err(c, SFM_ERANGE, "slot capacity below L * int(k / L)");
  ExtractLayout y;
  int rc;
  if ((rc = layout_of(c, B, H, W, &y)) || (rc = reserve(c, y))) return rc;
  const ExtractSwitches& sw = extract_switches();
  ExtractWs& x = c->ex;
  const int skip = x.extractions++ > 0 ? sw.skip : 0;
  if (c->gate && c->gate->armed) HIPCHK(c, hipStreamWaitEvent(st, c->gate->ev, 0));
  x.last_B = B;
  x.last_H = H;
  x.last_W = W;
  x.last_mapped = 0;
  operands_fused_clear(c);  // (a failed or non-fused extraction leaves no fused slots)
  Extraction e{c, sw, y, B, skip, st, xy, desc, conf, count, cap, MatchOperands{nullptr, nullptr, nullptr, nullptr, nullptr, 0}};
  return e.run(imgs);
}

extern "C" {

int32_t sfm_reserve(sfm_ctx* c, int32_t B, int32_t H, int32_t W) {
  if (!c || B < 1 || H < 1 || W < 1) return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  return extract_reserve(c, B, H, W);
}

int32_t sfm_extract_batch_dev(sfm_ctx* c, const float* imgs, int32_t B, int32_t H, int32_t W,
                              int32_t* xy, float* desc, int32_t* count, int64_t cap, void* stream) {
  if (!c || !imgs || !xy || !desc || !count) return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;  // exactly the caller's stream (NULL = null stream)
  return extract_impl(c, imgs, B, H, W, xy, desc, nullptr, count, cap, st);
}

int32_t sfm_extract_batch_u8_dev(sfm_ctx* c, const uint8_t* imgs, int32_t B, int32_t H, int32_t W,
                                 int32_t* xy, float* desc, int32_t* count, int64_t cap, void* stream) {
  if (!c || !imgs || !xy || !desc || !count || B < 1 || H < 1 || W < 1) return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;  // exactly the caller's stream (NULL = null stream)
  int rc = extract_reserve(c, B, H, W);
  if (rc) return rc;
  float* img0 = as<float>(c->ex.buf[kBufImg0]);
  launch_u8_to_f32(imgs, img0, (int64_t)B * H * W, st);
  return extract_impl(c, img0, B, H, W, xy, desc, nullptr, count, cap, st);
}

int32_t sfm_extract(sfm_ctx* c, const float* img, int32_t H, int32_t W, int64_t row_stride, int64_t* X,
                    int64_t* Y, float* desc, float* conf, int64_t cap, int64_t* n_out,
                    int32_t* level_counts) {
  if (!c || !img || !n_out) return SFM_EINVAL;
  if (H < 1 || W < 1 || row_stride < W) return set_err(c, SFM_EINVAL, "bad image shape or stride");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = extract_reserve(c, 1, H, W);
  if (rc) return rc;
  ExtractWs& x = c->ex;
  const int64_t scap = std::max<int64_t>(c->cap, 1);
  if ((rc = ensure(c, x.xy, (size_t)scap * 8))) return rc;
  if ((rc = ensure(c, x.desc, (size_t)scap * 128 * 4))) return rc;
  if ((rc = ensure(c, x.count, 16))) return rc;
  if ((rc = ensure(c, x.conf, (size_t)scap * 4))) return rc;
  hipStream_t st;
  if ((rc = host_stream(c, &st))) return rc;
  float* img0 = as<float>(x.buf[kBufImg0]);
  HIPCHK(c, hipMemcpy2DAsync(img0, (size_t)W * 4, img, (size_t)row_stride * 4, (size_t)W * 4, H,
                             hipMemcpyHostToDevice, st));
  rc = extract_impl(c, img0, 1, H, W, as<int32_t>(x.xy), as<float>(x.desc), as<float>(x.conf), as<int32_t>(x.count),
                    scap, st);
  if (rc) return rc;
  int32_t n = 0;
  std::vector<int32_t> lc(c->L);
  HIPCHK(c, hipMemcpyAsync(&n, x.count.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(lc.data(), x.buf[kBufLc].p, (size_t)c->L * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  *n_out = n;
  if (level_counts) memcpy(level_counts, lc.data(), (size_t)c->L * 4);
  if (n > cap) return set_err(c, SFM_ERANGE, "output capacity too small");
  if (n > 0) {
    std::vector<int32_t> hxy((size_t)n * 2);
    HIPCHK(c, hipMemcpyAsync(hxy.data(), x.xy.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    if (desc) HIPCHK(c, hipMemcpyAsync(desc, x.desc.p, (size_t)n * 128 * 4, hipMemcpyDeviceToHost, st));
    if (conf) HIPCHK(c, hipMemcpyAsync(conf, x.conf.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int32_t i = 0; i < n; ++i) {
      if (X) X[i] = hxy[2 * i];
      if (Y) Y[i] = hxy[2 * i + 1];
    }
  }
  return SFM_OK;
}

}  // extern "C"
