// extract_layout.h — the device layout of one batch extraction, computed in one place.
//
// Host-only (no HIP header: tests/test_extract_layout_cpu.py builds it with plain g++).  The
// workspace reservation, the launch sequence and sfm_debug_copy_level all read the levels,
// buffer sizes and per-level offsets from extract_layout(); it is recomputed per call.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sfmfeat.h"

namespace sfm {

// device constants the sizes depend on (api_extract.hip asserts them against kernels.h)
constexpr int kLayoutMedBins = 2048;        // kMedBins1
constexpr int kLayoutCounterStride = 32;    // kCounterStride
constexpr int kLayoutMedianStateBytes = 44; // sizeof(MedianState)
constexpr int kLayoutSelectMaxLevels = 4;   // kSelectMaxLevels
constexpr int kLayoutCounterBlocks = 4;     // median list, certified NMS, fallback NMS, Harris arrivals

struct Level {
  int h, w, fw;
  double scale;
};

// the extraction's workspace buffers, in reservation order
enum ExtractBuf {
  kBufImg0,     // f32 [B][H][W]: level 0 of the u8 / host-pointer entry points
  kBufLvl,      // f32 levels 1..L-1, packed by level
  kBufR,        // f32 R maps, packed by level
  kBufHist,     // u32 [L][B][kMedBins1]
  kBufMed,      // MedianState [L][B]
  kBufMedlist,  // u32 selection regions (exact-median lists)
  kBufCounts,   // u64 [4][L][B][kCounterStride]
  kBufCand,     // u64 NMS candidates, packed by level like R
  kBufScratch,  // u64 selection regions (tie lists)
  kBufKpx,      // i32 [L][B][max(kcap, 1)]
  kBufKpy,
  kBufKpc,      // f32, same shape
  kBufLc,       // i32 [L][B] keypoint counts per level
  kBufBmax,     // f32 block-maximum maps of the levels that carry one: [B] planes of ceil(h / 4) x (w / 4)
  kExtractBufs
};

// the switches that change the layout (SFMFEAT_PYR_FUSED, SFMFEAT_EXACT_PX, SFMFEAT_SELECT_MERGE,
// SFMFEAT_NMS_BLOCKS)
struct LayoutSwitches {
  bool pyr_fused = true;
  int exact_px = 128;
  bool select_merge = true;
  // -1: the size rule below; 0: no level; 1: every level whose shape allows it; n >= 2: the size
  // rule with the constant n in kNmsBlocksC's place (measurements)
  int nms_blocks = -1;
};

// The certified select's volume threshold (api_extract.hip): about vmin pixels of a plane lie at
// or above its candidate threshold.
inline int64_t select_vmin(int kcap) { return 65536 > (int64_t)128 * kcap ? 65536 : (int64_t)128 * kcap; }

// Which certified 3x3 NMS a level takes, from sizes only: the block-driven kernel (nms.hip
// k_nms_blocks, fed by a block-maximum map the Harris launch writes) pays where the pixels that
// can be candidates, about vmin of them, are a small share of the plane: h w >= kNmsBlocksC vmin.
// At the share 1 / kNmsBlocksC and below, most 4 x 4 blocks hold none (DESIGN_LOG.md §W).
constexpr int kNmsBlocksC = 4;
// floats between the maps of consecutive planes (kernels.h bmax_plane_stride: packed where
// h % 4 == 0, h w / 4 apart otherwise; each map is ceil(h / 4) x (w / 4), w % 4 == 0)
constexpr int64_t layout_bmax_stride(int h, int w) { return h % 4 == 0 ? (int64_t)h * w / 16 : (int64_t)h * w / 4; }
inline bool nms_blocks_shape_ok(int w, int ksize) { return ksize / 2 == 1 && w >= 4 && w % 4 == 0; }
inline bool nms_blocks_level(int h, int w, int kcap, int ksize, bool exact, int sw) {
  if (sw == 0 || exact || !nms_blocks_shape_ok(w, ksize)) return false;
  return sw == 1 || (int64_t)h * w >= (sw > 1 ? sw : kNmsBlocksC) * select_vmin(kcap);
}

struct ExtractLayout {
  int L = 0;
  int L_aux = 0;          // levels whose selection + descriptors run on the aux stream
  bool pyr_fused = false; // levels 1-3 written by the level-0 Harris launch
  bool select_merged = false;  // the caller stream's levels select in one launch
  Level lv[SFM_MAX_LEVELS];
  bool exact[SFM_MAX_LEVELS];  // too small to certify (a size-only decision)
  size_t bytes[kExtractBufs];
  // element offsets of level l
  int64_t plane[SFM_MAX_LEVELS];    // kBufR, kBufCand
  int64_t lvl[SFM_MAX_LEVELS];      // kBufLvl (level 0 is the caller's image: 0, unused)
  int64_t hist[SFM_MAX_LEVELS];     // kBufHist
  int64_t state[SFM_MAX_LEVELS];    // kBufMed, kBufLc
  int64_t kp[SFM_MAX_LEVELS];       // kBufKpx / Kpy / Kpc
  int64_t counter[SFM_MAX_LEVELS];  // inside each of the kBufCounts blocks
  int64_t counter_block = 0;        // u64 per counter block
  // kBufMedlist / kBufScratch: the aux stream's levels share region [0, B H W); the caller
  // stream's levels start behind it: each level its own region packed by level when one launch
  // selects them all (SFMFEAT_SERIAL, no aux levels: packed from 0), else one region they use
  // in turn
  int64_t sel[SFM_MAX_LEVELS];
  int64_t bmax[SFM_MAX_LEVELS];     // kBufBmax; -1: the level carries no block-maximum map
};

// The pyramid of an H x W image: level sizes, window widths and scales.
inline int extract_levels(const sfm_params* p, int H, int W, Level* lv, int* L_out) {
  const bool naive = p->mode == SFM_MODE_NAIVE;
  const int L = naive ? 1 : p->pyramid_level;
  if (L < 1 || L > SFM_MAX_LEVELS) return SFM_EINVAL;
  int h = H, w = W;
  for (int l = 0; l < L; ++l) {
    if (l > 0) {
      h = (int)((double)h / p->pyramid_scale_factor);  // int(h / s) (ScaleRotInvSIFT.py:114)
      w = (int)((double)w / p->pyramid_scale_factor);
    }
    if (h <= 0 || w <= 0) return SFM_EINVAL;
    const double scale = naive ? 1.0 : pow(p->pyramid_scale_factor, (double)l);
    int fw = naive ? p->feature_width : (int)((double)p->feature_width / scale);
    if (!naive && fw < 3) fw = 3;  // min_feature_width (:92,:96)
    lv[l] = Level{h, w, fw, scale};
  }
  *L_out = L;
  return SFM_OK;
}

inline int extract_layout(const sfm_params* p, int kcap, int B, int H, int W, bool serial, const LayoutSwitches& sw,
                          ExtractLayout* out) {
  ExtractLayout& y = *out;
  if (extract_levels(p, H, W, y.lv, &y.L) != SFM_OK) return SFM_EINVAL;
  const int L = y.L;
  const Level* lv = y.lv;
  // serial: one stream, no fork/join at all
  y.L_aux = serial ? 0 : (L < 2 ? L : 2);
  // Levels 1-3 exact 2x below level 0 (H, W multiples of 8): the level-0 Harris launch writes
  // them from its image tiles in LDS
  y.pyr_fused = sw.pyr_fused && L >= 4 && H % 8 == 0 && W % 8 == 0 && lv[1].h * 2 == H && lv[1].w * 2 == W &&
                lv[2].h * 4 == H && lv[2].w * 4 == W && lv[3].h * 8 == H && lv[3].w * 8 == W;
  y.select_merged = sw.select_merge && L - y.L_aux > 1 && L - y.L_aux <= kLayoutSelectMaxLevels;
  const int64_t A0 = (int64_t)H * W, kslots = kcap > 1 ? kcap : 1;
  int64_t plane = 0, lvl = 0, sel = y.select_merged && y.L_aux == 0 ? 0 : (int64_t)B * A0, bmax = 0;
  y.counter_block = (int64_t)L * B * kLayoutCounterStride;
  for (int l = 0; l < L; ++l) {
    const int64_t n = (int64_t)B * lv[l].h * lv[l].w;
    // levels of fewer than exact_px x kcap pixels skip certification (no host synchronisation)
    y.exact[l] = (int64_t)lv[l].h * lv[l].w < (int64_t)sw.exact_px * kcap;
    y.plane[l] = plane;
    plane += n;
    y.lvl[l] = l == 0 ? 0 : lvl;
    if (l > 0) lvl += n;
    y.hist[l] = (int64_t)l * B * kLayoutMedBins;
    y.state[l] = (int64_t)l * B;
    y.kp[l] = (int64_t)l * B * kslots;
    y.counter[l] = (int64_t)l * B * kLayoutCounterStride;
    y.sel[l] = l < y.L_aux ? 0 : sel;
    if (l >= y.L_aux && y.select_merged) sel += n;
    y.bmax[l] = -1;
    if (nms_blocks_level(lv[l].h, lv[l].w, kcap, p->ksize, y.exact[l], sw.nms_blocks)) {
      y.bmax[l] = bmax;
      bmax += (int64_t)B * layout_bmax_stride(lv[l].h, lv[l].w);
    }
  }
  const size_t all = (size_t)plane, rest = (size_t)lvl;  // B (A0 + Arest), B Arest
  // B (A0 + A0 + Arest) selection slots cover both region layouts at any pyramid_scale_factor
  const size_t sel_slots = (size_t)B * A0 + all;
  const size_t nk = (size_t)L * B * (size_t)kslots;
  y.bytes[kBufImg0] = (size_t)B * A0 * 4;
  y.bytes[kBufLvl] = rest * 4;
  y.bytes[kBufR] = all * 4;
  y.bytes[kBufHist] = (size_t)L * B * kLayoutMedBins * 4;
  y.bytes[kBufMed] = (size_t)L * B * kLayoutMedianStateBytes;
  y.bytes[kBufMedlist] = sel_slots * 4;
  y.bytes[kBufCounts] = (size_t)kLayoutCounterBlocks * y.counter_block * 8;
  y.bytes[kBufCand] = all * 8;
  y.bytes[kBufScratch] = sel_slots * 8;
  y.bytes[kBufKpx] = y.bytes[kBufKpy] = y.bytes[kBufKpc] = nk * 4;
  y.bytes[kBufLc] = (size_t)L * B * 4;
  y.bytes[kBufBmax] = (size_t)bmax * 4;
  return SFM_OK;
}

}  // namespace sfm
