// api_match.hip — NNRatio matching over a slot table (workspace c->match).
//
// Matching: operands of every slot (k_match_prep, or the extraction's descriptor launches:
// fused prep) -> row kernel (exact pairwise distances, best/second) -> per-pair compaction +
// (nndr, row) sort.  operands_claim below is the one place the operand owner record moves.
#include "ctx.h"

using namespace sfm;

namespace {

// slots beyond an extraction's batch the fused matcher operand buffers are sized for (a match
// of the batch's table with a few extra slots then needs no reallocation)
constexpr int kFusedPrepSpare = 8;

int64_t operand_rows(const sfm_ctx* c, int64_t cap) {  // capP: rows per slot in the operand buffers
  return c->match.direct ? (cap + 63) / 64 * 64 : (cap + 127) / 128 * 128;
}

// Every write of the operand buffers starts here: the owner record points at `table` and the
// buffers hold `nimg` slots of it.  A different table, or buffers too small (the reallocation
// loses their contents), leaves no fused slot and no prep valid.
int operands_claim(sfm_ctx* c, const float* desc, const int32_t* count, int64_t cap, int nimg) {
  MatchOperandsWs& o = c->match.ops;
  const int64_t capP = operand_rows(c, cap);
  const size_t rows = (size_t)nimg * capP;
  struct {
    DevBuf& b;
    size_t bytes;
  } mfma[] = {{o.hi, rows * 128 * 2}, {o.lo, rows * 128 * 2}, {o.norm2, rows * 4}, {o.rnorm, rows * 4},
              {o.imgmax, (size_t)nimg * match_pmax_bytes(capP)}},
    direct[] = {{o.descT, rows * 128 * 4}};
  bool fits = true;
  if (c->match.direct) {
    for (auto& e : direct) fits = fits && e.b.bytes >= e.bytes;
  } else {
    for (auto& e : mfma) fits = fits && e.b.bytes >= e.bytes;
  }
  if (!fits || o.desc != desc || o.count != count || o.cap != cap) {
    o.fused_B = 0;
    o.prep_nimg = -1;
  }
  o.desc = desc;
  o.count = count;
  o.cap = cap;
  if (fits) return SFM_OK;
  if (c->match.direct) {
    for (auto& e : direct)
      if (int rc = ensure(c, e.b, e.bytes)) return rc;
  } else {
    for (auto& e : mfma)
      if (int rc = ensure(c, e.b, e.bytes)) return rc;
  }
  return SFM_OK;
}

// Matcher operands for slots [lo, lo + n) of a table of nimg slots (buffers sized for
// the whole table; the kernels index slots relative to the offset base pointers).
// rest_of_fused: the slots the last extraction did not write itself instead (fused prep: the
// extraction's slots keep their operands while the buffers still hold them for this table)
int match_prep_range(sfm_ctx* c, const float* desc, const int32_t* count, int nimg, int64_t cap, int lo, int n,
                     hipStream_t st, bool rest_of_fused = false) {
  if (cap < 1 || cap > kMaxMatchRows)
    return set_err(c, SFM_EINVAL, "match capacity must be in [1, 16384]");
  if (lo < 0 || n < 0 || lo + n > nimg) return set_err(c, SFM_EINVAL, "prep slot range outside the table");
  MatchOperandsWs& o = c->match.ops;
  const int rc = operands_claim(c, desc, count, cap, nimg);
  o.prep_nimg = nimg;
  if (rc) return rc;
  if (rest_of_fused && o.fused_B <= nimg) {
    lo = o.fused_B;
    n = nimg - lo;
  }
  if (n == 0) return SFM_OK;
  const float* d0 = desc + (int64_t)lo * cap * 128;
  const int64_t capP = operand_rows(c, cap);
  StageScope sc(c, SFM_PROF_MATCH_PREP, st);
  if (c->match.direct) {
    launch_transpose_desc(d0, count + lo, n, cap, capP, as<float>(o.descT) + (int64_t)lo * 128 * capP, st);
  } else {
    const int64_t r = (int64_t)lo * capP;
    launch_match_prep(d0, count + lo, n, cap, capP, as<_Float16>(o.hi) + r * 128, as<_Float16>(o.lo) + r * 128,
                      as<float>(o.norm2) + r, as<float>(o.rnorm) + r,
                      as<char>(o.imgmax) + (size_t)lo * match_pmax_bytes(capP), st);
  }
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

int match_impl(sfm_ctx* c, const float* desc, const int32_t* count, int nimg, int64_t cap,
               const int32_t* pairs, int P, float ratio, int32_t* matches, float* conf,
               int32_t* nmatch, hipStream_t st, bool prep = true) {
  if (P <= 0) return SFM_OK;
  if (cap < 1 || cap > kMaxMatchRows)
    return set_err(c, SFM_EINVAL, "match capacity must be in [1, 16384]");
  int rc;
  MatchWs& m = c->match;
  MatchOperandsWs& o = m.ops;
  if (prep) {
    // slots the last extraction on this context wrote with their operands (fused prep) keep
    // them; only the rest of the table is prepped (none in BatchPipeline's own tables)
    if ((rc = match_prep_range(c, desc, count, nimg, cap, 0, nimg, st, true))) return rc;
  } else {  // operands from earlier sfm_match_prep_dev calls on this same table
    // (which slots the device-resident pairs touch, and whether their descriptors changed
    // since, cannot be checked without a host sync: that part is the caller's contract)
    if (o.desc != desc || o.count != count || o.prep_nimg != nimg || o.cap != cap)
      return set_err(c, SFM_ESTATE, "sfm_match_pairs_prepped_dev: this table was not the last one prepped "
                                    "(sfm_match_prep_dev) on this context");
  }
  // Per-pair workspace (row results, overflow list and, for the MFMA sweep, kMatchCandCap
  // admitted targets per query row: 512 B per row) is bounded: large P runs as consecutive
  // sub-launches over a fixed budget (SFMFEAT_MATCH_BUDGET_MB, default 4096 = 4 GiB) instead
  // of one allocation that grows with P * cap.
  const size_t per_pair = (size_t)cap * (sizeof(RowBest) + sizeof(int2) + (m.direct ? 0 : kMatchCandCap * 4 + 13));
  // (at most 2^kMatchUnitPairBits pairs per sub-launch: the sweep's work units hold the pair
  // index in that many bits, so a small capacity under a large budget cannot wrap it; and
  // fewer than 2^31 (pair, row) slots: the re-rank's work list holds them in 32 bits)
  const int Pmax = (int)std::max<size_t>(
      1, std::min<size_t>(std::min<size_t>(std::min<size_t>((size_t)P, m.budget / per_pair),
                                           (size_t)1 << kMatchUnitPairBits),
                          (size_t)0x7fffffff / (size_t)cap));
  if ((rc = ensure(c, m.rows, (size_t)Pmax * cap * sizeof(RowBest)))) return rc;
  if ((rc = ensure(c, m.ovf, (size_t)Pmax * cap * sizeof(int2)))) return rc;
  if (m.ovfc.bytes == 0) {  // the overflow counter starts at zero; k_match_compact re-zeroes it
    if ((rc = ensure(c, m.ovfc, 16))) return rc;
    HIPCHK(c, hipMemsetAsync(m.ovfc.p, 0, 16, st));
  }
  if (!m.direct) {  // admitted-target lists of the MFMA sweep (kMatchCandCap per row)
    if ((rc = ensure(c, m.cand, (size_t)Pmax * cap * kMatchCandCap * 4))) return rc;
    if ((rc = ensure(c, m.candn, (size_t)Pmax * cap * 4))) return rc;
    if ((rc = ensure(c, m.candt, (size_t)Pmax * cap * 4))) return rc;
    if ((rc = ensure(c, m.cands, (size_t)Pmax * cap))) return rc;  // one flag byte per row (proven unmatched)
    if ((rc = ensure(c, m.work, (size_t)Pmax * cap * 4))) return rc;  // the re-rank's work list: (pair, row) items
    if ((rc = ensure(c, m.units, match_units_words(Pmax, (int)cap) * 4))) return rc;
  }
  const int64_t capP = operand_rows(c, cap);
  const bool skip_sweep = (extract_switches().skip & 8) != 0;  // SFMFEAT_SKIP: all but the first sub-launch
  m.last_P = P;
  m.last_cap = cap;
  m.last_subs = (P + Pmax - 1) / Pmax;
  for (int p0 = 0; p0 < P; p0 += Pmax, ++m.calls) {
    const int Pn = std::min(Pmax, P - p0);
    const int32_t* pr = pairs + 2 * (int64_t)p0;
    {
      StageScope sc(c, SFM_PROF_MATCH, st);
      if (m.direct)
        launch_match_rows(as<float>(o.descT), count, capP, pr, Pn, ratio, as<RowBest>(m.rows), (int)cap, st);
      else if (!(m.calls > 0 && skip_sweep))
        launch_match_mfma(desc, count, cap, capP, as<_Float16>(o.hi), as<_Float16>(o.lo), as<float>(o.norm2),
                          as<float>(o.rnorm), o.imgmax.p, pr, Pn, ratio, as<RowBest>(m.rows), (int)cap,
                          as<uint32_t>(m.cand), as<int32_t>(m.candn), as<float>(m.candt), as<uint8_t>(m.cands),
                          as<uint32_t>(m.work), as<int>(m.ovfc), as<int2>(m.ovf), as<int32_t>(m.units), st);
    }
    {
      StageScope sc(c, SFM_PROF_MATCH_POST, st);
      launch_match_compact(as<RowBest>(m.rows), count, pr, Pn, (int)cap, cap, matches + (int64_t)p0 * cap * 2,
                           conf + (int64_t)p0 * cap, nmatch + p0, m.direct ? nullptr : as<int>(m.ovfc), st);
    }
  }
  HIPCHK(c, hipGetLastError());
  return SFM_OK;
}

}  // namespace

int operands_fused_begin(sfm_ctx* c, const float* desc, const int32_t* count, int64_t cap, int B,
                         MatchOperands* mo) {
  if (!c->match.fused_prep || c->match.direct) return SFM_OK;  // *mo stays "not written"
  MatchOperandsWs& o = c->match.ops;
  const int rc = operands_claim(c, desc, count, cap, B + kFusedPrepSpare);
  // the extraction rewrites slots [0, B): none is valid until it commits, and preps by earlier
  // sfm_match_prep_dev calls are stale even on this same table
  o.fused_B = 0;
  o.prep_nimg = -1;
  if (rc) return rc;
  *mo = MatchOperands{as<_Float16>(o.hi), as<_Float16>(o.lo), as<float>(o.norm2), as<float>(o.rnorm),
                      as<float2>(o.imgmax), operand_rows(c, cap)};
  return SFM_OK;
}

void operands_fused_commit(sfm_ctx* c, int B) { c->match.ops.fused_B = B; }

void operands_fused_clear(sfm_ctx* c) { c->match.ops.fused_B = 0; }

extern "C" {

int32_t sfm_match(sfm_ctx* c, const float* d1, int64_t n1, const float* d2, int64_t n2, float ratio,
                  int64_t* matches, float* conf, int64_t cap, int64_t* k_out) {
  if (!c || !k_out || n1 < 0 || n2 < 0) return SFM_EINVAL;
  if ((n1 > 0 && !d1) || (n2 > 0 && !d2)) return SFM_EINVAL;
  *k_out = 0;
  if (n1 >= 1 && n2 < 2) return set_err(c, SFM_EINDEX, "index 1 is out of bounds (fewer than 2 targets)");
  if (n1 == 0) return SFM_OK;
  HIPCHK(c, hipSetDevice(c->device));
  int64_t mcap = std::max(n1, n2);
  if (mcap > kMaxMatchRows) return set_err(c, SFM_EINVAL, "more than 16384 descriptors per side");
  int rc;
  hipStream_t st;
  if ((rc = host_stream(c, &st))) return rc;
  MatchWs& m = c->match;
  if ((rc = ensure(c, m.h_desc, (size_t)2 * mcap * 128 * 4))) return rc;
  if ((rc = ensure(c, m.h_count, 16))) return rc;
  if ((rc = ensure(c, m.h_pairs, 16))) return rc;
  if ((rc = ensure(c, m.h_matches, (size_t)mcap * 8))) return rc;
  if ((rc = ensure(c, m.h_conf, (size_t)mcap * 4))) return rc;
  if ((rc = ensure(c, m.h_nmatch, 16))) return rc;
  int32_t hcount[2] = {(int32_t)n1, (int32_t)n2};
  int32_t hpairs[2] = {0, 1};
  float* dd = as<float>(m.h_desc);
  HIPCHK(c, hipMemcpyAsync(dd, d1, (size_t)n1 * 128 * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(dd + mcap * 128, d2, (size_t)n2 * 128 * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(m.h_count.p, hcount, 8, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(m.h_pairs.p, hpairs, 8, hipMemcpyHostToDevice, st));
  rc = match_impl(c, dd, as<int32_t>(m.h_count), 2, mcap, as<int32_t>(m.h_pairs), 1, ratio,
                  as<int32_t>(m.h_matches), as<float>(m.h_conf), as<int32_t>(m.h_nmatch), st);
  if (rc) return rc;
  int32_t k = 0;
  HIPCHK(c, hipMemcpyAsync(&k, m.h_nmatch.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (k < 0) return set_err(c, SFM_EINDEX, "index 1 is out of bounds (fewer than 2 targets)");
  *k_out = k;
  if (k > cap) return set_err(c, SFM_ERANGE, "output capacity too small");
  if (k > 0) {
    std::vector<int32_t> mm((size_t)k * 2);
    HIPCHK(c, hipMemcpyAsync(mm.data(), m.h_matches.p, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    if (conf) HIPCHK(c, hipMemcpyAsync(conf, m.h_conf.p, (size_t)k * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (matches)
      for (int64_t i = 0; i < 2 * k; ++i) matches[i] = mm[i];
  }
  return SFM_OK;
}

int32_t sfm_match_pairs_dev(sfm_ctx* c, const float* desc, const int32_t* count, int32_t nimg,
                            int64_t cap, const int32_t* pairs, int32_t P, float ratio, int32_t* matches,
                            float* conf, int32_t* nmatch, void* stream) {
  if (!c || !desc || !count || !pairs || !matches || !conf || !nmatch || nimg < 1 || P < 0)
    return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;  // exactly the caller's stream (NULL = null stream)
  return match_impl(c, desc, count, nimg, cap, pairs, P, ratio, matches, conf, nmatch, st);
}

int32_t sfm_match_prep_dev(sfm_ctx* c, const float* desc, const int32_t* count, int32_t nimg, int64_t cap,
                           int32_t slot_lo, int32_t slot_n, void* stream) {
  if (!c || !desc || !count || nimg < 1) return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  return match_prep_range(c, desc, count, nimg, cap, slot_lo, slot_n, (hipStream_t)stream);
}

int32_t sfm_match_pairs_prepped_dev(sfm_ctx* c, const float* desc, const int32_t* count, int32_t nimg,
                                    int64_t cap, const int32_t* pairs, int32_t P, float ratio, int32_t* matches,
                                    float* conf, int32_t* nmatch, void* stream) {
  if (!c || !desc || !count || !pairs || !matches || !conf || !nmatch || nimg < 1 || P < 0)
    return SFM_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  return match_impl(c, desc, count, nimg, cap, pairs, P, ratio, matches, conf, nmatch, (hipStream_t)stream,
                    false);
}

int32_t sfm_debug_match_operands(sfm_ctx* c, int32_t slot, int64_t rows, uint16_t* hi, uint16_t* lo, float* norm2,
                                 float* rnorm, float* pmax) {
  if (!c || !hi || !lo || !norm2 || !rnorm || !pmax || slot < 0) return SFM_EINVAL;
  MatchOperandsWs& o = c->match.ops;
  if (c->match.direct) return set_err(c, SFM_ESTATE, "the direct matcher has no split-f16 operands");
  if (o.cap < 1 || !(slot < o.fused_B || slot < o.prep_nimg))
    return set_err(c, SFM_ESTATE, "no matcher operands for that slot on this context");
  const int64_t capP = operand_rows(c, o.cap);
  if (rows != capP) return set_err(c, SFM_EINVAL, "rows must be the table's capacity rounded up to 128");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  const size_t r0 = (size_t)slot * capP, nb = (size_t)capP;
  HIPCHK(c, hipMemcpy(hi, as<_Float16>(o.hi) + r0 * 128, nb * 128 * 2, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(lo, as<_Float16>(o.lo) + r0 * 128, nb * 128 * 2, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(norm2, as<float>(o.norm2) + r0, nb * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(rnorm, as<float>(o.rnorm) + r0, nb * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(pmax, as<char>(o.imgmax) + (size_t)slot * match_pmax_bytes(capP), match_pmax_bytes(capP),
                      hipMemcpyDeviceToHost));
  return SFM_OK;
}

int32_t sfm_debug_match_windows(sfm_ctx* c, int32_t pair, int64_t rows, int32_t* cand_n, float* cand_thr,
                                uint32_t* cand) {
  if (!c || !cand_n || !cand_thr || !cand || pair < 0 || rows < 1) return SFM_EINVAL;
  MatchWs& m = c->match;
  if (m.direct) return set_err(c, SFM_ESTATE, "the direct matcher keeps no windows");
  if (m.last_subs != 1)
    return set_err(c, SFM_ESTATE, m.last_subs ? "the last match call ran as more than one sub-launch"
                                              : "no match call on this context yet");
  if (pair >= m.last_P || rows > m.last_cap) return set_err(c, SFM_EINVAL, "pair or rows outside the last match call");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  const size_t r0 = (size_t)pair * (size_t)m.last_cap, n = (size_t)rows;
  HIPCHK(c, hipMemcpy(cand_n, as<int32_t>(m.candn) + r0, n * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(cand_thr, as<float>(m.candt) + r0, n * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(cand, as<uint32_t>(m.cand) + r0 * kMatchCandCap, n * kMatchCandCap * 4, hipMemcpyDeviceToHost));
  return SFM_OK;
}

int32_t sfm_debug_match_skips(sfm_ctx* c, int32_t pair, int64_t rows, uint8_t* skip) {
  if (!c || !skip || pair < 0 || rows < 1) return SFM_EINVAL;
  MatchWs& m = c->match;
  if (m.direct) return set_err(c, SFM_ESTATE, "the direct matcher keeps no windows");
  if (m.last_subs != 1)
    return set_err(c, SFM_ESTATE, m.last_subs ? "the last match call ran as more than one sub-launch"
                                              : "no match call on this context yet");
  if (pair >= m.last_P || rows > m.last_cap) return set_err(c, SFM_EINVAL, "pair or rows outside the last match call");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(skip, as<uint8_t>(m.cands) + (size_t)pair * (size_t)m.last_cap, (size_t)rows,
                      hipMemcpyDeviceToHost));
  return SFM_OK;
}

}  // extern "C"
