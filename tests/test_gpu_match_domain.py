"""The matcher outside unit-norm RootSIFT tables, and its prefilter seen from inside.

Final results of every case family of tests/match_ref.py (integers 0..255, signed, a common
offset with small noise, tiny magnitudes, mixed scales, one dominant element, zero rows,
elements at and beyond the float16 range) against the oracle; the split-f16 operands against
their restatement bit for bit (sfm_debug_match_operands); the windows the sweep leaves
(sfm_debug_match_windows) against invariants that follow from the bound E alone; the fused
operand writer against k_match_prep.

Measured on an MI355X (printed by the tests, never used as tolerances):
  max |thr - 2E - D2| / E per class (thr - 2E is the sweep's b2~: the share of E really used):
    unit 0.0025, u8 0.0006, signed 0.0110, offset 0.0120, tiny 0.0000, mixed 0.0088, spike 0.0071,
    zeros 0.0012, edge(255.9) 0.0005
  list entries per row (rows handed to the exact kernel): unit 2-17 (0), u8 2-32 (0), signed 2-14
    (0), offset(0.03) 5-21 (0), offset(0.01) 8-143 (0), offset(0.006) 33-622 (51 of 96),
    offset(0.003) 700 (all), tiny(1e-3) and tiny(1e-6) x 700 targets 700 (all), tiny(1e-6) x 33
    targets 33 (0), mixed 2-330 (134 of 260), spike 12-198 (0), zeros 2-6 (0), edge(255.9) 3-12 (0);
    edge(256), edge(1000), edge(1e4), huge: every row on the non-finite-bound path
  fused writer against k_match_prep: 0 of 872 rows differ in norm2 or rnorm
  On the commit before these tests the edge(256), edge(1000), edge(1e4) and huge cases differed
  from the oracle (huge: no match at all): f16 overflow of the scaled operands, now flagged.
"""
from __future__ import annotations

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from sfmfromscratch_amd import NNRatioFeatureMatcher, _abi, _native, synth
from tests import match_ref as R
from tests.golden_util import P_OCT, assert_matches_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = range(len(R.CASES))
HALF = R.HALF_CAP
UNBOUNDED = 0x7fff  # count word of a row whose bound is not finite


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def oracle_match(i):
    return O.match(*R.case(i), R.RATIO)


def new_context():
    return _native.Context(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), 0)


# ---------------------------------------------------------------- final results, host path
@pytest.mark.parametrize("i", ALL, ids=R.CASE_IDS)
def test_host_path_equals_the_oracle(i):
    q, t = R.case(i)
    m, c = NNRatioFeatureMatcher(R.RATIO).match_features_ratio_test(q, t)
    om, oc = oracle_match(i)
    assert_matches_equal(om, oc, m, c)


# ---------------------------------------------------------------- final results, slot table
# one slot per case class: (case id, which table, rows kept).  `unit` keeps one row, so every
# pair that targets it is the reference's IndexError (nmatch -1).
SLOT_CAP = 768
SLOTS = [("unit-130x700", 1, 1), ("u8-130x700", 1, 513), ("signed-260x700", 1, 257),
         ("offset(0.01)-96x700", 1, 700), ("tiny(1e-6)-96x700", 1, 700), ("mixed-260x700", 1, 300),
         ("spike-130x700", 1, 129), ("zeros-130x65", 1, 65), ("edge(256)-130x700", 1, 700),
         ("huge-130x700", 0, 130)]


@functools.lru_cache(maxsize=None)
def slot_host():
    """The table (host copy), its counts and the ordered pairs.  Rows 8..15 of every slot are
    perturbed copies (1 % relative) of the first rows of two other slots, so rows of one scale
    have their nearest neighbour inside a table of another scale and the pairs really match."""
    host = np.zeros((len(SLOTS), SLOT_CAP, 128), np.float32)
    counts = []
    for s, (cid, which, n) in enumerate(SLOTS):
        host[s, :n] = R.case(R.CASE_IDS.index(cid))[which][:n]
        counts.append(n)
    rng = np.random.default_rng(7)
    src = host.copy()
    for j in range(len(SLOTS)):
        if counts[j] < 16:
            continue
        for k, step in enumerate((1, 3)):
            i = (j + step) % len(SLOTS)
            m = min(4, counts[i])
            host[j, 8 + 4 * k: 8 + 4 * k + m] = src[i, :m] * (1 + 0.01 * rng.standard_normal((m, 128))).astype(np.float32)
    pairs = np.array([(i, j) for i in range(len(SLOTS)) for j in range(len(SLOTS)) if i != j], np.int32)
    host.setflags(write=False)
    return host, counts, pairs


def slot_match_case():
    """The slot table matched over all ordered pairs -> matches, conf, nmatch (host copies)."""
    import torch
    from sfmfromscratch_amd.pipeline import BatchMatcher, SlotTable
    host, counts, pairs = slot_host()
    slots = SlotTable(torch, len(SLOTS), SLOT_CAP, "cuda")
    slots.desc.copy_(torch.from_numpy(host.copy()))
    slots.count.copy_(torch.tensor(counts, dtype=torch.int32))
    mm, mc, nm = BatchMatcher(R.RATIO).match(slots, torch.from_numpy(pairs).cuda())
    torch.cuda.synchronize()
    return mm.cpu().numpy(), mc.cpu().numpy(), nm.cpu().numpy()


@functools.lru_cache(maxsize=None)
def slot_oracle():
    from concurrent.futures import ThreadPoolExecutor
    host, counts, pairs = slot_host()

    def ref(pq):
        i, j = pq
        try:
            return O.match(host[i, :counts[i]], host[j, :counts[j]], R.RATIO)
        except IndexError:
            return None
    with ThreadPoolExecutor(16) as pool:
        return list(pool.map(ref, [tuple(p) for p in pairs]))


FORMS = {"default": {}, "stage1-rerank1": {"SFMFEAT_MATCH_STAGE": "1", "SFMFEAT_RERANK2": "0"},
         "reg": {"SFMFEAT_MATCH_STAGE": "reg"}}


@pytest.mark.parametrize("form", list(FORMS))
def test_slot_table_of_every_class_all_ordered_pairs(form, tmp_path):
    """Queries of one scale against targets of another (tiny against u8, huge against zeros, ...):
    every ordered pair of the 10-slot table equals the oracle, in the default sweep form and, in
    one child process each (the library reads the switches once), the one-CU LDS-DMA sweep with
    the one-item re-rank and the register-staged sweep."""
    pytest.importorskip("torch")
    if form == "default":
        mm, mc, nm = slot_match_case()
    else:
        path = str(tmp_path / "slots.npz")
        code = ("import sys, numpy as np; sys.path.insert(0, %r); from tests import test_gpu_match_domain as t; "
                "mm, mc, nm = t.slot_match_case(); np.savez(%r, mm=mm, mc=mc, nm=nm)" % (ROOT, path))
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **FORMS[form]), cwd=ROOT,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(path)
        mm, mc, nm = z["mm"], z["mc"], z["nm"]
    _, counts, pairs = slot_host()
    refs = slot_oracle()
    assert len(pairs) == 90
    for p, (i, j) in enumerate(pairs):
        if refs[p] is None:
            assert counts[j] < 2 and nm[p] == -1, (SLOTS[i][0], SLOTS[j][0], nm[p])
            continue
        om, oc = refs[p]
        k = int(nm[p])
        assert k == len(oc), (SLOTS[i][0], SLOTS[j][0], k, len(oc))
        assert_matches_equal(om, oc, mm[p, :k], mc[p, :k])
    assert sum(r is None for r in refs) == 9 and sum(len(r[1]) > 0 for r in refs if r is not None) >= 40


# ---------------------------------------------------------------- operands
OPERAND_SLOTS = [("unit-130x700", 1, 300), ("u8-130x700", 1, 257), ("signed-130x65", 0, 130),
                 ("tiny(1e-3)-130x700", 1, 65), ("tiny(1e-6)-96x700", 0, 96), ("mixed-260x700", 0, 260),
                 ("edge(1e4)-260x65", 1, 65), ("zeros-130x65", 1, 0)]


def test_operands_after_prep_equal_the_restatement_bit_for_bit():
    """hi, lo, norm2, rnorm, the padding rows and the block maxima of every slot, as k_match_prep
    wrote them, against match_ref.operands (cap 300: 84 padding rows in the fullest slot; an
    empty slot; a slot with two rows outside the f16 range: zero hi / lo, +inf rnorm)."""
    torch = pytest.importorskip("torch")
    from sfmfromscratch_amd.pipeline import BatchMatcher, SlotTable
    cap = 300
    slots = SlotTable(torch, len(OPERAND_SLOTS), cap, "cuda")
    host = np.zeros((len(OPERAND_SLOTS), cap, 128), np.float32)
    for s, (cid, which, n) in enumerate(OPERAND_SLOTS):
        host[s, :n] = R.case(R.CASE_IDS.index(cid))[which][:n]
    slots.desc.copy_(torch.from_numpy(host))
    slots.count.copy_(torch.tensor([n for _, _, n in OPERAND_SLOTS], dtype=torch.int32))
    m = BatchMatcher(R.RATIO)
    with pytest.raises(RuntimeError):
        m.ctx.match_operands(0, cap)  # nothing prepped yet: SFM_ESTATE
    m.prep(slots)
    with pytest.raises(RuntimeError):
        m.ctx.match_operands(len(OPERAND_SLOTS), cap)  # outside the prepped table
    with pytest.raises(ValueError):
        m.ctx.match_operands(0, cap + 200)  # another capP
    for s, (cid, which, n) in enumerate(OPERAND_SLOTS):
        want = R.operands(host[s, :n], cap)
        hi, lo, norm2, rnorm, pmax = m.ctx.match_operands(s, cap)
        assert hi.shape == (384, 128) and pmax.shape == (24, 2)
        for name, got in (("hi", hi), ("lo", lo), ("norm2", norm2), ("rnorm", rnorm), ("pmax", pmax)):
            assert np.array_equal(bits(got), bits(want[name])), (cid, name)
        if cid.startswith("edge"):
            assert want["flagged"].sum() == 2 and np.isinf(rnorm[:n]).sum() == 2


def test_read_backs_refuse_what_they_cannot_answer(monkeypatch):
    """SFM_ESTATE: no match call yet; a match call that ran as several sub-launches; the direct
    matcher.  SFM_EINVAL: a pair or row count outside the last call."""
    q, t = R.case(R.CASE_IDS.index("u8-260x33"))
    ctx = new_context()
    with pytest.raises(RuntimeError):
        ctx.match_windows(0, 1)
    ctx.match(q, t, np.float32(R.RATIO))
    ctx.match_windows(0, 260)
    for pair, rows in ((1, 1), (0, 261), (0, 0), (-1, 1)):
        with pytest.raises(ValueError):
            ctx.match_windows(pair, rows)
    ctx.close()
    monkeypatch.setenv("SFMFEAT_MATCH_DIRECT", "1")
    ctx = new_context()
    monkeypatch.delenv("SFMFEAT_MATCH_DIRECT")
    ctx.match(q, t, np.float32(R.RATIO))
    with pytest.raises(RuntimeError):
        ctx.match_windows(0, 1)
    with pytest.raises(RuntimeError):
        ctx.match_operands(0, 260)
    ctx.close()
    torch = pytest.importorskip("torch")
    from sfmfromscratch_amd.pipeline import BatchMatcher, SlotTable
    monkeypatch.setenv("SFMFEAT_MATCH_BUDGET_MB", "1")  # 1 MiB / (768 x 1048 B): one pair per sub-launch
    m = BatchMatcher(R.RATIO)
    monkeypatch.delenv("SFMFEAT_MATCH_BUDGET_MB")
    slots = SlotTable(torch, 3, SLOT_CAP, "cuda")
    slots.desc[:, :33].copy_(torch.from_numpy(np.stack([t, t, t])))
    slots.count.fill_(33)
    m.match(slots, torch.tensor([[0, 1], [1, 2]], dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        m.ctx.match_windows(0, 33)
    m.match(slots, torch.tensor([[0, 1]], dtype=torch.int32, device="cuda"))
    m.ctx.match_windows(0, 33)


# ---------------------------------------------------------------- windows
@functools.lru_cache(maxsize=None)
def device_windows(i):
    """Case i through sfm_match on a context of its own -> (matches, conf, cand_n, cand_thr,
    cand) of its one pair."""
    q, t = R.case(i)
    ctx = new_context()
    try:
        m, c = ctx.match(q, t, np.float32(R.RATIO))
        return (m, c) + ctx.match_windows(0, q.shape[0])
    finally:
        ctx.close()


def row_entries(cn, cd, r):
    c0, c1 = int(cn[r]) & 0xffff, int(cn[r]) >> 16
    w = np.concatenate([cd[r, :min(c0, HALF)], cd[r, HALF:HALF + min(c1, HALF)]])
    return c0, c1, (w & 0xffff).astype(np.int64), R.bf16_down_value(w)


@pytest.mark.parametrize("i", ALL, ids=R.CASE_IDS)
def test_window_invariants(i, capsys):
    """What the sweep left for every query row of the case's pair.  D2: the reference's
    second-smallest float32 squared distance of the row; E: the restated bound.
      (a) every target with d_ref <= D2 is listed with stored d~ <= thr (the re-rank keeps it);
      (b) D2 + E <= thr <= D2 + 3E up to 2 ulp of thr: thr - 2E is the sweep's b2~, so
          |b2~ - D2| <= E is the bound measured at full precision;
      (c) every listed entry has stored d~ <= d_ref + E, an index below n2, and is listed once;
      (d) a row is handed to the exact kernel only when a half-list count exceeds 128, or (the
          0x7fff count word) when its E is not finite — which is every row of the pair as soon
          as one element of the target table is outside the f16 range, and no row otherwise."""
    m, c, cn, ct, cd = device_windows(i)
    assert_matches_equal(*oracle_match(i), m, c)
    a = R.analysis(i)
    n1, n2 = a["d32"].shape
    E, D2, d32 = a["E"], a["D2"], a["d32"]
    finite = np.isfinite(np.float32(2.0) * E)  # the sweep tests 2E, the quantity it carries
    if a["tb"]["flagged"].any():
        assert not finite.any()
    else:
        assert np.array_equal(~finite, a["qa"]["flagged"])
    assert np.array_equal(cn == UNBOUNDED, ~finite)
    worst = 0.0
    for r in np.flatnonzero(finite):
        c0, c1, idx, stored = row_entries(cn, cd, r)
        assert max(c0, c1) <= 16 * ((n2 + 31) // 32)  # a half-wave sees 16 targets of each sub-tile
        if c0 > HALF or c1 > HALF:
            continue  # k_match_overflow's row (exact over every target)
        e, thr = np.float64(E[r]), np.float64(ct[r])
        assert np.all(idx < n2) and len(set(idx.tolist())) == len(idx), (r, "c")
        assert np.all(stored.astype(np.float64) <= d32[r, idx].astype(np.float64) + e), (r, "c")
        need = np.flatnonzero(d32[r] <= D2[r])
        kept = set(idx[stored <= ct[r]].tolist())
        assert set(need.tolist()) <= kept, (r, "a", sorted(set(need.tolist()) - kept))
        ulp2 = 2.0 * np.float64(np.spacing(np.abs(ct[r])))
        d2 = np.float64(D2[r])
        assert d2 + e - ulp2 <= thr <= d2 + 3.0 * e + ulp2, (r, "b", d2, e, thr)
        worst = max(worst, abs(thr - 2.0 * e - d2) / e)
    with capsys.disabled():
        live = cn[finite]
        tot = (live & 0xffff) + (live >> 16)
        print("\n%s: max |thr - 2E - D2| / E = %.4f, list entries per row %s, overflowed rows %d of %d"
              % (R.CASE_IDS[i], worst, (int(tot.min()), int(tot.max())) if len(tot) else None,
                 int((((live & 0xffff) > HALF) | ((live >> 16) > HALF)).sum()) + int((~finite).sum()), n1))


def test_the_window_bands_were_hit_on_the_device():
    """The cases reach the structures they were built for: short lists, half-lists filled to
    between 32 and 128 entries, overflowed rows beside kept ones in one pair, a pair whose every
    row overflowed, and pairs whose every row took the non-finite-bound path."""
    def halves(cid):
        cn = device_windows(R.CASE_IDS.index(cid))[2]
        return cn & 0xffff, cn >> 16, cn
    c0, c1, _ = halves("unit-130x700")
    assert ((c0 + c1) <= 4).any()
    mid = False
    mixed_pair = False
    for cid in ("offset(0.01)-96x700", "offset(0.006)-96x700"):
        c0, c1, _ = halves(cid)
        ovf = (c0 > HALF) | (c1 > HALF)
        mid = mid or bool((((c0 >= 32) & (c0 <= HALF)) | ((c1 >= 32) & (c1 <= HALF))).any())
        mixed_pair = mixed_pair or bool(ovf.any() and (~ovf).any())
    assert mid and mixed_pair
    c0, c1, cn = halves("tiny(1e-6)-96x700")
    assert np.all(((c0 > HALF) | (c1 > HALF)) & (cn != UNBOUNDED))
    for cid in ("edge(256)-130x700", "edge(1e4)-260x65", "huge-130x700"):
        assert np.all(halves(cid)[2] == UNBOUNDED)
    assert not (halves("edge(255.9)-130x700")[2] == UNBOUNDED).any()


# ---------------------------------------------------------------- the fused operand writer
def test_fused_writer_operands_against_prep(capsys):
    """A fused extraction's operands (the descriptor kernel writes them) against k_match_prep of
    the same descriptors on a fresh context: hi and lo bit for bit; norm2 and rnorm within one
    ulp (the two sum the squared norm in double in different orders); +inf padding rows."""
    torch = pytest.importorskip("torch")
    from sfmfromscratch_amd.pipeline import BatchExtractor, BatchMatcher
    ex = BatchExtractor(dict(P_OCT, num_interest_points=600))
    ex.ctx.set_fused_prep(True)
    s = ex.extract(torch.from_numpy(synth.make_batch_u8(2, 270, 480, seed=77)).cuda())
    torch.cuda.synchronize()
    m = BatchMatcher(R.RATIO)
    m.prep(s)
    counts = s.count.cpu().numpy()
    desc = s.desc.cpu().numpy()
    differ = rows = 0
    for b in range(2):
        n = int(counts[b])
        assert n > 300
        fh, fl, fn2, frn, fpm = ex.ctx.match_operands(b, ex.cap)
        ph, pl, pn2, prn, ppm = m.ctx.match_operands(b, ex.cap)
        want = R.operands(desc[b, :n], ex.cap)
        assert np.array_equal(bits(ph), bits(want["hi"])) and np.array_equal(bits(pn2), bits(want["norm2"]))
        assert np.array_equal(fh, ph) and np.array_equal(fl, pl)
        assert np.all(np.isinf(fn2[n:])) and np.all(fn2[n:] > 0) and not frn[n:].any()
        assert np.isfinite(fn2[:n]).all()
        for f, p in ((fn2[:n], pn2[:n]), (frn[:n], prn[:n]), (fpm, ppm)):
            assert np.all(np.abs(bits(f).astype(np.int64) - bits(p).astype(np.int64)) <= 1)
        differ += int(((bits(fn2[:n]) != bits(pn2[:n])) | (bits(frn[:n]) != bits(prn[:n]))).sum())
        rows += n
    with capsys.disabled():
        print("\nfused vs prep: %d of %d rows differ in norm2 or rnorm" % (differ, rows))
