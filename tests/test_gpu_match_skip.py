"""Rows the sweep proves unmatched (csrc/match_mfma.hip proven_unmatched): the re-rank writes
"no match" for them without reading their windows, and nothing else may change.

Seven match calls of three pairs each through sfm_match_pairs_dev, in the default form and, in one
child process each (the library reads its switches once), with the one-workgroup-per-CU sweep
and / or the one-row-per-wavefront re-rank:
  sizes-a..d  a RootSIFT-like slot table with 300, 129, 64, 31, 2, 1 and 0 rows (every other
              row a near-duplicate of a common pool, the rest fresh), pairs mixing the sizes;
  sizes-e     the same table's slot of 300 copies of one row as targets: every query row's
              half-lists overflow (150 entries each) and its nndr is 1 — provable, but a row of
              the exact kernel, which the sweep must leave unflagged;
  identical   40 identical targets (e2 = 0 for the queries equal to them, nndr = 1 for the rest);
  straddle    rows whose exact nndr lies within 1e-6, 1e-4, 1e-3 of the ratio on both sides
              (tests/match_skip_ref.planted).
Per form: matches, conf and nmatch equal the oracle's; every flagged row (sfm_debug_match_skips)
is unmatched in the oracle and none is a row of the exact kernel; some row is flagged and some
unmatched row is not; the windows and thresholds (sfm_debug_match_windows) keep the invariants
tests/test_gpu_match_domain.py states for them, against tests/match_ref.py.

Measured on an MI355X (printed, never used as bounds), every form alike, all calls together:
1,014 flagged of 1,228 unmatched rows, 1,727 live rows of pairs with two targets or more, 160 rows
of the exact kernel.  (sizes-e also has the table's last slot, 300 rows, as the query side of a
256-row sweep block: the rows past the slot's padded capacity, DESIGN_LOG.md §R.)
"""
from __future__ import annotations

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from sfmfromscratch_amd import synth
from tests import match_ref as R
from tests import match_skip_ref as S
from tests.golden_util import assert_matches_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO = 0.85
HALF = R.HALF_CAP
FORMS = {"default": {},
         "stage3-rerank1": {"SFMFEAT_RERANK2": "0"},
         "stage1-rerank2": {"SFMFEAT_MATCH_STAGE": "1", "SFMFEAT_RERANK2": "1"},
         "stage1-rerank1": {"SFMFEAT_MATCH_STAGE": "1", "SFMFEAT_RERANK2": "0"}}
SIZES = (300, 129, 64, 31, 2, 1, 0, 300)   # the last slot: 300 copies of one row


@functools.lru_cache(maxsize=None)
def tables():
    """name -> (host table [slots, cap, 128], counts).  Read-only."""
    _, pool = synth.make_descriptor_table(300, 21)
    sizes = np.zeros((len(SIZES), 300, 128), np.float32)
    for s, n in enumerate(SIZES):
        if n:
            q, _ = synth.make_descriptor_table(n, 30 + s, dup_of=pool, jitter=2)
            fresh, _ = synth.make_descriptor_table(n, 50 + s)
            q = q.copy()
            q[1::2] = fresh[1::2]
            sizes[s, :n] = q
    sizes[7] = sizes[0, 1]
    mixed, _ = S.rootsift_mixed(64, 31, 9)
    v = mixed[1]
    ident = np.zeros((3, 64, 128), np.float32)
    ident[0, :31] = mixed[:31]
    ident[0, [0, 7, 30]] = v
    ident[1, :40] = v
    ident[2] = mixed
    q, t, _ = S.planted(RATIO)
    strad = np.zeros((2, t.shape[0], 128), np.float32)
    strad[0, :q.shape[0]] = q
    strad[1] = t
    out = {"sizes": (sizes, SIZES), "identical": (ident, (31, 40, 64)), "straddle": (strad, (q.shape[0], t.shape[0]))}
    for tab, _ in out.values():
        tab.setflags(write=False)
    return out


# call -> (table, three pairs)
CALLS = {"sizes-a": ("sizes", ((0, 1), (1, 0), (2, 3))),
         "sizes-b": ("sizes", ((3, 2), (0, 4), (4, 0))),
         "sizes-c": ("sizes", ((0, 5), (5, 0), (6, 0))),
         "sizes-d": ("sizes", ((0, 6), (2, 2), (1, 3))),
         "sizes-e": ("sizes", ((1, 7), (3, 7), (7, 0))),
         "identical": ("identical", ((0, 1), (2, 1), (1, 0))),
         "straddle": ("straddle", ((0, 1), (1, 0), (0, 0)))}


def run_calls() -> dict:
    """Every call on cuda:0 -> numpy results by name: matches, conf, nmatch per call; skip flags,
    count words, thresholds and lists per (call, pair) that has query rows and targets."""
    import torch

    from sfmfromscratch_amd.pipeline import BatchMatcher, SlotTable
    out = {}
    dev = {}
    for name, (tab, counts) in tables().items():
        slots = SlotTable(torch, tab.shape[0], tab.shape[1], "cuda")
        slots.desc.copy_(torch.from_numpy(tab.copy()))
        slots.count.copy_(torch.tensor(counts, dtype=torch.int32))
        dev[name] = (slots, BatchMatcher(RATIO))
    for call, (name, pairs) in CALLS.items():
        slots, m = dev[name]
        counts = tables()[name][1]
        mm, mc, nm = m.match(slots, torch.tensor(pairs, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        out[f"{call}_m"], out[f"{call}_c"], out[f"{call}_n"] = mm.cpu().numpy(), mc.cpu().numpy(), nm.cpu().numpy()
        for p, (i, j) in enumerate(pairs):
            if counts[i] >= 1 and counts[j] >= 1:
                out[f"{call}_{p}_skip"] = m.ctx.match_skips(p, counts[i])
                cn, ct, cd = m.ctx.match_windows(p, counts[i])
                out[f"{call}_{p}_cn"], out[f"{call}_{p}_ct"], out[f"{call}_{p}_cd"] = cn, ct, cd
    return out


@functools.lru_cache(maxsize=None)
def reference(call, p):
    """Pair p of `call` -> (oracle matches, conf) or None (the reference's IndexError), and the
    match_ref analysis of its two tables (None without two targets or without query rows)."""
    name, pairs = CALLS[call]
    tab, counts = tables()[name]
    i, j = pairs[p]
    q, t = tab[i, :counts[i]], tab[j, :counts[j]]
    try:
        ref = O.match(q, t, RATIO)
    except IndexError:
        ref = None
    a = None
    if counts[i] >= 1 and counts[j] >= 2:
        a = S.analysis_of(q, t)
        a["D2"] = np.sort(a["d32"], axis=1)[:, 1]
    return ref, a


def check_windows(tag, a, cn, ct, cd):
    """tests/test_gpu_match_domain.py test_window_invariants (a)-(d) for one pair inside the f16
    range: every target within the reference's second distance is listed with stored d~ <= thr;
    D2 + E <= thr <= D2 + 3E up to 2 ulp; listed entries are distinct targets with stored
    d~ <= d_ref + E; no row carries the non-finite-bound word."""
    n1, n2 = a["d32"].shape
    E, D2, d32 = a["E"], a["D2"], a["d32"]
    assert np.isfinite(np.float32(2.0) * E).all() and not (cn == 0x7fff).any(), tag
    for r in range(n1):
        c0, c1 = int(cn[r]) & 0xffff, int(cn[r]) >> 16
        assert max(c0, c1) <= 16 * ((n2 + 31) // 32), (tag, r)
        if c0 > HALF or c1 > HALF:
            continue
        w = np.concatenate([cd[r, :c0], cd[r, HALF:HALF + c1]])
        idx, stored = (w & 0xffff).astype(np.int64), R.bf16_down_value(w)
        e, thr = np.float64(E[r]), np.float64(ct[r])
        assert np.all(idx < n2) and len(set(idx.tolist())) == len(idx), (tag, r, "c")
        assert np.all(stored.astype(np.float64) <= d32[r, idx].astype(np.float64) + e), (tag, r, "c")
        need = set(np.flatnonzero(d32[r] <= D2[r]).tolist())
        assert need <= set(idx[stored <= ct[r]].tolist()), (tag, r, "a")
        ulp2 = 2.0 * np.float64(np.spacing(np.abs(ct[r])))
        assert np.float64(D2[r]) + e - ulp2 <= thr <= np.float64(D2[r]) + 3.0 * e + ulp2, (tag, r, "b")


@pytest.mark.parametrize("form", list(FORMS))
def test_skipped_rows_change_nothing(form, tmp_path, capsys):
    pytest.importorskip("torch")
    if form == "default":
        got = run_calls()
    else:
        path = str(tmp_path / "skip.npz")
        code = ("import sys, numpy as np; sys.path.insert(0, %r); from tests import test_gpu_match_skip as t; "
                "np.savez(%r, **t.run_calls())" % (ROOT, path))
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **FORMS[form]), cwd=ROOT,
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        got = dict(np.load(path))
    flagged = unmatched = live = exact = 0
    for call, (name, pairs) in CALLS.items():
        counts = tables()[name][1]
        for p, (i, j) in enumerate(pairs):
            tag = (form, call, p)
            ref, a = reference(call, p)
            k = int(got[f"{call}_n"][p])
            if ref is None:
                assert counts[j] < 2 and k == -1, tag
            else:
                assert k == len(ref[1]), tag + (k, len(ref[1]))
                assert_matches_equal(ref[0], ref[1], got[f"{call}_m"][p, :k], got[f"{call}_c"][p, :k])
            if counts[i] < 1 or counts[j] < 1:
                assert f"{call}_{p}_skip" not in got
                continue
            sk, cn = got[f"{call}_{p}_skip"], got[f"{call}_{p}_cn"]
            assert sk.shape == (counts[i],) and set(np.unique(sk).tolist()) <= {0, 1}, tag
            if counts[j] < 2:
                assert not sk.any(), tag   # one target: the second distance is +inf, nothing proven
                continue
            free = np.ones(counts[i], bool)
            free[ref[0][:, 0]] = False
            over = ((cn & 0xffff) > HALF) | ((cn >> 16) > HALF)
            assert not (sk.astype(bool) & ~free).any(), tag + (np.flatnonzero(sk.astype(bool) & ~free)[:8],)
            assert not (sk.astype(bool) & over).any(), tag
            check_windows(tag, a, cn, got[f"{call}_{p}_ct"], got[f"{call}_{p}_cd"])
            # the host restatement on the worst-case top-2 fires wherever the device may fire
            may = S.certificate(*S.adversarial_top2(a), a["E"], RATIO)
            assert not (sk.astype(bool) & ~may).any(), tag
            flagged, unmatched, live = flagged + int(sk.sum()), unmatched + int(free.sum()), live + counts[i]
            exact += int(over.sum())
            if call == "identical" and p < 2:
                same = np.all(tables()[name][0][i, :counts[i]] == tables()[name][0][1, 0], axis=1)
                assert same.sum() >= 1 and free.all() and not sk[same].any() and sk[~same].all(), tag
    with capsys.disabled():
        print("\n%s: flagged %d of %d unmatched rows (%d live rows of pairs with two targets or more, %d exact-kernel)"
              % (form, flagged, unmatched, live, exact))
    assert flagged >= 1 and unmatched > flagged and exact >= 1


def test_skip_read_back_refuses_what_it_cannot_answer(monkeypatch):
    """The state and argument rules of sfm_debug_match_windows."""
    from sfmfromscratch_amd import _abi, _native
    q, t = S.rootsift_mixed(64, 31, 9)
    ctx = _native.Context(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), 0)
    with pytest.raises(RuntimeError):
        ctx.match_skips(0, 1)
    ctx.match(q, t, np.float32(RATIO))
    assert ctx.match_skips(0, 64).sum() >= 1
    for pair, rows in ((1, 1), (0, 65), (0, 0), (-1, 1)):
        with pytest.raises(ValueError):
            ctx.match_skips(pair, rows)
    ctx.close()
    monkeypatch.setenv("SFMFEAT_MATCH_DIRECT", "1")
    ctx = _native.Context(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), 0)
    monkeypatch.delenv("SFMFEAT_MATCH_DIRECT")
    ctx.match(q, t, np.float32(RATIO))
    with pytest.raises(RuntimeError):
        ctx.match_skips(0, 1)
    ctx.close()
