"""k_select's branches, each on a plane built to take it.

sfm_debug_select runs what an extraction runs after Harris - select scan, certified NMS, one
k_select launch - on host planes.  The probe calls are built in tests/select_ref.py (where the CPU
test holds their claims to the route restatement).  Every case first asserts, from the library's
own branch sizes, which route its planes must take; only then is the device's answer compared,
exactly: the scan's fields, the certified candidate count, fallback as it reads after the launch,
the exact median's bits, and count, x, y and the confidences' bits against the numpy restatement
of NaiveSIFT.py:77-120.  No tolerance anywhere: keys are unique.
"""
from __future__ import annotations

import numpy as np
import pytest

from sfmfromscratch_amd import _native
from tests import select_ref as S

pytestmark = pytest.mark.gpu

BASE = S.FALLBACK_CONSTS   # only to enumerate the case names at collection; run() takes the library's


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(sp):
    """Assert the routes, run the probe, compare every plane exactly.  -> the probe's output."""
    k, ksize, vmin, fx = sp["k"], sp["ksize"], sp["vmin"], sp["force_exact"]
    base = _native.select_constants(1)
    consts = _native.select_constants(k)
    assert consts == S.consts_for(k, base)          # select_ref's rule for sel_cap and med_cap is the library's
    labels = S.route_labels(sp, base)
    out, c2 = _native.debug_select(sp["levels"], k, ksize, sp["hw"], vmin, fx)
    assert c2 == consts
    for l, R in enumerate(sp["levels"]):
        res, st = out[l], out[l]["state"]
        for b in range(R.shape[0]):
            at, lab = (l, b, labels[l][b]), labels[l][b]
            s = S.scan_ref(R[b], vmin, fx)
            for f in ("bucket0", "bucket1", "rank0", "rank1", "odd", "tnms", "tcert", "tsub0", "tsub1"):
                assert int(st[f][b]) == s[f], (f,) + at
            want_fb = s["fallback"] if lab[0] == "k0" else 0 if lab[0] == "certified" else 1
            assert int(st["fallback"][b]) == want_fb, at
            want_nc = 0 if s["fallback"] else int(S.certified_candidates(R[b], s["tnms"], ksize).sum())
            assert int(res["ncand"][b]) == want_nc, at
            x, y, c, med = S.select_ref(R[b], k, ksize, sp["hw"][l])
            if lab[0] in ("fallback_scan", "fallback_run"):
                assert bits(st["median"][b]) == bits(med), at + (st["median"][b], med)
            m = int(res["count"][b])
            assert m == x.size, at + (m, x.size)
            assert np.array_equal(res["x"][b, :m], x) and np.array_equal(res["y"][b, :m], y), at
            if (l, b) in sp["by_value"]:
                assert np.array_equal(res["conf"][b, :m], c), at
            else:
                assert np.array_equal(bits(res["conf"][b, :m]), bits(c)), at
    return out


def names(specs):
    return [sp["name"] for sp in specs]


@pytest.mark.parametrize("name", names(S.topk_specs(BASE)))
def test_topk_counts_ties_k_subsets_and_certification_edges(name):
    """Candidate counts k - 1 (run-time fall-back: the exact path's answer, fallback reads 1), k,
    sel_cap, sel_cap + 1, the register form's limit and one more; ties of kTieLdsCap, one more, the
    k-th as last tie and as first with nothing above, in the register and the global form; k of 0,
    1, 2048, 2049, 2500, 8192; the three subset routes and their boundaries; the k-th key on the
    first key above the median's bucket and on the last key inside it; a plane from 2^126 up."""
    run(S.pick(S.topk_specs(_native.select_constants(1)), name))


@pytest.mark.parametrize("name", names(S.median_specs(BASE)))
def test_exact_median_parities_buckets_and_list_lengths(name):
    """n odd and even, 16-byte and scalar loads; the middle pair in one bucket, in two, astride
    zero; an all-equal plane, a median of 0 among zeros, a negative median, a sum that rounds, one
    -0.0 pixel; collected lists of med_cap - 1, med_cap, med_cap + 1 (also with scalar loads),
    twice and four times med_cap, at k = 20 and k = 2500."""
    sp = S.pick(S.median_specs(_native.select_constants(1)), name)
    out = run(sp)
    for l, b in sp["by_value"]:   # the -0.0 pixel is among the keypoints, as +0
        m = int(out[l]["count"][b])
        assert m >= 1 and out[l]["conf"][b, m - 1] == 0 and bits(out[l]["conf"][b, m - 1]) == 0


@pytest.mark.parametrize("name", S.NMS_NAMES)
def test_exact_nms_rows_chunks_and_windows(name):
    """3 x 3 with float4 rows (widths across the 256-column chunk) and scalar rows (chunk pairs of
    128), heights around the 16 waves x 3 or 2 rows of a pass, and the window loop at ksize 1, 5, 7
    and 31; plateaus, large values, a flat zero half, zeros below a positive median and above a
    negative one, and for every window wider than a pixel the ring planes, where they fit (not at
    W = 4, W = 1 or H < 5: S.RING_LESS)."""
    run(S.pick(S.nms_specs(_native.select_constants(1)), name))


def test_edge_filter_keeps_the_order_and_can_empty_the_list():
    """hw 0, 1, 8 and min(H, W) / 2 on one plane whose best keypoints include border pixels."""
    sp = S.emit_spec()
    R = sp["levels"][0][0]
    x0, y0, _, _ = S.select_ref(R, sp["k"], 3, 0)
    assert np.any((x0 == 0) | (y0 == 0) | (x0 == 29) | (y0 == 19))
    out = run(sp)
    cnt = [int(o["count"][0]) for o in out]
    assert cnt[0] == x0.size and cnt[0] > cnt[1] > cnt[2] > 0 and cnt[3] == 0
    full = list(zip(out[0]["y"][0, :cnt[0]].tolist(), out[0]["x"][0, :cnt[0]].tolist()))
    for l in (1, 2):   # the filtered list is the unfiltered one with the border keypoints struck out
        h = sp["hw"][l]
        kept = [(y, x) for y, x in full if h <= y < 20 - h and h <= x < 30 - h]
        assert kept == list(zip(out[l]["y"][0, :cnt[l]].tolist(), out[l]["x"][0, :cnt[l]].tolist()))


def test_one_call_certified_runtime_fallback_and_all_zero_planes():
    out = run(S.batch_spec())
    assert out[0]["state"]["fallback"].tolist() == [0, 1, 1]
    assert out[0]["count"].tolist() == [100, 100, 100]


@pytest.mark.parametrize("i", range(2), ids=["certified", "forced_exact"])
def test_three_levels_of_two_planes_equal_the_single_plane_calls(i):
    """The level-major workgroup index and the per-level scratch regions: every (level, plane) of
    one launch over three shapes equals the launch of that plane alone."""
    sp = S.level_specs()[i]
    out = run(sp)
    for l, R in enumerate(sp["levels"]):
        for b in range(2):
            one, _ = _native.debug_select(R[b:b + 1], sp["k"], sp["ksize"], sp["hw"][l], sp["vmin"],
                                          sp["force_exact"])
            for f in ("x", "y", "count", "ncand"):
                assert np.array_equal(one[0][f][0], out[l][f][b]), (f, l, b)
            assert np.array_equal(bits(one[0]["conf"][0]), bits(out[l]["conf"][b]))
            for f, v in one[0]["state"].items():
                assert v.view(np.uint32)[0] == out[l]["state"][f].view(np.uint32)[b], (f, l, b)


def test_probe_rejects_what_a_context_rejects():
    R = np.zeros((1, 8, 8), np.float32)
    for kw in (dict(k=8193), dict(k=-1), dict(ksize=4), dict(ksize=33), dict(vmin=2), dict(half_window=-1)):
        args = dict(k=5, ksize=3, half_window=0, vmin=100)
        args.update(kw)
        with pytest.raises(ValueError):
            _native.debug_select(R, **args)
    _native.debug_select(R, 5, 33, 0, 100, force_exact=True)   # the window loop takes any odd size
    with pytest.raises(ValueError):
        _native.debug_select([R] * 5, 5, 3, 0, 100)


def test_every_route_label_is_asserted_by_some_case():
    """The union of the labels the cases above assert - the atoms of their full labels and of the
    atoms they require, not whatever else their planes happen to take; recomputed here, so that it
    does not depend on which of them ran - is every label path_ref can return."""
    base = _native.select_constants(1)
    asserted = set()
    for sp in S.all_specs(base):
        S.route_labels(sp, base, asserted)
    assert asserted == S.ALL_LABELS, (S.ALL_LABELS - asserted, asserted - S.ALL_LABELS)
