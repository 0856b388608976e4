"""The matcher's restatement (tests/match_ref.py) held against the C oracle, and the prefilter's
error bound E checked on the host for every case family of match_ref.CASES — tables far outside
the unit-norm RootSIFT rows the other matcher tests use (integers 0..255, signed, a common
offset with small noise, tiny magnitudes, mixed row scales, one dominant element, zero rows,
elements at and beyond the float16 range).

Measured on the host (printed by the tests, never used as tolerances): the largest share of E
that |d~_f64 - d_ref| + T2 + T3 + T4 (match_ref's docstring) uses, per class:
    unit 0.095, u8 0.412, signed 0.413, offset 0.389, tiny 0.000, mixed 0.442, spike 0.414,
    zeros 0.098, edge(255.9) 0.396
Emulated window sizes (#{j : d~ <= b2~ + 2E}) of the 96 x 700 offset cases:
    offset(0.03) 2-8, offset(0.01) 2-100, offset(0.006) 2-593, offset(0.003) 700-700
"""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import match_ref as R
from tests.golden_util import assert_matches_equal

ALL = range(len(R.CASES))
IN_RANGE = [i for i in ALL if R.in_f16_range(*R.case(i))]


def test_case_list_covers_the_shapes_and_classes():
    assert {c[1] for c in R.CASES} == {1, 96, 130, 260}
    assert {c[2] for c in R.CASES} == {2, 33, 65, 700}
    assert {c[0] for c in R.CASES} == set(R.GENERATORS)
    out = [R.CASES[i][0] for i in ALL if i not in IN_RANGE]
    assert sorted(set(out)) == ["edge(1000)", "edge(1e4)", "edge(256)", "huge"]
    q, t = R.case(R.CASE_IDS.index("u8-130x700"))
    assert q.min() >= 0 and t.max() == 255 and np.array_equal(q, np.round(q))
    q, t = R.case(R.CASE_IDS.index("edge(255.9)-130x700"))
    assert max(np.abs(q).max(), np.abs(t).max()) == np.float32(255.9)
    q, t = R.case(R.CASE_IDS.index("tiny(1e-6)-96x700"))
    tiny32 = np.finfo(np.float32).tiny
    assert ((q > 0) & (q < tiny32)).any() and ((t > 0) & (t < tiny32)).any()


@pytest.mark.parametrize("i", ALL, ids=R.CASE_IDS)
def test_literal_matcher_equals_the_oracle(i):
    """The reference's matcher written out in numpy == oracle.match on every case: the oracle is
    pinned outside RootSIFT tables too (ties as sets)."""
    q, t = R.case(i)
    m, c = R.match(q, t, R.RATIO)
    om, oc = O.match(q, t, R.RATIO)
    assert_matches_equal(m, c, om, oc)
    if R.CASES[i][0] != "zeros" and R.CASES[i][1] >= 130 and R.CASES[i][2] >= 33:
        assert len(c) > 0  # planted neighbours: the case really matches something


def test_zero_rows_follow_the_positive_second_distance_rule():
    q, t = R.case(R.CASE_IDS.index("zeros-130x65"))
    m, _ = R.match(q, t, R.RATIO)
    assert 0 not in m[:, 0].tolist()          # d1 = d2 = 0: no match
    assert [1, 2] in m.tolist()               # its copy at distance 0, second distance > 0
    q, t = R.case(R.CASE_IDS.index("zeros-1x2"))
    m, c = R.match(q, t, R.RATIO)
    assert m.tolist() == [[0, 0]] and c.tolist() == [0.0]


def test_operand_restatement_basics():
    """hi + lo 2^-11 reproduces x 2^8 to 2^-22 relative; padding rows, block maxima and the
    out-of-range flag are as k_match_prep writes them."""
    q, t = R.case(R.CASE_IDS.index("signed-130x65"))
    op = R.operands(t, 768)
    assert op["hi"].shape == (768, 128) and op["pmax"].shape == (48, 2)
    rec = op["hi"][:65].astype(np.float64) + op["lo"][:65].astype(np.float64) * 2.0 ** -11
    assert np.all(np.abs(rec - t.astype(np.float64) * 256) <= 2.0 ** -21 * np.abs(t) * 256 + 2.0 ** -36)
    assert np.all(np.isinf(op["norm2"][65:])) and not op["rnorm"][65:].any() and not op["hi"][65:].any()
    assert op["pmax"][4, 0] == op["norm2"][64] and not op["pmax"][5:].any()
    assert np.allclose(op["norm2"][:65], (t.astype(np.float64) ** 2).sum(axis=1), rtol=1e-7)
    q, t = R.case(R.CASE_IDS.index("edge(256)-130x700"))
    op = R.operands(t)
    rows = np.flatnonzero(op["flagged"])
    assert rows.tolist() == [700 // 3, 698]
    assert not op["hi"][rows].any() and np.all(np.isinf(op["rnorm"][rows])) and np.isfinite(op["norm2"][rows]).all()
    assert np.isinf(R.bound(R.operands(q), op)).all()
    assert not R.operands(R.case(R.CASE_IDS.index("edge(255.9)-130x700"))[1])["flagged"].any()


def test_bound_is_rigorous_inside_f16_range(capsys):
    """|d~_f64 - d_ref| + T2 + T3 + T4 <= E for every (query, target) of every case whose elements
    are inside the f16 range (T2..T4 derived from unit roundoff in match_ref's docstring)."""
    share = {}
    for i in IN_RANGE:
        a = R.analysis(i)
        t2, t3, t4 = R.rounding_terms(a["qa"], a["tb"], a["d64"])
        used = np.abs(a["dt"] - a["d32"].astype(np.float64)) + t2 + t3 + t4
        E = a["E"].astype(np.float64)[:, None]
        assert np.isfinite(E).all()
        s = float((used / E).max())
        share[R.class_of(i)] = max(share.get(R.class_of(i), 0.0), s)
        assert np.all(used <= E), (R.CASE_IDS[i], s)
    with capsys.disabled():
        print("\nlargest share of E used per class:", {k: round(v, 4) for k, v in share.items()})


def test_window_bands_of_the_offset_cases(capsys):
    """The emulated windows put each offset(amp) case where it exercises the list machinery:
    0.03 a few targets per row, 0.01 around the 128-entry half-list limit, 0.003 every target."""
    w = {}
    for amp in ("0.03", "0.01", "0.006", "0.003"):
        a = R.analysis(R.CASE_IDS.index("offset(%s)-96x700" % amp))
        w[amp] = R.windows(a["dt"], a["E"])
    with capsys.disabled():
        print("\nemulated window sizes:", {k: (int(v.min()), int(v.max())) for k, v in w.items()})
    assert w["0.03"].max() <= 16
    assert (w["0.01"] > 64).any() and (w["0.01"] < 8).any()
    assert np.all(w["0.003"] == 700)
    a = R.analysis(R.CASE_IDS.index("tiny(1e-6)-96x700"))
    assert np.all(R.windows(a["dt"], a["E"]) == 700)
    a = R.analysis(R.CASE_IDS.index("unit-130x700"))
    assert R.windows(a["dt"], a["E"]).max() <= 16
