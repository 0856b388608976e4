"""CPU: the structure stage's pieces that need no device — the restatement
(tests/structure_ref.py) against the reference's own outputs (tests/golden/structure.npz), the
conditions the GPU comparisons of tests/test_gpu_structure.py rely on, the argument checks
the Python layer makes before any device call, and the three new C-ABI symbols.

X_REF_TOL and COST_DELTA live in tests/structure_ref.py (the GPU tests use them too); how
they were measured is in the docstrings of the tests below.  Every figure is printed before
its assertion."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from sfmfromscratch_amd import _native, pose
from tests import structure_ref as SR
from tests.golden_util import load

REFINE_NAMES = list(SR.refine_cases().keys())
LINK_NAMES = list(SR.link_cases().keys())


def rcase(z, name):
    g = lambda k: z[f"{name}_{k}"]
    return g("X0"), g("p1"), g("p2"), g("P1"), g("P2")


def rel_err(X, ref):
    return np.linalg.norm(X - ref, axis=1) / np.linalg.norm(ref, axis=1)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The committed restatement run here, once per case (never modified)."""
    return SR.refine(*rcase(load("structure.npz"), name))


def test_fixture_holds_the_cases_of_structure_ref():
    z = load("structure.npz")
    assert list(z["names"]) == REFINE_NAMES and list(z["link_names"]) == LINK_NAMES
    for name, c in SR.refine_cases().items():
        for a, b in zip(rcase(z, name)[1:], c):
            assert np.array_equal(a, b), name
    for name, c in SR.link_cases().items():
        for key, b in zip(("tgt", "p3d", "qry", "nxt", "thr"), c):
            a = z[f"link_{name}_{key}"]
            assert np.array_equal(a, b) and a.dtype == np.asarray(b).dtype, (name, key)
    assert z["link_int64_tgt"].dtype == np.int64 and z["link_l64_65_tgt"].dtype == np.int32


@pytest.mark.parametrize("name", REFINE_NAMES)
def test_restatement_here_equals_the_fixture(name):
    """The restatement's outputs in the fixture were computed where the fixture was made; numpy
    here reproduces them (the marginal last steps may fall differently with another BLAS:
    X to 1e-10 relative, the cost to 1e-9)."""
    z = load("structure.npz")
    r = restated(name)
    ex = rel_err(r["X"], z[f"{name}_rest_X"]).max()
    ec = (np.abs(r["cost"] - z[f"{name}_rest_cost"]) / z[f"{name}_rest_cost"]).max()
    print(f"MEASURED {name}: restatement here vs fixture X {ex:.3e} cost {ec:.3e}")
    assert ex <= 1e-10 and ec <= 1e-9
    assert (r["iters"] >= z[f"{name}_rest_firm"]).all()


def test_restatement_vs_reference_clean_cases():
    """max ||X_ref - X_rest|| / ||X_rest|| over the clean cases, measured with the committed
    restatement: 3.874e-8 (c200; the others 5.4e-11 to 1.1e-8) — the reference's scipy solve
    stops at its own tolerances, short of the minimum.  X_REF_TOL = min(1e-6, 100 x 3.874e-8)
    = 1e-6, the cap.

    Condition (not a measurement): every clean case's own largest movement
    max ||X_rest - X_linear|| / ||X_rest|| is at least 10 x X_REF_TOL, so an implementation
    that returns its input fails the GPU comparison."""
    z = load("structure.npz")
    worst = 0.0
    for name in SR.CLEAN:
        r = restated(name)
        e = rel_err(z[f"{name}_Xref"], r["X"]).max()
        moved = rel_err(z[f"{name}_X0"], r["X"]).max()
        print(f"MEASURED {name}: restatement vs reference {e:.3e}; moved by the refinement {moved:.3e}")
        worst = max(worst, e)
        assert e <= SR.X_REF_TOL, name
        assert moved >= 10 * SR.X_REF_TOL, name
    print(f"MEASURED largest over the clean cases {worst:.3e} (X_REF_TOL {SR.X_REF_TOL:.1e})")
    assert SR.X_REF_TOL == min(1e-6, 100 * SR.X_REF_MEASURED)


def test_restatement_cost_never_above_the_reference():
    """For every point of every case, wild ones included (they are compared on cost only):
    cost_rest <= cost_ref (1 + COST_DELTA).  Largest positive relative excess measured with
    the committed restatement: COST_EXCESS_MEASURED in tests/structure_ref.py;
    COST_DELTA = 100 x that, floored at 1e-12 and capped at 1e-9."""
    z = load("structure.npz")
    worst = -np.inf
    for name in REFINE_NAMES:
        X0, p1, p2, P1, P2 = rcase(z, name)
        r = restated(name)
        cost_ref = SR.point_costs(z[f"{name}_Xref"], p1, p2, P1, P2)
        cost_rest = SR.point_costs(r["X"], p1, p2, P1, P2)
        assert np.allclose(cost_rest, r["cost"], rtol=1e-9, atol=0), name
        ex = ((r["cost"] - cost_ref) / cost_ref).max()
        gain = ((cost_ref - r["cost"]) / cost_ref).max()
        print(f"MEASURED {name}: largest relative cost excess over the reference {ex:.3e} (largest gain {gain:.3e})")
        worst = max(worst, ex)
        assert (r["cost"] <= cost_ref * (1 + SR.COST_DELTA)).all(), name
    print(f"MEASURED largest positive excess {max(worst, 0.0):.3e} (COST_DELTA {SR.COST_DELTA:.1e})")
    assert SR.COST_DELTA == min(1e-9, max(1e-12, 100 * SR.COST_EXCESS_MEASURED))


@pytest.mark.parametrize("name", REFINE_NAMES)
def test_printed_line(name):
    """The reference's printed line equals the restatement's mean to 4 decimals, and no fixture
    mean lies within 1e-7 of a rounding boundary (so 1e-10-level differences cannot flip it)."""
    z = load("structure.npz")
    X0, p1, p2, P1, P2 = rcase(z, name)
    mean, err = SR.reprojection_error(z[f"{name}_Xref"], p1, p2, P1, P2)
    assert str(z[f"{name}_line"]) == f"Mean Reprojection Error: {mean:.4f}"
    frac = (mean * 1e4) % 1.0
    print(f"MEASURED {name}: mean {mean:.10f}, distance to a 4-decimal rounding boundary {abs(frac - 0.5) * 1e-4:.3e}")
    assert abs(frac - 0.5) * 1e-4 > 1e-7
    assert err.shape == (len(p1), 2)


@pytest.mark.parametrize("name", LINK_NAMES)
def test_link_restatement_equals_a_direct_loop(name):
    z = load("structure.npz")
    g = lambda k: z[f"link_{name}_{k}"]
    tgt, qry, thr = g("tgt"), g("qry"), float(g("thr"))
    ti, qi = [], []
    for q in range(len(qry)):
        d = [np.linalg.norm(tgt[k] - qry[q]) for k in range(len(tgt))]
        k = int(np.argmin(d))
        if d[k] < thr:
            ti.append(k)
            qi.append(q)
    rp, rn, rti, rqi = SR.link_results(tgt, g("p3d"), qry, g("nxt"), thr)
    assert rti.tolist() == ti and rqi.tolist() == qi
    assert np.array_equal(rti, g("ti")) and np.array_equal(rqi, g("qi"))
    assert rp.shape == g("prev").shape and np.array_equal(rp, g("prev")) and rp.dtype == g("prev").dtype
    assert rn.shape == g("next").shape and np.array_equal(rn, g("next")) and rn.dtype == g("next").dtype


def test_link_fixture_covers_the_planted_edges():
    z = load("structure.npz")
    # duplicates and equal distances: the first index
    assert z["link_dups_ti"].tolist() == [0, 0, 0, 1, 0] and z["link_dups_qi"].tolist() == [0, 1, 2, 3, 4]
    # d = 5.0 exactly is not < 5.0; the offset (2, 4), d^2 = 20, is
    assert z["link_edge5_qi"].tolist() == [1]
    # the same scene at thresholds 5.0, 4.5 and 4.4: d^2 = 25 is never kept; d^2 = 20 (4.472) is kept
    # at 5.0 and 4.5 (no integer offset has 4.5 <= d < 5) and dropped at 4.4
    for name, expect in (("l64_65", True), ("thr4_5", True), ("thr4_4", False)):
        tgt, qry = z[f"link_{name}_tgt"].astype(np.int64), z[f"link_{name}_qry"].astype(np.int64)
        d2 = ((tgt[z[f"link_{name}_ti"]] - qry[z[f"link_{name}_qi"]]) ** 2).sum(1)
        assert (20 in d2.tolist()) == expect and 18 in d2.tolist() and 25 not in d2.tolist(), name
    assert len(z["link_thr4_4_ti"]) < len(z["link_thr4_5_ti"])
    assert len(z["link_nothing_ti"]) == 0 and z["link_nothing_prev"].shape == (0,)
    assert z["link_nothing_prev"].dtype == np.float64 and z["link_nothing_next"].dtype == np.float64
    assert len(z["link_l2561_300_tgt"]) == SR.LINK_CHUNK + 1
    print(f"MEASURED l2561_300: largest kept target index {z['link_l2561_300_ti'].max()}")


def test_argument_errors_come_before_any_device_call(monkeypatch):
    """ValueError from the Python layer alone: context_for is made to fail loudly."""
    def no_device(*a, **k):
        raise AssertionError("a device call was attempted")

    monkeypatch.setattr(pose, "context_for", no_device)
    z = load("structure.npz")
    g = lambda k: z[f"link_l64_65_{k}"]
    tgt, p3d, qry, nxt = g("tgt"), g("p3d"), g("qry"), g("nxt")
    with pytest.raises(ValueError, match="integer"):
        pose.link_points(tgt + 0.5, p3d, qry, nxt)
    with pytest.raises(ValueError, match="integer"):
        pose.link_points(tgt, p3d, qry.astype(np.float64) + 0.25, nxt)
    with pytest.raises(ValueError, match="argmin of an empty sequence"):
        pose.link_points(np.empty((0, 2), np.int32), np.empty((0, 3)), qry, nxt)
    with pytest.raises(ValueError):
        pose.link_points(tgt, p3d[:-1], qry, nxt)
    with pytest.raises(ValueError):
        pose.link_points(tgt, p3d, qry, nxt[:-1])
    with pytest.raises(ValueError):
        pose.link_points(tgt.ravel(), p3d, qry, nxt)
    with pytest.raises(ValueError, match="2\\^30"):
        pose.link_points(tgt.astype(np.int64) + (1 << 31), p3d, qry, nxt)
    X0, p1, p2, P1, P2 = rcase(z, "c12")
    for fn in (pose.non_linear_triangulation, pose.reprojection_error):
        with pytest.raises(ValueError):
            fn(X0[:, :2], p1, p2, P1, P2)
        with pytest.raises(ValueError):
            fn(X0, p1[:-1], p2, P1, P2)
        with pytest.raises(ValueError):
            fn(X0, p1, p2, P1[:2], P2)
    with pytest.raises(ValueError, match="case 1"):
        pose.refine_points_batch([(X0, p1, p2, P1, P2), (X0, p1, p2[:3], P1, P2)])
    # integral floats are integers (what np.round leaves), as for find_inliers
    assert pose._link_coords(tgt.astype(np.float64), "points_2d_prev").shape == tgt.shape


def test_new_symbols_resolve_in_the_built_library():
    L = _native.load_library()
    for name in ("sfm_refine_points_dev", "sfm_reprojection_error_dev", "sfm_link_points_dev"):
        assert name in _native.SIGNATURES and getattr(L, name) is not None
    assert L.sfm_abi_version() == 1
    # a null context is an argument error of every call, before any device use
    from sfmfromscratch_amd import _abi
    assert L.sfm_refine_points_dev(None, None, None, None, 0, None, 1, None, 50, None, None, None, None) == _abi.SFM_EINVAL
    assert L.sfm_reprojection_error_dev(None, None, None, None, 0, None, None, None, None, None) == _abi.SFM_EINVAL
    assert L.sfm_link_points_dev(None, None, 1, None, 0, 5.0, None, None, None, None) == _abi.SFM_EINVAL
