"""CPU: the fixture of per-sample PnP hypotheses in 60 digits (tests/golden/pnp_fits.npz,
tests/pnp_ref.py hypotheses_mp / dlt_all_mp) and everything tests/test_gpu_pnp_fits.py takes
from it without measuring it on the device: the admission (sigma_1 / sigma_11 <= 1e4 and
cond M <= 1e3 by the reference, at most 5 % of a case's samples left out), the deviation of the
two float64 routes of the restatement from the reference (the device's bound is 100 x that,
capped at 1e-8), and what the restatement does on the degenerate scenes.

Measured here (the constants of tests/pnp_ref.py are held to these figures):
  samples   18 of 1,165 samples of the pnp.npz cases left out (it300 10 of 300, bigrot 2 of 50),
            slab1 1 of 50; over the admitted ones the elimination restatement differs from the
            reference by at most 2.4e-11 in R (n65) and 2.9e-11 in t (n63), the SVD route by
            4.0e-11 (n65) and 1.7e-11 (it300)
  DLT       sigma_11 / sigma_12 from 133 (n7) to 171 (dltskew): all admitted; eigh of A^T A
            differs by at most 4.4e-13 in R and 3.5e-12 in t (n6), the SVD of A by 6.3e-15 and
            5.2e-14
  scenes    plane: 50 of 50 samples NaN; ident: all NaN; dup: 12 of 50 NaN (a sample that draws
            both copies of a correspondence), three samples tie at 60 of 60; tilted (1 NaN),
            slab3 (none): every other hypothesis finite, every count 0; collinear: 23 of 50
            NaN, every count 0; slab1: winner 59 of 60; lattice: 4 NaN with the first largest
            pivot row, 5 with the last, winner 60 of 60"""
from __future__ import annotations

import os

import numpy as np
import pytest

from tests import pnp_ref as PR
from tests.golden_util import GOLDEN, load

FITS = PR.fits_cases()
CAPPED = [k for k in FITS if k != "dup"]   # dup is a degenerate scene: its NaN samples are the point
DEG = PR.degenerate_cases()


def test_fixture_regenerates_byte_for_byte():
    pytest.importorskip("mpmath")
    data = PR.fixture_bytes(PR.fixture_arrays())
    assert data == open(os.path.join(GOLDEN, "pnp_fits.npz"), "rb").read()
    assert len(data) < os.path.getsize(os.path.join(GOLDEN, "pnp.npz"))


def test_fixture_holds_the_cases():
    z = load("pnp_fits.npz")
    assert [str(k) for k in z["fits"]] == list(FITS) and [str(k) for k in z["degenerate"]] == list(DEG)
    assert [str(k) for k in z["dlt"]] == list(PR.dlt_cases())
    for name, (X, x, K, iters) in DEG.items():
        assert np.array_equal(z[f"{name}_X"], X) and np.array_equal(z[f"{name}_x"], x), name
        assert np.array_equal(z[f"{name}_K"], K) and int(z[f"{name}_iters"]) == iters
        assert len(X) <= 2600 and iters <= 300
    for name, (X, x, K) in PR.dlt_cases().items():
        if name.startswith("dlt"):
            assert np.array_equal(z[f"{name}_X"], X) and np.array_equal(z[f"{name}_x"], x), name
            assert np.array_equal(X, X.astype(np.float32)) and np.array_equal(x, x.astype(np.float32))
    for name, (X, x, K, iters) in FITS.items():
        assert z[f"{name}_R"].shape == (iters, 3, 3) and z[f"{name}_admitted"].shape == (iters,)
        assert len(X) <= 2600 and iters <= 300
    for k, v in PR.fit_bounds().items():
        assert float(z[k]) == v and 0 < v <= PR.FIT_CAP
    assert len(PR.DLT_CASES_N) == 8 and sorted(len(PR.dlt_cases()[k][0]) for k in PR.DLT_CASES_N) == \
        [6, 7, 64, 65, 255, 256, 257, 513]


@pytest.mark.parametrize("name", CAPPED)
def test_at_most_5_percent_of_a_cases_samples_are_left_out(name):
    z = load("pnp_fits.npz")
    a = z[f"{name}_admitted"]
    assert np.array_equal(a, (z[f"{name}_s111"] <= PR.S_MAX) & (z[f"{name}_condM"] <= PR.CONDM_MAX))
    print(f"MEASURED {name}: {int((~a).sum())} of {len(a)} samples left out")
    assert (~a).mean() <= PR.MAX_LEFT_OUT
    assert np.isfinite(z[f"{name}_R"][a]).all() and np.isfinite(z[f"{name}_t"][a]).all()


def test_left_out_total_of_the_old_fixture_cases():
    z = load("pnp_fits.npz")
    old = [k for k in FITS if k not in PR.DEG_REFERENCED]
    left = {k: int((~z[f"{k}_admitted"]).sum()) for k in old}
    assert len(old) == 18 and sum(len(z[f"{k}_admitted"]) for k in old) == 1165
    assert sum(left.values()) == 18 and left["bigrot"] == 2


def test_float64_routes_against_the_reference_give_the_device_bounds():
    z = load("pnp_fits.npz")
    mR = mt = 0.0
    for name, (X, x, K, iters) in FITS.items():
        a = z[f"{name}_admitted"]
        idx = PR.samples(len(X), iters)
        for route in ("elim", "svd"):
            R, t = PR.hypotheses(X, x, K, idx, route)
            assert np.isfinite(R[a]).all() and np.isfinite(t[a]).all(), (name, route)
            dR, dt = PR.pose_deviation(R[a], t[a], z[f"{name}_R"][a], z[f"{name}_t"][a])
            print(f"MEASURED {name} {route}: max |dR| {dR.max():.3e} |dt| {dt.max():.3e} over {int(a.sum())} samples")
            mR, mt = max(mR, float(dR.max())), max(mt, float(dt.max()))
    print(f"MEASURED routes vs the 60-digit reference: max |dR| {mR:.3e} |dt| {mt:.3e}")
    # the constants are the measurement rounded up: not below it, not above twice it
    assert mR <= PR.CPU_MEASURED_R <= 2 * mR and mt <= PR.CPU_MEASURED_T <= 2 * mt


def test_dlt_routes_against_the_reference_and_every_dlt_case_is_admitted():
    z = load("pnp_fits.npz")
    mR = mt = 0.0
    for name, (X, x, K) in PR.dlt_cases().items():
        gap = float(z[f"{name}_dlt_gap"])
        assert gap >= PR.DLT_GAP_MIN, name
        for f in (PR.dlt_all, PR.dlt_all_svd):
            R, t = f(X, x, K)
            dR, dt = PR.pose_deviation(R[None], t[None], z[f"{name}_dlt_R"][None], z[f"{name}_dlt_t"][None])
            print(f"MEASURED dlt {name} {f.__name__}: sigma11/sigma12 {gap:.1f} max |dR| {dR[0]:.3e} |dt| {dt[0]:.3e}")
            mR, mt = max(mR, float(dR[0])), max(mt, float(dt[0]))
    assert mR <= PR.CPU_MEASURED_DLT_R <= 2 * mR and mt <= PR.CPU_MEASURED_DLT_T <= 2 * mt


def test_reference_is_a_rotation_and_agrees_with_the_planted_pose():
    z = load("pnp_fits.npz")
    for name in FITS:
        a = z[f"{name}_admitted"]
        R = z[f"{name}_R"][a]
        assert PR.rotation_defect(R).max() < 1e-15 and (np.linalg.det(R) > 0).all(), name
    for name in PR.dlt_cases():   # every point planted: the DLT's pose is the scene's to the pixel noise
        R = z[f"{name}_dlt_R"]
        assert PR.rotation_defect(R[None])[0] < 1e-15 and np.linalg.det(R) > 0
        assert np.abs(R - (PR.rot(0.12, -0.05, 0.03))).max() < 2e-2, name


def test_restatement_on_the_degenerate_scenes():
    got = {}
    for name, (X, x, K, iters) in DEG.items():
        idx = PR.samples(len(X), iters)
        with np.errstate(all="ignore"):   # (ident divides by a mean distance of 0)
            R, t = PR.hypotheses(X, x, K, idx)
        nan = np.isnan(R[:, 0, 0])
        whole = np.isnan(R).all(axis=(1, 2)) & np.isnan(t).all(axis=1)
        assert np.array_equal(nan, whole) and np.isfinite(R[~nan]).all() and np.isfinite(t[~nan]).all(), name
        counts = PR.inlier_mask(X, x, K, R, t).sum(axis=1)
        got[name] = (int(nan.sum()), int(counts.max()))
        print(f"MEASURED {name}: {int(nan.sum())} NaN hypotheses of {iters}, largest count {int(counts.max())} of {len(X)}")
        if name == "dup":   # the NaN samples are those that drew both copies of a correspondence
            twice = np.array([len(set(r // 2)) < 6 for r in idx])
            assert np.array_equal(nan, twice)
    assert got["plane"] == (PR.DEG_ITERS, 0) and got["ident"] == (9, 0)
    assert got["tilted"][1] == 0 and got["slab3"] == (0, 0)   # near-planar: finite hypotheses, worthless
    assert got["slab1"][0] == 0 and got["slab1"][1] >= PR.DEG_N - 2
    assert got["dup"][1] == PR.DEG_N and 0 < got["dup"][0] < PR.DEG_ITERS
    assert got["collinear"][1] == 0
    assert got["lattice"][1] == PR.DEG_N


def test_lattice_tells_the_first_largest_pivot_row_from_the_last():
    """The rule takes the first row of the largest magnitude.  On the lattice the other choice
    gives another NaN set and, in 26 of 50 samples, other bits."""
    X, x, K, iters = DEG["lattice"]
    idx = PR.samples(len(X), iters)
    Rf, tf = PR.hypotheses(X, x, K, idx)
    Rl, tl = PR.hypotheses(X, x, K, idx, route="elim_last")
    nf, nl = np.isnan(Rf[:, 0, 0]), np.isnan(Rl[:, 0, 0])
    differ = int(((Rf != Rl).any(axis=(1, 2)) & ~nf & ~nl).sum())
    print(f"MEASURED lattice: NaN samples {np.flatnonzero(nf)} (first), {np.flatnonzero(nl)} (last); {differ} finite "
          f"samples with other bits")
    assert not np.array_equal(nf, nl) and differ >= 10


def test_exact_plane_columns_are_exactly_zero():
    """Why the plane's NaN set is not a rounding question: the centred z of six points with the
    same z is exactly 0, so columns 2, 6 and 10 of every sample's system are."""
    X, x, K, iters = DEG["plane"]
    idx = PR.samples(len(X), iters)
    A, s, c = PR.sample_systems(X[idx], PR.normalised_pixels(x, K)[idx])
    assert (A[:, :, [2, 6, 10]] == 0).all() and np.isfinite(s).all()
    Xi, xi, Ki, it = DEG["ident"]
    with np.errstate(all="ignore"):
        A, s, c = PR.sample_systems(Xi[PR.samples(6, it)], PR.normalised_pixels(xi, Ki)[PR.samples(6, it)])
    assert np.isinf(s).all()


def test_dup_has_a_tie_for_the_maximum():
    X, x, K, iters = DEG["dup"]
    r = PR.pnp_ransac(X, x, K, iters)
    top = np.flatnonzero(r["counts"] == r["counts"].max())
    print(f"MEASURED dup: {len(top)} samples share the largest count {int(r['counts'].max())}; the first is {top[0]}")
    assert len(top) >= 2 and r["iteration"] == top[0]
