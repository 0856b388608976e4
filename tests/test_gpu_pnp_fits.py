"""GPU: every sample of the PnP RANSAC (pnp.hip: k_pnp_hyp, k_pnp_count, k_pnp_select) and the
start pose of k_pnp_dlt_all through the read-back sfm_debug_pnp_fits: the 12 doubles (R, t) and
the inlier count of every sample, not only the integer table and the winner.

a. Every admitted sample's (R, t) against rule 2 of DESIGN.md §13D computed in 60 digits
   (tests/golden/pnp_fits.npz; admitted: sigma_1 / sigma_11 <= 1e4 and cond M <= 1e3 by the
   reference, at most 5 % of a case left out, tests/test_pnp_fits_cpu.py).  Bound: 100 x the
   larger deviation of the two float64 routes on the CPU (elimination restatement, LAPACK SVD)
   from the same reference over the same samples — 5e-9 in R, 3.5e-9 in |dt| / max(1, |t|); for
   the all-points DLT (eigh of A^T A, SVD of A) 5.5e-11 and 4.5e-10.  The bounds are read from
   the fixture; none comes from the device.  Orthogonality of every finite R: 100 x the
   restatement's own defect over the same samples.
   Measured on the MI355X: samples max |dR| 1.597e-11, |dt| 1.867e-11 (both n65; the other
   cases 6e-15 to 1.0e-11); DLT 3.447e-14 and 2.680e-13 (n6; 2e-16 to 9e-16 in R for n >= 64);
   max |R R^T - I| 1.1e-15 to 6.7e-7 (it300, a left-out sample), at most 2.2 x the restatement's.
b. counts[s] against the device's own hypothesis: the number of points with depth > 0 and
   error < thr under the read-back (R, t), in longdouble; an entry within the rounding band of
   the threshold or of depth 0 (rounding_bands; floor BAND) is decided by tests/pnp_ref.py
   errors, which repeats the device's float64 operations in their order.  Every entry is
   decided, none is left out.  Measured: no count differs anywhere; the band holds an entry
   only where the threshold is set to a point's own error.
c. Selection against the read-back: the first strict maximum, the mask under hyp[out_iter] in
   input order, start_Rt with hyp[out_iter]'s bits.
d. Degenerate scenes: what the rule guarantees and nothing more.  Measured: plane 50 of 50 and
   ident 9 of 9 NaN, no pose; tilted 1 NaN, slab3 none, collinear 28 NaN, every count 0, no
   pose; dup 12 NaN (the restatement's 12), winner 28 of the tied 28, 29, 49 with 60 of 60;
   lattice: 7.0e-13 from the first-row pivot choice, 14.7 from the last-row one in sample 10.
e. k_pnp_dlt_all's pose after sfm_pnp_dev against the 60-digit DLT.
f. Refinement statuses 3 (iteration limit 1 and 2: [1, 3, 1, 1], [1, 3, 2, 2], cost within
   1.2e-14 of the restatement's) and 2 ([1, 2, 0, 0], cost [inf, inf]) on the device.

Every test prints its figures before asserting; the tables are in DESIGN.md §13D.  Against
arithmetic mutants of pnp.hip (§13D): the last-largest pivot row fails the lattice test,
`error <= thr` the own-error threshold tests, a count round short the n64 / lm256 / n2600 /
2560 / 2561 cases, the wrong dropped row every case of (a); `depth >= 0` computes the same
function (at depth 0 the error is inf or NaN) and no test can tell it apart."""
from __future__ import annotations

import time

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native, pose
from tests import pnp_ref as PR
from tests.golden_util import load

pytestmark = pytest.mark.gpu

COST_TOL = 1.662e-11   # tests/test_gpu_pnp.py COST_TOL
BAND = 1e-9            # px: the floor of the band in which float64's own operations decide an entry
LD = np.longdouble

_Z = {}


def fits():
    if "fits" not in _Z:
        _Z["fits"] = load("pnp_fits.npz")
    return _Z["fits"]


def old():
    if "old" not in _Z:
        _Z["old"] = load("pnp.npz")
    return _Z["old"]


def case(name):
    """(X, x, K, iters) of a case of either fixture."""
    z = fits()
    if f"{name}_X" in z.files:
        return z[f"{name}_X"], z[f"{name}_x"], z[f"{name}_K"], int(z[f"{name}_iters"]) if f"{name}_iters" in z.files else 0
    z = old()
    return z[f"{name}_X"], z[f"{name}_x"], z[f"{name}_K"], int(z[f"{name}_iters"])


FIT_CASES = [str(k) for k in fits()["fits"]]
DEG_CASES = [str(k) for k in fits()["degenerate"]]
DLT_CASES = [str(k) for k in fits()["dlt"]]


def test_case_lists_are_the_modules():
    assert FIT_CASES == list(PR.fits_cases()) and DEG_CASES == list(PR.degenerate_cases())
    assert DLT_CASES == list(PR.dlt_cases())


def ctx():
    return _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))


def run(X, x, K, iters, thr=PR.THRESHOLD, mi=pose.REFINE_MAX_ITER):
    """One sfm_pnp_ransac_dev call and its read-back -> dict of host arrays."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    c = ctx()
    t0 = time.perf_counter()
    o = pose._pnp_ransac_dev(t(X), t(x), t(K).reshape(-1), iters, thr, mi, dev, ctx=c)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    sampled = len(X) >= 6 and iters > 0
    hyp, counts, start = c.pnp_fits(iters if sampled else 0)
    r = {k: v.cpu().numpy() for k, v in o.items()}
    r["counts"] = r["counts"][:iters]
    r.update(hyp=hyp, rb_counts=counts, start=start, ms=ms, on=int(r["n"][0]), it=int(r["iteration"][0]))
    if sampled:   # the table the call returns is the table the selection read
        assert np.array_equal(counts, r["counts"])
    return r


def run_pnp(X, x, K, mi=pose.REFINE_MAX_ITER):
    """One sfm_pnp_dev call and its read-back (start_Rt: the DLT's pose)."""
    import torch
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    c = ctx()
    dX, dx, dK = t(X), t(x), t(K).reshape(-1)
    R, tt, cost = (torch.empty(k, dtype=torch.float64, device=dev) for k in (9, 3, 2))
    st = torch.empty(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _native.check(c.lib.sfm_pnp_dev(c.handle, dX.data_ptr(), dx.data_ptr(), dK.data_ptr(), len(X), mi, R.data_ptr(),
                                    tt.data_ptr(), st.data_ptr(), cost.data_ptr(), None), c.handle)
    torch.cuda.synchronize()
    start = c.pnp_fits(0)[2]
    return dict(R=R.cpu().numpy(), t=tt.cpu().numpy(), status=st.cpu().numpy(), cost=cost.cpu().numpy(), start=start)


_RUNS = {}


def device(name):
    """One device run of a case at the threshold 8 and 50 refinement iterations, shared (never modified)."""
    if name not in _RUNS:
        X, x, K, iters = case(name)
        _RUNS[name] = run(X, x, K, iters)
        print(f"MEASURED {name}: device call {_RUNS[name]['ms']:.1f} ms")
    return _RUNS[name]


def split(hyp):
    return hyp[:, :9].reshape(-1, 3, 3), hyp[:, 9:]


def whole_nan(hyp, what):
    """Each hypothesis is finite or NaN as a whole -> the NaN rows."""
    nan = np.isnan(hyp).all(axis=1)
    assert np.isfinite(hyp[~nan]).all(), f"{what}: samples {np.flatnonzero(~nan & ~np.isfinite(hyp).all(axis=1))[:8]} partly finite"
    return nan


def rounding_bands(X, x, K, R, t):
    """What float64 can be wrong by at each (sample, point), from the sizes of the terms it adds
    (in longdouble): (band of the error [S, n], band of the depth [S, n]).  With A_k = sum_j
    |R_kj X_j| + |t_k|, the camera coordinates carry about eps A_k, the projection
    eps (|K| A) / |q2| and, through the division, eps |p| A_2 / |a_2|; 64 eps covers the dozen
    operations of the chain with room to spare."""
    eps = LD(np.finfo(np.float64).eps)
    aX, aK = np.abs(X).astype(LD), np.abs(K).astype(LD)
    A = [np.abs(R[:, k, :]).astype(LD) @ aX.T + np.abs(t[:, k, None]).astype(LD) for k in range(3)]
    e, z = PR.errors(X.astype(LD), x.astype(LD), K.astype(LD), R.astype(LD), t.astype(LD))
    with np.errstate(all="ignore"):
        q2 = np.abs(LD(K[2, 2]) * z)
        mag = ((aK[0, 0] * A[0] + aK[0, 1] * A[1] + aK[0, 2] * A[2]) + (aK[1, 1] * A[1] + aK[1, 2] * A[2])) / q2
        p = (e + np.abs(x[None, :, 0]) + np.abs(x[None, :, 1])).astype(LD)   # |p| <= e + |x|
        be = 64 * eps * (mag + p * (1 + A[2] / np.abs(z))) + LD(BAND)
        bz = 8 * eps * A[2]
    return e, z, be, bz


def decided_mask(X, x, K, hyp, thr, what):
    """[S, n] bool: depth > 0 and error < thr under each read-back hypothesis — in longdouble,
    and by the float64 repetition of the device's operations for the entries within the
    rounding band of the threshold or of depth 0.  NaN hypotheses hold nothing."""
    R, t = split(hyp)
    e, z, be, bz = rounding_bands(X, x, K, R, t)
    e64, z64 = PR.errors(X, x, K, R, t)
    with np.errstate(invalid="ignore"):
        wide = (z > 0) & (e < LD(thr))
        exact = (z64 > 0) & (e64 < thr)
        band = ((np.abs(e - LD(thr)) <= be) & (z > -bz)) | (np.abs(z) <= bz)
    print(f"MEASURED {what} thr={thr}: {int(band.sum())} of {band.size} entries within the rounding band of the "
          f"threshold or of depth 0 ({int((band & (wide != exact)).sum())} of them decided otherwise by float64), "
          f"none left out")
    assert band.mean() <= 0.02, what   # (the longdouble evaluation decides all but a few)
    assert not (wide != exact)[~band].any(), what   # outside the band the two evaluations cannot differ
    return np.where(band, exact, wide)


def check_counts(X, x, K, hyp, counts, thr, what):
    nan = whole_nan(hyp, what)
    mask = decided_mask(X, x, K, hyp, thr, what)
    want = mask.sum(axis=1)
    print(f"MEASURED {what} thr={thr}: {int(nan.sum())} NaN hypotheses of {len(hyp)}, counts "
          f"{int(counts.min()) if len(counts) else 0}..{int(counts.max()) if len(counts) else 0}, differing "
          f"{int((counts != want).sum())}")
    assert counts.dtype == np.int32 and (counts[nan] == 0).all(), f"{what}: a NaN hypothesis has a count"
    bad = np.flatnonzero(counts != want)
    assert len(bad) == 0, f"{what}: samples {bad[:8]} count {counts[bad[:8]]}, their own hypotheses hold {want[bad[:8]]}"
    return mask


def check_selection(r, mask, n, what, refined=True):
    """k_pnp_select and the outputs against the read-back counts and hypotheses."""
    counts, hyp = r["rb_counts"], r["hyp"]
    if len(counts) == 0 or counts.max() <= 0:
        assert r["it"] == -1 and r["on"] == (-1 if n < 6 else 0), what
        assert np.isnan(r["start"]).all() and r["status"].tolist() == [0, -1, 0, 0], what
        assert np.isnan(r["R"]).all() and np.isnan(r["t"]).all() and np.isnan(r["cost"]).all(), what
        return
    best = int(np.argmax(counts))   # numpy's argmax is the first maximum
    assert r["it"] == best and r["on"] == int(counts[best]), what
    assert np.array_equal(r["inliers"][:r["on"]], np.flatnonzero(mask[best]).astype(np.int32)), what
    assert r["start"].tobytes() == hyp[best].tobytes(), what
    if not refined:
        return
    assert r["status"][0] == 1 and r["status"][1] in (0, 1, 3) and np.isfinite(r["R"]).all() and np.isfinite(r["t"]).all()
    assert np.isfinite(r["cost"]).all() and r["cost"][1] <= r["cost"][0], what


# ------------------------------------------------------------------ a. (R, t) per sample
@pytest.mark.parametrize("name", FIT_CASES)
def test_pose_of_every_admitted_sample_vs_the_60_digit_reference(name):
    """Measured on the MI355X: see the table of DESIGN.md §13D."""
    z = fits()
    X, x, K, iters = case(name)
    r = device(name)
    R, t = split(r["hyp"])
    a = z[f"{name}_admitted"]
    bR, bt = float(z["bound_R"]), float(z["bound_t"])
    assert np.isfinite(r["hyp"][a]).all(), f"{name}: an admitted sample has no hypothesis"
    dR, dt = PR.pose_deviation(R[a], t[a], z[f"{name}_R"][a], z[f"{name}_t"][a])
    print(f"MEASURED {name}: max |dR| {dR.max():.3e} (bound {bR:.1e}) |dt| / max(1, |t|) {dt.max():.3e} (bound {bt:.1e}) "
          f"over {int(a.sum())} admitted samples of {iters}")
    assert dR.max() <= bR and dt.max() <= bt
    # every finite R is a rotation, to 100 x what the restatement's own R is at the same samples
    nan = whole_nan(r["hyp"], name)
    Rr, _ = PR.hypotheses(X, x, K, PR.samples(len(X), iters))
    both = ~nan & np.isfinite(Rr).all(axis=(1, 2))
    d_dev, d_rest = PR.rotation_defect(R[~nan]), PR.rotation_defect(Rr[both])
    print(f"MEASURED {name}: max |R R^T - I| {d_dev.max():.3e} over {int((~nan).sum())} finite samples "
          f"(restatement {d_rest.max():.3e}, bound 100 x)")
    assert d_dev.max() <= 100 * d_rest.max() and (np.linalg.det(R[~nan]) > 0).all()
    if name != "dup":   # (dup's NaN samples are test d's)
        assert np.array_equal(nan, np.isnan(Rr[:, 0, 0])), name


# ------------------------------------------------------------------ b. counts against the device's own hypotheses
@pytest.mark.parametrize("name", FIT_CASES)
def test_counts_and_selection_vs_own_hypotheses_on_every_case(name):
    X, x, K, iters = case(name)
    r = device(name)
    mask = check_counts(X, x, K, r["hyp"], r["rb_counts"], PR.THRESHOLD, name)
    check_selection(r, mask, len(X), name)


@pytest.mark.parametrize("thr", [0.5, 2.0])
@pytest.mark.parametrize("name", ["n63", "n64", "n65", "n130", "n2600", "skew", "slab1", "dup"])
def test_counts_and_selection_at_thresholds_inside_the_pixel_noise(name, thr):
    """Pixels are rounded and carry sigma = 0.6 noise: at 0.5 and 2 px many planted points sit
    near the threshold.  The hypotheses do not depend on the threshold."""
    X, x, K, iters = case(name)
    r = run(X, x, K, iters, thr)
    assert r["hyp"].tobytes() == device(name)["hyp"].tobytes()
    mask = check_counts(X, x, K, r["hyp"], r["rb_counts"], thr, name)
    check_selection(r, mask, len(X), f"{name} thr={thr}")


@pytest.mark.parametrize("n", [2559, 2560, 2561])
def test_counts_around_the_lds_chunk(n):
    """kRansacChunk = 2560 points are staged at a time: one below, the chunk, one above."""
    X, x, _, _, _ = PR.scene(200 + n % 7, n, 0.2)
    for thr in (PR.THRESHOLD, 0.5, 2.0):
        r = run(X, x, PR.K_SCENE, 24, thr)
        mask = check_counts(X, x, PR.K_SCENE, r["hyp"], r["rb_counts"], thr, f"n={n}")
        check_selection(r, mask, n, f"n={n} thr={thr}")
        if thr == PR.THRESHOLD:
            assert r["on"] > 0.5 * n   # 80 % are planted


@pytest.mark.parametrize("iters", [7, 8, 9, 63, 64, 65, 129])
def test_counts_around_the_workgroup_sizes(iters):
    """kPnpWaves = 8 samples per k_pnp_count workgroup, 64 per k_pnp_hyp workgroup: one below,
    the size, one above, and one above two k_pnp_hyp workgroups."""
    X, x, K, _ = case("n130")
    for thr in (PR.THRESHOLD, 0.5, 2.0):
        r = run(X, x, K, iters, thr)
        mask = check_counts(X, x, K, r["hyp"], r["rb_counts"], thr, f"n130 iters={iters}")
        check_selection(r, mask, len(X), f"n130 iters={iters} thr={thr}")
        key = f"n130/129/{thr}"
        if key not in _RUNS:
            _RUNS[key] = run(X, x, K, 129, thr)
        full = _RUNS[key]
        assert r["hyp"].tobytes() == full["hyp"][:iters].tobytes()   # the same stream's prefix
        assert np.array_equal(r["rb_counts"], full["rb_counts"][:iters])


@pytest.mark.parametrize("name", ["n65", "n130"])
def test_threshold_equal_to_one_points_error(name):
    """thr = the float64 error of an inlier of the winner under the winner's own hypothesis, as
    the device's operations give it (tests/pnp_ref.py errors repeats them): error < thr is false
    for that entry and true for every smaller error, which only the strict comparison gets
    right.  The longdouble evaluation cannot decide the entry; the band hands it to float64."""
    X, x, K, iters = case(name)
    r0 = device(name)
    s = r0["it"]
    R, t = split(r0["hyp"])
    e64, z64 = PR.errors(X, x, K, R, t)
    inl = r0["inliers"][:r0["on"]]
    j = int(inl[np.argsort(e64[s, inl])[len(inl) // 2]])   # the median inlier of the winner
    thr = float(e64[s, j])
    r = run(X, x, K, iters, thr)
    assert r["hyp"].tobytes() == r0["hyp"].tobytes()
    mask = check_counts(X, x, K, r["hyp"], r["rb_counts"], thr, f"{name} thr=e[{s},{j}]")
    check_selection(r, mask, len(X), f"{name} thr=e[{s},{j}]")
    below = int((e64[s, inl] < thr).sum())
    print(f"MEASURED {name}: thr = e[{s}, {j}] = {thr!r}: sample {s} counts {int(r['rb_counts'][s])}, "
          f"{below} of its former {len(inl)} inliers lie strictly below")
    assert e64[s, j] == thr and not mask[s, j] and r["rb_counts"][s] == below
    if r["it"] == s:
        assert j not in r["inliers"][:r["on"]].tolist()


# ------------------------------------------------------------------ c. selection with a tie
def test_first_of_several_equal_maxima_wins():
    X, x, K, iters = case("dup")
    r = device("dup")
    counts = r["rb_counts"]
    top = np.flatnonzero(counts == counts.max())
    print(f"MEASURED dup: samples {top} share the largest count {int(counts.max())} of {len(X)}; winner {r['it']}")
    assert len(top) >= 2 and counts.max() == len(X) and r["it"] == top[0]
    assert np.array_equal(r["inliers"][:r["on"]], np.arange(len(X)))


# ------------------------------------------------------------------ d. degenerate samples
@pytest.mark.parametrize("name", ["plane", "ident"])
def test_exactly_degenerate_scenes_give_no_pose(name):
    """plane: the centred z of every sample are exactly 0 and with them three columns of its
    system; ident: the mean distance to the centroid is 0.  Not a rounding question."""
    X, x, K, iters = case(name)
    r = device(name)
    print(f"MEASURED {name}: {int(np.isnan(r['hyp']).all(axis=1).sum())} of {iters} hypotheses NaN, on {r['on']}, "
          f"status {r['status'].tolist()}")
    assert np.isnan(r["hyp"]).all() and (r["rb_counts"] == 0).all()
    assert r["on"] == 0 and r["it"] == -1 and r["status"].tolist() == [0, -1, 0, 0]
    assert np.isnan(r["R"]).all() and np.isnan(r["t"]).all() and np.isnan(r["cost"]).all() and np.isnan(r["start"]).all()
    pe = pose.PnPRansac(X, x, K=K, ransac_max_it=iters)
    assert pe.R is None and pe.t is None and pe.inliers is None


def test_duplicated_correspondences():
    """A sample that drew both copies of a correspondence has two identical pairs of rows, which
    cancel exactly: its NaN is the restatement's NaN.  The others find the pose."""
    z = fits()
    X, x, K, iters = case("dup")
    r = device("dup")
    idx = PR.samples(len(X), iters)
    Rr, tr = PR.hypotheses(X, x, K, idx)
    nan = whole_nan(r["hyp"], "dup")
    print(f"MEASURED dup: {int(nan.sum())} NaN hypotheses of {iters} (restatement {int(np.isnan(Rr[:, 0, 0]).sum())}), "
          f"winner {r['it']} with {r['on']} of {len(X)}")
    assert np.array_equal(nan, np.isnan(Rr[:, 0, 0]))
    assert np.array_equal(nan, np.array([len(set(row // 2)) < 6 for row in idx]))
    assert r["on"] == len(X) and r["status"][0] == 1
    # where the reference admits the sample and no error of the restatement is within 1e-6 px
    # of the threshold, the restatement's count is the device's
    e, depth = PR.errors(X, x, K, Rr, tr)
    with np.errstate(invalid="ignore"):
        clear = z["dup_admitted"] & (np.abs(e - PR.THRESHOLD) > 1e-6).all(axis=1) & (np.abs(depth) > 1e-6).all(axis=1)
    want = PR.inlier_mask(X, x, K, Rr, tr).sum(axis=1)
    print(f"MEASURED dup: {int(clear.sum())} samples with an admitted table; counts differing there "
          f"{int((want != r['rb_counts'])[clear].sum())}")
    assert clear.sum() >= 30 and np.array_equal(want[clear], r["rb_counts"][clear])


def test_lattice_takes_the_first_row_of_the_largest_magnitude():
    """On the integer lattice many pivot columns hold two rows of equal magnitude, and some samples'
    systems have a null space of two dimensions, of which the elimination's rounding picks the
    member.  The rule takes the first of the equal rows; taking the last gives another member in
    sample 10 (1.9 apart in R, cond M 61 either way) and other bits in 26 samples
    (tests/test_pnp_fits_cpu.py).  The restatement repeats the device's elimination operation for
    operation, so: a zero pivot there is a NaN here; a projection matrix with cond M <= 1e3 there
    is a finite pose here (beyond that the polar factor's own rounding decides, as the rule
    allows); and where the two choices part by more than 1e-9 the device stands by the first."""
    X, x, K, iters = case("lattice")
    r = device("lattice")
    idx = PR.samples(len(X), iters)
    Rf, tf = PR.hypotheses(X, x, K, idx)
    Rl, tl = PR.hypotheses(X, x, K, idx, route="elim_last")
    cm = PR.elimination_cond_m(X, x, K, idx)
    nan = whole_nan(r["hyp"], "lattice")
    flat = lambda R, t: np.concatenate([R.reshape(len(R), -1), t], axis=1)
    with np.errstate(invalid="ignore"):
        apart = np.abs(flat(Rf, tf) - flat(Rl, tl)).max(axis=1)
        to_first = np.abs(r["hyp"] - flat(Rf, tf)).max(axis=1)
        to_last = np.abs(r["hyp"] - flat(Rl, tl)).max(axis=1)
        far = (apart > 1e-9) & (cm <= PR.CONDM_MAX)
    print(f"MEASURED lattice: NaN samples {np.flatnonzero(nan)} (restatement: zero pivot {np.flatnonzero(np.isinf(cm))}, "
          f"cond M > 1e3 {np.flatnonzero(np.isfinite(cm) & (cm > PR.CONDM_MAX))}), winner {r['it']} with {r['on']} of {len(X)}")
    print(f"MEASURED lattice: samples {np.flatnonzero(far)} part by {apart[far].tolist()} between the two choices: "
          f"device to the first {to_first[far].tolist()}, to the last {to_last[far].tolist()}; largest distance to "
          f"the first over cond M <= 1e3: {np.nanmax(to_first[cm <= PR.CONDM_MAX]):.3e}")
    assert nan[np.isinf(cm)].all() and not nan[cm <= PR.CONDM_MAX].any()
    assert far.any() and (to_first[far] < 1e-3 * to_last[far]).all()
    mask = check_counts(X, x, K, r["hyp"], r["rb_counts"], PR.THRESHOLD, "lattice")
    check_selection(r, mask, len(X), "lattice")
    assert r["on"] == len(X)


@pytest.mark.parametrize("name", ["tilted", "slab3", "collinear"])
def test_nearly_degenerate_scenes_are_consistent(name):
    """Nothing is exactly 0 here, so which samples are NaN is a rounding question and no
    hypothesis is worth anything; what holds: a hypothesis is NaN or finite as a whole, the
    counts are those of the sample's own hypothesis, the selection follows the counts and the
    outputs follow the selection."""
    X, x, K, iters = case(name)
    r = device(name)
    mask = check_counts(X, x, K, r["hyp"], r["rb_counts"], PR.THRESHOLD, name)
    check_selection(r, mask, len(X), name)
    print(f"MEASURED {name}: {int(np.isnan(r['hyp']).all(axis=1).sum())} NaN hypotheses of {iters}, largest count "
          f"{int(r['rb_counts'].max())} of {len(X)}, on {r['on']}, status {r['status'].tolist()}")
    pe = pose.PnPRansac(X, x, K=K, ransac_max_it=iters)
    assert (pe.R is None) == (r["on"] <= 0)
    if pe.R is not None:
        assert pe.R.tobytes() == r["R"].tobytes() and np.array_equal(pe.inliers[:, 0], r["inliers"][:r["on"]])


# ------------------------------------------------------------------ e. the all-points DLT
@pytest.mark.parametrize("name", DLT_CASES)
def test_dlt_pose_vs_the_60_digit_reference(name):
    z = fits()
    X, x, K, _ = case(name)
    gap = float(z[f"{name}_dlt_gap"])
    assert gap >= PR.DLT_GAP_MIN   # admitted by the reference (asserted for every case on the CPU)
    r = run_pnp(X, x, K)
    assert np.isfinite(r["start"]).all() and r["status"][0] == 1
    R, t = split(r["start"][None])
    dR, dt = PR.pose_deviation(R, t, z[f"{name}_dlt_R"][None], z[f"{name}_dlt_t"][None])
    bR, bt = float(z["bound_dlt_R"]), float(z["bound_dlt_t"])
    defect = PR.rotation_defect(R)[0]
    print(f"MEASURED dlt {name}: n {len(X)} sigma11/sigma12 {gap:.1f} max |dR| {dR[0]:.3e} (bound {bR:.1e}) "
          f"|dt| / max(1, |t|) {dt[0]:.3e} (bound {bt:.1e}) |R R^T - I| {defect:.3e}")
    assert dR[0] <= bR and dt[0] <= bt
    Rr, _ = PR.dlt_all(X, x, K)
    assert defect <= 100 * max(PR.rotation_defect(Rr[None])[0], np.finfo(np.float64).eps) and np.linalg.det(R[0]) > 0
    # the refinement started there: its start cost is the cost at the read-back pose
    c0 = PR.residuals(X, x, K, R[0], t[0])[2]
    assert abs(r["cost"][0] - c0) <= COST_TOL * c0


# ------------------------------------------------------------------ f. refinement statuses
@pytest.mark.parametrize("limit", [1, 2])
@pytest.mark.parametrize("name", ["n65", "lm256"])
def test_iteration_limit_gives_status_3(name, limit):
    X, x, K, iters = case(name)
    r = run(X, x, K, iters, mi=limit)
    assert r["hyp"].tobytes() == device(name)["hyp"].tobytes() and r["it"] == device(name)["it"]
    inl = r["inliers"][:r["on"]]
    ref = PR.refine(X[inl], x[inl], K, r["start"][:9].reshape(3, 3), r["start"][9:], max_iter=limit)
    e0, e1 = abs(r["cost"][0] - ref["cost0"]) / ref["cost0"], abs(r["cost"][1] - ref["cost"]) / ref["cost"]
    print(f"MEASURED {name} limit {limit}: status {r['status'].tolist()} (restatement status {ref['status']} accepted "
          f"{ref['iters']}, all firm {ref['all_firm']}), cost {e1:.3e} start cost {e0:.3e} (bound {COST_TOL:.3e})")
    assert ref["status"] == PR.ST_MAXITER and ref["all_firm"]
    assert r["status"].tolist() == [1, PR.ST_MAXITER, ref["iters"], limit]
    assert e0 <= COST_TOL and e1 <= COST_TOL
    # the same limit through sfm_pnp_dev, from the DLT's pose over all points
    q = run_pnp(X[inl], x[inl], K, mi=limit)
    qref = PR.refine(X[inl], x[inl], K, q["start"][:9].reshape(3, 3), q["start"][9:], max_iter=limit)
    eq = abs(q["cost"][1] - qref["cost"]) / qref["cost"]
    print(f"MEASURED {name} limit {limit} (PnP): status {q['status'].tolist()} (restatement {qref['status']} accepted "
          f"{qref['iters']}, all firm {qref['all_firm']}), cost {eq:.3e}")
    assert qref["status"] == PR.ST_MAXITER
    assert q["status"][0] == 1 and q["status"][1] == PR.ST_MAXITER and q["status"][3] == limit
    if qref["all_firm"]:
        assert q["status"][2] == qref["iters"] and eq <= COST_TOL


def test_non_finite_start_cost_is_status_2():
    """Status 2 through the public call: two pixels of 1.2e154 (their squares are finite, the sum
    of the two is not) and a threshold of 1e200, under which every point in front of the camera
    is an inlier.  The samples without those two points give the planted pose, the first of them
    wins with all 65 points, and the cost over its inliers is inf: the start pose comes back
    unrefined with status 2, no iteration run."""
    X, x, K, iters = case("n65")
    x = x.copy()
    x[[3, 40], 0] = 1.2e154
    thr = 1e200
    r = run(X, x, K, iters, thr)
    with np.errstate(all="ignore"):
        ref = PR.pnp_ransac(X, x, K, iters, threshold=thr)
    print(f"MEASURED status 2: winner {r['it']} (restatement {ref['iteration']}) with {r['on']} of {len(X)}, status "
          f"{r['status'].tolist()} (restatement {ref['status']}), cost {r['cost'].tolist()}")
    assert ref["status"] == PR.ST_NONFINITE and np.isfinite(ref["R0"]).all()   # the rule reaches it on this input
    mask = check_counts(X, x, K, r["hyp"], r["rb_counts"], thr, "status 2")
    check_selection(r, mask, len(X), "status 2", refined=False)
    assert r["on"] == len(X) and np.isfinite(r["start"]).all()
    assert r["status"].tolist() == [1, PR.ST_NONFINITE, 0, 0]
    assert np.isinf(r["cost"][0]) and r["cost"][0] > 0 and r["cost"][1].tobytes() == r["cost"][0].tobytes()
    assert r["R"].tobytes() == r["start"][:9].tobytes() and r["t"].tobytes() == r["start"][9:].tobytes()
    # the samples without the two pixels are n65's own: their counts are the restatement's (no error
    # is near 1e200); what a sample with a pixel of 1e154 gives is worth nothing on either side
    sane = ~np.isin(PR.samples(len(X), iters), [3, 40]).any(axis=1)
    assert r["hyp"][sane].tobytes() == device("n65")["hyp"][sane].tobytes()
    assert np.array_equal(r["rb_counts"][sane], ref["counts"][sane]) and r["it"] == ref["iteration"]


@pytest.mark.parametrize("which,value", [("all", 1e153), ("one", 2e154), ("one", 5e154)])
def test_huge_pixels_end_in_status_2_or_no_pose(which, value):
    """sfm_pnp_dev on finite float64 pixels whose squares are finite and whose sum of squared
    residuals is not: every u scaled to about 1e153, or one u set to 2e154 or 5e154.  Whatever
    the DLT makes of them, the rule allows two ends: a finite start pose with a non-finite start
    cost is status 2 with the start pose returned unrefined; a NaN start pose is "no pose".
    Measured on the MI355X: "no pose" all three times (the DLT's M is singular to rounding when a
    pixel is that large), so sfm_pnp_dev's status 2 has no finite input here; the RANSAC call's
    has (test_non_finite_start_cost_is_status_2)."""
    X, x, K, _ = case("n12")
    xs = x.copy()
    if which == "all":
        xs[:, 0] *= value / 500.0
    else:
        xs[0, 0] = value
    scale = f"{which} {value:.0e}"
    assert np.isfinite(xs).all()
    r = run_pnp(X, xs, K)
    print(f"MEASURED huge pixels {scale}: start pose finite {bool(np.isfinite(r['start']).all())}, status "
          f"{r['status'].tolist()}, cost {r['cost'].tolist()}")
    whole_nan(r["start"][None], "huge pixels")
    if np.isfinite(r["start"]).all() and not np.isfinite(r["cost"][0]):
        assert r["status"].tolist() == [1, PR.ST_NONFINITE, 0, 0]
        assert r["R"].tobytes() == r["start"][:9].tobytes() and r["t"].tobytes() == r["start"][9:].tobytes()
    elif np.isfinite(r["start"]).all():
        assert r["status"][0] == 1 and r["status"][1] in (0, 1, 3) and np.isfinite(r["cost"]).all()
    else:
        assert r["status"].tolist() == [0, -1, 0, 0] and np.isnan(r["R"]).all() and np.isnan(r["cost"]).all()


# ------------------------------------------------------------------ the read-back itself
def test_read_back_follows_the_last_call():
    X, x, K, iters = case("n12")
    c = _native.Context(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), 0)
    try:
        with pytest.raises(Exception, match="sfm_debug_pnp_fits"):
            c.pnp_fits(0)            # no PnP call yet
        import torch
        dev = torch.device("cuda", 0)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
        o = pose._pnp_ransac_dev(t(X), t(x), t(K).reshape(-1), 12, 8.0, 50, dev, ctx=c)
        hyp, counts, start = c.pnp_fits(12)
        assert np.array_equal(counts, o["counts"][:12].cpu().numpy()) and np.isfinite(start).all()
        for bad in (11, 13, 0):
            with pytest.raises(Exception, match="sfm_debug_pnp_fits"):
                c.pnp_fits(bad)
        L, h = c.lib, c.handle
        E = _abi.SFM_EINVAL
        buf = np.zeros(12 * 12)
        i32 = np.zeros(12, np.int32)
        assert L.sfm_debug_pnp_fits(h, None, i32.ctypes.data, buf.ctypes.data, 12) == E
        assert L.sfm_debug_pnp_fits(h, buf.ctypes.data, None, buf.ctypes.data, 12) == E
        assert L.sfm_debug_pnp_fits(h, buf.ctypes.data, i32.ctypes.data, None, 12) == E
        assert L.sfm_debug_pnp_fits(h, buf.ctypes.data, i32.ctypes.data, buf.ctypes.data, -1) == E
        assert L.sfm_debug_pnp_fits(None, buf.ctypes.data, i32.ctypes.data, buf.ctypes.data, 12) == E
        assert b"sfm_debug_pnp_fits" in L.sfm_last_error(h)
        # without the caller's table the workspace's own is the one the kernels wrote
        f64 = lambda k: torch.empty(k, dtype=torch.float64, device=dev)
        i32d = lambda k: torch.empty(k, dtype=torch.int32, device=dev)
        dX, dx, dK = t(X), t(x), t(K).reshape(-1)
        R, tt, cost, inl, on, oit, st = f64(9), f64(3), f64(2), i32d(len(X)), i32d(1), i32d(1), i32d(4)
        torch.cuda.synchronize()
        _native.check(L.sfm_pnp_ransac_dev(h, dX.data_ptr(), dx.data_ptr(), dK.data_ptr(), len(X), 12, 8.0, 50,
                                           R.data_ptr(), tt.data_ptr(), inl.data_ptr(), on.data_ptr(), oit.data_ptr(),
                                           st.data_ptr(), cost.data_ptr(), None, None), h)
        hyp2, counts2, start2 = c.pnp_fits(12)
        assert hyp2.tobytes() == hyp.tobytes() and np.array_equal(counts2, counts) and start2.tobytes() == start.tobytes()
        # fewer than 6 points, or no iterations: no sample ran, only start_Rt (NaN) is defined
        pose._pnp_ransac_dev(t(X[:5]), t(x[:5]), t(K).reshape(-1), 12, 8.0, 50, dev, ctx=c)
        assert np.isnan(c.pnp_fits(0)[2]).all()
        with pytest.raises(Exception):
            c.pnp_fits(12)
        pose._pnp_ransac_dev(t(X), t(x), t(K).reshape(-1), 0, 8.0, 50, dev, ctx=c)
        assert np.isnan(c.pnp_fits(0)[2]).all()
        # after sfm_pnp_dev: the DLT's pose, no samples
        _native.check(L.sfm_pnp_dev(h, dX.data_ptr(), dx.data_ptr(), dK.data_ptr(), len(X), 50, R.data_ptr(),
                                    tt.data_ptr(), st.data_ptr(), cost.data_ptr(), None), h)
        s3 = c.pnp_fits(0)[2]
        assert np.isfinite(s3).all() and s3.tobytes() != start.tobytes()
        with pytest.raises(Exception):
            c.pnp_fits(12)
    finally:
        c.close()
