"""CPU: the conditions the GPU tests of sfm_homography_matches_dev and sfm_two_view_pose_dev
(tests/test_gpu_two_view.py) rest on — the four-index sampler of the restatement
(tests/two_view_ref.py), pose.ransac_stop_ratios at sample size 4, how far every decision of every
case compared on the GPU sits from equality, which cases stop early, the class of every scene kind
on the restatement alone, and the calls' argument errors.

Bounds (each set like ransac_ref.D_BOUND: min(1e-6, 100 x the largest difference measured between
two float64 routes of the same quantity), figures printed before their assertions):
* H inequality: fit_H against fit_H_solve (LAPACK's LU) moves lhs / rhs by at most 3.6e-8 over the
  entries within a factor 2 of equality (n2700_bad, backward test) -> H_GAP_BOUND = 1e-6; the
  closest case measured here is n2700_bad at 4.7e-6.
* depth: candidates moved by 3.3e-14 (the difference test_gpu_pose measured between the device's
  candidates and the reference's) move a depth by at most 9.5e-8 of itself (r255, whose points lie
  near infinity) -> DEPTH_GAP_BOUND = 1e-6; every depth measured here is farther than 0.99 of
  itself from 1e-6.  The depth's sign is the sign of the homogeneous coordinate v_w, so |v_w| / |v|
  must stay above W_BOUND = 1e-9: the perturbation above moves it by 3e-14, the smallest measured
  is 3.6e-7 (r255).
* parallax: the same perturbation moves d^2 / rhs by at most 4.4e-14 -> WIDE_GAP_BOUND = 4.4e-12;
  the closest case measured here is p40 with its own intrinsics at 1.1e-4."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native, pose
from tests import pose_ref as PR
from tests import two_view_ref as TV
from tests import verify_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H_ROUTES_MEASURED = 3.6e-8
H_GAP_BOUND = min(1e-6, 100 * H_ROUTES_MEASURED)
DEPTH_MOVED_MEASURED = 9.5e-8
DEPTH_GAP_BOUND = min(1e-6, 100 * DEPTH_MOVED_MEASURED)
W_BOUND = 1e-9
WIDE_MOVED_MEASURED = 4.4e-14
WIDE_GAP_BOUND = min(1e-6, 100 * WIDE_MOVED_MEASURED)
ORDER_BOUND = 1e-9   # the device-order construction against pose_ref.candidates(route="eig")


# ---------------------------------------------------------------- the sampler
def dense_sample(seed, a, b, it, n):
    """The rule on a real arange(n) in numpy uint64 arithmetic: shares no code with TV.sample."""
    u = np.uint64
    with np.errstate(over="ignore"):
        def mix(z):
            z = u(z)
            z ^= z >> u(30)
            z *= u(0xBF58476D1CE4E5B9)
            z ^= z >> u(27)
            z *= u(0x94D049BB133111EB)
            z ^= z >> u(31)
            return z
        key = mix(mix(u(seed & VR.M64) ^ u(0x486F6D6F67726170)) + u((a << 32) | b))
        arr = np.arange(n)
        for k in range(4):
            r = int(mix(key + u(4 * it + k + 1) * u(VR.G)) >> u(32))
            j = k + ((r * (n - k)) >> 32)
            arr[k], arr[j] = arr[j], arr[k]
    return arr[:4].tolist()


@pytest.mark.parametrize("n", [4, 5, 11, 2561])
def test_sample_indices_are_distinct_and_in_range(n):
    for a, b in ((0, 1), (2, 0), (255, 254)):
        s = TV.samples(TV.SEED, a, b, n, 300)
        assert s.shape == (300, 4) and s.min() >= 0 and s.max() < n
        assert all(len(set(row)) == 4 for row in s.tolist())
        if n == 4:
            assert (np.sort(s, axis=1) == np.arange(4)).all()   # a permutation
        for it in (0, 1, 255, 299):
            assert s[it].tolist() == dense_sample(TV.SEED, a, b, it, n)


def test_pinned_samples_and_the_stream_is_not_verifys():
    assert TV.sample(5, 0, 1, 0, 4) == [2, 3, 1, 0]
    assert TV.sample(5, 2, 0, 3, 40) == [17, 13, 22, 7]
    assert TV.sample(-7, 1, 2, 599, 40000) == [6971, 14974, 11161, 34511]
    for seed, a, b, n in ((5, 2, 0, 40), (5, 0, 1, 2561), (-7, 1, 2, 40000)):
        own = TV.samples(seed, a, b, n, 64)
        theirs = VR.samples(seed, a, b, n, 64)[:, :4]
        assert (own != theirs).any(axis=1).mean() > 0.9
        # nor verify's draws regrouped by four: the key differs, not only the counter
        assert VR.pair_key((seed & VR.M64) ^ TV.H_XOR, a, b) != VR.pair_key(seed, a, b)
    base = TV.sample(5, 3, 7, 11, 100)
    assert TV.sample(6, 3, 7, 11, 100) != base and TV.sample(5, 7, 3, 11, 100) != base
    assert TV.sample(5, 3, 7, 12, 100) != base


# ---------------------------------------------------------------- the stop table
def test_stop_ratios_at_eight_are_unchanged_and_at_four_meet_their_equation():
    for conf in (0.98, 0.5, 0.999999):
        r = np.arange(1, 65, dtype=np.float64)
        before = (-np.expm1(np.log1p(-np.float64(conf)) / (256.0 * r))) ** 0.125   # the expression as it stood
        assert pose.ransac_stop_ratios(conf, 64).tobytes() == before.tobytes()
        assert pose.ransac_stop_ratios(conf, 64, 8).tobytes() == before.tobytes()
        w = pose.ransac_stop_ratios(conf, 64, sample_size=4)
        got = 1.0 - (1.0 - w ** 4) ** (256 * r)
        print(f"confidence {conf}: worst |1 - (1 - w^4)^(256 r) - confidence| = {np.abs(got - conf).max():.3e}")
        assert np.abs(got - conf).max() < 1e-12
        assert (np.diff(w) < 0).all() and (w > 0).all() and (w < 1).all()
    with pytest.raises(ValueError):
        pose.ransac_stop_ratios(0.98, 3, 0)
    assert pose.calculate_num_ransac_iterations(0.98, 4, 0.4) == 150


# ---------------------------------------------------------------- the homography cases
def test_fit_maps_its_own_sample_and_both_routes_agree():
    p1, p2 = TV.scene("planar", 83, 40, 0.0)
    worst, used = 0.0, 0
    for it in range(20):
        s = TV.sample(5, 2, 0, it, 40)
        H, piv = TV.fit_H(p1[s], p2[s])
        assert piv == list(range(8))
        if np.linalg.cond(H) > 1e8:   # three of the four points on a line (sample 15): H is singular
            continue
        used += 1
        res = TV.transfer_residuals(H, p1[s].astype(float), p2[s].astype(float))
        assert res.max() < 1e-6     # four points determine H: the sample is mapped exactly
        H2 = TV.fit_H_solve(p1[s], p2[s])
        worst = max(worst, np.abs(H / H[2, 2] - H2 / H2[2, 2]).max())
    print(f"fit_H against fit_H_solve over {used} samples: {worst:.3e}")
    assert worst < 1e-6 and used >= 15


@pytest.mark.parametrize("name", list(TV.SINGLE))
def test_every_homography_case_keeps_its_distance_from_equality(name):
    """Over all 600 samples (a superset of what any iteration count or stop table evaluates)."""
    tab = TV.single(name)
    r = TV.homography(tab, stop=None)
    n = int(tab["nmatch"][0])
    print(f"{name}: n {n}, hstat {r['hstat'][0].tolist()}, closest relative gap {r['gap'][0]:.3e}")
    if n < 4:
        assert r["hstat"][0].tolist() == [-1, -1, 0, 0] and not r["hkeep"].any() and np.isnan(r["H"]).all()
        return
    assert r["gap"][0] > H_GAP_BOUND
    assert r["hkeep"][0].sum() == r["hstat"][0, 0] and not r["hkeep"][0, n:].any()


def test_two_float64_routes_of_the_fit_move_a_decision_by_less_than_the_bound():
    worst = 0.0
    for name in ("n40", "n255", "n257"):
        tab = TV.single(name)
        _, n, valid, p1, p2 = TV.correspondences(tab, 0)
        idx, H, terms = TV.sample_table(tab, 0, TV.ITERS)
        H2 = np.full_like(H, np.nan)
        for it in np.flatnonzero(valid[idx].all(axis=1)):
            H2[it] = TV.fit_H_solve(p1[idx[it]], p2[idx[it]])
        other = (*TV.transfer_terms(H2, p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]),
                 *TV.transfer_terms(TV.adjugate(H2), p2[:, 0], p2[:, 1], p1[:, 0], p1[:, 1]))
        t2 = TV.thr2_of(TV.THRESHOLD)
        with np.errstate(all="ignore"):
            for k in (0, 2):
                qa, qb = terms[k] / (t2 * terms[k + 1]), other[k] / (t2 * other[k + 1])
                near = (qa > 0.5) & (qa < 2) & np.isfinite(qb)
                worst = max(worst, float(np.abs(qa / qb - 1)[near].max()))
    print(f"lhs / rhs between the two routes, entries within a factor 2 of equality: {worst:.3e}")
    assert worst <= H_ROUTES_MEASURED


def test_both_branches_of_the_stop_test_are_taken():
    stop = TV.stop_ratios()
    assert len(stop) == 3
    for name, samples in TV.STOPS_EARLY.items():
        s = TV.homography(TV.single(name), stop=stop)["hstat"][0]
        full = TV.homography(TV.single(name), stop=None)["hstat"][0]
        print(name, "with the 0.98 table", s.tolist(), "fixed", full.tolist())
        assert s[2] == samples and full[2] == TV.ITERS
    for name in TV.RUNS_ALL:
        s = TV.homography(TV.single(name), stop=stop)["hstat"][0]
        assert s[2] == TV.ITERS
    t = TV.single("n2700_bad")
    _, n, valid, _, _ = TV.correspondences(t, 0)
    _, H, _ = TV.sample_table(t, 0, VR.ROUND)
    dead = int(np.isnan(H[:, 0, 0]).sum())
    print(f"n2700_bad: n {n}, {int((~valid).sum())} invalid matches, {dead} of the first 256 samples contain one")
    assert n > 2560 and (~valid).sum() == TV.BAD_ROWS["n2700_bad"] and 0 < dead < VR.ROUND
    # a stop changes the winner where a later round holds a better sample
    assert any(TV.homography(TV.single(k), stop=stop)["hstat"][0, 0] < TV.homography(TV.single(k))["hstat"][0, 0]
               for k in TV.STOPS_EARLY)


@pytest.mark.parametrize("threshold", [0.0, -1.0, float("nan"), float("inf")])
def test_degenerate_thresholds(threshold):
    r = TV.homography(TV.single("n40"), iters=300, threshold=threshold)
    n = 40
    if threshold == float("inf"):
        assert r["hstat"][0].tolist()[:2] == [n, 0] and r["hkeep"][0, :n].all()
    else:
        assert r["hstat"][0].tolist() == [0, 0, 300, 0] and not r["hkeep"].any() and np.isnan(r["H"]).all()


def test_the_mixed_table_attempts_what_verify_attempts():
    t = TV.mixed()
    r = TV.homography(t, iters=VR.MIXED_ITERS, stop=TV.stop_ratios(iters=VR.MIXED_ITERS))
    print("hstat", r["hstat"].tolist(), "gaps", r["gap"].tolist())
    assert (r["hstat"][:, 0] >= 0).tolist() == [True, False, True, True, False, False, False, True, True]
    assert (r["gap"][r["hstat"][:, 0] >= 0] > H_GAP_BOUND).all()   # (pair 8 has 7 matches: enough for H)
    _, H, _ = TV.sample_table(t, 7, VR.MIXED_ITERS)
    assert np.isnan(H[:, 0, 0]).any() and np.isfinite(H[:, 0, 0]).any()


# ---------------------------------------------------------------- the pose cases and the classes
def pose_results(name, K2):
    tab, v = TV.pose_case(name, K2)
    K = np.stack([K2, PR.K_SCENE, PR.K_SCENE])   # slot 2 is the first camera, slot 0 the second
    att = v["stat"][:, 3]
    h = TV.homography(tab, iters=150, stop=TV.stop_ratios(iters=150), attempt=att)
    p = TV.two_view_pose(tab, v["keep"], v["F"], K, attempt=att)
    return tab, v, h, p


@pytest.mark.parametrize("own_intrinsics", [False, True])
@pytest.mark.parametrize("name", list(TV.POSE))
def test_every_pose_case_keeps_its_margins_and_its_class(name, own_intrinsics):
    kind, _, n, _ = TV.POSE[name]
    tab, v, h, p = pose_results(name, TV.K_OTHER if own_intrinsics else PR.K_SCENE)
    cfg = TV.classify(v["stat"], h["hstat"], p["pstat"])
    print(f"{name}: verify {v['stat'][0].tolist()} margin {v['margin'][0]:.3e}, hstat {h['hstat'][0].tolist()} "
          f"gap {h['gap'][0]:.3e}, pstat {p['pstat'][0].tolist()}, depth gap {p['depth_gap'][0]:.3e}, "
          f"|v_w|/|v| {p['w_gap'][0]:.3e}, parallax gap {p['wide_gap'][0]:.3e}, order {p['order_err'][0]:.1e}, "
          f"class {cfg.tolist()}")
    from tests import ransac_ref as RR
    assert v["margin"][0] > RR.D_BOUND
    assert cfg.tolist() == [TV.CLASS[kind]]
    if kind == "random":
        assert p["pstat"][0].tolist() == [-1, -1, 0, 0] and h["hstat"][0].tolist() == [-1, -1, 0, 0]
        return
    assert h["gap"][0] > H_GAP_BOUND
    assert p["depth_gap"][0] > DEPTH_GAP_BOUND and p["w_gap"][0] > W_BOUND
    assert p["wide_gap"][0] > WIDE_GAP_BOUND and p["order_err"][0] < ORDER_BOUND
    assert p["pstat"][0, 3] == v["stat"][0, 0] and p["pstat"][0, 0] > 0


def test_candidates_moved_in_their_last_bits_move_no_decision():
    rng = np.random.default_rng(1)
    dz = dq = 0.0
    for name in TV.POSE:
        if TV.POSE[name][0] == "random":
            continue
        tab, v = TV.pose_case(name)
        a = TV.two_view_pose(tab, v["keep"], v["F"], PR.K_SCENE)
        b = TV.two_view_pose(tab, v["keep"], v["F"], PR.K_SCENE, perturb=(rng, 3.3e-14))
        assert np.array_equal(a["pstat"], b["pstat"])
        dz = max(dz, float(np.abs(b["z"][0] / a["z"][0] - 1).max()))
        dq = max(dq, float(np.abs(b["q"][0] / a["q"][0] - 1).max()))
    print(f"candidates moved by 3.3e-14: depths move by {dz:.3e} of themselves, d^2 / rhs by {dq:.3e}")
    assert dz <= DEPTH_MOVED_MEASURED and dq <= WIDE_MOVED_MEASURED


def test_planted_motion_is_recovered_by_the_restatement():
    want_t = TV.T_TRUE / np.linalg.norm(TV.T_TRUE)
    for name in TV.PLANTED:
        tab, v = TV.pose_case(name)
        p = TV.two_view_pose(tab, v["keep"], v["F"], PR.K_SCENE)
        eR = np.abs(p["pose"][0, :9].reshape(3, 3) - TV.R_TRUE).max()
        et = np.abs(p["pose"][0, 9:] - want_t).max()
        print(f"{name}: restatement against the planted motion |dR| {eR:.3e} |dt| {et:.3e}")
        assert eR < 0.05 and et < 0.2   # integer pixels: the GPU test's bound is twice these figures


def test_pipeline_table_classes_and_initial_pair():
    t = TV.pipeline_table()
    v = VR.verify(t, iters=TV.VERIFY_ITERS, stop=VR.stop_ratios(iters=TV.VERIFY_ITERS))
    h = TV.homography(t, iters=150, stop=TV.stop_ratios(iters=150), attempt=v["stat"][:, 3])
    p = TV.two_view_pose(t, v["keep"], v["F"], PR.K_SCENE, attempt=v["stat"][:, 3])
    cfg = TV.classify(v["stat"], h["hstat"], p["pstat"])
    print("verify", v["stat"].tolist(), "hstat", h["hstat"].tolist(), "pstat", p["pstat"].tolist(), "class", cfg.tolist())
    print("gaps", v["margin"].tolist(), h["gap"].tolist(), p["depth_gap"].tolist(), p["w_gap"].tolist(),
          p["wide_gap"].tolist())
    from tests import ransac_ref as RR
    assert cfg.tolist() == [1, 2, 2, 0, 1, 0]
    att = v["stat"][:, 3] != 0
    assert (v["margin"][v["stat"][:, 0] >= 0] > RR.D_BOUND).all() and (h["gap"][att] > H_GAP_BOUND).all()
    assert (p["depth_gap"][att] > DEPTH_GAP_BOUND).all() and (p["w_gap"][att] > W_BOUND).all()
    assert (p["wide_gap"][att] > WIDE_GAP_BOUND).all()
    assert p["pstat"][0, 2] > p["pstat"][4, 2] > 0   # pair 0 has the most wide points: the initial pair


# ---------------------------------------------------------------- the C ABI
C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}


def header_prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfmfeat.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sfmfeat.h"
    args = [ctypes.c_void_p if "*" in a else C_TYPES[a.replace("const ", "").split()[0]]
            for a in (a.strip() for a in m.group(2).split(","))]
    return C_TYPES[m.group(1)], args


@pytest.mark.parametrize("name", ["sfm_homography_matches_dev", "sfm_two_view_pose_dev"])
def test_abi_declares_the_calls_and_rejects_bad_arguments_before_any_device_call(name):
    res, args = header_prototype(name)
    assert _native.SIGNATURES[name] == (res, args)
    lib = _native.load_library()
    fn = getattr(lib, name)
    assert fn(*[None if a is ctypes.c_void_p else 0 for a in args]) == _abi.SFM_EINVAL
    # without a context (none can be made without a device) every call returns SFM_EINVAL at once,
    # whatever else is passed; the per-argument errors are tests/test_gpu_two_view.py's
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    good = [None] + [p if a is ctypes.c_void_p else 1 for a in args[1:-1]] + [None]
    assert fn(*good) == _abi.SFM_EINVAL


def test_docs_name_the_step_and_13h_no_longer_leaves_it_out():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    h = design[design.index("13H"):]
    line = next(l for l in h.splitlines() if l.lstrip("*- ").lower().startswith("out of scope"))
    assert "homography" not in line.lower() and "degeneracy" not in line.lower(), line
    assert "13I" in design
    for rel in ("README.md", "INTEGRATION.md", "include/sfmfeat.h", "sfmfromscratch_amd/sequence.py", "DESIGN.md"):
        assert "two_view" in open(os.path.join(ROOT, rel)).read(), rel
