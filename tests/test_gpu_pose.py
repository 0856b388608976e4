"""GPU: the initial pair's pose RANSAC and the triangulation (pose.hip; pose.ransac_camera_motion,
triangulate, triangulate_points) against the reference's own outputs and the restatement's
per-iteration table (tests/golden/pose.npz, tests/pose_ref.py).  Every case meets the
admission condition asserted in tests/test_pose_cpu.py, so the winning iteration and the
inlier arrays are compared exactly.

Tolerances.  R, t: max absolute difference to the reference's values; X: ||dX|| / ||X|| on
the points whose 4 x 4 system has sigma3 / sigma4 >= 10 by the restatement (at most 2 % are
left out, asserted on the CPU; none is in this fixture).  Each bound is 100 x the largest value
measured on the MI355X over the fixture cases, capped at 1e-8 (R, t) and 1e-6 (X):
measured 3.3e-14 for R, t (largest: t of the n = 24 golden case, 3.202e-14) and 8.5e-14 for X
(largest: the non-identity-base winner's inliers, 8.456e-14; the 1000-point set 7.1e-14), so
the bounds are 3.3e-12 and 8.5e-12.  Every figure is printed before its assertion."""
from __future__ import annotations

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native, pose
from tests import pose_ref as PR
from tests.golden_util import load

pytestmark = pytest.mark.gpu

RT_TOL = min(1e-8, 100 * 3.3e-14)
X_TOL = min(1e-6, 100 * 8.5e-14)

POSE_CASES = ["g0", "g1", "g2", "g3", "g4", "k1k2", "base"]
PLANTED = ["n8_i60", "n65_i60", "n130_i60", "n2600_i48", "n50_i1", "n50_i300"]


def case(z, name):
    g = lambda k: z[f"{name}_{k}"]
    return (g("p1"), g("p2"), g("K1"), g("K2"), g("Rb"), g("Tb"), float(g("thr")), int(g("iters")))


def run(z, name):
    """The single-pair host call, its per-iteration candidate table and its per-iteration counts."""
    p1, p2, K1, K2, Rb, Tb, thr, iters = case(z, name)
    ctx = _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))
    r = ctx.ransac_camera_motion(p1, p2, K1, K2, Rb, Tb, thr, iters)
    return r, ctx.pose_candidates(1, iters)[0], ctx.ransac_fits(1, iters)[1][0]


def check_pose(z, name):
    (R, t, in1, in2, it), cand, counts = run(z, name)
    assert it == int(z[f"{name}_win"])
    assert np.array_equal(in1, z[f"{name}_in1"]) and np.array_equal(in2, z[f"{name}_in2"])
    dR, dt = np.abs(R - z[f"{name}_R"]).max(), np.abs(t - z[f"{name}_t"]).max()
    print(f"MEASURED {name}: |dR| {dR:.3e} |dt| {dt:.3e}")
    assert dR <= RT_TOL and dt <= RT_TOL
    # per iteration: some candidate valid (iterations without an inlier are skipped: -1)
    want = z[f"{name}_valid"].any(axis=1) & (z[f"{name}_counts"] > 0)
    assert np.array_equal(cand >= 0, want)
    # every sample's inlier count, zeroed where no candidate passed the cheirality check
    assert np.array_equal(counts, np.where(z[f"{name}_valid"].any(axis=1), z[f"{name}_counts"], 0))
    # the public call: the same arrays with the input dtype
    p1, p2, K1, K2, Rb, Tb, thr, iters = case(z, name)
    r = pose.ransac_camera_motion(p1, p2, K1, K2, Rb, Tb, threshold=thr, max_iterations=iters)
    assert np.array_equal(r[0], R) and np.array_equal(r[1], t)
    assert np.array_equal(r[2], z[f"{name}_in1"]) and r[2].dtype == z[f"{name}_in1"].dtype
    assert np.array_equal(r[3], z[f"{name}_in2"]) and r[3].dtype == z[f"{name}_in2"].dtype


@pytest.mark.parametrize("name", POSE_CASES)
def test_golden_cases_vs_reference(name):
    check_pose(load("pose.npz"), name)


@pytest.mark.parametrize("name", PLANTED)
def test_planted_sizes_vs_reference_and_table(name):
    """n = 8, 65, 130 (around the 64-lane rounds) and 2600 (above the 2560-point LDS chunk);
    1 iteration and 300 (above one 256-sample workgroup of the count kernel)."""
    check_pose(load("pose.npz"), name)


def assert_no_pose(r):
    assert r[0] is None and r[1] is None and r[2].shape == (0,) and r[3].shape == (0,)


def test_conventions():
    z = load("pose.npz")
    a = case(z, "n7")
    assert pose.ransac_camera_motion(*a[:6], max_iterations=a[7]) == (None, None, None, None)
    for name in ("iters0", "random"):
        c = case(z, name)
        assert_no_pose(pose.ransac_camera_motion(*c[:6], threshold=c[6], max_iterations=c[7]))
    # after a call that found a pose (stale counters, candidates and winners on the device)
    g = case(z, "g1")
    assert pose.ransac_camera_motion(*g[:6], max_iterations=g[7])[0] is not None
    for name in ("iters0", "random"):
        c = case(z, name)
        assert_no_pose(pose.ransac_camera_motion(*c[:6], threshold=c[6], max_iterations=c[7]))
    assert_no_pose(pose.ransac_camera_motion(*g[:6], max_iterations=0))
    rb = pose.ransac_camera_motion_batch([g[:6], a[:6], case(z, "g0")[:6]], max_iterations=0)
    assert rb[1] == (None, None, None, None)
    assert_no_pose(rb[0])
    assert_no_pose(rb[2])


def test_float_coordinates_raise():
    z = load("pose.npz")
    p1, p2, K1, K2, Rb, Tb, _, _ = case(z, "g0")
    with pytest.raises(ValueError):
        pose.ransac_camera_motion(p1 + 0.5, p2, K1, K2, Rb, Tb, max_iterations=10)
    with pytest.raises(ValueError):
        pose.ransac_camera_motion_batch([(p1, p2 + 0.25, K1, K2, Rb, Tb)], max_iterations=10)


def test_batch_equals_single_calls():
    """Mixed n, one n < 8 entry, per-pair K and base; one iteration count for the batch."""
    z = load("pose.npz")
    names = ["g0", "k1k2", "n7", "g1", "base", "g2", "random", "g3"]
    cases = [case(z, n)[:6] for n in names]
    info = {}
    rb = pose.ransac_camera_motion_batch(cases, threshold=1.0, max_iterations=40, info=info)
    ctx = _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))
    for name, c, r, it, cand in zip(names, cases, rb, info["out_iter"], info["candidates"]):
        s = ctx.ransac_camera_motion(*c, 1.0, 40)
        if s is None:
            assert r == (None, None, None, None) and it == -1 and cand is None, name
            continue
        assert it == s[4], name
        assert np.array_equal(cand, ctx.pose_candidates(1, 40)[0]), name
        if s[0] is None:
            assert_no_pose(r)
            continue
        assert np.array_equal(r[0], s[0]) and np.array_equal(r[1], s[1]), name
        assert np.array_equal(r[2], s[2]) and np.array_equal(r[3], s[3]), name
        assert r[2].dtype == c[0].dtype
    # at the fixture's iteration count the batch reproduces the golden winner too
    g = case(z, "g3")
    info = {}
    r = pose.ransac_camera_motion_batch([g[:6], case(z, "n7")[:6]], max_iterations=g[7], info=info)[0]
    assert info["out_iter"][0] == int(z["g3_win"]) and np.array_equal(r[2], z["g3_in1"])
    assert np.abs(r[0] - z["g3_R"]).max() <= RT_TOL and np.abs(r[1] - z["g3_t"]).max() <= RT_TOL


def rel_err(X, ref):
    return np.linalg.norm(X - ref, axis=1) / np.linalg.norm(ref, axis=1)


@pytest.mark.parametrize("N", PR.TRI_SIZES)
@pytest.mark.parametrize("normalize", [0, 1])
def test_triangulation_vs_reference(N, normalize):
    z = load("pose.npz")
    p1, p2, P1, P2 = z["tri_p1"][:N], z["tri_p2"][:N], z["tri_P1"], z["tri_P2"]
    fn = pose.triangulate_points if normalize else pose.triangulate
    X = fn(p1, p2, P1, P2)
    assert X.shape == (N, 3) and X.dtype == np.float64
    if normalize and N == 1:
        # one point has no Hartley scale (sqrt(2) / 0): the reference's SVD raises LinAlgError,
        # the device returns no finite coordinate
        assert not np.isfinite(X).any()
        return
    ref = z[f"tri_Xn{N}"] if normalize else z["tri_X"][:N]
    Xr, gap = (PR.triangulate_points if normalize else PR.triangulate)(p1, p2, P1, P2)
    ok = gap >= 10
    e, er = rel_err(X, ref)[ok].max(), rel_err(X, Xr)[ok].max()
    print(f"MEASURED triangulate N={N} normalize={normalize}: vs reference {e:.3e} vs restatement {er:.3e} "
          f"({int((~ok).sum())} points left out)")
    assert e <= X_TOL and er <= X_TOL


def test_triangulation_cpu_tensor_and_device_tensor():
    torch = pytest.importorskip("torch")
    z = load("pose.npz")
    p1, p2, P1, P2 = z["tri_p1"][:65], z["tri_p2"][:65], z["tri_P1"], z["tri_P2"]
    X = pose.triangulate(p1, p2, P1, P2)
    Xc = pose.triangulate(torch.from_numpy(p1), torch.from_numpy(p2), torch.from_numpy(P1), torch.from_numpy(P2))
    assert isinstance(Xc, np.ndarray) and np.array_equal(X, Xc)
    Xd = pose.triangulate(torch.from_numpy(p1).cuda().double(), torch.from_numpy(p2).cuda().double(),
                          torch.from_numpy(P1).cuda(), torch.from_numpy(P2).cuda())
    assert Xd.is_cuda and np.array_equal(Xd.cpu().numpy(), X)
    # a third homogeneous column is ignored (Runner.py:202-208 passes [x, y, 1])
    h = np.column_stack((p1, np.ones(len(p1))))
    assert np.array_equal(pose.triangulate(h, p2, P1, P2), X)


@pytest.mark.parametrize("name", POSE_CASES)
def test_triangulation_of_the_golden_winners(name):
    """The snippet that replaces Runner.py:202-208: the winner's inliers with its pose."""
    z = load("pose.npz")
    p1, p2, K1, K2, Rb, Tb, thr, iters = case(z, name)
    R, t, in1, in2 = pose.ransac_camera_motion(p1, p2, K1, K2, Rb, Tb, threshold=thr, max_iterations=iters)
    Pa = pose.calculate_projection_matrix(Rb, Tb, K1)
    Pb = pose.calculate_projection_matrix(R, t, K2)
    assert np.array_equal(Pa, K1 @ np.hstack([Rb, Tb.reshape(3, 1)]))
    for fn, rf, key in ((pose.triangulate, PR.triangulate, "X"), (pose.triangulate_points, PR.triangulate_points, "Xn")):
        X = fn(in1, in2, Pa, Pb)
        _, gap = rf(in1, in2, Pa, Pb)
        ok = gap >= 10
        e = rel_err(X, z[f"{name}_{key}"])[ok].max()
        print(f"MEASURED {name} {key}: {e:.3e} ({int((~ok).sum())} of {len(ok)} points left out)")
        assert e <= X_TOL
