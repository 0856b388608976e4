"""GPU: the point registry and the BA-input score (registry.hip; pose.PointRegistry) against the
reference's own add_points / prepare_for_ba / total_reprojection_error recorded in
tests/golden/registry.npz and the restatement of tests/registry_ref.py.  Registry results are
integers and copied coordinates: every comparison is exact (coordinates bitwise).  The
conditions the comparisons rely on are asserted on the CPU in tests/test_registry_cpu.py.

Scoring tolerances: 100 x the value measured on the MI355X, capped at 1e-10 (the cap of
tests/test_gpu_structure.py); every figure is printed before its assertion.
  ERR_TOL   per-observation errors against the restatement, |e_gpu - e_rest| / (e_rest + |obs|)
            over the 900 observations (4 cameras, one with r = 0): measured 2.595e-15 (num_points
            900; 5.804e-16 over the first 300), bound 2.595e-13
  MEAN_TOL  |mean_gpu - mean_rest| / mean_rest: measured 2.001e-15 (num_points 300; 2.335e-16 at
            900; 0 on the sequence case's prepare_for_ba output), bound 2.001e-13.  The device
            mean is 4.0e-15 / 3.3e-15 from the reference's recorded means.
(On the CPU the restatement is 1.4e-15 from the same formula in extended precision under the
first measure, and its mean 3.0e-15 from the reference's.)
ring9's tables (nine cameras from -pi to pi, 192 observations): errors 3.610e-16, mean 2.772e-16;
with two camera vectors a whole turn off their principal form (|w| up to 8.63) 5.967e-16 and 0."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native, pose
from tests import registry_ref as RR
from tests.golden_util import load

pytestmark = pytest.mark.gpu

MEASURED_ERR = 2.595e-15
MEASURED_MEAN = 2.001e-15
ERR_TOL = min(1e-10, 100 * MEASURED_ERR)
MEAN_TOL = min(1e-10, 100 * MEASURED_MEAN)

CASES = RR.cases()


def feed(reg, calls, device_tensors=False):
    import torch
    for p3d, p2d, f in calls:
        if device_tensors and len(p3d):
            p3d, p2d = torch.from_numpy(p3d).cuda(), torch.from_numpy(p2d).cuda()
        reg.add_points(p3d, p2d, f)
    return reg


def assert_equals_golden(reg, name):
    z = load("registry.npz")
    pi, fi, G = reg.point_indices, reg.frame_indices, reg.points_3d
    assert pi.dtype == np.int64 and np.array_equal(pi, z[f"{name}_pt_idx"]), name
    assert np.array_equal(fi, z[f"{name}_frame_idx"]), name
    assert G.dtype == np.float64 and G.shape == z[f"{name}_p3d"].shape, name
    assert G.tobytes() == z[f"{name}_p3d"].tobytes(), name
    assert len(reg) == len(z[f"{name}_p3d"])


@pytest.mark.parametrize("name", list(CASES))
def test_registry_equals_reference(name):
    """Order and ties, threshold edge, empty and tiny, the chunk and grid edges (registries of
    1, C - 1, C, C + 1, 2C + 3 entries, batches of 1, 63, 64, 65, 257), the contested cloud, the
    sequence replay, the two halves of split invariance."""
    reg = feed(pose.PointRegistry(), CASES[name])
    assert_equals_golden(reg, name)
    p2 = reg.points_2d
    want = np.concatenate([c[1] for c in CASES[name]])
    assert p2.dtype == want.dtype and np.array_equal(p2, want)


def test_order_and_ties():
    info = {}
    reg = pose.PointRegistry()
    reg.add_points(*CASES["order_ties"][0], info=info)
    assert info["point_indices"].cpu().tolist() == [0, 0, 1, 2, 3, 2, 0]
    assert info["is_new"].cpu().tolist() == [1, 0, 1, 1, 1, 0, 0]
    assert len(reg) == 4


def test_threshold_edge():
    reg = pose.PointRegistry()
    z3, z2 = np.zeros((1, 3)), np.zeros((1, 2))
    reg.add_points(z3, z2, 0)
    info = {}
    reg.add_points(np.array([[0.0, 0.0, np.nextafter(1e-6, 0)]]), z2, 0, info=info)
    assert info["is_new"].cpu().tolist() == [0] and info["point_indices"].cpu().tolist() == [0]
    reg.add_points(np.array([[1e-6, 0.0, 0.0]]), z2, 0, info=info)  # distance exactly the threshold: new
    assert info["is_new"].cpu().tolist() == [1] and info["point_indices"].cpu().tolist() == [1]
    # the threshold is an argument
    wide = pose.PointRegistry(threshold=0.5)
    wide.add_points(np.array([[0.0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0.75, 0, 0]]), np.zeros((4, 2)), 0)
    assert wide.point_indices.tolist() == [0, 0, 1, 1]


def test_empty_and_tiny():
    reg = pose.PointRegistry()
    assert len(reg) == 0 and reg.point_indices.shape == (0,) and reg.points_3d.shape == (0, 3)
    one = np.array([[0.25, -1.5, 3.0]])
    reg.add_points(one, np.array([[3, 4]]), 0)
    reg.add_points(np.empty((0, 3)), np.empty((0, 2)), 1)
    reg.add_points(np.array([]), np.array([]), 1)  # a frame without links (Runner.py:249-250)
    assert len(reg) == 1 and reg.point_indices.tolist() == [0]
    reg.add_points(one.copy(), np.array([[5, 6]]), 2)
    assert len(reg) == 1 and reg.point_indices.tolist() == [0, 0] and reg.frame_indices.tolist() == [0, 2]
    assert reg.points_2d.tolist() == [[3, 4], [5, 6]]


def test_split_invariance():
    a = feed(pose.PointRegistry(), CASES["split_whole"])
    b = feed(pose.PointRegistry(), CASES["split_parts"])
    assert np.array_equal(a.point_indices, b.point_indices) and len(a.point_indices) == 257
    assert a.points_3d.tobytes() == b.points_3d.tobytes()


def test_two_registries_do_not_cross_talk():
    a, b = pose.PointRegistry(), pose.PointRegistry()
    other = f"chunk_{RR.CHUNK + 1}"
    ca, cb = CASES["contested"], CASES[other]
    for k in range(max(len(ca), len(cb))):
        if k < len(ca):
            a.add_points(*ca[k])
        if k < len(cb):
            b.add_points(*cb[k])
    assert_equals_golden(a, "contested")
    assert_equals_golden(b, other)


def test_device_tensors_in():
    reg = feed(pose.PointRegistry(), CASES["sequence"], device_tensors=True)
    assert_equals_golden(reg, "sequence")
    assert np.array_equal(reg.points_3d_device.cpu().numpy(), reg.points_3d)


def test_prepare_for_ba_save_and_load(tmp_path):
    z = load("registry.npz")
    reg = feed(pose.PointRegistry(), CASES["sequence"])
    poses, Ks = RR.sequence_poses()
    ba = reg.prepare_for_ba(poses, Ks)
    assert ba[0] == int(z["ba_num_cameras"]) and ba[1] == int(z["ba_num_points"])
    for got, key in zip(ba[2:], ("ba_camera_indices", "ba_point_indices", "ba_points_2D", "ba_camera_params",
                                 "ba_points_3D", "ba_K")):
        assert np.array_equal(np.asarray(got), z[key]) and np.asarray(got).dtype == z[key].dtype, key
    mean = reg.total_reprojection_error(*ba[1:])
    rest = RR.reprojection_errors(ba[1], *ba[2:])
    rel = abs(mean - rest.sum() / len(rest)) / (rest.sum() / len(rest))
    print(f"MEASURED prepare_for_ba score: mean {mean:.6f}, vs restatement {rel:.3e}")
    assert rel <= MEAN_TOL
    path = str(tmp_path / "model.npz")
    reg.save(path)
    f = np.load(path)
    assert sorted(f.files) == ["frame_idx", "p3d", "pt_idx"]
    assert np.array_equal(f["p3d"], z["sequence_p3d"]) and np.array_equal(f["pt_idx"], z["sequence_pt_idx"])
    back = pose.PointRegistry.load(path)
    assert back.points_3d.tobytes() == reg.points_3d.tobytes()
    assert np.array_equal(back.point_indices, reg.point_indices)
    assert np.array_equal(back.frame_indices, reg.frame_indices)
    info = {}
    back.add_points(reg.points_3d[[5, 0, 5]], np.zeros((3, 2)), 9, info=info)  # and it goes on from there
    assert info["point_indices"].cpu().tolist() == [5, 0, 5] and len(back) == len(reg)


def test_arguments():
    torch = pytest.importorskip("torch")
    reg = pose.PointRegistry()
    with pytest.raises(ValueError):
        reg.add_points(np.zeros((3, 3)), np.zeros((2, 2)), 0)
    with pytest.raises(ValueError):
        reg.add_points(np.zeros((3, 2)), np.zeros((3, 2)), 0)
    with pytest.raises(ValueError):
        reg.add_points(np.array([[0.0, np.nan, 0.0]]), np.zeros((1, 2)), 0)
    with pytest.raises(ValueError):
        reg.add_points(np.array([[0.0, np.inf, 0.0]]), np.zeros((1, 2)), 0)
    with pytest.raises(ValueError):
        pose.PointRegistry(threshold=0.0)
    assert len(reg) == 0 and reg.point_indices.shape == (0,)
    ctx = _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))
    L, h = ctx.lib, ctx.handle
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    p, pc = buf.data_ptr(), cnt.data_ptr()

    def add(tab=p, count=pc, cap=8, pts=p, n=2, thr=1e-6, oi=pc, on=pc):
        _native.check(L.sfm_registry_add_dev(h, tab, count, cap, pts, n, ctypes.c_double(thr), oi, on, None), h)

    for kw in ({"tab": None}, {"count": None}, {"cap": -1}, {"pts": None}, {"n": -1}, {"thr": 0.0}, {"thr": -1e-6},
               {"thr": float("nan")}, {"oi": None}, {"on": None}, {"cap": 1}):
        with pytest.raises(ValueError, match="sfm_registry_add_dev"):
            add(**kw)
    add(n=0, pts=None, oi=None, on=None)  # nothing to do
    assert L.sfm_registry_add_dev(None, p, pc, 8, p, 2, ctypes.c_double(1e-6), pc, pc, None) == _abi.SFM_EINVAL

    def score(ci=pc, pi=pc, obs=p, M=2, cams=p, nc=1, K=p, X=p, npts=1, err=p, mean=p):
        _native.check(L.sfm_total_reprojection_error_dev(h, ci, pi, obs, M, cams, nc, K, X, npts, err, mean, None), h)

    for kw in ({"ci": None}, {"pi": None}, {"obs": None}, {"M": -1}, {"cams": None}, {"K": None}, {"X": None},
               {"err": None}, {"mean": None}, {"nc": 0}, {"npts": 0}):
        with pytest.raises(ValueError, match="sfm_total_reprojection_error_dev"):
            score(**kw)
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [0, 0, 0, 0]
    cam, pt, obs, cp, X, K = RR.score_case()
    with pytest.raises(IndexError):
        reg.total_reprojection_error(10, np.full(10, 4), pt, obs, cp, X, K)
    with pytest.raises(IndexError):
        reg.total_reprojection_error(10, cam, np.full(10, -1), obs, cp, X, K)
    with pytest.raises(ValueError):
        reg.total_reprojection_error(901, cam, pt, obs, cp, X, K)


_score = {}


def scored(k):
    """One device score per num_points, shared by the tests (never modified)."""
    if k not in _score:
        info = {}
        mean = pose.PointRegistry().total_reprojection_error(k, *RR.score_case(), info=info)
        _score[k] = (mean, info["errors"])
    return _score[k]


@pytest.mark.parametrize("k", [300, 900])
def test_total_reprojection_error(k):
    z = load("registry.npz")
    cam, pt, obs, cp, X, K = RR.score_case()
    rest = RR.reprojection_errors(k, cam, pt, obs, cp, X, K)
    mean, err = scored(k)
    assert err.shape == (k,) and err.dtype == np.float64
    d = float((np.abs(err - rest) / (rest + np.linalg.norm(obs[:k], axis=1))).max())
    rm = rest.sum() / k
    dm = abs(mean - rm) / rm
    dr = abs(mean - float(z[f"score_mean_{k}"])) / float(z[f"score_mean_{k}"])
    ident = cam[:k] == 1  # the camera with r = 0
    print(f"MEASURED score num_points {k}: errors vs restatement {d:.3e}, mean {mean:.12g} vs restatement {dm:.3e}, "
          f"vs the reference {dr:.3e}; {int(ident.sum())} observations through the identity branch")
    assert ident.sum() > 20
    assert d <= ERR_TOL
    assert dm <= MEAN_TOL
    # the same bits every run, and device tensors in give the same
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    again = pose.PointRegistry().total_reprojection_error(k, t(cam), t(pt), t(obs), t(cp), t(X), t(K))
    assert np.float64(again).tobytes() == np.float64(mean).tobytes()


def test_total_reprojection_error_of_nothing_is_nan():
    cam, pt, obs, cp, X, K = RR.score_case()
    assert np.isnan(pose.PointRegistry().total_reprojection_error(0, cam, pt, obs, cp, X, K))


def test_total_reprojection_error_at_the_angles_of_an_orbit():
    """k_total_reproj's rodrigues on ring9's own tables (tests/ba_ref.py): nine cameras from -pi to
    pi, six of them beyond pi / 2 (score_case stays within 0.35 rad), then the same cameras with two
    start vectors a whole turn below and above their principal form.  The existing measures and
    bounds."""
    from tests import ba_ref as BR
    rings = BR.ring_cases()
    sc, nq = rings["ring9"], rings["ring9_nonprincipal"]
    M = len(sc["obs"])
    assert M == 192
    th = np.sqrt((sc["cams"][:, :3] ** 2).sum(1))
    assert (th > np.pi / 2).sum() >= 6 and th.max() > 3.13
    rest = RR.reprojection_errors(M, sc["cam_idx"], sc["pt_idx"], sc["obs"], sc["cams"], sc["X"], sc["K"])
    scale = rest + np.linalg.norm(sc["obs"], axis=1)
    rm = rest.sum() / M
    for name, cams in (("ring9", sc["cams"]), ("ring9_nonprincipal", nq["cams"])):
        info = {}
        mean = pose.PointRegistry().total_reprojection_error(M, sc["cam_idx"], sc["pt_idx"], sc["obs"], cams, sc["X"],
                                                             sc["K"], info=info)
        err = info["errors"]
        assert err.shape == (M,) and err.dtype == np.float64
        d = float((np.abs(err - rest) / scale).max())     # the non-principal run against the principal restatement too
        dm = abs(mean - rm) / rm
        print(f"MEASURED score {name}: {M} observations, |w| up to {np.sqrt((cams[:, :3] ** 2).sum(1)).max():.4f}: errors vs "
              f"restatement {d:.3e}, mean {mean:.12g} vs restatement {dm:.3e}")
        assert d <= ERR_TOL and dm <= MEAN_TOL
