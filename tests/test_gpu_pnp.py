"""GPU: PnP on the device (pnp.hip; pose.PnPRansac, pose.PnP, pose.next_structure) against this
repository's numpy restatement and scipy's minimum (tests/golden/pnp.npz, tests/pnp_ref.py).
The conditions the comparisons rely on are asserted on the CPU in tests/test_pnp_cpu.py.  OpenCV
is not a reference here: its outputs are not pinned.

The winner's iteration, the whole counts table and the inlier indices must be identical to the
restatement's.  Tolerances: each is 100 x the largest value measured on the MI355X over the
fixture, with its cap (1e-6 for poses, 1e-8 for costs); every figure is printed before its
assertion.
  R_TOL, T_TOL   PnPRansac's pose against the restatement's, max |dR| and |dt| / max(1, |t|):
                 measured 1.951e-10 and 1.447e-9 (both n65; the others 6e-16 to 3e-11 and 8e-16 to
                 2.4e-10), bounds 1.951e-8 and 1.447e-7
  COST_TOL       |cost_gpu - cost_rest| / cost_rest, at the returned pose and at the winning
                 hypothesis: measured 6.884e-14 (n7) and 1.662e-13 (it50), bound 1.662e-11
  EXCESS_TOL     (cost_gpu - cost_scipy) / cost_scipy where positive: never positive on the fixture
                 (-4e-14 to -1.8e-9: scipy stops a little short of the minimum), so the floor,
                 1e-12, is the bound (a cost is evaluated to about 1e-13 relative,
                 tests/structure_ref.py)
  PNP_R_TOL, PNP_T_TOL   PnP's pose against the restatement's: measured 9.024e-12 and 9.357e-11
                 (both n6), bounds 9.024e-10 and 9.357e-9
  PNP_START_TOL  PnP's cost at the DLT's own pose against the restatement's (whose eigenvector is
                 LAPACK's, the device's a cyclic Jacobi's): measured 6.977e-13 (lm256), bound
                 6.977e-11
No case of the fixture is free of marginal comparisons (the last accepted steps change the cost
by less than 1e-9 of it), so the status and the accepted steps are compared through `firm`: the
device takes at least the 3 (PnP: 2) accepted steps that precede the first marginal one.
Measured: accepted steps 3 to 7 against the restatement's 3 to 6, status 0 or 1 on both sides.
Accepting a step on "cost strictly smaller" locates a minimiser to about sqrt(eps) of its scale
(DESIGN.md §13B), which is what two implementations of the rule differ by."""
from __future__ import annotations

import sys

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native, pose
from tests import pnp_ref as PR
from tests.golden_util import load

pytestmark = pytest.mark.gpu

MEASURED_R = 1.951e-10
MEASURED_T = 1.447e-9
MEASURED_COST = 1.662e-13
MEASURED_EXCESS = 0.0
MEASURED_PNP_R = 9.024e-12
MEASURED_PNP_T = 9.357e-11
MEASURED_PNP_START = 6.977e-13
R_TOL = min(1e-6, 100 * MEASURED_R)
T_TOL = min(1e-6, 100 * MEASURED_T)
COST_TOL = min(1e-8, 100 * MEASURED_COST)
EXCESS_TOL = min(1e-8, max(1e-12, 100 * MEASURED_EXCESS))
PNP_R_TOL = min(1e-6, 100 * MEASURED_PNP_R)
PNP_T_TOL = min(1e-6, 100 * MEASURED_PNP_T)
PNP_START_TOL = min(1e-8, 100 * MEASURED_PNP_START)

NAMES = list(PR.ransac_cases())

_cache = {}


def inputs(z, name):
    g = lambda k: z[f"{name}_{k}"]
    # what Runner.py:258-259 hands over: float32 arrays (the fixture's values convert exactly)
    return g("X").astype(np.float32), g("x").astype(np.float32), g("K"), int(g("iters"))


def estimated(name):
    """One device PnPRansac per case, shared by the tests (never modified)."""
    if name not in _cache:
        X, x, K, iters = inputs(load("pnp.npz"), name)
        info = {}
        pe = pose.PnPRansac(X, x, K=K, ransac_max_it=iters, info=info)
        _cache[name] = (pe, info)
    return _cache[name]


def estimated_pnp(name):
    key = name + "/pnp"
    if key not in _cache:
        X, x, K, _ = inputs(load("pnp.npz"), name)
        info = {}
        pe = pose.PnP(X, x, K=K, info=info)
        _cache[key] = (pe, info)
    return _cache[key]


def dpose(R, t, Rr, tr):
    return float(np.abs(R - Rr).max()), float(np.linalg.norm(t.ravel() - tr.ravel()) / max(1.0, np.linalg.norm(tr)))


@pytest.mark.parametrize("name", NAMES)
def test_ransac_equals_restatement(name):
    z = load("pnp.npz")
    g = lambda k: z[f"{name}_{k}"]
    pe, info = estimated(name)
    print(f"MEASURED ransac {name}: winner {info['iteration']} (restatement {int(g('iteration'))}), inliers "
          f"{0 if pe.inliers is None else len(pe.inliers)} (restatement {len(g('inliers'))}), counts differing "
          f"{int((info['counts'] != g('counts')).sum())} of {len(g('counts'))}")
    assert info["counts"].dtype == np.int32 and np.array_equal(info["counts"], g("counts"))
    assert info["iteration"] == int(g("iteration"))
    if not bool(g("found")):
        assert pe.R is None and pe.t is None and pe.inliers is None
        assert info["status"] == -1 and info["iters"] == 0
        return
    assert pe.R.shape == (3, 3) and pe.R.dtype == np.float64 and pe.t.shape == (3, 1) and pe.t.dtype == np.float64
    assert pe.inliers.dtype == np.int32 and pe.inliers.shape == (len(g("inliers")), 1)
    assert np.array_equal(pe.inliers[:, 0], g("inliers"))


@pytest.mark.parametrize("name", PR.HOLDS)
def test_refinement_vs_restatement_and_scipy(name):
    z = load("pnp.npz")
    g = lambda k: z[f"{name}_{k}"]
    pe, info = estimated(name)
    dR, dt = dpose(pe.R, pe.t, g("rest_R"), g("rest_t"))
    c, cr, cs = info["cost"], float(g("rest_cost")), float(g("sp_cost"))
    ec, ex = abs(c - cr) / cr, (c - cs) / cs
    e0 = abs(info["cost0"] - float(g("rest_cost0"))) / float(g("rest_cost0"))
    print(f"MEASURED refine {name}: max |dR| {dR:.3e} |dt| {dt:.3e} cost {ec:.3e} start cost {e0:.3e} excess over "
          f"scipy {ex:.3e}; status {info['status']} (restatement {int(g('rest_status'))}) accepted {info['iters']} "
          f"(restatement {int(g('rest_iters'))}, firm {int(g('rest_firm'))}, all firm {bool(g('rest_all_firm'))}) "
          f"iterations {info['lm_iters']} (restatement {int(g('rest_lm_iters'))})")
    assert dR <= R_TOL and dt <= T_TOL
    assert ec <= COST_TOL and e0 <= COST_TOL
    assert ex <= EXCESS_TOL
    assert c <= info["cost0"]
    # where no comparison of the restatement's run was marginal the device takes the same path
    if bool(g("rest_all_firm")):
        assert info["status"] == int(g("rest_status")) and info["iters"] == int(g("rest_iters"))
    # and it takes at least the accepted steps that came before the first marginal one
    assert info["iters"] >= int(g("rest_firm"))
    assert info["status"] in (0, 1, 3) and 1 <= info["lm_iters"] <= pose.REFINE_MAX_ITER
    # the rotation is one, and the planted pose is near
    assert np.abs(pe.R @ pe.R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(pe.R) > 0
    assert np.abs(pe.R - g("R_true")).max() < 2e-2


@pytest.mark.parametrize("name", PR.LM_CASES)
def test_pnp_vs_restatement_and_scipy(name):
    z = load("pnp.npz")
    g = lambda k: z[f"{name}_pnp_{k}"]
    pe, info = estimated_pnp(name)
    assert pe.inliers is None and pe.R.shape == (3, 3) and pe.t.shape == (3, 1)
    dR, dt = dpose(pe.R, pe.t, g("rest_R"), g("rest_t"))
    c, cr, cs = info["cost"], float(g("rest_cost")), float(g("sp_cost"))
    ec, ex = abs(c - cr) / cr, (c - cs) / cs
    e0 = abs(info["cost0"] - float(g("rest_cost0"))) / float(g("rest_cost0"))
    print(f"MEASURED pnp {name}: max |dR| {dR:.3e} |dt| {dt:.3e} cost {ec:.3e} start cost (the DLT's) {e0:.3e} "
          f"excess over scipy {ex:.3e}; status {info['status']} (restatement {int(g('rest_status'))}) accepted "
          f"{info['iters']} (restatement {int(g('rest_iters'))}, firm {int(g('rest_firm'))})")
    assert dR <= PNP_R_TOL and dt <= PNP_T_TOL
    assert ec <= COST_TOL
    assert ex <= EXCESS_TOL
    if bool(g("rest_all_firm")):
        assert info["status"] == int(g("rest_status")) and info["iters"] == int(g("rest_iters"))
    assert info["iters"] >= int(g("rest_firm"))
    assert e0 <= PNP_START_TOL


@pytest.mark.parametrize("name", PR.LM_CASES + ["n2600", "skew"])
def test_two_runs_give_the_same_bits(name):
    X, x, K, iters = inputs(load("pnp.npz"), name)
    pe, info = estimated(name)
    info2 = {}
    pe2 = pose.PnPRansac(X, x, K=K, ransac_max_it=iters, info=info2)
    assert pe.R.tobytes() == pe2.R.tobytes() and pe.t.tobytes() == pe2.t.tobytes()
    assert np.array_equal(pe.inliers, pe2.inliers) and np.array_equal(info["counts"], info2["counts"])
    for k in ("cost0", "cost", "status", "iters", "lm_iters", "iteration"):
        assert np.float64(info[k]).tobytes() == np.float64(info2[k]).tobytes(), k
    if name in PR.LM_CASES:
        q, qi = estimated_pnp(name)
        qi2 = {}
        q2 = pose.PnP(X, x, K=K, info=qi2)
        assert q.R.tobytes() == q2.R.tobytes() and q.t.tobytes() == q2.t.tobytes()
        assert np.float64(qi["cost"]).tobytes() == np.float64(qi2["cost"]).tobytes() and qi["iters"] == qi2["iters"]


def test_device_tensors_in_device_tensors_out():
    torch = pytest.importorskip("torch")
    X, x, K, iters = inputs(load("pnp.npz"), "n65")
    pe, info = estimated("n65")
    dX, dx = torch.from_numpy(X).cuda(), torch.from_numpy(x).cuda()
    d = pose.PnPRansac(dX, dx, K=K, ransac_max_it=iters)
    assert d.R.is_cuda and d.t.is_cuda and d.inliers.is_cuda
    assert d.R.dtype == torch.float64 and d.inliers.dtype == torch.int32
    assert tuple(d.R.shape) == (3, 3) and tuple(d.t.shape) == (3, 1) and tuple(d.inliers.shape) == pe.inliers.shape
    assert np.array_equal(d.R.cpu().numpy(), pe.R) and np.array_equal(d.t.cpu().numpy(), pe.t)
    assert np.array_equal(d.inliers.cpu().numpy(), pe.inliers)
    q = pose.PnP(dX, dx, K=torch.from_numpy(K).cuda())
    assert q.R.is_cuda and q.inliers is None
    # CPU tensors behave as numpy
    c = pose.PnPRansac(torch.from_numpy(X), torch.from_numpy(x), K=K, ransac_max_it=iters)
    assert isinstance(c.R, np.ndarray) and np.array_equal(c.R, pe.R) and np.array_equal(c.inliers, pe.inliers)
    # float64 input with the same values gives the same bits
    e = pose.PnPRansac(X.astype(np.float64), x.astype(np.float64), K=K, ransac_max_it=iters)
    assert np.array_equal(e.R, pe.R) and np.array_equal(e.t, pe.t)
    with pytest.raises(ValueError):
        pose.PnPRansac(torch.full((7, 3), float("nan"), device="cuda"), torch.zeros((7, 2), device="cuda"), K=K)


def test_two_contexts_used_alternately():
    torch = pytest.importorskip("torch")
    z = load("pnp.npz")
    dev = torch.device("cuda", 0)
    params = _abi.params_from_dict({}, _abi.SFM_MODE_NAIVE)
    ctxs = [_native.Context(params, 0), _native.Context(params, 0)]
    try:
        for rnd in range(2):
            for k, name in enumerate(["n12", "n63", "n7", "n64"]):
                X, x, K, iters = inputs(z, name)
                t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
                o = pose._pnp_ransac_dev(t(X), t(x), t(K).reshape(-1), iters, 8.0, pose.REFINE_MAX_ITER, dev,
                                         ctx=ctxs[(k + rnd) % 2])
                pe, info = estimated(name)
                n = int(o["n"].cpu()[0])
                assert n == len(pe.inliers) and np.array_equal(o["inliers"][:n].cpu().numpy(), pe.inliers[:, 0])
                assert np.array_equal(o["R"].cpu().numpy().reshape(3, 3), pe.R), (rnd, name)
                assert np.array_equal(o["t"].cpu().numpy().reshape(3, 1), pe.t)
                assert np.array_equal(o["counts"][:iters].cpu().numpy(), info["counts"])
    finally:
        for c in ctxs:
            c.close()


def three_frames(seed=7, n=180):
    """A planted three-frame scene: n points, integer pixels in three 960 x 540 views (f = 800),
    sigma = 0.5 pixel noise; the matches of pair (2, 3) are a subset of pair (1, 2)'s second-image
    points, a few of them moved by 3 or 7 pixels, plus points pair (1, 2) never saw."""
    rng = np.random.default_rng(seed)
    K = PR.K_SCENE
    Xw = rng.uniform([-3, -2, 5], [3, 2, 12], (n, 3))
    poses = [(np.eye(3), np.zeros(3)), (PR.rot(0.10, -0.02, 0.01), np.array([-1.0, 0.05, 0.1])),
             (PR.rot(0.21, -0.03, 0.02), np.array([-2.0, 0.08, 0.25]))]
    px = []
    for R, t in poses:
        q = (Xw @ R.T + t) @ K.T
        px.append(np.round(q[:, :2] / q[:, 2:] + rng.normal(0, 0.5, (n, 2))).astype(np.int64))
    first = np.arange(0, 140)            # pair (1, 2) sees these
    second = np.arange(40, n)            # pair (2, 3) sees these: 100 shared, 40 new
    p1b = px[1][second].copy()
    p1b[::9] += np.array([3, 0])         # still within dist_threshold = 5
    p1b[4::17] += np.array([0, 7])       # beyond it
    return K, poses, (px[0][first], px[1][first]), (p1b, px[2][second])


def test_next_structure_is_the_chain_of_its_parts_and_a_sequence_runs_without_cv2():
    K, poses, (a1, a2), (b1, b2) = three_frames()
    R2, t2, in1, in2, p3d, mean0 = pose.initial_structure(a1, a2, K, K, 200)
    assert R2 is not None and len(in1) >= 30
    P2 = pose.calculate_projection_matrix(R2, t2, K)
    info = {}
    R3, t3, inl, rp, rn, P3, p3d_new, mean = pose.next_structure(in2, p3d, P2, b1, b2, K, ransac_max_it=200, info=info)
    # the same steps one by one (Runner.py:241-282)
    rp2, rn2 = pose.link_points(in2, p3d, b1, b2, dist_threshold=5.0)
    pe = pose.PnPRansac(np.asarray(rp2, dtype=np.float32), np.asarray(rn2, dtype=np.float32), K=K, ransac_max_it=200)
    assert np.array_equal(rp, rp2) and np.array_equal(rn, rn2) and len(rp) >= 20
    assert R3.tobytes() == pe.R.tobytes() and t3.tobytes() == pe.t.tobytes() and np.array_equal(inl, pe.inliers)
    P3b = pose.calculate_projection_matrix(pe.R, pe.t, K)
    assert P3.tobytes() == P3b.tobytes() and P3.shape == (3, 4)
    X = pose.non_linear_triangulation(pose.triangulate(b1, b2, P2, P3b), b1, b2, P2, P3b)
    assert p3d_new.dtype == np.float64 and p3d_new.tobytes() == X.tobytes()
    m, _ = pose.reprojection_error(X, b1, b2, P2, P3b)
    assert np.float64(mean).tobytes() == np.float64(m).tobytes()
    # the third pose relative to the second is the planted one up to the initial pair's scale
    Rrel = poses[2][0] @ poses[1][0].T
    print(f"MEASURED next_structure: {len(rp)} links, {len(inl)} inliers, winner {info['iteration']}, mean error "
          f"{mean:.4f}, max |R3 R2^T - planted| {np.abs(R3 @ R2.T - Rrel).max():.3e}")
    # (sanity of the planted scene, not a pinned figure: one point in nine of pair (2, 3) was moved
    # by 3 pixels and one in seventeen by 7, and they are triangulated with the rest)
    assert len(inl) >= 0.8 * len(rp) and np.abs(R3 @ R2.T - Rrel).max() < 2e-2 and mean < pose.PNP_THRESHOLD
    # what INTEGRATION.md §1 shows: the registry and the score before bundle adjustment, no OpenCV
    reg = pose.PointRegistry()
    reg.add_points(p3d, in2, 0)
    reg.add_points(rp, rn, 1)
    reg.add_points(p3d_new, b2, 1)
    global_poses = [(pose.rodrigues(R2)[0], t2), (pose.rodrigues(R3)[0], t3)]
    ba = reg.prepare_for_ba(global_poses, [K, K])
    total = reg.total_reprojection_error(*ba[1:])
    print(f"MEASURED three-frame sequence: {len(reg)} registered points, total reprojection error {total:.4f}")
    assert np.isfinite(total) and total < pose.PNP_THRESHOLD
    assert "cv2" not in sys.modules
    # no pose: Runner.py:263's case
    r = pose.next_structure(in2[:3], p3d[:3], P2, b1 + 500, b2, K, ransac_max_it=10)
    assert r[0] is None and r[5] is None and r[6] is None


def test_c_abi_argument_errors_leave_a_message():
    torch = pytest.importorskip("torch")
    ctx = _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))
    L, h = ctx.lib, ctx.handle
    buf = torch.zeros(256, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    E = _abi.SFM_EINVAL
    msg = lambda: (L.sfm_last_error(h) or b"").decode()

    def ransac(X=p, x=p, K=p, n=8, iters=4, thr=8.0, mi=50, R=p, t=p, inl=p, on=p, oit=p, st=p, cost=p, counts=None):
        return L.sfm_pnp_ransac_dev(h, X, x, K, n, iters, thr, mi, R, t, inl, on, oit, st, cost, counts, None)

    for kw in ({"X": None}, {"x": None}, {"K": None}, {"n": -1}, {"iters": -1}, {"thr": 0.0}, {"thr": float("nan")},
               {"mi": 0}, {"mi": 1 << 24}, {"R": None}, {"t": None}, {"inl": None}, {"on": None}, {"oit": None},
               {"st": None}, {"cost": None}):
        assert ransac(**kw) == E and "sfm_pnp_ransac_dev" in msg(), kw
    assert L.sfm_pnp_ransac_dev(None, p, p, p, 8, 4, 8.0, 50, p, p, p, p, p, p, p, None, None) == E

    def pnp(X=p, x=p, K=p, n=8, mi=50, R=p, t=p, st=p, cost=p):
        return L.sfm_pnp_dev(h, X, x, K, n, mi, R, t, st, cost, None)

    for kw in ({"X": None}, {"x": None}, {"K": None}, {"n": -1}, {"mi": 0}, {"R": None}, {"t": None}, {"st": None},
               {"cost": None}):
        assert pnp(**kw) == E and "sfm_pnp_dev" in msg(), kw
    # no points at all is a defined "no pose", not an error
    st = torch.full((4,), 9, dtype=torch.int32, device="cuda")
    on = torch.full((2,), 9, dtype=torch.int32, device="cuda")
    assert L.sfm_pnp_ransac_dev(h, None, None, p, 0, 4, 8.0, 50, p, p, None, on.data_ptr(), on[1:].data_ptr(),
                                st.data_ptr(), p, None, None) == _abi.SFM_OK
    torch.cuda.synchronize()
    assert on.cpu().tolist() == [-1, -1] and st.cpu().tolist() == [0, -1, 0, 0]
    # five points through the raw calls (the classes return before the device): no pose, NaN outputs,
    # every sample's count 0
    z = load("pnp.npz")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
    o = pose._pnp_ransac_dev(t(z["n5_X"]), t(z["n5_x"]), t(z["n5_K"]).reshape(-1), 9, 8.0, 50, torch.device("cuda", 0))
    assert int(o["n"].cpu()[0]) == -1 and int(o["iteration"].cpu()[0]) == -1
    assert o["status"].cpu().tolist() == [0, -1, 0, 0] and o["counts"].cpu().tolist() == [0] * 9
    assert bool(torch.isnan(o["R"]).all()) and bool(torch.isnan(o["t"]).all()) and bool(torch.isnan(o["cost"]).all())
    X5, x5, K5 = t(z["n5_X"]), t(z["n5_x"]), t(z["n5_K"]).reshape(-1)
    st.fill_(9)
    assert L.sfm_pnp_dev(h, X5.data_ptr(), x5.data_ptr(), K5.data_ptr(), 5, 50, p, buf[16:].data_ptr(),
                         st.data_ptr(), buf[32:].data_ptr(), None) == _abi.SFM_OK
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, -1, 0, 0] and bool(torch.isnan(buf[:9]).all())
