"""GPU: bundle adjustment on the device (ba.hip; pose.BundleAdjustment, PointRegistry.set_points_3d)
against this repository's numpy restatement, scipy's tight-tolerance minimum and the reference's
own recorded run (tests/golden/ba.npz, tests/ba_ref.py).  The conditions the comparisons rely on
are asserted on the CPU in tests/test_ba_cpu.py.  Which iterate scipy's TRF path stops at is not
pinned; the minimum is.

Tolerances: each is 100 x the largest value measured on the MI355X over the fixture, against the
restatement or scipy and never against the device's own output, with its cap (1e-6 for poses and
points, 1e-8 for costs; the excess over scipy has a floor of 1e-12); every figure is printed
before its assertion.  A cost below NOISE = M (4 eps max |obs|)^2 is rounding (M squared
residuals, each a pixel coordinate evaluated to a few ulps) and is added to every cost bound: the
one-camera case ends at a cost of 1e-26.
  COST_TOL    |cost_gpu - cost_rest| / cost_rest, start and final, at ftol = 1e-2 and 0:
              measured 6.513e-14 (idle_rows, final, ftol 1e-2; start costs to 3.3e-15), bound
              6.513e-12
  CAM_TOL     cameras against the restatement's where two cameras are fixed (no gauge freedom):
              max |d omega|, |d t| / max(1, |t|): measured 3.000e-11 (obs_256) and 1.140e-11
              (tile_11), both at ftol 0; at ftol 1e-2 2e-14 at most; bound 3.000e-9
  PT_TOL      points, same cases, max |dX| / max(1, |X|): measured 3.312e-10 (tile_11 at ftol 0; at
              ftol 1e-2 1e-13 at most), bound 3.312e-8
  EXCESS_TOL  (cost_gpu - cost_scipy) / cost_scipy where positive, at ftol = 0: measured 2.567e-14
              (two_cams; -1.2e-14 to 6e-15 elsewhere), below the floor, so 1e-12 is the bound (a cost
              is evaluated to about 1e-13 relative, tests/structure_ref.py)
Measured at ftol = 0: accepted steps 5 to 8 against the restatement's 4 to 9 (firm 3 to 6), status
0 or 1 on both sides, not always the same one; no factorisation was rejected anywhere.  The
227-, 228- and 256-camera scenes (built and solved by the restatement at test time) measure 1.9e-14
(cost), 1.4e-14 (cameras) and 4.4e-14 (points), inside the same bounds.
At ftol = 1e-2 no comparison of the restatement's runs is marginal: status and accepted steps are
equal.  At ftol = 0 every run but the one-camera case ends among steps that change the cost by less than 1e-9 of it, so
the device takes at least the restatement's firm steps.  Accepting a step on "cost strictly
smaller" locates a minimiser to about sqrt(eps) of its scale, which is what two
implementations of the rule differ by.
The ring scenes (BR.ring_cases: cameras on a whole orbit, solved by the restatement at test time) are
held to the same bounds.  Measured: at ftol 1e-2 every run has the restatement's status and 2 accepted
steps, costs to 1.2e-14, rotations as matrices to 8.9e-16, vectors to 8.9e-16, points to 8.0e-16;
ring9 returns 6 of 9 cameras through rodrigues_inv's c < 0 branch (min pi - theta 1.2e-3), ring9_flat
5 of 9 (8.0e-4, and one camera on each side of pi / 2), ring8 4 of 8, ring5_quarter 1 of 5, the
non-principal start 6 of 9, all principal.  At ftol 0: costs to 8.9e-15; ring8 measures 1.150e-10 in
the vectors (1.066e-10 as matrices; ring9_flat 5.3e-11) and 1.226e-10 in the points, above
MEASURED_CAM = 3.000e-11 and inside CAM_TOL / PT_TOL, which stay as they are: both sides end
there among steps that change the cost by less than 1e-9 of it, with different last steps (device
status 1 after 5 accepted steps, restatement 0 after 5), which is the sqrt(eps) of the paragraph
above and not the angle: the same cameras agree to 8.9e-16 at ftol 1e-2, and ring9, whose cameras
come closest to pi, to 2.5e-15 at ftol 0."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native, pose
from tests import ba_ref as BR
from tests.golden_util import load

pytestmark = pytest.mark.gpu

MEASURED_COST = 6.513e-14
MEASURED_CAM = 3.000e-11
MEASURED_PT = 3.312e-10
MEASURED_EXCESS = 2.567e-14
COST_TOL = min(1e-8, 100 * MEASURED_COST)
CAM_TOL = min(1e-6, 100 * MEASURED_CAM)
PT_TOL = min(1e-6, 100 * MEASURED_PT)
EXCESS_TOL = min(1e-8, max(1e-12, 100 * MEASURED_EXCESS))

_SCENES = BR.cases()
NAMES = list(_SCENES)
FTOLS = {"f2": 1e-2, "f0": 0.0}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cache = {}


def scene_of(z, name):
    g = lambda k: z[f"{name}_{k}"]
    return dict(n_cam=int(g("n_cam")), n_pts=int(g("n_pts")), cam_idx=g("cam_idx").astype(np.int64),
                pt_idx=g("pt_idx").astype(np.int64), obs=g("obs"), cams=g("cams"), K=g("K"), X=g("X"), fixed=g("fixed"))


def noise_floor(sc):
    return len(sc["obs"]) * (4 * np.finfo(np.float64).eps * np.abs(sc["obs"]).max()) ** 2


def adjust(sc, ftol, max_iter=BR.MAX_ITER, **kw):
    info = {}
    ba = pose.BundleAdjustment(sc["n_cam"], sc["n_pts"], sc["cam_idx"], sc["pt_idx"], sc["obs"], sc["cams"], sc["X"],
                               sc["K"], fixed_cameras=sc["fixed"].astype(bool), ftol=ftol, max_iter=max_iter, info=info,
                               **kw)
    cams, X = ba.sparse_bundle_adjustment()
    return cams, X, info


def adjusted(name, tag):
    """One device run per (case, ftol), shared by the tests (never modified)."""
    if (name, tag) not in _cache:
        _cache[name, tag] = adjust(scene_of(load("ba.npz"), name), FTOLS[tag])
    return _cache[name, tag]


@pytest.mark.parametrize("tag", list(FTOLS))
@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name, tag):
    z = load("ba.npz")
    sc = scene_of(z, name)
    g = lambda k: z[f"{name}_{tag}_{k}"]
    cams, X, info = adjusted(name, tag)
    assert cams.shape == (sc["n_cam"], 6) and cams.dtype == np.float64
    assert X.shape == (sc["n_pts"], 3) and X.dtype == np.float64
    floor = noise_floor(sc)
    c0, c, r0, rc = info["cost0"], info["cost"], float(g("cost0")), float(g("cost"))
    e0, ec = abs(c0 - r0) / r0, max(abs(c - rc) - floor, 0.0) / max(rc, floor)
    print(f"MEASURED ba {name} ftol {FTOLS[tag]:g}: start cost {e0:.3e} final cost {ec:.3e} ({c:.10g} vs {rc:.10g}); "
          f"status {info['status']} (restatement {int(g('status'))}) accepted {info['iters']} (restatement "
          f"{int(g('iters'))}, firm {int(g('firm'))}, all firm {bool(g('all_firm'))}) iterations {info['lm_iters']} "
          f"(restatement {int(g('lm_iters'))}) rejected factorisations {info['rejected_factorisations']}")
    assert e0 <= COST_TOL and ec <= COST_TOL
    assert c <= c0
    if bool(g("all_firm")):
        assert info["status"] == int(g("status")) and info["iters"] == int(g("iters"))
    assert info["iters"] >= int(g("firm"))
    assert info["status"] in (0, 1, 3) and 1 <= info["lm_iters"] <= BR.MAX_ITER
    # rows that do not move keep their bits
    ca, pa = BR.active(sc)
    assert cams[~ca].tobytes() == sc["cams"][~ca].tobytes() and X[~pa].tobytes() == sc["X"][~pa].tobytes()
    assert (np.sqrt((cams[:, :3] ** 2).sum(1)) <= np.pi + 1e-12).all()
    if int(sc["fixed"].sum()) >= 2 and f"{name}_{tag}_X" in z.files:   # no gauge freedom: poses and points
        rcams, rX = g("cams"), g("X")
        dw = float(np.abs(cams[:, :3] - rcams[:, :3]).max())
        dt = float((np.linalg.norm(cams[:, 3:] - rcams[:, 3:], axis=1) / np.maximum(1.0, np.linalg.norm(rcams[:, 3:], axis=1))).max())
        dX = float((np.linalg.norm(X - rX, axis=1) / np.maximum(1.0, np.linalg.norm(rX, axis=1))).max())
        print(f"MEASURED ba {name} ftol {FTOLS[tag]:g}: max |d omega| {dw:.3e} |dt| {dt:.3e} |dX| {dX:.3e}")
        assert dw <= CAM_TOL and dt <= CAM_TOL and dX <= PT_TOL
    else:   # gauge freedom (or a large case): the cost of the returned model is the device's own figure
        back = BR.cost_of(sc, cams, X)
        print(f"MEASURED ba {name} ftol {FTOLS[tag]:g}: cost of the returned model {back:.10g}")
        assert abs(back - c) <= COST_TOL * c + floor


@pytest.mark.parametrize("name", [n for n in NAMES if _SCENES[n]["n_pts"] <= 100])
def test_against_scipys_minimum(name):
    z = load("ba.npz")
    sc = scene_of(z, name)
    _, _, info = adjusted(name, "f0")
    cs, floor = float(z[f"{name}_sp_cost"]), noise_floor(sc)
    ex = (info["cost"] - cs - floor) / max(cs, floor)
    print(f"MEASURED ba {name}: excess over scipy {ex:.3e} ({info['cost']:.12g} vs {cs:.12g})")
    assert ex <= EXCESS_TOL


@pytest.mark.parametrize("n_cam", [BR.LDS_EDGE - 1, BR.LDS_EDGE, 256])
def test_schur_row_either_side_of_64_kib(n_cam):
    """The row of S one camera's wave keeps in LDS passes 64 KiB at 228 cameras; 256 is the cap
    (72 KiB, a 1,536-square system).  The restatement runs here: the scene is too large to store."""
    sc = BR.many_cameras(n_cam)
    r = BR.solve(sc, ftol=1e-2)
    cams, X, info = adjust(sc, 1e-2)
    e0, ec = abs(info["cost0"] - r["cost0"]) / r["cost0"], abs(info["cost"] - r["cost"]) / r["cost"]
    dw = float(np.abs(cams[:, :3] - r["cams"][:, :3]).max())
    dX = float((np.linalg.norm(X - r["X"], axis=1) / np.maximum(1.0, np.linalg.norm(r["X"], axis=1))).max())
    print(f"MEASURED ba {n_cam} cameras: start cost {e0:.3e} final cost {ec:.3e} max |d omega| {dw:.3e} |dX| {dX:.3e}; "
          f"status {info['status']} accepted {info['iters']} (restatement {r['status']}, {r['iters']}, all firm "
          f"{r['all_firm']})")
    assert r["all_firm"] and info["status"] == r["status"] and info["iters"] == r["iters"]
    assert e0 <= COST_TOL and ec <= COST_TOL and dw <= CAM_TOL and dX <= PT_TOL


def test_score_not_above_the_references_recorded_run():
    z = load("ba.npz")
    name = str(z["ref_case"])
    sc = scene_of(z, name)
    cams, X, info = adjusted(name, "f0")
    reg = pose.PointRegistry()
    args = (sc["n_pts"], sc["cam_idx"], sc["pt_idx"], sc["obs"])
    before = reg.total_reprojection_error(*args, sc["cams"], sc["X"], sc["K"])
    after = reg.total_reprojection_error(*args, cams, X, sc["K"])
    print(f"MEASURED ba {name}: score {before:.6f} -> {after:.6f} (the reference: {float(z['ref_score_before']):.6f} -> "
          f"{float(z['ref_score_after']):.6f}); cost {info['cost']:.8f} (the reference's {float(z['ref_cost_after']):.8f})")
    assert abs(before - float(z["ref_score_before"])) <= 1e-9 * before
    assert after <= float(z["ref_score_after"])
    assert info["cost"] <= float(z["ref_cost_after"])


@pytest.mark.parametrize("name", ["four_cams_1fixed", "tile_11", "camlist_257"])
def test_two_runs_give_the_same_bits(name):
    sc = scene_of(load("ba.npz"), name)
    a = adjusted(name, "f2")
    b = adjust(sc, 1e-2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_device_tensors_equal_numpy_inputs():
    torch = pytest.importorskip("torch")
    name = "three_cams_2fixed"
    sc = scene_of(load("ba.npz"), name)
    a = adjusted(name, "f2")
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()
    info = {}
    ba = pose.BundleAdjustment(sc["n_cam"], sc["n_pts"], t(sc["cam_idx"]), t(sc["pt_idx"]), t(sc["obs"]), t(sc["cams"]),
                               t(sc["X"]), t(sc["K"]), fixed_cameras=[0, 1], ftol=1e-2, max_iter=BR.MAX_ITER, info=info)
    cams, X = ba.sparse_bundle_adjustment(as_device=True)
    assert cams.is_cuda and X.is_cuda and cams.dtype == torch.float64
    assert cams.cpu().numpy().tobytes() == a[0].tobytes() and X.cpu().numpy().tobytes() == a[1].tobytes()
    assert info == a[2]


def test_two_problems_alternated_on_one_context():
    z = load("ba.npz")
    names = ("tile_12", "two_cams")
    alone = [adjusted(n, "f2") for n in names]
    for _ in range(2):
        for n, ref in zip(names, alone):
            cams, X, info = adjust(scene_of(z, n), 1e-2)
            assert cams.tobytes() == ref[0].tobytes() and X.tobytes() == ref[1].tobytes() and info == ref[2]


def test_non_finite_start_and_empty_problem():
    sc = BR.nonfinite_case()
    cams, X, info = adjust(sc, 1e-2)
    assert info["status"] == 2 and info["iters"] == 0 and info["lm_iters"] == 0 and not np.isfinite(info["cost0"])
    assert cams.tobytes() == sc["cams"].tobytes() and X.tobytes() == sc["X"].tobytes()
    sc = BR.empty_case()
    cams, X, info = adjust(sc, 1e-2)
    assert info == dict(cost0=0.0, cost=0.0, status=0, iters=0, lm_iters=0, rejected_factorisations=0)
    assert cams.tobytes() == sc["cams"].tobytes() and X.tobytes() == sc["X"].tobytes()


def test_max_iter_ends_with_status_3():
    sc = scene_of(load("ba.npz"), "two_cams")
    _, _, info = adjust(sc, 0.0, max_iter=2)
    assert info["status"] == 3 and info["lm_iters"] == 2 and info["iters"] == 2
    costs = load("ba.npz")["two_cams_f0_costs"]
    assert abs(info["cost"] - costs[1]) <= COST_TOL * costs[1]


def test_python_argument_errors():
    sc = scene_of(load("ba.npz"), "two_cams")
    bad = dict(sc, cam_idx=sc["cam_idx"].copy())
    bad["cam_idx"][3] = 2
    with pytest.raises(IndexError):
        adjust(bad, 1e-2)
    bad = dict(sc, pt_idx=sc["pt_idx"].copy())
    bad["pt_idx"][0] = -1
    with pytest.raises(IndexError):
        adjust(bad, 1e-2)
    with pytest.raises(ValueError):
        adjust(sc, -1.0)
    with pytest.raises(ValueError):
        adjust(sc, float("nan"))
    with pytest.raises(ValueError):
        adjust(sc, 1e-2, max_iter=0)


def test_c_abi_argument_errors_leave_a_message():
    torch = pytest.importorskip("torch")
    ctx = _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))
    L, h = ctx.lib, ctx.handle
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    E = _abi.SFM_EINVAL
    msg = lambda: (L.sfm_last_error(h) or b"").decode()

    def ba(ci=p, pi=p, obs=p, M=4, cams=p, n_cam=2, K=p, X=p, n_pts=3, fixed=None, ftol=1e-2, mi=5, oc=p, oX=p,
           cost=None, st=None):
        return L.sfm_bundle_adjust_dev(h, ci, pi, obs, M, cams, n_cam, K, X, n_pts, fixed, ctypes.c_double(ftol), mi, oc,
                                       oX, cost, st, None)

    for kw in ({"n_cam": 0}, {"n_cam": 257}, {"n_pts": -1}, {"n_pts": (1 << 24) + 1}, {"M": -1}, {"M": (1 << 26) + 1},
               {"ci": None}, {"pi": None}, {"obs": None}, {"cams": None}, {"K": None}, {"X": None}, {"oc": None},
               {"oX": None}, {"ftol": -1e-3}, {"ftol": float("nan")}, {"mi": 0}, {"mi": 1 << 24}, {"n_pts": 0}):
        assert ba(**kw) == E and "sfm_bundle_adjust_dev" in msg(), kw
    assert L.sfm_bundle_adjust_dev(None, p, p, p, 4, p, 2, p, p, 3, None, ctypes.c_double(1e-2), 5, p, p, None, None,
                                   None) == E
    # the optional pointers may be null: four observations of point 0 by camera 0 (all zeros) — the
    # start cost is not finite (0 / 0), so everything comes back unchanged
    st = torch.full((4,), 9, dtype=torch.int32, device="cuda")
    assert ba(oc=buf[1024:].data_ptr(), oX=buf[2048:].data_ptr(), st=st.data_ptr()) == _abi.SFM_OK
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [2, 0, 0, 0]


def test_integration_snippet_runs_as_written(tmp_path, monkeypatch, capsys):
    """INTEGRATION.md §1's Runner.py:290-306 block, executed verbatim on a registry built the way
    perform builds it."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "pose.BundleAdjustment(" in b]
    assert len(blocks) == 1
    z = load("ba.npz")
    sc = scene_of(z, "three_cams_2fixed")
    reg = pose.PointRegistry()
    for f in range(sc["n_cam"]):
        sel = sc["cam_idx"] == f
        reg.add_points(sc["X"][sc["pt_idx"][sel]], sc["obs"][sel], f)

    class Runner:
        global_poses = [(c[:3].reshape(3, 1), c[3:].reshape(3, 1)) for c in sc["cams"]]
        global_K = list(sc["K"])
        model_name = "adjusted"

    monkeypatch.chdir(tmp_path)
    os.mkdir("output")
    ns = {"pose": pose, "reg": reg, "self": Runner()}
    exec(compile(blocks[0], "INTEGRATION.md", "exec"), ns)
    out = capsys.readouterr().out
    before, after = (float(m) for m in re.findall(r"Total reprojection error (?:before|after) BA: (\S+)", out))
    print(f"MEASURED ba snippet: {before:.6f} -> {after:.6f}")
    assert after < before
    saved = np.load("output/adjusted.npz")
    assert saved["p3d"].tobytes() == np.ascontiguousarray(ns["optimized_points_3D"]).tobytes()
    assert saved["p3d"].tobytes() == reg.points_3d.tobytes() and len(saved["pt_idx"]) == len(sc["obs"])
    with pytest.raises(ValueError):
        reg.set_points_3d(np.zeros((len(reg) + 1, 3)))


# ---------------- cameras that orbit the cloud: rotations beyond pi / 2 (BR.ring_cases) ----------------
# The fixture's cameras turn by 0.52 rad at most, so k_ba_finish's rodrigues_inv never left its
# first branch there.  The restatement solves these scenes here (0.01 to 0.15 s each); their
# conditions are asserted on the CPU (tests/test_ba_cpu.py).  The bounds are the ones above.

_RINGS = BR.ring_cases()
_ring = {}


def ring_adjusted(name, tag):
    """One device run and one restatement run per (ring case, ftol), shared by the tests (never modified)."""
    if (name, tag) not in _ring:
        _ring[name, tag] = adjust(_RINGS[name], FTOLS[tag]) + (BR.solve(_RINGS[name], ftol=FTOLS[tag]),)
    return _ring[name, tag]


def rotations(cams):
    return np.array([BR.rodrigues_to_matrix(w) for w in np.asarray(cams)[:, :3]])


@pytest.mark.parametrize("tag", list(FTOLS))
@pytest.mark.parametrize("name", list(_RINGS))
def test_ring_against_the_restatement(name, tag):
    sc = _RINGS[name]
    cams, X, info, r = ring_adjusted(name, tag)
    floor = noise_floor(sc)
    e0 = abs(info["cost0"] - r["cost0"]) / r["cost0"]
    ec = max(abs(info["cost"] - r["cost"]) - floor, 0.0) / max(r["cost"], floor)
    c, th = BR.rotation_angles(cams)
    print(f"MEASURED ba {name} ftol {FTOLS[tag]:g}: start cost {e0:.3e} final cost {ec:.3e} ({info['cost']:.10g} vs "
          f"{r['cost']:.10g}); status {info['status']} (restatement {r['status']}) accepted {info['iters']} (restatement "
          f"{r['iters']}, firm {r['firm']}, all firm {r['all_firm']}); {int((c < 0).sum())} of {len(c)} cameras returned "
          f"through rodrigues_inv's c < 0 branch, min pi - theta {np.pi - th.max():.3e}")
    assert e0 <= COST_TOL and ec <= COST_TOL
    assert info["cost"] <= info["cost0"]
    if r["all_firm"]:
        assert info["status"] == r["status"] and info["iters"] == r["iters"]
    assert info["iters"] >= r["firm"] and info["rejected_factorisations"] == 0
    ca, pa = BR.active(sc)
    assert cams[~ca].tobytes() == sc["cams"][~ca].tobytes() and pa.all()
    assert (np.sqrt((cams[ca, :3] ** 2).sum(1)) <= np.pi + 1e-12).all()
    assert (c[ca] < 0).sum() >= (3 if name != "ring5_quarter" else 1)   # free cameras through the second branch
    dR = float(np.abs(rotations(cams) - rotations(r["cams"])).max())
    dw = float(np.abs(cams[:, :3] - r["cams"][:, :3]).max())
    dt = float((np.linalg.norm(cams[:, 3:] - r["cams"][:, 3:], axis=1) / np.maximum(1.0, np.linalg.norm(r["cams"][:, 3:], axis=1))).max())
    dX = float((np.linalg.norm(X - r["X"], axis=1) / np.maximum(1.0, np.linalg.norm(r["X"], axis=1))).max())
    print(f"MEASURED ba {name} ftol {FTOLS[tag]:g}: max |dR| {dR:.3e} |d omega| {dw:.3e} |dt| {dt:.3e} |dX| {dX:.3e}")
    assert dR <= CAM_TOL and dw <= CAM_TOL and dt <= CAM_TOL and dX <= PT_TOL


@pytest.mark.parametrize("tag", list(FTOLS))
def test_ring_non_principal_start_comes_back_principal(tag):
    p, q = _RINGS["ring9"], _RINGS["ring9_nonprincipal"]
    cams, X, info, _ = ring_adjusted("ring9_nonprincipal", tag)
    _, _, pinfo, pr = ring_adjusted("ring9", tag)
    moved = sorted(BR.NONPRINCIPAL_CAMS)
    assert (np.sqrt((q["cams"][moved, :3] ** 2).sum(1)) > np.pi).all()
    e0 = abs(info["cost0"] - pr["cost0"]) / pr["cost0"]
    dR = float(np.abs(rotations(cams) - rotations(pr["cams"])).max())
    dw = float(np.abs(cams[:, :3] - pr["cams"][:, :3]).max())
    print(f"MEASURED ba ring9_nonprincipal ftol {FTOLS[tag]:g}: start cost against ring9's restatement {e0:.3e} (the device's "
          f"own two starts differ by {abs(info['cost0'] - pinfo['cost0']) / pinfo['cost0']:.3e}); cameras against ring9's "
          f"restatement max |dR| {dR:.3e} |d omega| {dw:.3e}")
    assert e0 <= COST_TOL
    fixed = q["fixed"].astype(bool)
    assert cams[fixed].tobytes() == q["cams"][fixed].tobytes()
    assert (np.sqrt((cams[~fixed, :3] ** 2).sum(1)) <= np.pi + 1e-12).all()
    assert dR <= CAM_TOL and dw <= CAM_TOL


def test_ring_two_runs_give_the_same_bits():
    a = ring_adjusted("ring9", "f2")
    b = adjust(_RINGS["ring9"], 1e-2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
