"""CPU: the numpy restatement of the bundle-adjustment rule (tests/ba_ref.py)
against itself (block / Schur form == dense form), against scipy's recorded tight-tolerance
minimum and against the reference's own recorded run (tests/golden/ba.npz), plus the conditions
the GPU comparisons of tests/test_gpu_ba.py rely on.  No test imports the reference."""
from __future__ import annotations

import numpy as np
import pytest

from tests import ba_ref as BR
from tests import registry_ref as RR
from tests.golden_util import load

_SCENES = BR.cases()
NAMES = list(_SCENES)
SMALL = [n for n in NAMES if not n.startswith(("camlist", "obs_2000"))]   # the dense form stays small


def scene_of(z, name):
    g = lambda k: z[f"{name}_{k}"]
    return dict(n_cam=int(g("n_cam")), n_pts=int(g("n_pts")), cam_idx=g("cam_idx").astype(np.int64),
                pt_idx=g("pt_idx").astype(np.int64), obs=g("obs"), cams=g("cams"), K=g("K"), X=g("X"), fixed=g("fixed"))


def noise_floor(sc):
    """A cost below this is rounding: M squared residuals, each a pixel coordinate evaluated to a
    few ulps."""
    return len(sc["obs"]) * (4 * np.finfo(np.float64).eps * np.abs(sc["obs"]).max()) ** 2


def test_fixture_holds_the_scenes_of_the_builders():
    z = load("ba.npz")
    assert [str(n) for n in z["names"]] == NAMES
    for name, sc in _SCENES.items():
        f = scene_of(z, name)
        assert f["n_cam"] == sc["n_cam"] and f["n_pts"] == sc["n_pts"]
        assert np.array_equal(f["cam_idx"], sc["cam_idx"]) and np.array_equal(f["pt_idx"], sc["pt_idx"])
        for k in ("obs", "cams", "X"):  # (libm's sin / cos may differ in the last place between machines)
            assert np.allclose(f[k], sc[k], rtol=1e-12, atol=1e-12), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_schur_step_equals_dense_step(name):
    """One step of each form from the same linearisation, at two dampings."""
    sc = scene_of(load("ba.npz"), name)
    R = np.array([RR.rodrigues_to_matrix(sc["cams"][k, :3]) for k in range(sc["n_cam"])])
    r, Jc, Jp = BR.linearise(sc, R, sc["cams"][:, 3:], sc["X"])
    for lam in (1e-3, 10.0):
        dc, dX = BR.step_schur(sc, r, Jc, Jp, lam)
        ec, eX = BR.step_dense(sc, r, Jc, Jp, lam)
        scale = max(np.abs(ec).max(), np.abs(eX).max())
        err = max(np.abs(dc - ec).max(), np.abs(dX - eX).max()) / scale
        print(f"{name} lambda {lam:g}: forms differ by {err:.3e} of the step")
        assert err < 1e-8


@pytest.mark.parametrize("name", SMALL)
def test_two_forms_agree_on_the_whole_run(name):
    z = load("ba.npz")
    sc = scene_of(z, name)
    a = BR.solve(sc, ftol=1e-2, form="schur")
    b = BR.solve(sc, ftol=1e-2, form="dense")
    tol = 1e-9 * a["cost"] + noise_floor(sc)
    print(f"{name}: schur {a['cost']:.12g} dense {b['cost']:.12g} accepted {a['iters']} / {b['iters']}")
    assert abs(a["cost"] - b["cost"]) <= tol and a["iters"] == b["iters"] and a["status"] == b["status"]
    # and the recorded run is this one
    assert abs(a["cost"] - float(z[f"{name}_f2_cost"])) <= tol and a["iters"] == int(z[f"{name}_f2_iters"])


@pytest.mark.parametrize("name", [n for n in NAMES if _SCENES[n]["n_pts"] <= 100])
def test_restatement_reaches_scipys_minimum(name):
    z = load("ba.npz")
    sc = scene_of(z, name)
    c, cs = float(z[f"{name}_f0_cost"]), float(z[f"{name}_sp_cost"])
    ex = (c - cs) / max(cs, noise_floor(sc))
    print(f"{name}: restatement {c:.12g} scipy {cs:.12g} excess {ex:.3e}")
    assert c - cs <= 1e-9 * cs + noise_floor(sc)
    assert int(z[f"{name}_f0_status"]) in (BR.ST_CONVERGED, BR.ST_LAMBDA)
    assert int(z[f"{name}_f0_rejected"]) == 0   # no Cholesky failed
    costs = z[f"{name}_f0_costs"]
    assert len(costs) == int(z[f"{name}_f0_iters"]) and (np.diff(np.concatenate([[float(z[f"{name}_f0_cost0"])], costs])) < 0).all()


def test_not_above_the_references_recorded_run():
    z = load("ba.npz")
    name = str(z["ref_case"])
    sc = scene_of(z, name)
    c0, cref = float(z[f"{name}_f0_cost"]), float(z["ref_cost_after"])
    print(f"{name}: restatement at ftol 0 {c0:.10g}; the reference's after-BA cost {cref:.10g}; its scores "
          f"{float(z['ref_score_before']):.6f} -> {float(z['ref_score_after']):.6f}")
    assert c0 <= cref
    assert abs(BR.cost_of(sc, z["ref_cams"], z["ref_X"]) - cref) <= 1e-9 * cref
    # what the GPU test relies on: the score the runner prints (the mean over the first num_points
    # observations) is not above the reference's at the restatement's minimum either
    r = BR.solve(sc, ftol=0.0)
    score = RR.reprojection_errors(sc["n_pts"], sc["cam_idx"], sc["pt_idx"], sc["obs"], r["cams"], r["X"], sc["K"]).mean()
    print(f"restatement's score after BA {score:.6f}")
    assert score <= float(z["ref_score_after"])
    # every camera free and half the points observed once: the reference's situation
    assert not sc["fixed"].any() and (np.bincount(sc["pt_idx"], minlength=sc["n_pts"]) == 1).sum() >= sc["n_pts"] // 2


def test_fixed_and_unobserved_rows_do_not_move():
    z = load("ba.npz")
    sc = scene_of(z, "idle_rows")
    ca, pa = BR.active(sc)
    assert (~ca).sum() == 3 and (~pa).sum() == 1   # two fixed cameras, one idle camera, one idle point
    for tag in ("f2", "f0"):
        cams = z[f"idle_rows_{tag}_cams"]
        assert cams[~ca].tobytes() == sc["cams"][~ca].tobytes()
        assert not np.array_equal(cams[ca], sc["cams"][ca])
        assert z[f"idle_rows_{tag}_X"][~pa].tobytes() == sc["X"][~pa].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_rodrigues_round_trip_of_the_outputs(name):
    z = load("ba.npz")
    for tag in ("f2", "f0"):
        for w in z[f"{name}_{tag}_cams"][:, :3]:
            assert np.sqrt(w @ w) <= np.pi + 1e-12
            back = RR.rodrigues_to_vector(RR.rodrigues_to_matrix(w)).reshape(3)
            assert np.abs(back - w).max() < 1e-12


def test_conditions_of_the_gpu_comparisons():
    z = load("ba.npz")
    M = {n: len(z[f"{n}_cam_idx"]) for n in NAMES}
    assert [M[f"obs_{k}"] for k in (255, 256, 257)] == [255, 256, 257] and M["obs_2000"] == 2000
    for k in (255, 256, 257):
        assert (z[f"camlist_{k}_cam_idx"] == 1).sum() == k
    assert [int(z[f"tile_{n}_n_cam"]) * 6 for n in (10, 11, 12)] == [60, 66, 72]   # around BR.TILE = 64
    sc = scene_of(z, "four_cams_1fixed")
    pairs = sc["cam_idx"] * sc["n_pts"] + sc["pt_idx"]
    assert len(np.unique(pairs)) < len(pairs)   # a duplicated (c, j)
    per_point = np.bincount(scene_of(z, "tile_10")["pt_idx"])
    assert {1, 2, 10} <= set(per_point.tolist())
    assert [int(scene_of(z, n)["fixed"].sum()) for n in ("three_cams_free", "two_cams", "three_cams_2fixed")] == [0, 1, 2]
    sc = scene_of(z, "exact_cam")
    R = np.array([RR.rodrigues_to_matrix(sc["cams"][k, :3]) for k in range(3)])
    r, _, _ = BR.linearise(sc, R, sc["cams"][:, 3:], sc["X"], jac=False)
    assert np.abs(r[sc["cam_idx"] == 2]).max() < 1e-10 < np.abs(r[sc["cam_idx"] != 2]).max()
    # every run at the reference's ftol is free of marginal comparisons: status and accepted steps are
    # compared exactly there; at ftol = 0 only the one-camera case is, and `firm` bounds the accepted steps from below
    assert all(bool(z[f"{n}_f2_all_firm"]) for n in NAMES)
    assert all(int(z[f"{n}_f2_status"]) == BR.ST_CONVERGED for n in NAMES)
    assert all(int(z[f"{n}_f0_firm"]) >= 3 for n in NAMES)
    # the start that is not finite, and the empty problem
    assert BR.solve(BR.nonfinite_case())["status"] == BR.ST_NONFINITE
    e = BR.solve(BR.empty_case())
    assert e["status"] == 0 and e["cost"] == 0.0 and e["iters"] == 0


# ---------------- the ring scenes: rotations beyond pi / 2 (BR.ring_cases, solved here) ----------------

_RINGS = BR.ring_cases()
_ring_runs = {}


def ring_run(name, ftol, form="schur"):
    """One solve per (case, ftol, form), shared by the tests (never modified)."""
    if (name, ftol, form) not in _ring_runs:
        _ring_runs[name, ftol, form] = BR.solve(_RINGS[name], ftol=ftol, form=form)
    return _ring_runs[name, ftol, form]


def test_scene_defaults_are_the_arc_and_tilt_of_the_fixture():
    """arc = 0.5 and tilt = 1 are what scene() always built: the same bits."""
    a = BR.scene(5, 4, 30, BR._mixed(4), fixed=(0,), dup=5)
    b = BR.scene(5, 4, 30, BR._mixed(4), fixed=(0,), dup=5, arc=0.5, tilt=1.0)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.mark.parametrize("ftol", [1e-2, 0.0])
@pytest.mark.parametrize("name", list(_RINGS))
def test_ring_two_forms_agree(name, ftol):
    sc = _RINGS[name]
    a, b = ring_run(name, ftol), ring_run(name, ftol, "dense")
    tol = 1e-9 * a["cost"] + noise_floor(sc)
    dc = float(np.abs(a["cams"] - b["cams"]).max())
    print(f"{name} ftol {ftol:g}: schur {a['cost']:.12g} dense {b['cost']:.12g} accepted {a['iters']} / {b['iters']} "
          f"status {a['status']} / {b['status']} all firm {a['all_firm']}; cameras differ by {dc:.3e}")
    assert abs(a["cost"] - b["cost"]) <= tol and a["rejected"] == b["rejected"] == 0
    assert dc <= 1e-9   # two fixed cameras: no gauge freedom (measured 9.3e-12 at most, ring9_flat at ftol 0)
    if ftol:            # free of marginal comparisons: status and accepted steps are compared exactly
        assert a["all_firm"] and a["iters"] == b["iters"] == 2 and a["status"] == b["status"] == BR.ST_CONVERGED
    else:
        assert a["firm"] >= 3 and a["status"] in (BR.ST_CONVERGED, BR.ST_LAMBDA)


def test_ring_conditions_of_the_gpu_comparisons():
    """What tests/test_gpu_ba.py and test_gpu_registry.py rely on: the output cameras cross pi / 2
    (rodrigues_inv's symmetric branch, c < 0) without coming so close to pi that the sign of the
    vector is rounding.  Measured: ring9 6 of 9 cameras with c < 0, min pi - theta 1.2e-3; ring9_flat
    5 of 9, 8.0e-4, theta 1.5726 and 1.5693 either side of pi / 2; ring8 4 of 8; ring5_quarter 1 of 5."""
    assert all(sc["n_cam"] <= 9 and len(sc["obs"]) <= 192 and int(sc["fixed"].sum()) == 2 for sc in _RINGS.values())
    assert len(_RINGS["ring9"]["obs"]) == 192
    for name in _RINGS:
        for ftol in (1e-2, 0.0):
            c, th = BR.rotation_angles(ring_run(name, ftol)["cams"])
            print(f"{name} ftol {ftol:g}: {(c < 0).sum()} of {len(c)} cameras with c < 0, min pi - theta "
                  f"{np.pi - th.max():.3e}, theta {np.round(th, 4).tolist()}")
            assert (c < 0).sum() >= (4 if name != "ring5_quarter" else 1)
            assert np.pi - th.max() >= 1e-4     # comparing vectors is safe
    for ftol in (1e-2, 0.0):
        _, th = BR.rotation_angles(ring_run("ring9_flat", ftol)["cams"])
        near = th[np.abs(th - np.pi / 2) < 5e-3]
        assert (near < np.pi / 2).any() and (near > np.pi / 2).any()   # an output camera on each side
    sc = _RINGS["ring9_flat"]
    assert (sc["cams"][:, [0, 2]][sc["fixed"].astype(bool)] == 0).all() and not sc["cams"][4, :3].any()  # the identity
    _, th0 = BR.rotation_angles(_RINGS["ring5_quarter"]["cams"])
    assert (np.abs(th0[[0, 4]] - np.pi / 2) < 5e-3).all()   # the end cameras start beside pi / 2


def test_ring_non_principal_start_is_the_principal_problem():
    p, q = _RINGS["ring9"], _RINGS["ring9_nonprincipal"]
    moved = sorted(BR.NONPRINCIPAL_CAMS)
    assert not p["fixed"][moved].any()
    for k in p:
        if k != "cams":
            assert np.asarray(p[k]).tobytes() == np.asarray(q[k]).tobytes()
    same = np.ones(9, bool)
    same[moved] = False
    assert p["cams"][same].tobytes() == q["cams"][same].tobytes() and p["cams"][:, 3:].tobytes() == q["cams"][:, 3:].tobytes()
    nq = np.sqrt((q["cams"][moved, :3] ** 2).sum(1))
    np_ = np.sqrt((p["cams"][moved, :3] ** 2).sum(1))
    assert nq[0] > np.pi and nq[1] > 2 * np.pi
    assert np.allclose(np.abs(nq - np_), [2 * np.pi - 2 * np_[0], 2 * np.pi], atol=1e-12)   # theta - 2 pi, theta + 2 pi
    Rp = np.array([RR.rodrigues_to_matrix(w) for w in p["cams"][moved, :3]])
    Rq = np.array([RR.rodrigues_to_matrix(w) for w in q["cams"][moved, :3]])
    assert np.abs(Rp - Rq).max() < 1e-14
    for ftol in (1e-2, 0.0):
        a, b = ring_run("ring9", ftol), ring_run("ring9_nonprincipal", ftol)
        rel0, rel = abs(a["cost0"] - b["cost0"]) / a["cost0"], abs(a["cost"] - b["cost"]) / a["cost"]
        print(f"non-principal start, ftol {ftol:g}: start cost differs by {rel0:.3e}, final by {rel:.3e}")
        assert rel0 <= 1e-13 and rel <= 1e-13
        assert (np.sqrt((b["cams"][:, :3] ** 2).sum(1))[~p["fixed"].astype(bool)] <= np.pi + 1e-12).all()
