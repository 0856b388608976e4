"""GPU: the two-view geometry record on the device (sequence.two_view_geometry, twoview.hip) against
the numpy restatement of tests/two_view_ref.py: hstat, hkeep and pstat byte for byte, the winning H
through its transfer residuals, (R, t) within the tolerance tests/test_gpu_pose.py uses for the
candidates.  The conditions the cases must meet (every decision farther from equality than the
last bits of a fit can move it, both branches of the stop test, the class of every scene kind) are
asserted on the CPU in tests/test_two_view_cpu.py.

H_RES_BOUND: measured on the MI355X, the device's winning H and the restatement's give every valid
match of every case the same transfer residuals to the last bit (largest difference 0: the fit has
the restatement's operation order, and float64 division and square root round alike).  The bound
keeps the six orders of magnitude tests/test_gpu_verify.py gives F, counted from one unit in the
last place of a 1 px residual: 1e6 x 2.2e-16 = 2.2e-10 px (relative to the residual above 1 px).
Planted motion: the restatement's own error on the same integer-pixel data, times two (the device
differs from numpy only in the eigen-solver's last bits); the restatement measures |dR| 2.3e-3 to
5.0e-3 and |dt| 8.4e-3 to 1.24e-1 (n = 8), so the bounds are 4.5e-3 to 9.9e-3 and 1.7e-2 to 2.5e-1.
Every figure is printed before its assertion."""
from __future__ import annotations

import types

import numpy as np
import pytest

from tests import pose_ref as PR
from tests import two_view_ref as TV
from tests import verify_ref as VR

pytestmark = pytest.mark.gpu

H_RES_BOUND = 1e6 * 2.220446049250313e-16
RT_TOL = min(1e-8, 100 * 3.3e-14)   # tests/test_gpu_pose.py's tolerance for R, t


def table_of(tab):
    import torch
    dev = torch.device("cuda", 0)
    return types.SimpleNamespace(count=torch.from_numpy(np.ascontiguousarray(tab["count"], np.int32)).to(dev),
                                 xy=torch.from_numpy(np.ascontiguousarray(tab["xy"], np.int32)).to(dev))


def context():
    from sfmfromscratch_amd import _abi
    from sfmfromscratch_amd._native import context_for
    return context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), 0)


def up(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(torch.device("cuda", 0))


def run_h(tab, iters=TV.ITERS, threshold=TV.THRESHOLD, confidence=None, seed=TV.SEED, attempt=None, want_keep=True,
          table=None):
    """sfm_homography_matches_dev by hand -> dict(H [P, 3, 3], hkeep [P, cap] or None, hstat [P, 4])."""
    import torch
    t = table or table_of(tab)
    dev = t.xy.device
    P, cap = len(tab["pairs"]), tab["cap"]
    H = torch.zeros((P, 9), dtype=torch.float64, device=dev)
    hkeep = torch.full((P, cap), 7, dtype=torch.uint8, device=dev) if want_keep else None
    hstat = torch.full((P, 4), 99, dtype=torch.int32, device=dev)
    context().homography_matches_dev(t.xy, t.count, up(tab["pairs"], np.int32), up(tab["matches"], np.int32),
                                     up(tab["nmatch"], np.int32), None if attempt is None else up(attempt, np.int32),
                                     iters, threshold, seed, TV.stop_ratios(confidence, iters) if iters else None,
                                     H, hkeep, hstat)
    torch.cuda.synchronize()
    return dict(H=H.cpu().numpy().reshape(-1, 3, 3), hkeep=None if hkeep is None else hkeep.cpu().numpy(),
                hstat=hstat.cpu().numpy())


def run_pose(tab, keep, F, K, attempt=None, cos2_min=TV.COS2_MIN, table=None):
    """sfm_two_view_pose_dev by hand -> dict(pose [P, 12], pstat [P, 4])."""
    import torch
    t = table or table_of(tab)
    dev = t.xy.device
    P, nimg = len(tab["pairs"]), len(tab["count"])
    K = np.broadcast_to(np.asarray(K, np.float64), (nimg, 3, 3)) if np.ndim(K) == 2 else np.asarray(K, np.float64)
    pose = torch.zeros((P, 12), dtype=torch.float64, device=dev)
    pstat = torch.full((P, 4), 99, dtype=torch.int32, device=dev)
    context().two_view_pose_dev(t.xy, t.count, up(tab["pairs"], np.int32), up(tab["matches"], np.int32),
                                up(tab["nmatch"], np.int32), up(keep, np.uint8), up(np.reshape(F, (P, 9)), np.float64),
                                up(K.reshape(nimg, 9), np.float64), None if attempt is None else up(attempt, np.int32),
                                cos2_min, pose, pstat)
    torch.cuda.synchronize()
    return dict(pose=pose.cpu().numpy(), pstat=pstat.cpu().numpy())


def assert_h_equals_restatement(g, tab, e):
    assert np.array_equal(g["hstat"], e["hstat"]), (g["hstat"].tolist(), e["hstat"].tolist())
    if g["hkeep"] is not None:
        assert np.array_equal(g["hkeep"], e["hkeep"])
    for p in range(len(tab["pairs"])):
        if not np.isfinite(e["H"][p]).all():
            assert np.isnan(g["H"][p]).all(), p
            continue
        _, _, valid, p1, p2 = TV.correspondences(tab, p)
        with np.errstate(all="ignore"):
            rd = TV.transfer_residuals(g["H"][p], p1[valid], p2[valid])
            rr = TV.transfer_residuals(e["H"][p], p1[valid], p2[valid])
            ok = np.isfinite(rr)
            worst = float((np.abs(rd - rr)[ok] / np.maximum(1.0, rr[ok])).max())
        print(f"MEASURED {tab['name']} pair {p}: transfer residuals of H against the restatement's {worst:.3e} px")
        assert worst <= H_RES_BOUND and np.isfinite(rd[ok]).all()


# ---------------------------------------------------------------- the homography call
@pytest.mark.parametrize("confidence", [None, TV.CONFIDENCE])
@pytest.mark.parametrize("name", list(TV.SINGLE))
def test_homography_equals_the_restatement(name, confidence):
    """n = 3 (not attempted), 4, 5, 40, 255, 257, 300, 2560, 2561 (around one staging chunk) and 2700
    with 60 rows outside [0, count); 600 samples, fixed and with the 0.98 table."""
    tab = TV.single(name)
    g = run_h(tab, confidence=confidence)
    e = TV.homography(tab, stop=TV.stop_ratios(confidence))
    print(name, confidence, g["hstat"].tolist())
    assert_h_equals_restatement(g, tab, e)
    if confidence:
        assert g["hstat"][0, 2] == TV.STOPS_EARLY.get(name, TV.ITERS if name != "n3" else 0)


@pytest.mark.parametrize("iters", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("name", ["n5", "n40", "n257", "n2561", "n2700_bad"])
def test_iteration_counts_around_a_round(name, iters):
    tab = TV.single(name)
    table = table_of(tab)
    for confidence in (None, TV.CONFIDENCE):
        g = run_h(tab, iters=iters, confidence=confidence, table=table)
        e = TV.homography(tab, iters=iters, stop=TV.stop_ratios(confidence, iters) if iters else None)
        assert_h_equals_restatement(g, tab, e)
    if iters == 0:
        assert g["hstat"].tolist() == [[0, -1, 0, 0]] and not g["hkeep"].any() and np.isnan(g["H"]).all()


@pytest.mark.parametrize("threshold", [0.0, -1.0, float("nan"), float("inf")])
def test_edge_thresholds(threshold):
    tab = TV.mixed()
    g = run_h(tab, iters=VR.MIXED_ITERS, threshold=threshold)
    e = TV.homography(tab, iters=VR.MIXED_ITERS, threshold=threshold)
    assert np.array_equal(g["hstat"], e["hstat"]) and np.array_equal(g["hkeep"], e["hkeep"])
    attempted = e["hstat"][:, 0] >= 0
    if threshold == float("inf"):
        for p in np.flatnonzero(attempted):
            _, n, valid, _, _ = TV.correspondences(tab, p)
            assert g["hstat"][p, 0] <= valid.sum()   # w == 0 still admits nothing
    else:
        assert not g["hkeep"].any() and np.isnan(g["H"]).all()
        assert g["hstat"][attempted].tolist() == [[0, 0, VR.MIXED_ITERS, 0]] * int(attempted.sum())
    assert g["hstat"][~attempted].tolist() == [[-1, -1, 0, 0]] * int((~attempted).sum())


def test_one_call_of_mixed_pairs_attempt_and_null_hkeep():
    """verify_ref.mixed's kinds of bad pair in one call: the restatement's bytes, each pair what it
    gets alone; attempt null, all 0 and mixed; hkeep null."""
    tab = TV.mixed()
    table = table_of(tab)
    P = len(tab["pairs"])
    kw = dict(iters=VR.MIXED_ITERS, confidence=TV.CONFIDENCE, table=table)
    stop = TV.stop_ratios(TV.CONFIDENCE, VR.MIXED_ITERS)
    g = run_h(tab, **kw)
    assert_h_equals_restatement(g, tab, TV.homography(tab, iters=VR.MIXED_ITERS, stop=stop))
    for p in range(P):
        one = VR.sub_table(tab, [p], f"tv_mixed_{p}")
        a = run_h(one, **kw)
        assert a["hkeep"].tobytes() == g["hkeep"][p].tobytes() and a["hstat"].tobytes() == g["hstat"][p].tobytes()
        assert a["H"].tobytes() == g["H"][p].tobytes()
    none = run_h(tab, attempt=np.zeros(P, np.int32), **kw)
    assert none["hstat"].tolist() == [[-1, -1, 0, 0]] * P and not none["hkeep"].any() and np.isnan(none["H"]).all()
    att = np.array([1, 1, 0, 5, 1, 1, 1, 0, -1], np.int32)
    some = run_h(tab, attempt=att, **kw)
    assert_h_equals_restatement(some, tab, TV.homography(tab, iters=VR.MIXED_ITERS, stop=stop, attempt=att))
    for p in range(P):
        src = g if att[p] else none
        assert some["hstat"][p].tobytes() == src["hstat"][p].tobytes()
        assert some["H"][p].tobytes() == src["H"][p].tobytes()
    nokeep = run_h(tab, want_keep=False, **kw)
    assert nokeep["hkeep"] is None and nokeep["hstat"].tobytes() == g["hstat"].tobytes()
    assert nokeep["H"].tobytes() == g["H"].tobytes()


def test_determinism_permutation_and_split():
    tab = TV.mixed()
    table = table_of(tab)
    kw = dict(iters=VR.MIXED_ITERS, confidence=TV.CONFIDENCE, table=table)
    raw = lambda r: r["H"].tobytes() + r["hkeep"].tobytes() + r["hstat"].tobytes()
    a, b = run_h(tab, **kw), run_h(tab, **kw)
    assert raw(a) == raw(b)
    perm, order = VR.permuted_pairs(tab, 9)
    q = run_h(perm, **kw)
    assert q["hkeep"].tobytes() == a["hkeep"][order].tobytes() and q["hstat"].tobytes() == a["hstat"][order].tobytes()
    assert q["H"].tobytes() == a["H"][order].tobytes()
    P = len(tab["pairs"])
    lo = run_h(VR.sub_table(tab, np.arange(4), "tv_lo"), **kw)
    hi = run_h(VR.sub_table(tab, np.arange(4, P), "tv_hi"), **kw)
    assert lo["hkeep"].tobytes() + hi["hkeep"].tobytes() == a["hkeep"].tobytes()
    assert lo["hstat"].tobytes() + hi["hstat"].tobytes() == a["hstat"].tobytes()
    assert lo["H"].tobytes() + hi["H"].tobytes() == a["H"].tobytes()
    assert run_h(tab, seed=6, **kw)["hstat"].tobytes() != a["hstat"].tobytes()


# ---------------------------------------------------------------- the pose call
def assert_pose_equals_restatement(g, e, what):
    assert np.array_equal(g["pstat"], e["pstat"]), (what, g["pstat"].tolist(), e["pstat"].tolist())
    for p in range(len(e["pstat"])):
        if e["pstat"][p, 1] < 0:
            assert np.isnan(g["pose"][p]).all(), (what, p)
            continue
        d = float(np.abs(g["pose"][p] - e["pose"][p]).max())
        print(f"MEASURED {what} pair {p}: |d(R, t)| against the restatement {d:.3e}")
        assert d <= RT_TOL


@pytest.mark.parametrize("own_intrinsics", [False, True])
@pytest.mark.parametrize("name", list(TV.POSE))
def test_pose_equals_the_restatement(name, own_intrinsics):
    """Every case of the CPU test, with one K for all slots and with K per slot (two different
    intrinsics); pstat exact, (R, t) within test_gpu_pose's tolerance."""
    K2 = TV.K_OTHER if own_intrinsics else PR.K_SCENE
    tab, v = TV.pose_case(name, K2)
    K = np.stack([K2, PR.K_SCENE, PR.K_SCENE]) if own_intrinsics else PR.K_SCENE
    att = v["stat"][:, 3]
    g = run_pose(tab, v["keep"], v["F"], K, attempt=att)
    e = TV.two_view_pose(tab, v["keep"], v["F"], K, attempt=att)
    print(name, own_intrinsics, g["pstat"].tolist())
    assert_pose_equals_restatement(g, e, name)
    # attempt null: F decides alone (a pair that was not verified still has its winner's F)
    g0 = run_pose(tab, v["keep"], v["F"], K)
    assert_pose_equals_restatement(g0, TV.two_view_pose(tab, v["keep"], v["F"], K), name)


@pytest.mark.parametrize("name", TV.PLANTED)
def test_planted_motion(name):
    tab, v = TV.pose_case(name)
    g = run_pose(tab, v["keep"], v["F"], PR.K_SCENE)
    e = TV.two_view_pose(tab, v["keep"], v["F"], PR.K_SCENE)
    want_t = TV.T_TRUE / np.linalg.norm(TV.T_TRUE)
    err = lambda r: (np.abs(r["pose"][0, :9].reshape(3, 3) - TV.R_TRUE).max(), np.abs(r["pose"][0, 9:] - want_t).max())
    (gR, gt), (eR, et) = err(g), err(e)
    print(f"MEASURED {name}: device |dR| {gR:.3e} |dt| {gt:.3e}; restatement |dR| {eR:.3e} |dt| {et:.3e}")
    assert gR <= 2 * eR and gt <= 2 * et


def test_pose_of_pairs_without_points_or_without_F():
    tab, v = TV.pose_case("g64")
    zero = run_pose(tab, np.zeros_like(v["keep"]), v["F"], PR.K_SCENE)
    assert zero["pstat"].tolist() == [[0, -1, 0, 0]] and np.isnan(zero["pose"]).all()
    assert np.array_equal(zero["pstat"], TV.two_view_pose(tab, np.zeros_like(v["keep"]), v["F"], PR.K_SCENE)["pstat"])
    for bad in (np.nan, np.inf):
        F = v["F"].copy()
        F[0, 1, 2] = bad
        r = run_pose(tab, v["keep"], F, PR.K_SCENE)
        assert r["pstat"].tolist() == [[-1, -1, 0, 0]] and np.isnan(r["pose"]).all()
    off = run_pose(tab, v["keep"], v["F"], PR.K_SCENE, attempt=np.zeros(1, np.int32))
    assert off["pstat"].tolist() == [[-1, -1, 0, 0]] and np.isnan(off["pose"]).all()
    # the mixed table's bad pairs with a finite F everywhere: slots out of range and a == b are not
    # attempted, rows outside [0, count) are no points
    t = TV.mixed()
    P = len(t["pairs"])
    keep = np.ones((P, t["cap"]), np.uint8)
    F = np.broadcast_to(v["F"][0], (P, 3, 3)).copy()
    g = run_pose(t, keep, F, PR.K_SCENE)
    e = TV.two_view_pose(t, keep, F, PR.K_SCENE)
    print("mixed pstat", g["pstat"].tolist())
    assert np.array_equal(g["pstat"][:, 0] < 0, e["pstat"][:, 0] < 0)   # (this F fits none of these pairs: the
    assert np.array_equal(g["pstat"][:, 3], e["pstat"][:, 3])           # counts have no margin, the points do)
    assert (g["pstat"][[4, 5, 6]] == [-1, -1, 0, 0]).all() and g["pstat"][7, 3] == 90 and g["pstat"][1, 3] == 0


# ---------------------------------------------------------------- the Python path
def triple_of(tab, dev):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(tab["matches"])).to(dev), None,
            torch.from_numpy(np.ascontiguousarray(tab["nmatch"])).to(dev))


def test_python_path_end_to_end():
    """verify_matches -> two_view_geometry on the 6-slot table: classes, the initial pair, the
    restatement's numbers, and the bytes of the two C calls made by hand."""
    import torch
    from sfmfromscratch_amd import sequence as S
    tab = TV.pipeline_table()
    t = table_of(tab)
    dev = t.xy.device
    trip = triple_of(tab, dev)
    v = S.verify_matches(t, tab["pairs"], trip, max_iterations=TV.VERIFY_ITERS)
    tv = S.two_view_geometry(t, tab["pairs"], trip, v, PR.K_SCENE)
    ev = VR.verify(tab, iters=TV.VERIFY_ITERS, stop=VR.stop_ratios(iters=TV.VERIFY_ITERS))
    assert np.array_equal(v.stat, ev["stat"]) and np.array_equal(v.keep, ev["keep"])
    att = ev["stat"][:, 3]
    eh = TV.homography(tab, iters=150, stop=TV.stop_ratios(iters=150), attempt=att)
    ep = TV.two_view_pose(tab, v.keep, v.F, PR.K_SCENE, attempt=att)
    print("config", tv.config.tolist(), "n_wide", tv.n_wide.tolist(), "initial pair", tv.initial_pair())
    assert tv.config.dtype == np.int8 and tv.config.tolist() == [1, 2, 2, 0, 1, 0]
    assert tv.initial_pair() == 0 and tv.n_wide[0] > tv.n_wide[4] > 0
    assert np.array_equal(tv.n_homography, eh["hstat"][:, 0]) and np.array_equal(tv.hkeep_dev.cpu().numpy(), eh["hkeep"])
    assert np.array_equal(tv.n_front, ep["pstat"][:, 0]) and np.array_equal(tv.n_wide, ep["pstat"][:, 2])
    assert tv.H.shape == (6, 3, 3) and tv.R.shape == (6, 3, 3) and tv.t.shape == (6, 3)
    ok = ep["pstat"][:, 1] >= 0
    assert np.abs(np.column_stack((tv.R.reshape(6, 9), tv.t))[ok] - ep["pose"][ok]).max() <= RT_TOL
    assert np.isnan(tv.R[~ok]).all() and np.isnan(tv.t[~ok]).all()
    # the two C calls by hand
    gh = run_h(tab, iters=150, confidence=0.98, attempt=v.stat[:, 3], table=t)
    gp = run_pose(tab, v.keep, v.F, PR.K_SCENE, attempt=v.stat[:, 3], table=t)
    assert gh["H"].tobytes() == tv.H.tobytes() and gh["hstat"].tobytes() == tv.hstat_dev.cpu().numpy().tobytes()
    assert gh["hkeep"].tobytes() == tv.hkeep_dev.cpu().numpy().tobytes()
    assert gp["pose"].tobytes() == tv.pose_dev.cpu().numpy().tobytes()
    assert gp["pstat"].tobytes() == tv.pstat_dev.cpu().numpy().tobytes()
    # K per slot on the device, and a schedule without a general pair
    Kd = torch.from_numpy(np.broadcast_to(PR.K_SCENE, (6, 3, 3)).copy()).to(dev)
    tv2 = S.two_view_geometry(t, tab["pairs"], trip, v, Kd)
    assert tv2.pose_dev.cpu().numpy().tobytes() == tv.pose_dev.cpu().numpy().tobytes()
    sub = VR.sub_table(tab, [1, 2, 3], "tv_pipeline_sub")
    vs = S.verify_matches(t, sub["pairs"], triple_of(sub, dev), max_iterations=TV.VERIFY_ITERS)
    assert S.two_view_geometry(t, sub["pairs"], triple_of(sub, dev), vs, PR.K_SCENE).initial_pair() == -1
    # the host list of match_schedule gives the same bytes
    host = [(tab["matches"][p, :max(int(tab["nmatch"][p]), 0)].astype(np.int64), np.ones(max(int(tab["nmatch"][p]), 0),
                                                                                         np.float32)) for p in range(6)]
    tvh = S.two_view_geometry(t, tab["pairs"], host, v, PR.K_SCENE)
    assert tvh.pstat_dev.cpu().numpy().tobytes() == tv.pstat_dev.cpu().numpy().tobytes()
    assert tvh.hstat_dev.cpu().numpy().tobytes() == tv.hstat_dev.cpu().numpy().tobytes()


def test_captured_into_one_graph_after_verify_and_replayed():
    import torch
    tab = TV.pipeline_table()
    t = table_of(tab)
    dev = t.xy.device
    ctx = context()
    P, cap, nimg = len(tab["pairs"]), tab["cap"], len(tab["count"])
    pt, mm, nm = up(tab["pairs"], np.int32), up(tab["matches"], np.int32), up(tab["nmatch"], np.int32)
    K = up(np.broadcast_to(PR.K_SCENE, (nimg, 3, 3)).reshape(nimg, 9), np.float64)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    keep, F, stat = z((P, cap), torch.uint8), z((P, 9), torch.float64), z((P, 4), torch.int32)
    H, hkeep, hstat = z((P, 9), torch.float64), z((P, cap), torch.uint8), z((P, 4), torch.int32)
    pose, pstat, att = z((P, 12), torch.float64), z((P, 4), torch.int32), z((P,), torch.int32)
    vstop, hstop = VR.stop_ratios(iters=TV.VERIFY_ITERS), TV.stop_ratios(iters=150)

    def enqueue(stream):
        ctx.verify_matches_dev(t.xy, t.count, pt, mm, nm, TV.VERIFY_ITERS, 1.0, 16, 5, vstop, keep, F, stat, stream)
        att.copy_(stat[:, 3])
        ctx.homography_matches_dev(t.xy, t.count, pt, mm, nm, att, 150, 2.0, 5, hstop, H, hkeep, hstat, stream)
        ctx.two_view_pose_dev(t.xy, t.count, pt, mm, nm, keep, F, K, att, TV.COS2_MIN, pose, pstat, stream)

    outs = (keep, F, stat, H, hkeep, hstat, pose, pstat)
    raw = lambda: b"".join(o.cpu().numpy().tobytes() for o in outs)
    enqueue(torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    want = raw()
    assert stat.cpu().numpy()[:, 3].any()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue(torch.cuda.current_stream(dev).cuda_stream)
    for _ in range(2):
        for o in outs:
            o.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        assert raw() == want


def test_binding_and_argument_errors():
    import torch
    from sfmfromscratch_amd import _abi
    from sfmfromscratch_amd import sequence as S
    tab = TV.pipeline_table()
    t = table_of(tab)
    dev = t.xy.device
    trip = triple_of(tab, dev)
    v = S.verify_matches(t, tab["pairs"], trip, max_iterations=32)
    with pytest.raises(ValueError, match=r"K must be"):
        S.two_view_geometry(t, tab["pairs"], trip, v, np.eye(4))
    with pytest.raises(ValueError, match=r"K must be"):
        S.two_view_geometry(t, tab["pairs"], trip, v, np.zeros((5, 3, 3)))
    with pytest.raises(ValueError, match="verified must be"):
        S.two_view_geometry(t, tab["pairs"][:3], trip, v, PR.K_SCENE)
    with pytest.raises(ValueError, match="int32"):
        S.two_view_geometry(t, tab["pairs"], (trip[0].long(), None, trip[2]), v, PR.K_SCENE)
    with pytest.raises(ValueError, match="min_parallax_deg"):
        S.two_view_geometry(t, tab["pairs"], trip, v, PR.K_SCENE, min_parallax_deg=100.0)
    for bad in (dict(h_iterations=-1), dict(h_iterations=(1 << 20) + 1)):
        with pytest.raises(ValueError, match="sfm_homography_matches_dev"):
            S.two_view_geometry(t, tab["pairs"], trip, v, PR.K_SCENE, **bad)
    ctx = context()
    P, cap, nimg = len(tab["pairs"]), tab["cap"], len(tab["count"])
    pt, mm, nm = up(tab["pairs"], np.int32), trip[0], trip[2]
    H = torch.empty((P, 9), dtype=torch.float64, device=dev)
    hkeep = torch.empty((P, cap), dtype=torch.uint8, device=dev)
    hstat = torch.empty((P, 4), dtype=torch.int32, device=dev)
    pose = torch.empty((P, 12), dtype=torch.float64, device=dev)
    pstat = torch.empty((P, 4), dtype=torch.int32, device=dev)
    K = up(np.broadcast_to(PR.K_SCENE, (nimg, 3, 3)).reshape(nimg, 9), np.float64)
    att = v.stat_dev[:, 3].contiguous()
    with pytest.raises(ValueError, match="n_stop"):
        ctx.homography_matches_dev(t.xy, t.count, pt, mm, nm, None, 10, 2.0, 5, np.full(65, 0.5), H, hkeep, hstat)
    with pytest.raises(ValueError, match="float64"):
        ctx.homography_matches_dev(t.xy, t.count, pt, mm, nm, None, 10, 2.0, 5, None, H.float(), hkeep, hstat)
    with pytest.raises(ValueError, match="contiguous"):
        ctx.homography_matches_dev(t.xy, t.count, pt, mm, nm, v.stat_dev[:, 3], 10, 2.0, 5, None, H, hkeep, hstat)
    with pytest.raises(ValueError, match="fewer"):
        ctx.two_view_pose_dev(t.xy, t.count, pt, mm, nm, v.keep_dev, v.F_dev, K[:2], att, 0.99, pose, pstat)
    with pytest.raises(ValueError, match="uint8"):
        ctx.two_view_pose_dev(t.xy, t.count, pt, mm, nm, v.keep_dev.int(), v.F_dev, K, att, 0.99, pose, pstat)
    # every SFM_EINVAL of the two calls, with a live context
    h_args = [t.xy.data_ptr(), t.count.data_ptr(), nimg, cap, pt.data_ptr(), P, mm.data_ptr(), nm.data_ptr(),
              att.data_ptr(), 10, 2.0, 5, None, 0, H.data_ptr(), hkeep.data_ptr(), hstat.data_ptr(), None]
    fn = ctx.lib.sfm_homography_matches_dev
    assert fn(ctx.handle, *h_args) == _abi.SFM_OK
    for k, val in ((0, None), (1, None), (2, 0), (3, 0), (4, None), (5, -1), (6, None), (7, None), (9, -1),
                   (9, (1 << 20) + 1), (13, -1), (13, 65), (13, 1), (14, None), (16, None)):
        bad = list(h_args)
        bad[k] = val
        assert fn(ctx.handle, *bad) == _abi.SFM_EINVAL, k
    for k in (8, 15):   # attempt and hkeep may be null
        okay = list(h_args)
        okay[k] = None
        assert fn(ctx.handle, *okay) == _abi.SFM_OK
    empty = list(h_args)
    for k in (4, 6, 7, 14, 15, 16):
        empty[k] = None
    empty[5] = 0
    assert fn(ctx.handle, *empty) == _abi.SFM_OK
    p_args = [t.xy.data_ptr(), t.count.data_ptr(), nimg, cap, pt.data_ptr(), P, mm.data_ptr(), nm.data_ptr(),
              v.keep_dev.data_ptr(), v.F_dev.data_ptr(), K.data_ptr(), att.data_ptr(), 0.99, pose.data_ptr(),
              pstat.data_ptr(), None]
    fn = ctx.lib.sfm_two_view_pose_dev
    assert fn(ctx.handle, *p_args) == _abi.SFM_OK
    for k, val in ((0, None), (1, None), (2, 0), (3, 0), (4, None), (5, -1), (6, None), (7, None), (8, None), (9, None),
                   (10, None), (13, None), (14, None)):
        bad = list(p_args)
        bad[k] = val
        assert fn(ctx.handle, *bad) == _abi.SFM_EINVAL, k
    okay = list(p_args)
    okay[11] = None
    assert fn(ctx.handle, *okay) == _abi.SFM_OK
    torch.cuda.synchronize()
