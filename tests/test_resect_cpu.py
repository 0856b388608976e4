"""CPU: what tests/test_gpu_resect.py relies on, asserted on the restatement alone
(tests/resect_ref.py): the sampler against a dense Fisher-Yates; the link list; for every slot of
every table that the two routes of the hypothesis ("elim", "svd") give the same masks at all three
thresholds, that every decided error of an admitted sample lies farther than 1e-6 px from them and
that at most pnp_ref.MAX_LEFT_OUT of the samples fall outside pnp_ref.admitted; the constants the
device's bounds are made of, held to their measurement (not below it, not above twice it); the
driver loop on tracks_ref.planted_scene(); the C ABI and the documents.  No test here needs a
device."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from tests import pnp_ref as PR
from tests import resect_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def held(constant, measured, what):
    print(f"MEASURED {what}: {measured:.4e} (constant {constant:.4e})")
    assert measured <= constant <= 2 * measured, what


# ---------------------------------------------------------------- the sampler
def test_sampler_equals_a_dense_fisher_yates_and_depends_on_seed_slot_and_sample_only():
    for s in (0, 1, 7, 255, 70000):
        for n in (6, 7, 12, 64, 257, 2561):
            for it in (0, 1, 63, 247, (1 << 20) - 1):
                a = RR.sample(RR.SEED, s, it, n)
                assert a == RR.sample_dense(RR.SEED, s, it, n)
                assert len(set(a)) == 6 and min(a) >= 0 and max(a) < n
    assert RR.sample(5, 3, 10, 100) != RR.sample(5, 4, 10, 100) != RR.sample(6, 4, 10, 100)
    assert RR.sample(5, 3, 10, 100) != RR.sample(5, 3, 11, 100)
    assert RR.SEED_XOR == int.from_bytes(b"Resectio", "big")
    # a prefix of the stream is the stream of fewer samples
    assert np.array_equal(RR.samples(5, 2, 40, 9), RR.samples(5, 2, 40, 65)[:9])
    # n = 6: every sample is a permutation of all six links
    assert all(sorted(RR.sample(5, 0, it, 6)) == list(range(6)) for it in range(32))


def test_default_iterations_are_the_098_count_of_a_six_point_sample_at_half_inliers():
    from sfmfromscratch_amd import pose
    assert pose.calculate_num_ransac_iterations(0.98, 6, 0.5) == RR.ITERS == 248


# ---------------------------------------------------------------- the link list
@pytest.mark.parametrize("name", list(RR.TABLES))
def test_links_are_the_planted_ones_among_every_kind_of_row_that_is_not_a_link(name):
    tab = RR.table(name)
    cap, T = tab["cap"], tab["n_tracks"]
    for s, n in enumerate(tab["sizes"]):
        rows, X, x = RR.links(tab, s)
        assert len(rows) == n and (np.diff(rows) > 0).all()
        c = int(tab["count"][s])
        nt = tab["node_track"][s]
        assert c < cap and ((nt[c:] >= 0) & (nt[c:] < T)).all()        # beyond count: tracks with a point, no link
        inside = nt[:c]
        for v in (-1, -2, -3):
            assert (inside == v).any()
        assert (inside >= T).any()
        bad = inside[(inside >= 0) & (inside < T)]
        Xb = tab["X"][bad]
        assert np.isnan(Xb).any(axis=1).any() and np.isinf(Xb).any(axis=1).any()
        assert np.isfinite(X).all() and np.array_equal(x, tab["xy"][s, rows].astype(np.float64))
    assert len({tuple(np.round(R.reshape(-1), 6)) for R in tab["R"]}) == len(tab["sizes"])   # a pose per slot
    if len(tab["sizes"]) >= 3:   # one slot in three has the skewed K
        assert any((K == PR.K_SKEW).all() for K in tab["K"]) and any((K == PR.K_SCENE).all() for K in tab["K"])


# ---------------------------------------------------------------- the margins and the routes
def test_every_slot_meets_the_margins_and_the_routes_differ_by_the_recorded_constants():
    dR = dt = 0.0
    margin, left = np.inf, 0.0
    for name in RR.TABLES:
        tab = RR.table(name)
        for s, n in enumerate(tab["sizes"]):
            if n < 6:
                continue
            rows, X, x = RR.links(tab, s)
            m = RR.slot_margins(X, x, tab["K"][s], RR.samples(RR.SEED, s, n, RR.ITERS))
            print(f"MEASURED {name} slot {s} n {n}: same masks {m['same_masks']}, nearest decided error "
                  f"{m['margin']:.3e} px from a threshold, {100 * m['left_out']:.1f} % left out, routes |dR| "
                  f"{m['dR']:.3e} |dt| {m['dt']:.3e}, defect {m['defect']:.3e}")
            assert m["same_masks"], (name, s)
            assert m["margin"] > RR.MARGIN, (name, s)
            assert m["left_out"] <= PR.MAX_LEFT_OUT, (name, s)
            dR, dt, margin, left = max(dR, m["dR"]), max(dt, m["dt"]), min(margin, m["margin"]), max(left, m["left_out"])
    print(f"MEASURED overall: nearest {margin:.3e} px, most left out {100 * left:.1f} %")
    held(RR.CPU_ROUTES_R, dR, "routes max |dR| on admitted samples")
    held(RR.CPU_ROUTES_T, dt, "routes |dt| on admitted samples")
    bR, bt = RR.hyp_bounds()
    assert bR == min(1e-8, 100 * RR.CPU_ROUTES_R) and bt == min(1e-8, 100 * RR.CPU_ROUTES_T)


def test_the_iteration_edges_are_prefixes_of_one_stream():
    tab = RR.table("small")
    full = RR.expected("small", 248, 8.0, refine=False)
    assert RR.ITER_EDGES == (0, 1, 7, 8, 9, 63, 64, 65, 129, 248)
    for iters in RR.ITER_EDGES[1:-1]:
        e = RR.resect(tab, iters, 8.0, refine=False)
        assert np.array_equal(e["counts"], full["counts"][:, :iters])
        assert np.array_equal(e["hyp"], full["hyp"][:, :iters], equal_nan=True)
    e0 = RR.resect(tab, 0, 8.0)
    assert e0["rstat"].tolist()[0] == [-1, -1, 0, 5, 0, -1, 0, 0] and e0["rstat"].tolist()[1] == [0, -1, 0, 6, 0, -1, 0, 0]
    assert np.isnan(e0["pose"]).all() and not e0["rkeep"].any()


def test_cases_cover_posed_unposed_and_unattempted_slots_and_min_inliers():
    posed = unposed = 0
    for name, iters, thr in RR.CASES:
        e = RR.expected(name, iters, thr)
        st = e["rstat"]
        posed += int((st[:, 4] == 1).sum())
        unposed += int(((st[:, 4] == 0) & (st[:, 0] >= 0)).sum())
        for s in np.flatnonzero(st[:, 4] == 1):
            assert st[s, 0] >= RR.MIN_INLIERS and e["rkeep"][s].sum() == st[s, 0] == e["counts"][s].max()
            assert st[s, 1] == int(np.argmax(e["counts"][s]))
        for s in np.flatnonzero(st[:, 4] == 0):
            assert np.isnan(e["pose"][s]).all() and not e["rkeep"][s].any()
    assert posed >= 10 and unposed >= 5
    small = RR.expected("small", 248, 8.0)
    assert small["rstat"][0, 0] == -1 and 0 < small["rstat"][3, 0] < RR.MIN_INLIERS   # n = 5; 12 links, 9 inliers


# ---------------------------------------------------------------- the refinement against scipy
def test_the_winners_refinement_reaches_scipys_minimum_within_the_recorded_constants():
    wR = wt = 0.0
    for name, iters, thr in RR.CASES:
        tab, e = RR.table(name), RR.expected(name, iters, thr)
        for s, f in e["fit"].items():
            rows, X, x = RR.links(tab, s)
            inl = np.flatnonzero(e["rkeep"][s][rows])
            h = e["hyp"][s, e["rstat"][s, 1]]
            Rm, tm, cm = PR.scipy_minimum(X[inl], x[inl], tab["K"][s], h[:9].reshape(3, 3), h[9:])
            dR, dt = PR.pose_deviation(f["R"][None], f["t"][None], Rm[None], tm[None])
            print(f"MEASURED {name} iters {iters} thr {thr} slot {s}: {len(inl)} inliers, status {f['status']}, vs scipy "
                  f"|dR| {dR[0]:.3e} |dt| {dt[0]:.3e}, cost excess {(f['cost'] - cm) / cm:.3e}")
            assert f["cost"] <= f["cost0"] and (f["cost"] - cm) / cm <= 1e-6
            wR, wt = max(wR, float(dR[0])), max(wt, float(dt[0]))
    held(RR.CPU_SCIPY_R, wR, "refinement vs scipy max |dR|")
    held(RR.CPU_SCIPY_T, wt, "refinement vs scipy |dt|")


# ---------------------------------------------------------------- the driver loop
def test_the_loop_poses_every_frame_of_the_planted_scene_from_pair_0_1():
    sc, tr = RR.planted_tracks()
    seed_pair = (0, 1) + RR.relative_pose(sc, 0, 1)
    wR = wt = 0.0
    for per_round, n_rounds in ((None, 1), (1, 4)):
        r = RR.reconstruct(sc, tr, seed_pair, per_round=per_round)
        eR, et = RR.gauge_error(r["R"], r["t"], sc)
        print(f"MEASURED planted scene per_round {per_round}: rounds {r['rounds']}, links per round "
              f"{[l.tolist() for l in r['n_links']]}, against the planted poses |dR| {eR:.3e} |dt| {et:.3e}")
        assert r["posed"].all() and r["rounds"][0] == [0, 1] and r["rounds"][-1] == []
        assert len(r["rounds"]) - 2 == n_rounds and sorted(sum(r["rounds"][1:], [])) == [2, 3, 4, 5]
        wR, wt = max(wR, eR), max(wt, et)
    held(RR.CPU_PLANTED_R, wR, "loop vs planted poses max |dR|")
    held(RR.CPU_PLANTED_T, wt, "loop vs planted poses |dt|")


# ---------------------------------------------------------------- host classes without a device
def test_next_views_orders_by_inliers_with_the_lowest_slot_first_on_a_tie_and_seed_picks_the_pair():
    import torch
    from sfmfromscratch_amd import sequence as S
    rstat = np.zeros((6, 8), np.int32)
    rstat[:, 0] = (40, 55, -1, 55, 30, 70)
    rstat[:, 4] = (1, 1, 0, 1, 0, 1)
    pose = np.full((6, 12), np.nan)
    pose[[0, 1, 3, 5]] = np.concatenate([np.eye(3).reshape(9), [1.0, 2.0, 3.0]])
    K = np.tile(PR.K_SCENE.reshape(1, 9), (6, 1))
    r = S.Resected(torch.from_numpy(pose), torch.from_numpy(rstat), torch.zeros((6, 2), dtype=torch.float64),
                   torch.zeros((6, 4), dtype=torch.uint8), torch.from_numpy(K))
    assert r.next_views().tolist() == [5, 1, 3, 0]
    assert r.posed.tolist() == [True, True, False, True, False, True] and r.n_inliers.tolist() == rstat[:, 0].tolist()
    assert np.allclose(r.P[1], PR.K_SCENE @ np.column_stack([np.eye(3), [1.0, 2.0, 3.0]])) and np.isnan(r.P[2]).all()
    # TwoView.seed: pair 2 is the general pair with the most wide points
    P = 4
    rt = np.full((P, 12), np.nan)
    rt[1] = rt[2] = np.concatenate([PR.rot(0.1).reshape(9), [1.0, 0.0, 0.0]])
    pstat = np.array([[0, -1, 0, 0], [30, 0, 10, 40], [50, 1, 25, 60], [0, -1, 0, 0]], np.int32)
    vstat = np.array([[0, -1, 0, 0], [40, 3, 256, 1], [60, 5, 256, 1], [20, 1, 256, 0]], np.int32)
    tv = S.TwoView(torch.zeros((P, 9), dtype=torch.float64), torch.zeros((P, 4), dtype=torch.int32), None,
                   torch.from_numpy(rt), torch.from_numpy(pstat), torch.from_numpy(vstat), 0.8)
    pairs = np.array([[0, 1], [0, 2], [1, 2], [2, 3]])
    a, b, R, t = tv.seed(pairs)
    assert (a, b) == (1, 2) and np.array_equal(R, PR.rot(0.1)) and t.tolist() == [1.0, 0.0, 0.0]
    assert tv.seed(pairs, 1)[:2] == (0, 2)
    for bad in (0, 7, -1):
        with pytest.raises(ValueError):
            tv.seed(pairs, bad)
    none = S.TwoView(torch.zeros((1, 9), dtype=torch.float64), torch.zeros((1, 4), dtype=torch.int32), None,
                     torch.full((1, 12), float("nan"), dtype=torch.float64), torch.zeros((1, 4), dtype=torch.int32),
                     torch.zeros((1, 4), dtype=torch.int32), 0.8)
    with pytest.raises(ValueError):
        none.seed(pairs[:1])


# ---------------------------------------------------------------- the C ABI and the documents
C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}


def header_prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfmfeat.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sfmfeat.h"
    args = [ctypes.c_void_p if "*" in a else C_TYPES[a.replace("const ", "").split()[0]]
            for a in (a.strip() for a in m.group(2).split(","))]
    return C_TYPES[m.group(1)], args


def test_abi_declares_the_call_and_rejects_it_without_a_context():
    from sfmfromscratch_amd import _abi, _native
    res, args = header_prototype("sfm_resect_tracks_dev")
    assert _native.SIGNATURES["sfm_resect_tracks_dev"] == (res, args) and len(args) == 22
    fn = _native.load_library().sfm_resect_tracks_dev
    assert fn(*[None if a is ctypes.c_void_p else 0 for a in args]) == _abi.SFM_EINVAL
    buf = np.zeros(64, np.float64)
    good = [None] + [buf.ctypes.data if a is ctypes.c_void_p else 1 for a in args[1:-1]] + [None]
    assert fn(*good) == _abi.SFM_EINVAL   # the per-argument errors are tests/test_gpu_resect.py's


def test_documents_name_the_call_the_loop_and_what_is_out_of_scope():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "13J" in design
    j = design[design.index("13J"):].lower()
    for word in ("out of scope", "bundle adjustment inside the loop", "reprojection error", "re-resection",
                 "early-stop", "colmap", "resect_bench.txt"):
        assert word in j, word
    for rel, words in (("README.md", ("resect.hip", "reconstruct")),
                       ("INTEGRATION.md", ("S.reconstruct(", "ba_inputs()", "sfm_resect_tracks_dev")),
                       ("include/sfmfeat.h", ("sfm_resect_tracks_dev", "0x526573656374696F")),
                       ("sfmfromscratch_amd/sequence.py", ("def resect_frames", "def reconstruct", "def seed"))):
        text = open(os.path.join(ROOT, rel)).read()
        for w in words:
            assert w in text, (rel, w)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "(PnP, §13D); cam_valid marks the others" not in integ   # the by-hand gap is closed
