"""GPU: resection from tracks on the device (sfm_resect_tracks_dev, resect.hip; sequence.resect_frames
and sequence.reconstruct) against the numpy restatement of tests/resect_ref.py.

Every bound traces to a constant tests/test_resect_cpu.py measured against the restatement, scipy
or the planted truth (tests/resect_ref.py CPU_*); nothing comes from the device:
a. n_links, out_counts, rstat[0..4] and rkeep equal the restatement byte for byte on every case (the
   CPU test asserts the margins that makes possible), and follow from the device's own out_hyp by
   tests/pnp_ref.py errors with the rounding band of tests/test_gpu_pnp_fits.py: every entry
   decided, none left out.
b. out_hyp of every admitted sample within min(1e-8, 100 x the two CPU routes' largest mutual
   difference); every finite R a rotation within 100 x the restatement's own defect for that sample.
c. The refined pose against pnp_ref.refine run from the device's winning hypothesis over the
   device's inliers within 100 x the restatement's distance from scipy's minimum; the final cost
   within pnp_ref.MARGINAL relative; status and accepted steps through the `firm` count.
d. One mixed call equals each slot alone, two runs, and the table split over two calls, byte for
   byte (pose bits included); the optional outputs; bad K; min_inliers; iters = 0; n_tracks = 0; an
   all-NaN X; graph capture and replay; the argument errors.
e. resect_frames equals the C call by hand; reconstruct on tracks_ref.planted_scene() equals the
   restatement's rounds and poses the frames within twice the restatement's own error; its
   ba_inputs() run through BundleAdjustment.
Every figure is printed before its assertion.

Measured on the MI355X: 0 counts differing of 4,692, every entry decided; out_hyp max |dR| 6.7e-11,
|dt| 5.7e-11 on admitted samples (bounds 1e-8, 9e-9), rotation defect at most 40 x the restatement's
(bound 100 x); refined pose max |dR| 2.3e-10, |dt| 2.0e-9 (bounds 1.2e-4, 1.3e-3), final cost
8.7e-14 relative (bound 1e-9); the planted poses within 6.5e-3 / 4.1e-2 (bounds 1.4e-2, 9.0e-2)."""
from __future__ import annotations

import functools
import types

import numpy as np
import pytest

from tests import pnp_ref as PR
from tests import resect_ref as RR
from tests import test_gpu_pnp_fits as PF

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16
OUT_KEYS = ("pose", "rstat", "rcost", "rkeep", "counts", "hyp")


def context():
    from sfmfromscratch_amd import _abi
    from sfmfromscratch_amd._native import context_for
    return context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), 0)


def up(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(torch.device("cuda", 0))


@functools.lru_cache(maxsize=None)
def device_table(name):
    tab = RR.table(name)
    return dict(xy=up(tab["xy"], np.int32), count=up(tab["count"], np.int32), node_track=up(tab["node_track"], np.int32),
                X=up(tab["X"], np.float64), K=up(tab["K"].reshape(-1, 9), np.float64))


def run(name, iters, thr, min_inliers=RR.MIN_INLIERS, seed=RR.SEED, attempt=None, want=("rkeep", "counts", "hyp"),
        K=None, X="table", n_tracks=None, max_refine_iter=PR.MAX_ITER):
    """sfm_resect_tracks_dev by hand over table `name` -> dict of numpy outputs (None where not asked
    for).  Every output starts from a fill the call must overwrite."""
    import torch
    tab, d = RR.table(name), device_table(name)
    dev = d["xy"].device
    nimg, cap = len(tab["count"]), tab["cap"]
    pose = torch.full((nimg, 12), 7.0, dtype=torch.float64, device=dev)
    rstat = torch.full((nimg, 8), 99, dtype=torch.int32, device=dev)
    rcost = torch.full((nimg, 2), 7.0, dtype=torch.float64, device=dev)
    rkeep = torch.full((nimg, cap), 7, dtype=torch.uint8, device=dev) if "rkeep" in want else None
    counts = torch.full((nimg, iters), 99, dtype=torch.int32, device=dev) if "counts" in want else None
    hyp = torch.full((nimg, iters, 12), 7.0, dtype=torch.float64, device=dev) if "hyp" in want else None
    Xd = d["X"] if isinstance(X, str) else (None if X is None else up(X, np.float64))
    T = tab["n_tracks"] if n_tracks is None else n_tracks
    context().resect_tracks_dev(d["xy"], d["count"], d["node_track"], Xd, T, d["K"] if K is None else up(K, np.float64),
                                None if attempt is None else up(attempt, np.uint8), iters, thr, min_inliers, seed,
                                max_refine_iter, pose, rstat, rcost, rkeep, counts, hyp)
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return dict(pose=host(pose), rstat=host(rstat), rcost=host(rcost), rkeep=host(rkeep), counts=host(counts),
                hyp=host(hyp))


@functools.lru_cache(maxsize=None)
def device(name, iters, thr):
    return run(name, iters, thr)


def slot_bytes(g, s):
    return b"".join(g[k][s].tobytes() for k in OUT_KEYS if g[k] is not None)


@functools.lru_cache(maxsize=None)
def admitted(name, s):
    tab = RR.table(name)
    rows, X, x = RR.links(tab, s)
    return RR.slot_margins(X, x, tab["K"][s], RR.samples(RR.SEED, s, len(rows), RR.ITERS))["admitted"]


# ---------------------------------------------------------------- a. the integer outputs
@pytest.mark.parametrize("case", RR.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_integer_outputs_equal_the_restatement(case):
    g, e = device(*case), RR.expected(*case)
    print(case, g["rstat"].tolist())
    assert np.array_equal(g["rstat"][:, 3], e["rstat"][:, 3])
    print(f"MEASURED {case}: counts differing {int((g['counts'] != e['counts']).sum())} of {e['counts'].size}")
    assert g["counts"].dtype == np.int32 and np.array_equal(g["counts"], e["counts"])
    assert np.array_equal(g["rstat"][:, :5], e["rstat"][:, :5])
    assert g["rkeep"].dtype == np.uint8 and np.array_equal(g["rkeep"], e["rkeep"])
    not_posed = g["rstat"][:, 4] == 0
    assert np.isnan(g["pose"][not_posed]).all() and np.isnan(g["rcost"][not_posed]).all()
    assert (g["rstat"][not_posed, 5:] == (-1, 0, 0)).all()
    assert np.isfinite(g["pose"][~not_posed]).all()


@pytest.mark.parametrize("case", RR.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_counts_winner_and_keep_follow_from_the_devices_own_hypotheses(case):
    name, iters, thr = case
    tab, g = RR.table(name), device(*case)
    for s in range(len(tab["count"])):
        rows, X, x = RR.links(tab, s)
        st = g["rstat"][s]
        if st[0] < 0:   # not attempted: zero counts, NaN hypotheses
            assert not g["counts"][s].any() and np.isnan(g["hyp"][s]).all() and not g["rkeep"][s].any()
            continue
        mask = PF.decided_mask(X, x, tab["K"][s], g["hyp"][s], thr, f"{case} slot {s}")
        want = mask.sum(axis=1)
        assert np.array_equal(g["counts"][s], want), s
        best = int(np.argmax(want))
        assert st[0] == want[best] and st[1] == best and st[2] == iters
        posed = want[best] > 0 and want[best] >= RR.MIN_INLIERS
        assert st[4] == int(posed)
        keep = np.zeros(tab["cap"], np.uint8)
        if posed:
            keep[rows[mask[best]]] = 1
        assert np.array_equal(g["rkeep"][s], keep), s


@pytest.mark.parametrize("iters", RR.ITER_EDGES)
def test_every_iteration_edge_equals_a_prefix_of_the_248_sample_restatement(iters):
    """iters = 0, 1 (one lane of the hypothesis kernel, a one-entry selection), 7 (a partial count
    workgroup), 8 (exactly one), 9, 63, 64, 65 (the hypothesis wave's edges), 129, 248 on table
    "small": the stream is a function of (seed, slot, sample), so the counts and hypotheses are the
    first `iters` of the 248-sample restatement's and the winner follows from them; the refinement
    against pnp_ref.refine run from the device's own winner, with the bounds of test c."""
    tab, g, full = RR.table("small"), run("small", iters, 8.0), RR.expected("small", 248, 8.0, refine=False)
    e = RR.resect(tab, iters, 8.0, refine=False)
    assert np.array_equal(e["counts"], full["counts"][:, :iters])
    print(f"iters {iters}: rstat {g['rstat'].tolist()}; counts differing "
          f"{int((g['counts'] != full['counts'][:, :iters]).sum())} of {g['counts'].size}")
    assert g["counts"].shape == (len(tab["count"]), iters) and np.array_equal(g["counts"], full["counts"][:, :iters])
    assert np.array_equal(g["rstat"][:, :5], e["rstat"][:, :5])
    assert np.array_equal(g["rkeep"], e["rkeep"])
    bR, bt = RR.hyp_bounds()
    for s in range(len(tab["count"])):
        if g["rstat"][s, 0] < 0:
            assert np.isnan(g["hyp"][s]).all()
            continue
        hd, he = g["hyp"][s], full["hyp"][s, :iters]
        nan = np.isnan(hd).all(axis=1)
        assert np.array_equal(nan, np.isnan(he).all(axis=1)) and np.isfinite(hd[~nan]).all()
        adm = admitted("small", s)[:iters] & ~nan
        if adm.any():
            dR, dt = PR.pose_deviation(hd[adm, :9].reshape(-1, 3, 3), hd[adm, 9:], he[adm, :9].reshape(-1, 3, 3),
                                       he[adm, 9:])
            print(f"MEASURED iters {iters} slot {s}: hypotheses max |dR| {dR.max():.3e} |dt| {dt.max():.3e}")
            assert dR.max() <= bR and dt.max() <= bt
    not_posed = g["rstat"][:, 4] == 0
    assert np.isnan(g["pose"][not_posed]).all() and np.isnan(g["rcost"][not_posed]).all()
    assert (g["rstat"][not_posed, 5:] == (-1, 0, 0)).all()
    for s in np.flatnonzero(~not_posed):
        rows, X, x = RR.links(tab, s)
        inl = np.flatnonzero(g["rkeep"][s][rows])
        h = g["hyp"][s, g["rstat"][s, 1]]
        f = PR.refine(X[inl], x[inl], tab["K"][s], h[:9].reshape(3, 3), h[9:])
        dR, dt = PR.pose_deviation(g["pose"][s, :9].reshape(1, 3, 3), g["pose"][s, 9:][None], f["R"][None], f["t"][None])
        ec = abs(g["rcost"][s, 1] - f["cost"]) / f["cost"]
        print(f"MEASURED iters {iters} slot {s}: refined pose max |dR| {dR[0]:.3e} |dt| {dt[0]:.3e} cost {ec:.3e}")
        assert dR[0] <= 100 * RR.CPU_SCIPY_R and dt[0] <= 100 * RR.CPU_SCIPY_T and ec <= PR.MARGINAL
        assert g["rstat"][s, 6] >= f["firm"] and 1 <= g["rstat"][s, 7] <= PR.MAX_ITER


# ---------------------------------------------------------------- b. the hypotheses
@pytest.mark.parametrize("case", RR.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_hypotheses_against_the_restatement(case):
    name, iters, thr = case
    tab, g, e = RR.table(name), device(*case), RR.expected(*case)
    bR, bt = RR.hyp_bounds()
    for s in range(len(tab["count"])):
        if g["rstat"][s, 0] < 0:
            continue
        hd, he = g["hyp"][s], e["hyp"][s]
        nan = PF.whole_nan(hd, f"{case} slot {s}")
        assert np.array_equal(nan, np.isnan(he).all(axis=1))
        adm = admitted(name, s)[:iters] & ~nan
        Rd, td = hd[:, :9].reshape(-1, 3, 3), hd[:, 9:]
        Re, te = he[:, :9].reshape(-1, 3, 3), he[:, 9:]
        dR, dt = PR.pose_deviation(Rd[adm], td[adm], Re[adm], te[adm]) if adm.any() else (np.zeros(1), np.zeros(1))
        dd, de = PR.rotation_defect(Rd[~nan]), PR.rotation_defect(Re[~nan])
        ratio = float((dd / np.maximum(de, EPS)).max()) if (~nan).any() else 0.0
        print(f"MEASURED {case} slot {s}: {int(adm.sum())} admitted of {iters}, max |dR| {dR.max():.3e} |dt| {dt.max():.3e} "
              f"(bounds {bR:.1e}, {bt:.1e}); defect at most {ratio:.2f} x the restatement's (largest {dd.max() if dd.size else 0:.3e})")
        assert dR.max() <= bR and dt.max() <= bt
        assert (dd <= 100 * np.maximum(de, EPS)).all()
        assert (np.linalg.det(Rd[~nan]) > 0).all()


# ---------------------------------------------------------------- c. the refinement
@pytest.mark.parametrize("case", RR.CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_refinement_against_the_restatement_run_from_the_devices_winner(case):
    name, iters, thr = case
    tab, g = RR.table(name), device(*case)
    for s in np.flatnonzero(g["rstat"][:, 4] == 1):
        rows, X, x = RR.links(tab, s)
        inl = np.flatnonzero(g["rkeep"][s][rows])
        h = g["hyp"][s, g["rstat"][s, 1]]
        f = PR.refine(X[inl], x[inl], tab["K"][s], h[:9].reshape(3, 3), h[9:])
        Rd, td = g["pose"][s, :9].reshape(3, 3), g["pose"][s, 9:]
        dR, dt = PR.pose_deviation(Rd[None], td[None], f["R"][None], f["t"][None])
        c0, c1 = g["rcost"][s]
        ec, e0 = abs(c1 - f["cost"]) / f["cost"], abs(c0 - f["cost0"]) / f["cost0"]
        st = g["rstat"][s]
        print(f"MEASURED {case} slot {s}: {len(inl)} inliers, refined pose vs the restatement max |dR| {dR[0]:.3e} |dt| "
              f"{dt[0]:.3e} (bounds {100 * RR.CPU_SCIPY_R:.1e}, {100 * RR.CPU_SCIPY_T:.1e}), cost {ec:.3e} start cost "
              f"{e0:.3e}; status {st[5]} (restatement {f['status']}) accepted {st[6]} (restatement {f['iters']}, firm "
              f"{f['firm']}, all firm {f['all_firm']}) iterations {st[7]} (restatement {f['lm_iters']})")
        assert dR[0] <= 100 * RR.CPU_SCIPY_R and dt[0] <= 100 * RR.CPU_SCIPY_T
        assert ec <= PR.MARGINAL and e0 <= PR.MARGINAL
        assert c1 <= c0
        if f["all_firm"]:
            assert st[5] == f["status"] and st[6] == f["iters"]
        assert st[6] >= f["firm"]
        assert st[5] in (0, 1, 3) and 1 <= st[7] <= PR.MAX_ITER
        assert np.abs(Rd @ Rd.T - np.eye(3)).max() < 1e-12 and np.linalg.det(Rd) > 0


# ---------------------------------------------------------------- d. batching and determinism
def test_a_slot_gets_the_same_bytes_alone_in_a_mixed_call_split_over_calls_and_twice():
    name, iters, thr = "small", 65, 8.0
    nimg = len(RR.table(name)["count"])
    full = run(name, iters, thr)
    again = run(name, iters, thr)
    assert all(slot_bytes(full, s) == slot_bytes(again, s) for s in range(nimg))
    mixed_mask = np.array([s % 2 for s in range(nimg)], np.uint8)
    mixed, rest = run(name, iters, thr, attempt=mixed_mask), run(name, iters, thr, attempt=1 - mixed_mask)
    none = run(name, iters, thr, attempt=np.zeros(nimg, np.uint8))
    for s in range(nimg):
        alone = np.zeros(nimg, np.uint8)
        alone[s] = 1
        one = run(name, iters, thr, attempt=alone)
        assert slot_bytes(one, s) == slot_bytes(full, s), s
        assert slot_bytes(mixed if mixed_mask[s] else rest, s) == slot_bytes(full, s), s
        skipped = rest if mixed_mask[s] else mixed
        for g in (none, skipped):   # not attempted: the record says so, n_links all the same
            assert g["rstat"][s].tolist() == [-1, -1, 0, full["rstat"][s, 3], 0, -1, 0, 0]
            assert np.isnan(g["pose"][s]).all() and np.isnan(g["rcost"][s]).all() and not g["rkeep"][s].any()
            assert not g["counts"][s].any() and np.isnan(g["hyp"][s]).all()
        others = [o for o in range(nimg) if o != s]
        assert (one["rstat"][others, 0] == -1).all()


def test_optional_outputs_may_be_null():
    name, iters, thr = "small", 65, 8.0
    full = device(name, iters, thr) if (name, iters, thr) in RR.CASES else run(name, iters, thr)
    for want in ((), ("rkeep",), ("counts",), ("hyp",)):
        g = run(name, iters, thr, want=want)
        for k in ("pose", "rstat", "rcost") + want:
            assert g[k].tobytes() == full[k].tobytes(), (want, k)


def test_a_slot_with_a_bad_K_is_not_attempted_while_its_neighbours_are():
    name, iters, thr = "small", 65, 8.0
    tab = RR.table(name)
    full = run(name, iters, thr)
    K = tab["K"].reshape(-1, 9).copy()
    K[4, 2] = np.nan
    K[6, 3] = 1e-3       # below the diagonal
    K[8, 4] = 0.0        # a zero on the diagonal
    g = run(name, iters, thr, K=K)
    for s in range(len(K)):
        if s in (4, 6, 8):
            assert g["rstat"][s].tolist() == [-1, -1, 0, tab["sizes"][s], 0, -1, 0, 0] and np.isnan(g["pose"][s]).all()
            assert not g["rkeep"][s].any() and not g["counts"][s].any()
        else:
            assert slot_bytes(g, s) == slot_bytes(full, s), s


def test_min_inliers_iters_0_no_tracks_and_an_all_nan_X():
    name, thr = "small", 8.0
    tab = RR.table(name)
    nimg, sizes = len(tab["count"]), np.array(tab["sizes"])
    full = device(name, 248, thr)
    g = run(name, 248, thr, min_inliers=10 ** 6)
    assert np.array_equal(g["counts"], full["counts"]) and np.array_equal(g["rstat"][:, :4], full["rstat"][:, :4])
    assert not g["rstat"][:, 4].any() and np.isnan(g["pose"]).all() and not g["rkeep"].any()
    low = run(name, 248, thr, min_inliers=0)   # a best count of 0 is no pose even then; every other slot is posed
    assert np.array_equal(low["rstat"][:, 4], (full["rstat"][:, 0] > 0).astype(np.int32))
    z = run(name, 0, thr)
    for s in range(nimg):
        assert z["rstat"][s].tolist() == ([0, -1, 0, sizes[s], 0, -1, 0, 0] if sizes[s] >= 6 else
                                          [-1, -1, 0, sizes[s], 0, -1, 0, 0])
    assert np.isnan(z["pose"]).all() and np.isnan(z["rcost"]).all() and not z["rkeep"].any()
    for g in (run(name, 9, thr, X=None, n_tracks=0), run(name, 9, thr, X=np.full_like(tab["X"], np.nan))):
        assert (g["rstat"] == (-1, -1, 0, 0, 0, -1, 0, 0)).all() and np.isnan(g["pose"]).all()
        assert not g["rkeep"].any() and not g["counts"].any() and np.isnan(g["hyp"]).all()


def test_the_call_is_captured_into_a_graph_after_one_warm_call_and_replayed():
    import torch
    name, iters, thr = "big1", 63, 2.0
    tab, d = RR.table(name), device_table(name)
    dev = d["xy"].device
    want = device(name, iters, thr)
    nimg, cap = len(tab["count"]), tab["cap"]
    outs = dict(pose=torch.zeros((nimg, 12), dtype=torch.float64, device=dev),
                rstat=torch.zeros((nimg, 8), dtype=torch.int32, device=dev),
                rcost=torch.zeros((nimg, 2), dtype=torch.float64, device=dev),
                rkeep=torch.zeros((nimg, cap), dtype=torch.uint8, device=dev),
                counts=torch.zeros((nimg, iters), dtype=torch.int32, device=dev),
                hyp=torch.zeros((nimg, iters, 12), dtype=torch.float64, device=dev))
    ctx = context()

    def enqueue(stream):
        ctx.resect_tracks_dev(d["xy"], d["count"], d["node_track"], d["X"], tab["n_tracks"], d["K"], None, iters, thr,
                              RR.MIN_INLIERS, RR.SEED, PR.MAX_ITER, outs["pose"], outs["rstat"], outs["rcost"],
                              outs["rkeep"], outs["counts"], outs["hyp"], stream)

    enqueue(0)   # the warm call: the workspace has its size
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue(torch.cuda.current_stream(dev).cuda_stream)
    for _ in range(2):
        for o in outs.values():
            o.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        for k in OUT_KEYS:
            assert outs[k].cpu().numpy().tobytes() == want[k].tobytes(), k


def test_argument_errors_of_the_c_call_and_of_the_binding():
    import torch
    from sfmfromscratch_amd import _abi
    name = "small"
    tab, d = RR.table(name), device_table(name)
    dev = d["xy"].device
    nimg, cap, T = len(tab["count"]), tab["cap"], tab["n_tracks"]
    pose = torch.zeros((nimg, 12), dtype=torch.float64, device=dev)
    rstat = torch.zeros((nimg, 8), dtype=torch.int32, device=dev)
    rcost = torch.zeros((nimg, 2), dtype=torch.float64, device=dev)
    ctx = context()
    fn = ctx.lib.sfm_resect_tracks_dev
    base = dict(xy=d["xy"].data_ptr(), count=d["count"].data_ptr(), nimg=nimg, cap=cap, nt=d["node_track"].data_ptr(),
                X=d["X"].data_ptr(), T=T, K=d["K"].data_ptr(), attempt=None, iters=9, thr=8.0, min_inliers=12, seed=5,
                lm=50, pose=pose.data_ptr(), rstat=rstat.data_ptr(), rcost=rcost.data_ptr())

    def call(**kw):
        a = dict(base, **kw)
        return fn(ctx.handle, a["xy"], a["count"], a["nimg"], a["cap"], a["nt"], a["X"], a["T"], a["K"], a["attempt"],
                  a["iters"], a["thr"], a["min_inliers"], a["seed"], a["lm"], a["pose"], a["rstat"], a["rcost"], None,
                  None, None, None)

    assert call() == _abi.SFM_OK
    torch.cuda.synchronize()
    for kw in (dict(nimg=0), dict(cap=0), dict(T=-1), dict(iters=-1), dict(iters=(1 << 20) + 1), dict(thr=0.0),
               dict(thr=float("nan")), dict(min_inliers=-1), dict(lm=0), dict(lm=1 << 24), dict(xy=None),
               dict(count=None), dict(nt=None), dict(X=None), dict(K=None), dict(pose=None), dict(rstat=None),
               dict(rcost=None)):
        assert call(**kw) == _abi.SFM_EINVAL, kw
    # the binding: shapes, dtypes and devices are checked before the call
    ok = (d["xy"], d["count"], d["node_track"], d["X"], T, d["K"], None, 9, 8.0, 12, 5, 50, pose, rstat, rcost)
    ctx.resect_tracks_dev(*ok)
    torch.cuda.synchronize()
    for i, bad in ((0, d["xy"][:, :, 0]), (1, d["count"].long()), (2, d["node_track"][:, :-1]), (3, d["X"].cpu()),
                   (5, d["K"][:-1]), (6, torch.zeros(nimg, dtype=torch.int32, device=dev)), (12, pose[:-1]),
                   (13, rstat.float()), (14, None)):
        args = list(ok)
        args[i] = bad
        with pytest.raises(ValueError):
            ctx.resect_tracks_dev(*args)
    with pytest.raises(ValueError):   # the C call's own SFM_EINVAL
        ctx.resect_tracks_dev(*(ok[:8] + (-1.0,) + ok[9:]))


# ---------------------------------------------------------------- e. the Python side
def six_slot_tracks():
    """The first six slots of table "small" as a sequence.Tracks (only what resect_frames reads)."""
    from sfmfromscratch_amd import sequence as S
    d = device_table("small")
    return S.Tracks(None, None, None, d["node_track"][:6].contiguous(), None, d["xy"][:6].contiguous(),
                    count=d["count"][:6].contiguous())


def test_resect_frames_equals_the_c_call_by_hand():
    import torch
    from sfmfromscratch_amd import sequence as S
    tab = RR.table("small")
    tr = six_slot_tracks()
    want = device("small", 248, 8.0)
    r = S.resect_frames(tr, tab["X"], tab["K"][:6])
    assert r.pose_dev.cpu().numpy().tobytes() == want["pose"][:6].tobytes()
    assert np.array_equal(r.stat, want["rstat"][:6]) and np.array_equal(r.cost, want["rcost"][:6], equal_nan=True)
    assert np.array_equal(r.keep_dev.cpu().numpy(), want["rkeep"][:6])
    assert np.array_equal(r.n_links, tab["sizes"][:6]) and np.array_equal(r.posed, want["rstat"][:6, 4] != 0)
    assert np.array_equal(r.R.reshape(-1, 9), want["pose"][:6, :9], equal_nan=True)
    for s in np.flatnonzero(r.posed):
        assert np.array_equal(r.P[s], tab["K"][s] @ np.column_stack([r.R[s], r.t[s]]))
    assert r.next_views().tolist() == sorted(np.flatnonzero(r.posed), key=lambda s: (-r.n_inliers[s], s))
    # posed slots are skipped; a device X and a single K are taken as they are
    skip = np.array([0, 0, 0, 0, 1, 0], bool)
    r2 = S.resect_frames(tr, torch.from_numpy(tab["X"]).cuda(), tab["K"][:6], posed=skip, iterations=65, threshold=2.0)
    w2 = device("small", 129, 2.0)
    assert r2.stat[4].tolist() == [-1, -1, 0, 63, 0, -1, 0, 0]
    assert np.array_equal(r2.stat[5, 2:4], [65, 64]) and r2.stat[5, 0] == w2["counts"][5, :65].max()
    with pytest.raises(ValueError):
        S.resect_frames(tr, tab["X"], np.array([[800.0, 0, 480], [1.0, 800, 270], [0, 0, 1]]))
    with pytest.raises(ValueError):
        S.resect_frames(tr, tab["X"][:, :2], tab["K"][:6])
    with pytest.raises(ValueError):
        S.resect_frames(tr, tab["X"], tab["K"][:6], posed=np.zeros(5, bool))


def planted_device_tracks(sc):
    from sfmfromscratch_amd import sequence as S
    table = types.SimpleNamespace(count=up(sc["count"], np.int32), xy=up(sc["xy"], np.int32))
    matches = [(sc["matches"][p, :sc["nmatch"][p]],) for p in range(len(sc["pairs"]))]
    return S.build_tracks(table, sc["pairs"], matches)


@pytest.mark.parametrize("per_round", [None, 1])
def test_reconstruct_poses_the_planted_scene_as_the_restatement_does(per_round):
    from sfmfromscratch_amd import sequence as S
    from sfmfromscratch_amd.pose import BundleAdjustment
    sc, tr = RR.planted_tracks()
    seed_pair = (0, 1) + RR.relative_pose(sc, 0, 1)
    e = RR.reconstruct(sc, tr, seed_pair, per_round=per_round)
    tracks = planted_device_tracks(sc)
    rec = S.reconstruct(tracks, sc["K"], seed_pair, per_round=per_round)
    print(f"per_round {per_round}: rounds {rec.rounds} (restatement {e['rounds']})")
    assert rec.rounds == e["rounds"] and np.array_equal(rec.posed, e["posed"]) and rec.posed.all()
    assert len(rec.rounds) - 2 == (1 if per_round is None else 4)
    dR, dt = RR.gauge_error(rec.R, rec.t, sc)
    print(f"MEASURED per_round {per_round}: against the planted poses max |dR| {dR:.3e} |dt| {dt:.3e} (bounds "
          f"{2 * RR.CPU_PLANTED_R:.1e}, {2 * RR.CPU_PLANTED_T:.1e})")
    assert dR <= 2 * RR.CPU_PLANTED_R and dt <= 2 * RR.CPU_PLANTED_T
    assert np.allclose(rec.P, sc["K"] @ np.concatenate([rec.R, rec.t[:, :, None]], axis=2))
    assert rec.X.shape == (tracks.n_tracks, 3) and rec.views.shape == (tracks.n_tracks,)
    cam, pt, xy, params, X3 = rec.ba_inputs()
    good = np.isfinite(rec.X).all(axis=1)
    assert len(X3) == good.sum() and np.isfinite(X3).all() and pt.max() == len(X3) - 1 and len(cam) == len(pt) == len(xy)
    assert params.shape == (6, 6) and np.isfinite(params).all() and not params[0].any()
    info = {}
    nimg = len(sc["count"])
    ba = BundleAdjustment(nimg, len(X3), cam, pt, xy, params, X3, np.broadcast_to(sc["K"], (nimg, 3, 3)).copy(),
                          fixed_cameras=[0], info=info)
    cams, pts = ba.sparse_bundle_adjustment()
    print(f"MEASURED per_round {per_round}: bundle adjustment cost {info['cost0']:.6e} -> {info['cost']:.6e}")
    assert info["cost"] <= info["cost0"] and np.isfinite(cams).all() and np.isfinite(pts).all()


def test_two_view_seed_feeds_reconstruct():
    import torch
    from sfmfromscratch_amd import sequence as S
    sc, _ = RR.planted_tracks()
    R01, t01 = RR.relative_pose(sc, 0, 1)
    P = len(sc["pairs"])
    rt = np.full((P, 12), np.nan)
    rt[0] = np.concatenate([R01.reshape(9), t01])
    pstat = np.zeros((P, 4), np.int32)
    pstat[0] = (60, 0, 40, 65)
    vstat = np.zeros((P, 4), np.int32)
    vstat[0] = (65, 0, 256, 1)
    dev = torch.device("cuda", 0)
    tv = S.TwoView(torch.zeros((P, 9), dtype=torch.float64, device=dev), torch.zeros((P, 4), dtype=torch.int32, device=dev),
                   None, up(rt, np.float64), up(pstat, np.int32), up(vstat, np.int32), 0.8)
    a, b, R, t = tv.seed(sc["pairs"])
    assert (a, b) == (0, 1) and np.array_equal(R, R01) and np.array_equal(t, t01)
    with pytest.raises(ValueError):
        tv.seed(sc["pairs"], 3)
    rec = S.reconstruct(planted_device_tracks(sc), sc["K"], tv.seed(sc["pairs"]), max_rounds=0)
    assert rec.rounds == [[0, 1]] and rec.posed.tolist() == [True, True] + [False] * 4
