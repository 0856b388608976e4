"""GPU: geometric verification on the device (sequence.verify_matches, verify.hip) against the numpy
restatement of tests/verify_ref.py: stat and keep byte for byte, the winner's F through its epipolar
distances within ransac_ref.D_BOUND.  The conditions the cases must meet (every evaluated distance
farther than D_BOUND from the threshold, both branches of the stop test) are asserted on the CPU
in tests/test_verify_cpu.py."""
from __future__ import annotations

import types

import numpy as np
import pytest

from tests import ransac_ref as RR
from tests import verify_ref as VR

pytestmark = pytest.mark.gpu


def table_of(tab):
    import torch
    dev = torch.device("cuda", 0)
    return types.SimpleNamespace(count=torch.from_numpy(np.ascontiguousarray(tab["count"], np.int32)).to(dev),
                                 xy=torch.from_numpy(np.ascontiguousarray(tab["xy"], np.int32)).to(dev))


def triple_of(tab, dev):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(tab["matches"])).to(dev), None,
            torch.from_numpy(np.ascontiguousarray(tab["nmatch"])).to(dev))


def run(tab, iters=VR.ITERS, threshold=VR.THRESHOLD, min_inliers=16, confidence=None, seed=VR.SEED, table=None):
    from sfmfromscratch_amd import sequence as S
    table = table or table_of(tab)
    return S.verify_matches(table, tab["pairs"], triple_of(tab, table.xy.device), threshold=threshold,
                            max_iterations=iters, confidence=confidence, min_inliers=min_inliers, seed=seed)


def raw_bytes(v):
    return v.keep.tobytes() + v.F.tobytes() + v.stat.tobytes()


def assert_equals_restatement(v, tab, e):
    assert v.stat.dtype == np.int32 and v.keep.dtype == np.uint8 and v.F.dtype == np.float64
    assert np.array_equal(v.stat, e["stat"]), (v.stat.tolist(), e["stat"].tolist())
    assert np.array_equal(v.keep, e["keep"])
    assert np.array_equal(v.n_inliers, e["stat"][:, 0]) and np.array_equal(v.best_iter, e["stat"][:, 1])
    assert np.array_equal(v.samples, e["stat"][:, 2]) and np.array_equal(v.verified, e["stat"][:, 3] != 0)
    for p in range(len(tab["pairs"])):
        if not np.isfinite(e["F"][p]).all():
            assert np.isnan(v.F[p]).all(), p
            continue
        _, _, valid, p1, p2 = VR.correspondences(tab, p)
        d = RR.distances(v.F[p], p1[valid], p2[valid], np.float64)
        dr = RR.distances(e["F"][p], p1[valid], p2[valid], np.float64)
        worst = float(np.abs(d - dr).max())
        print(f"{tab['name']} pair {p}: |d(F) - d(F_restated)| <= {worst:.3e} px")
        assert worst <= RR.D_BOUND


@pytest.mark.parametrize("confidence", [None, VR.CONFIDENCE])
@pytest.mark.parametrize("name", list(VR.SINGLE))
def test_equals_the_restatement(name, confidence):
    """n = 7, 8, 9, 40, 255, 257, 300 and 2560, 2561, 5121 (around one and two staging chunks), 700
    samples, fixed and with the 0.98 table; n = 2700 with 60 rows outside [0, count): samples drawn
    from global memory that contain an invalid match, and a stop between restaged rounds."""
    tab = VR.single(name)
    v = run(tab, confidence=confidence)
    e = VR.verify(tab, stop=VR.stop_ratios(confidence))
    print(name, confidence, v.stat.tolist())
    assert_equals_restatement(v, tab, e)


@pytest.mark.parametrize("iters", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("name", ["n9", "n40", "n257", "n2561", "n2700_bad"])
def test_iteration_counts_around_a_round(name, iters):
    tab = VR.single(name)
    for confidence in (None, VR.CONFIDENCE):
        v = run(tab, iters=iters, confidence=confidence)
        e = VR.verify(tab, iters=iters, stop=VR.stop_ratios(confidence, iters) if iters else None)
        assert_equals_restatement(v, tab, e)
    if iters == 0:
        assert v.stat.tolist() == [[0, -1, 0, 0]] and not v.keep.any() and np.isnan(v.F).all()


def test_min_inliers_at_the_winning_count():
    tab = VR.single("n40")
    best = int(VR.verify(tab)["stat"][0, 0])
    for mi in (0, best, best + 1):
        v = run(tab, min_inliers=mi)
        assert_equals_restatement(v, tab, VR.verify(tab, min_inliers=mi))
        assert bool(v.verified[0]) == (mi <= best) and v.keep.sum() == (best if mi <= best else 0)


@pytest.mark.parametrize("threshold", [1.0, 1e-9])
def test_one_call_of_mixed_pairs(threshold):
    """nmatch -1 and > cap, a == b, slots outside the table, rows >= count and negative rows, a pure
    random pair, fewer than 8 matches: the restatement's bytes, and each pair what it gets alone."""
    from sfmfromscratch_amd import sequence as S
    tab = VR.mixed()
    table = table_of(tab)
    conf = VR.CONFIDENCE
    v = run(tab, iters=VR.MIXED_ITERS, threshold=threshold, confidence=conf, table=table)
    e = VR.verify(tab, iters=VR.MIXED_ITERS, threshold=threshold, stop=VR.stop_ratios(conf, VR.MIXED_ITERS))
    assert_equals_restatement(v, tab, e)
    for p in range(len(tab["pairs"])):
        one = VR.sub_table(tab, [p], f"mixed_{p}")
        a = run(one, iters=VR.MIXED_ITERS, threshold=threshold, confidence=conf, table=table)
        assert a.keep.tobytes() == v.keep[p].tobytes() and a.stat.tobytes() == v.stat[p].tobytes()
        assert a.F.tobytes() == v.F[p].tobytes()
    if threshold != 1.0:
        assert np.isnan(v.F[VR.MIXED_RANDOM]).all() and v.stat[VR.MIXED_RANDOM].tolist() == [0, 0, VR.MIXED_ITERS, 0]
    # P = 0
    z = S.verify_matches(table, np.zeros((0, 2), np.int32), triple_of(VR.sub_table(tab, [], "none"), table.xy.device))
    assert z.keep.shape == (0, tab["cap"]) and z.stat.shape == (0, 4) and z.F.shape == (0, 3, 3)
    assert z.inlier_matches() == []


def test_determinism_permutation_and_split():
    tab = VR.mixed()
    table = table_of(tab)
    kw = dict(iters=VR.MIXED_ITERS, confidence=VR.CONFIDENCE, table=table)
    a, b = run(tab, **kw), run(tab, **kw)
    assert raw_bytes(a) == raw_bytes(b)
    perm, order = VR.permuted_pairs(tab, 9)
    q = run(perm, **kw)
    assert q.keep.tobytes() == a.keep[order].tobytes() and q.stat.tobytes() == a.stat[order].tobytes()
    assert q.F.tobytes() == a.F[order].tobytes()
    P = len(tab["pairs"])
    lo, hi = run(VR.sub_table(tab, np.arange(4), "lo"), **kw), run(VR.sub_table(tab, np.arange(4, P), "hi"), **kw)
    assert lo.keep.tobytes() + hi.keep.tobytes() == a.keep.tobytes()
    assert lo.stat.tobytes() + hi.stat.tobytes() == a.stat.tobytes()
    assert lo.F.tobytes() + hi.F.tobytes() == a.F.tobytes()
    # another seed draws other samples
    assert run(tab, seed=6, **kw).stat.tobytes() != a.stat.tobytes()


def test_edge_thresholds():
    tab = VR.mixed()
    table = table_of(tab)
    attempted = VR.verify(tab, iters=VR.MIXED_ITERS)["stat"][:, 0] >= 0
    for thr in (0.0, -1.0, float("nan")):
        v = run(tab, iters=VR.MIXED_ITERS, threshold=thr, min_inliers=0, table=table)
        assert not v.keep.any() and np.isnan(v.F).all()
        assert v.stat[attempted].tolist() == [[0, 0, VR.MIXED_ITERS, 0]] * int(attempted.sum())
        assert v.stat[~attempted].tolist() == [[-1, -1, 0, 0]] * int((~attempted).sum())
    v = run(tab, iters=VR.MIXED_ITERS, threshold=float("inf"), min_inliers=0, table=table)
    for p in range(len(tab["pairs"])):
        ok, n, valid, _, _ = VR.correspondences(tab, p)
        want = np.zeros(tab["cap"], np.uint8)
        if ok:
            want[:n] = valid
            assert v.stat[p, 0] == valid.sum() and v.stat[p, 3] == 1
        assert np.array_equal(v.keep[p], want), p


def test_through_the_real_path():
    """synth frames -> FeatureCache -> all-pairs matches -> verify_matches (from the device triple and
    from the host list: identical) -> build_tracks(keep=...), against the restatements."""
    import torch
    from sfmfromscratch_amd import sequence as S, synth
    from sfmfromscratch_amd.pipeline import BatchMatcher
    from tests import tracks_ref as TR
    from tests.golden_util import P_OCT
    frames = [synth.make_frame(180, 300, 61, i) for i in range(4)]
    cache = S.FeatureCache(frames, dict(P_OCT, num_interest_points=300))
    pairs = S.pair_schedule(4, "all")
    dev = cache.slots.desc.device
    triple = BatchMatcher(0.85, device=0, ctx=cache.extractor.ctx).match(cache.slots, torch.from_numpy(pairs).to(dev))
    host = S.match_schedule(cache, pairs, 0.85)
    thr, iters = 1.0, 512
    v = S.verify_matches(cache, pairs, triple, threshold=thr, max_iterations=iters)
    vh = S.verify_matches(cache, pairs, host, threshold=thr, max_iterations=iters)
    assert raw_bytes(v) == raw_bytes(vh)
    cap = cache.cap
    nm = triple[2].cpu().numpy()
    mm = triple[0].cpu().numpy()
    xy, count = cache.slots.xy.cpu().numpy(), cache.slots.count.cpu().numpy()
    print("nmatch", nm.tolist(), "stat", v.stat.tolist())
    assert (v.verified).any()
    sums = v.keep.sum(axis=1)
    assert np.array_equal(sums, np.where(v.verified, v.n_inliers, 0))
    for p in range(len(pairs)):
        n = max(int(nm[p]), 0)
        assert not v.keep[p, n:].any()
        if not v.verified[p]:
            continue
        a, b = pairs[p]
        p1, p2 = xy[a, mm[p, :n, 0]], xy[b, mm[p, :n, 1]]   # every match of the matcher is valid
        d = RR.distances(v.F[p], p1, p2, np.float64)[0]
        k = v.keep[p, :n] != 0
        assert (d[k] < thr + RR.D_BOUND).all() and (d[~k] > thr - RR.D_BOUND).all()
    # the filtered host list holds exactly the kept matches and their confidences, value for value,
    # from the device triple and from the host list alike
    for res in (v, vh):
        for p, (m, c) in enumerate(res.inlier_matches()):
            sel = np.flatnonzero(res.keep[p])
            assert len(m) == sums[p] and len(c) == sums[p]
            if sums[p]:
                assert m.dtype == np.int64 and c.dtype == np.float32
                assert np.array_equal(m, host[p][0][sel]) and np.array_equal(c, host[p][1][sel])
                assert np.array_equal(m, mm[p, sel])
    # a caller without confidences (conf=None in the triple, bare match arrays in the list) gets ones
    for res in (S.verify_matches(cache, pairs, (triple[0], None, triple[2]), threshold=thr, max_iterations=iters),
                S.verify_matches(cache, pairs, [h[0] for h in host], threshold=thr, max_iterations=iters)):
        assert raw_bytes(res) == raw_bytes(v)
        for p, (m, c) in enumerate(res.inlier_matches()):
            assert len(c) == sums[p] and (np.asarray(c) == 1).all()
    with pytest.raises(ValueError, match="verify_matches: pair 0 has"):
        S.verify_matches(cache, pairs, [(host[0][0], host[0][1][:-1])] + host[1:], threshold=thr, max_iterations=iters)
    with pytest.raises(ValueError, match="verify_matches: one"):
        S.verify_matches(cache, pairs, host[:-1], threshold=thr, max_iterations=iters)
    # and the tracks are those of the restatement with that mask
    for min_len in (2, 3):
        tr = S.build_tracks(cache, pairs, triple, keep=v.keep_dev, min_len=min_len)
        e = TR.build_tracks(count, cap, pairs, mm, nm, v.keep, min_len)
        assert tr.stats == dict(zip(TR.STATS, e["out_n"].tolist()))
        for key in ("offsets", "obs_slot", "obs_row", "node_track"):
            assert np.array_equal(getattr(tr, key), e[key]), key
    assert tr.n_tracks > 0


def test_binding_rejects_tensors_the_c_abi_would_misread():
    """Contiguity, dtype, device and size are checked before the address is handed over; argument
    errors of the call itself come back as SFM_EINVAL."""
    import torch
    from sfmfromscratch_amd import sequence as S
    tab = VR.mixed()
    t = table_of(tab)
    dev = t.xy.device
    mm, _, nm = triple_of(tab, dev)
    kw = dict(max_iterations=10)
    with pytest.raises(ValueError, match="int32"):
        S.verify_matches(t, tab["pairs"], (mm.long(), None, nm), **kw)
    with pytest.raises(ValueError, match="contiguous"):
        S.verify_matches(t, tab["pairs"], (mm.flip(2).transpose(0, 1).contiguous().transpose(0, 1), None, nm), **kw)
    with pytest.raises(ValueError, match="context's device"):
        S.verify_matches(t, tab["pairs"], (mm, None, nm.cpu()), **kw)
    with pytest.raises(ValueError, match="fewer"):
        S.verify_matches(t, tab["pairs"], (mm, None, nm[:3]), **kw)
    with pytest.raises(ValueError):
        S.verify_matches(t, tab["pairs"], (mm[:, :4], None, nm), **kw)
    with pytest.raises(ValueError, match="int32"):
        S.verify_matches(types.SimpleNamespace(count=t.count, xy=t.xy.long()), tab["pairs"], (mm, None, nm), **kw)
    with pytest.raises(ValueError, match="fewer"):
        S.verify_matches(types.SimpleNamespace(count=t.count[:2], xy=t.xy), tab["pairs"], (mm, None, nm), **kw)
    # the call's own argument checks
    for bad in (dict(max_iterations=-1), dict(max_iterations=(1 << 20) + 1), dict(max_iterations=10, min_inliers=-1)):
        with pytest.raises(ValueError, match="sfm_verify_matches_dev"):
            S.verify_matches(t, tab["pairs"], (mm, None, nm), **bad)
    from sfmfromscratch_amd import _abi
    from sfmfromscratch_amd._native import context_for
    ctx = context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), 0)
    P, cap = len(tab["pairs"]), tab["cap"]
    keep = torch.empty((P, cap), dtype=torch.uint8, device=dev)
    F = torch.empty((P, 9), dtype=torch.float64, device=dev)
    stat = torch.empty((P, 4), dtype=torch.int32, device=dev)
    pt = torch.from_numpy(tab["pairs"]).to(dev)
    with pytest.raises(ValueError, match="n_stop"):
        ctx.verify_matches_dev(t.xy, t.count, pt, mm, nm, 10, 1.0, 0, 5, np.full(65, 0.5), keep, F, stat)
    with pytest.raises(ValueError, match="uint8"):
        ctx.verify_matches_dev(t.xy, t.count, pt, mm, nm, 10, 1.0, 0, 5, None, keep.int(), F, stat)
    with pytest.raises(ValueError, match="fewer"):
        ctx.verify_matches_dev(t.xy, t.count, pt, mm, nm, 10, 1.0, 0, 5, None, keep, F[:2], stat)
    args = [t.xy.data_ptr(), t.count.data_ptr(), len(tab["count"]), cap, pt.data_ptr(), P, mm.data_ptr(),
            nm.data_ptr(), 10, 1.0, 0, 5, None, 0, keep.data_ptr(), F.data_ptr(), stat.data_ptr(), None]
    fn = ctx.lib.sfm_verify_matches_dev
    assert fn(ctx.handle, *args) == _abi.SFM_OK
    for k, val in ((0, None), (1, None), (2, 0), (3, 0), (4, None), (5, -1), (6, None), (7, None), (13, 1), (14, None),
                   (15, None), (16, None)):
        bad = list(args)
        bad[k] = val
        assert fn(ctx.handle, *bad) == _abi.SFM_EINVAL, k
    empty = list(args)
    for k in (4, 6, 7, 14, 15, 16):   # every array indexed by p may be null when P == 0
        empty[k] = None
    empty[5] = 0
    assert fn(ctx.handle, *empty) == _abi.SFM_OK
    torch.cuda.synchronize()


def test_captured_into_a_graph_and_replayed():
    """The call allocates nothing and synchronises nothing: captured on a side stream and replayed,
    it writes the bytes of the plain call."""
    import torch
    if not (hasattr(torch.cuda, "CUDAGraph") and hasattr(torch.cuda, "graph")):
        pytest.skip("this torch build has no stream capture (torch.cuda.graph)")
    from sfmfromscratch_amd import _abi
    from sfmfromscratch_amd._native import context_for
    tab = VR.mixed()
    t = table_of(tab)
    dev = t.xy.device
    mm, _, nm = triple_of(tab, dev)
    plain = run(tab, iters=VR.MIXED_ITERS, confidence=VR.CONFIDENCE, table=t)
    want = raw_bytes(plain)
    ctx = context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), 0)
    P, cap = len(tab["pairs"]), tab["cap"]
    keep = torch.zeros((P, cap), dtype=torch.uint8, device=dev)
    F = torch.zeros((P, 9), dtype=torch.float64, device=dev)
    stat = torch.zeros((P, 4), dtype=torch.int32, device=dev)
    pt = torch.from_numpy(tab["pairs"]).to(dev)
    stop = VR.stop_ratios(VR.CONFIDENCE, VR.MIXED_ITERS)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.verify_matches_dev(t.xy, t.count, pt, mm, nm, VR.MIXED_ITERS, 1.0, 16, VR.SEED, stop, keep, F, stat,
                               torch.cuda.current_stream(dev).cuda_stream)
    for _ in range(2):
        keep.fill_(7)
        F.zero_()
        stat.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = keep.cpu().numpy().tobytes() + F.cpu().numpy().tobytes() + stat.cpu().numpy().tobytes()
        assert got == want
