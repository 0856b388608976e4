"""GPU: feature tracks on the device (sequence.build_tracks, tracks.hip) against the numpy
restatement of tests/tracks_ref.py.  Every comparison is integer equality; the conditions the
cases must meet are asserted on the CPU in tests/test_tracks_cpu.py."""
from __future__ import annotations

import types

import numpy as np
import pytest

from tests import tracks_ref as TR

pytestmark = pytest.mark.gpu

OUT_KEYS = ("offsets", "obs_slot", "obs_row", "node_track")


def table_of(c, xy=None):
    """A slot table stand-in (count, xy) on the device for case c."""
    import torch
    dev = torch.device("cuda", 0)
    nimg, cap = len(c["count"]), c["cap"]
    if xy is None:
        xy = np.arange(nimg * cap * 2, dtype=np.int32).reshape(nimg, cap, 2)
    return types.SimpleNamespace(count=torch.from_numpy(np.ascontiguousarray(c["count"], np.int32)).to(dev),
                                 xy=torch.from_numpy(np.ascontiguousarray(xy, np.int32)).to(dev))


def run_case(c, min_len=2, table=None):
    """The case through sequence.build_tracks with its matches as the device triple."""
    import torch
    from sfmfromscratch_amd import sequence as S
    table = table or table_of(c)
    dev = table.xy.device
    mm = torch.from_numpy(c["matches"]).to(dev)
    nm = torch.from_numpy(c["nmatch"]).to(dev)
    keep = None if c["keep"] is None else torch.from_numpy(c["keep"]).to(dev)
    return S.build_tracks(table, c["pairs"], (mm, None, nm), keep=keep, min_len=min_len)


def assert_equals_restatement(tr, e):
    assert tr.stats == dict(zip(TR.STATS, e["out_n"].tolist()))
    for k in OUT_KEYS:
        got = getattr(tr, k)
        assert got.dtype == np.int32 and np.array_equal(got, e[k]), k
    assert tr.n_tracks == len(e["offsets"]) - 1


def raw_bytes(tr):
    return b"".join(np.ascontiguousarray(getattr(tr, k)).tobytes() for k in OUT_KEYS) + \
        np.array(list(tr.stats.values()), np.int32).tobytes()


@pytest.mark.parametrize("min_len", [2, 3])
@pytest.mark.parametrize("name", TR.CASE_NAMES)
def test_tracks_equal_the_restatement(name, min_len):
    """The hand graph, the size edges (cap 1, 63, 64, 65, 257 x nimg 2, 3, 65; P = 0; all counts
    zero), the 300-slot chain listed backwards, the two giant components and the random graph."""
    tr = run_case(TR.case(name), min_len)
    print(name, min_len, tr.stats)
    assert_equals_restatement(tr, TR.expected(name, min_len))


def test_hand_graph_from_the_host_list():
    """The hand graph as match_schedule's host list with one keep mask per pair (nmatch -1 cannot
    be written that way: that pair is given empty, which is the same graph)."""
    from sfmfromscratch_amd import sequence as S
    c = TR.case("hand")
    host, keep = [], []
    for p in range(len(c["pairs"])):
        k = max(int(c["nmatch"][p]), 0)
        host.append((c["matches"][p, :k].astype(np.int64), np.ones(k, np.float32)) if k
                    else (np.array([]), np.array([])))
        keep.append(c["keep"][p, :k])
    tr = S.build_tracks(table_of(c), c["pairs"], host, keep=keep)
    assert_equals_restatement(tr, TR.expected("hand", 2))
    nt = tr.node_track
    assert nt[0, 1] == nt[1, 1] == nt[2, 1] == nt[2, 2] == -2 and nt[2, 3] == -1
    assert tr.offsets.tolist() == [0, 4, 6]


@pytest.mark.parametrize("name", ["random", "giant", "long_path"])
def test_order_independence_and_determinism(name):
    """The pairs permuted and the matches permuted within each pair, and the same call twice: the
    same bytes."""
    c = TR.case(name)
    a = raw_bytes(run_case(c, 3))
    b = raw_bytes(run_case(c, 3))
    p = raw_bytes(run_case(TR.permuted(c, 5), 3))
    assert a == b
    assert a == p


def test_through_the_real_path():
    """synth frames -> FeatureCache -> all-pairs matches -> build_tracks, from the host list and
    from the device triple: both equal the restatement applied to those matches."""
    import torch
    from sfmfromscratch_amd import sequence as S, synth
    from sfmfromscratch_amd.pipeline import BatchMatcher
    from tests.golden_util import P_OCT
    frames = [synth.make_frame(180, 300, 61, i) for i in range(4)]
    cache = S.FeatureCache(frames, dict(P_OCT, num_interest_points=300))
    pairs = S.pair_schedule(4, "all")
    host = S.match_schedule(cache, pairs, 0.85)
    count = cache.slots.count.cpu().numpy()
    cap = cache.cap
    mm = np.zeros((len(pairs), cap, 2), np.int32)
    nm = np.zeros(len(pairs), np.int32)
    for p, (m, _) in enumerate(host):
        nm[p] = len(m)
        mm[p, :len(m)] = np.asarray(m).reshape(-1, 2)
    assert nm.sum() > 0
    for min_len in (2, 3):
        e = TR.build_tracks(count, cap, pairs, mm, nm, None, min_len)
        assert e["out_n"][0] > 0
        assert_equals_restatement(S.build_tracks(cache, pairs, host, min_len=min_len), e)
        dev = cache.slots.desc.device
        matcher = BatchMatcher(0.85, device=0, ctx=cache.extractor.ctx)
        triple = matcher.match(cache.slots, torch.from_numpy(pairs).to(dev))
        tr = S.build_tracks(cache, pairs, triple, min_len=min_len)
        assert_equals_restatement(tr, e)
    # the observations' pixels are the table's
    xy = cache.slots.xy.cpu().numpy()
    assert np.array_equal(tr.obs_xy, xy[tr.obs_slot, tr.obs_row])


def test_save_load_round_trip_and_ba_inputs(tmp_path):
    from sfmfromscratch_amd import sequence as S
    c = TR.case("random")
    rng = np.random.default_rng(3)
    xy = rng.integers(0, 2000, (len(c["count"]), c["cap"], 2)).astype(np.int32)
    tr = run_case(c, 3, table_of(c, xy))
    cam, pt, p2 = tr.ba_inputs()
    off = tr.offsets
    assert cam.dtype == np.int64 and pt.dtype == np.int64 and p2.dtype == np.float64 and p2.shape == (tr.n_obs, 2)
    for t in (0, tr.n_tracks // 2, tr.n_tracks - 1):
        sl = slice(off[t], off[t + 1])
        assert (pt[sl] == t).all() and np.array_equal(cam[sl], tr.obs_slot[sl])
        assert np.array_equal(p2[sl], xy[tr.obs_slot[sl], tr.obs_row[sl]].astype(np.float64))
    assert np.array_equal(np.bincount(pt, minlength=tr.n_tracks), np.diff(off))
    path = str(tmp_path / "tracks.npz")
    tr.save(path)
    with np.load(path) as z:
        assert str(z["format"]) == "sfmfeat-tracks-v1"
    back = S.Tracks.load(path)
    assert raw_bytes(back) == raw_bytes(tr) and back.min_len == 3
    for a, b in zip(back.ba_inputs(), (cam, pt, p2)):
        assert np.array_equal(a, b)
    bad = str(tmp_path / "bad.npz")
    np.savez(bad, format=np.array("sfmfeat-matches-v1"))
    with pytest.raises(ValueError):
        S.Tracks.load(bad)


def test_binding_rejects_tensors_the_c_abi_would_misread():
    """Contiguity, dtype, device and size are checked before the address is handed over."""
    import torch
    from sfmfromscratch_amd import sequence as S
    c = TR.case("hand")
    t = table_of(c)
    dev = t.xy.device
    mm = torch.from_numpy(c["matches"]).to(dev)
    nm = torch.from_numpy(c["nmatch"]).to(dev)
    with pytest.raises(ValueError, match="int32"):
        S.build_tracks(t, c["pairs"], (mm.long(), None, nm))
    with pytest.raises(ValueError, match="contiguous"):
        S.build_tracks(t, c["pairs"], (mm.flip(2).transpose(0, 1).contiguous().transpose(0, 1), None, nm))
    with pytest.raises(ValueError, match="context's device"):
        S.build_tracks(t, c["pairs"], (mm, None, nm.cpu()))
    with pytest.raises(ValueError, match="fewer"):
        S.build_tracks(t, c["pairs"], (mm, None, nm[:3]))
    with pytest.raises(ValueError):
        S.build_tracks(t, c["pairs"], (mm[:, :4], None, nm))
    with pytest.raises(ValueError, match="min_len"):
        S.build_tracks(t, c["pairs"], (mm, None, nm), min_len=1)
