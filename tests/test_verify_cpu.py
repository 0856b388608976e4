"""CPU: the conditions the GPU tests of sfm_verify_matches_dev (tests/test_gpu_verify.py) rest on —
the counter-based sampler of the restatement (tests/verify_ref.py), pose.ransac_stop_ratios, the
distance of every evaluated (sample, valid match) from the threshold in every case compared on the
GPU, both branches of the stop test, and the call's argument errors.

Figures printed before their assertions: the closest |d - threshold| per case (the bound is
ransac_ref.D_BOUND = 1e-6 px, the project's measured bound for two float64 routes of this fit)."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native, pose
from tests import ransac_ref as RR
from tests import verify_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the sampler
def dense_sample(seed, a, b, it, n):
    """The rule on a real arange(n) in numpy uint64 arithmetic: an implementation that shares no
    code with verify_ref.sample (which records only the swapped positions)."""
    u = np.uint64
    with np.errstate(over="ignore"):
        def mix(z):
            z = u(z)
            z ^= z >> u(30)
            z *= u(0xBF58476D1CE4E5B9)
            z ^= z >> u(27)
            z *= u(0x94D049BB133111EB)
            z ^= z >> u(31)
            return z
        key = mix(mix(u(seed & VR.M64)) + u((a << 32) | b))
        arr = np.arange(n)
        for k in range(8):
            r = int(mix(key + u(8 * it + k + 1) * u(VR.G)) >> u(32))
            j = k + ((r * (n - k)) >> 32)
            arr[k], arr[j] = arr[j], arr[k]
    return arr[:8].tolist()


@pytest.mark.parametrize("n", [8, 9, 255, 256, 257, 40000])
def test_sample_indices_are_distinct_and_in_range(n):
    for a, b in ((0, 1), (2, 0), (255, 254)):
        s = VR.samples(VR.SEED, a, b, n, 300)
        assert s.shape == (300, 8) and s.min() >= 0 and s.max() < n
        assert all(len(set(row)) == 8 for row in s.tolist())
        if n == 8:
            assert (np.sort(s, axis=1) == np.arange(8)).all()   # a permutation
        for it in (0, 1, 255, 299):
            assert s[it].tolist() == dense_sample(VR.SEED, a, b, it, n)


def test_stream_depends_on_seed_slots_and_sample_only():
    base = VR.sample(5, 3, 7, 11, 100)
    assert VR.sample(5, 3, 7, 11, 100) == base
    assert VR.sample(6, 3, 7, 11, 100) != base and VR.sample(5, 7, 3, 11, 100) != base
    assert VR.sample(5, 3, 8, 11, 100) != base and VR.sample(5, 3, 7, 12, 100) != base
    # a negative seed is its two's complement
    assert VR.sample(-7, 3, 7, 11, 100) == VR.sample((1 << 64) - 7, 3, 7, 11, 100)
    # the samples of a call are those of its pairs alone: samples() takes nothing else
    assert VR.samples(5, 3, 7, 100, 20)[11].tolist() == base


def test_pinned_samples_and_uniformity():
    # worked through by hand from the rule (and equal to dense_sample above)
    assert VR.mix64(0) == 0 and VR.mix64(1) == 0x5692161D100B05E5
    assert VR.sample(5, 0, 1, 0, 8) == [3, 5, 4, 6, 2, 7, 0, 1]
    assert VR.sample(5, 2, 0, 3, 40) == [22, 38, 20, 5, 15, 34, 14, 24]
    assert VR.sample(-7, 1, 2, 699, 40000) == [14492, 26459, 35066, 30111, 24151, 12475, 35847, 20347]
    hits = np.bincount(VR.samples(5, 0, 1, 11, 20000).ravel(), minlength=11)
    print("20,000 samples at n = 11, hits per index:", hits.min(), "-", hits.max(), "(expected 14,545)")
    assert hits.min() == 14409 and hits.max() == 14628


# ---------------------------------------------------------------- the stop table
def test_stop_ratios_reach_the_confidence_and_decrease():
    for conf in (0.98, 0.5, 0.999999):
        w = pose.ransac_stop_ratios(conf, 64)
        r = np.arange(1, 65)
        assert w.dtype == np.float64 and w.shape == (64,)
        got = 1.0 - (1.0 - w ** 8) ** (256 * r)
        print(f"confidence {conf}: worst |1 - (1 - w^8)^(256 r) - confidence| = {np.abs(got - conf).max():.3e}")
        assert np.abs(got - conf).max() < 1e-12
        assert (np.diff(w) < 0).all() and (w > 0).all() and (w < 1).all()
    assert len(pose.ransac_stop_ratios(0.98, 0)) == 0
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            pose.ransac_stop_ratios(bad, 3)


# ---------------------------------------------------------------- the cases of the GPU tests
GPU_ITERS = (0, 1, 255, 256, 257, 700)


@pytest.mark.parametrize("name", list(VR.SINGLE))
def test_every_case_keeps_its_distance_from_the_threshold(name):
    """Over all 700 samples (a superset of what any iteration count or stop table evaluates)."""
    tab = VR.single(name)
    r = VR.verify(tab, stop=None)
    n = int(tab["nmatch"][0])
    print(f"{name}: n {n}, stat {r['stat'][0].tolist()}, closest |d - threshold| {r['margin'][0]:.3e} px")
    if n < 8:
        assert r["stat"][0].tolist() == [-1, -1, 0, 0] and not r["keep"].any() and np.isnan(r["F"]).all()
        return
    assert r["margin"][0] > RR.D_BOUND
    assert r["keep"][0].sum() == (r["stat"][0, 0] if r["stat"][0, 3] else 0)
    assert tab["cap"] > n and not r["keep"][0, n:].any()


def test_both_branches_of_the_stop_test_are_taken():
    stop = VR.stop_ratios()
    assert len(stop) == 3
    for name, samples in VR.STOPS_EARLY.items():
        s = VR.verify(VR.single(name), stop=stop)["stat"][0]
        full = VR.verify(VR.single(name), stop=None)["stat"][0]
        print(name, "with the 0.98 table", s.tolist(), "fixed", full.tolist())
        assert s[2] == samples and full[2] == VR.ITERS
    for name in VR.RUNS_ALL:
        s = VR.verify(VR.single(name), stop=stop)["stat"][0]
        print(name, "with the 0.98 table", s.tolist())
        assert s[2] == VR.ITERS
    # the multi-chunk case with invalid rows: its first round (the only one the table lets it run)
    # holds samples that contain an invalid match, and samples that do not
    t = VR.single("n2700_bad")
    _, n, valid, _, _ = VR.correspondences(t, 0)
    _, F, _ = VR.sample_table(t, 0, VR.ROUND)
    dead = int(np.isnan(F[:, 0, 0]).sum())
    print(f"n2700_bad: n {n}, {int((~valid).sum())} invalid matches, {dead} of the first 256 samples contain one")
    assert n > 2560 and (~valid).sum() == VR.BAD_ROWS["n2700_bad"] and 0 < dead < VR.ROUND
    # a stop changes the winner where a later round holds a better sample
    assert any(VR.verify(VR.single(k), stop=stop)["stat"][0, 0] < VR.verify(VR.single(k))["stat"][0, 0]
               for k in VR.SINGLE if VR.SINGLE[k][1] >= 8)


def test_min_inliers_decides_at_the_winning_count():
    tab = VR.single("n40")
    best = int(VR.verify(tab)["stat"][0, 0])
    assert best > 16
    for mi, ok in ((0, 1), (best, 1), (best + 1, 0)):
        r = VR.verify(tab, min_inliers=mi)
        assert r["stat"][0].tolist()[::3] == [best, ok] and r["keep"].sum() == best * ok
        assert np.isfinite(r["F"]).all()   # the winner's F, verified or not


@pytest.mark.parametrize("threshold", [1.0, 1e-9])
def test_the_mixed_table_holds_what_its_docstring_says(threshold):
    t = VR.mixed()
    nimg, cap = len(t["count"]), t["cap"]
    assert cap == 131 and t["nmatch"].max() > cap and t["nmatch"].min() == -1
    r = VR.verify(t, iters=VR.MIXED_ITERS, threshold=threshold, stop=VR.stop_ratios(iters=VR.MIXED_ITERS))
    print(f"threshold {threshold}: stat {r['stat'].tolist()}, margins {r['margin'].tolist()}")
    attempted = r["stat"][:, 0] >= 0
    assert attempted.tolist() == [True, False, True, True, False, False, False, True, False]
    assert (r["margin"][attempted] > RR.D_BOUND).all()
    _, n7, valid7, _, _ = VR.correspondences(t, 7)
    assert n7 == 120 and valid7.sum() == 90
    _, n2, valid2, _, _ = VR.correspondences(t, 2)
    assert n2 == cap and valid2.sum() == 120
    m7 = t["matches"][7, :n7]
    assert (m7[:, 0] >= cap).any() and (m7[:, 1] < 0).any() and ((m7[:, 0] >= 120) & (m7[:, 0] < cap)).any()
    if threshold == 1.0:
        assert r["stat"][[0, 2, 7], 3].all() and r["stat"][0, 2] < VR.MIXED_ITERS     # one of them stops early
        assert r["stat"][VR.MIXED_RANDOM].tolist()[::3] == [8, 0]                      # a sample's own points only
        # some samples of pair 7 contain an invalid match and count 0
        idx, F, _ = VR.sample_table(t, 7, VR.MIXED_ITERS)
        assert np.isnan(F[:, 0, 0]).any() and np.isfinite(F[:, 0, 0]).any()
    else:
        assert not r["keep"].any() and np.isnan(r["F"]).all() and (r["stat"][attempted, 0] == 0).all()
        assert (r["stat"][attempted, 1] == 0).all()


# ---------------------------------------------------------------- the C ABI
C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}


def header_prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfmfeat.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sfmfeat.h"
    args = [ctypes.c_void_p if "*" in a else C_TYPES[a.replace("const ", "").split()[0]]
            for a in (a.strip() for a in m.group(2).split(","))]
    return C_TYPES[m.group(1)], args


def test_abi_declares_the_call_and_rejects_bad_arguments_before_any_device_call():
    res, args = header_prototype("sfm_verify_matches_dev")
    assert _native.SIGNATURES["sfm_verify_matches_dev"] == (res, args)
    lib = _native.load_library()
    fn = lib.sfm_verify_matches_dev
    assert lib.sfm_abi_version() == 1
    assert fn(*[None if a is ctypes.c_void_p else 0 for a in args]) == _abi.SFM_EINVAL
    # a context made without touching the device would be needed for the per-argument messages;
    # without one every call returns SFM_EINVAL at once, whatever else is passed
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    assert fn(None, p, p, 1, 1, p, 1, p, p, 10, 1.0, 0, 5, p, 1, p, p, p, None) == _abi.SFM_EINVAL


def test_docs_no_longer_leave_verification_to_the_caller():
    for rel in ("README.md", "include/sfmfeat.h", "sfmfromscratch_amd/sequence.py", "DESIGN.md"):
        text = open(os.path.join(ROOT, rel)).read()
        assert "none is built in" not in text and "No geometric verification is built in" not in text, rel
        assert "verify_matches" in text, rel
