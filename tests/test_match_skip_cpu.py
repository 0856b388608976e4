"""The sweep's "proven unmatched" certificate on the host: restated in numpy float32
(tests/match_skip_ref.py) over match_ref's operands, E and d~, it never fires for a row the
reference matches — on every in-range case family of match_ref.CASES and on tables whose rows'
exact nndr lies within 1e-6, 1e-4 and 1e-3 of the ratio, at ratios 0.5, 0.85, 1.0 and 1.5, with
the two smallest d~ taken both as float32 roundings of match_ref's float64 d~ and at the worst
point (largest smallest, smallest second smallest) the device's float32 evaluation of d~ can
reach (T2 + T3 of match_ref's docstring away).

Measured on the host (printed, never used as bounds): rows the certificate fires for, of the
reference's unmatched rows, of all rows, per ratio over the in-range cases and the two mixed
RootSIFT-like tables (adversarial top-2):
    0.5: 1160 / 2375 / 3538, 0.85: 891 / 2335 / 3538, 1.0: 0 / 2 / 3538, 1.5: 0 / 2 / 3538
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native
from tests import match_ref as R
from tests import match_skip_ref as S
from tests.test_abi_cpu import header_prototype

IN_RANGE = [i for i in range(len(R.CASES)) if R.in_f16_range(*R.case(i))]


@functools.lru_cache(maxsize=None)
def case_rows(i):
    """Case i -> (reference nndr per row, E, nominal (r1, r2), adversarial (r1, r2))."""
    a = R.analysis(i)
    return S.reference_nndr(*R.case(i)), a["E"], S.nominal_top2(a), S.adversarial_top2(a)


MIXED = ((130, 300, 7), (64, 31, 9))   # match_skip_ref.rootsift_mixed tables (n1, n2, seed)


@functools.lru_cache(maxsize=None)
def mixed_rows(k):
    q, t = S.rootsift_mixed(*MIXED[k])
    a = S.analysis_of(q, t)
    return S.reference_nndr(q, t), a["E"], S.nominal_top2(a), S.adversarial_top2(a)


@functools.lru_cache(maxsize=None)
def planted_rows(ratio):
    q, t, offs = S.planted(ratio)
    a = S.analysis_of(q, t)
    return S.reference_nndr(q, t), a["E"], S.nominal_top2(a), S.adversarial_top2(a), offs


@pytest.mark.parametrize("ratio", S.RATIOS)
def test_certificate_never_fires_for_a_row_the_reference_matches(ratio, capsys):
    fired = un = rows = 0
    sets = [(R.CASE_IDS[i], case_rows(i)) for i in IN_RANGE]
    sets += [("mixed%d" % k, mixed_rows(k)) for k in range(len(MIXED))]
    for name, (nndr, E, nominal, adversarial) in sets:
        assert np.isfinite(np.float32(2.0) * E).all()
        free = S.unmatched(nndr, ratio)
        for r1, r2 in (nominal, adversarial):
            f = S.certificate(r1, r2, E, ratio)
            assert not (f & ~free).any(), (name, ratio, np.flatnonzero(f & ~free)[:8])
        fired, un, rows = fired + int(f.sum()), un + int(free.sum()), rows + len(free)
        if ratio >= 1.0:
            assert not f.any(), name
    with capsys.disabled():
        print("\nratio %s: certificate fires for %d of %d unmatched rows (%d rows)" % (ratio, fired, un, rows))


@pytest.mark.parametrize("ratio", S.RATIOS)
def test_certificate_on_rows_planted_around_the_ratio(ratio):
    """Rows whose exact nndr sits within each band of the ratio the table was planted for, on both
    sides of it below 1; at 1.5 (no nndr exceeds 1) the table planted for 1.0 stands in."""
    base = min(ratio, 1.0)
    nndr, E, nominal, adversarial, offs = planted_rows(base)
    for k, dl in enumerate(S.DELTAS):
        band = slice(2 * S.PLANT_REPS * k, 2 * S.PLANT_REPS * (k + 1))
        dev = nndr[band].astype(np.float64) - np.float64(np.float32(base))
        assert np.all(np.abs(dev) <= dl), (dl, dev)
        if base < 1.0:
            assert (dev > 0).any() and (dev < 0).any(), (dl, dev)
    free = S.unmatched(nndr, ratio)
    if ratio < 1.0:
        assert free.any() and (~free).any()
    for r1, r2 in (nominal, adversarial):
        f = S.certificate(r1, r2, E, ratio)
        assert not (f & ~free).any(), (ratio, np.flatnonzero(f & ~free))
        if ratio >= 1.0:
            assert not f.any()


def test_certificate_is_not_vacuous_on_rootsift_like_tables():
    """It fires on RootSIFT-like tables at 0.85 and leaves a row just above the ratio alone.  Every
    query row of match_ref's `unit` cases is a near-duplicate of a target and matches, so nothing
    sound can fire there (asserted); the tables of match_skip_ref.rootsift_mixed come from the same
    generator with every other query row fresh, and there it must fire."""
    for i in IN_RANGE:
        if R.class_of(i) == "unit":
            nndr, E, (r1, r2), _ = case_rows(i)
            assert not S.unmatched(nndr, 0.85).any() and not S.certificate(r1, r2, E, 0.85).any()
    for k in range(len(MIXED)):
        nndr, E, (r1, r2), _ = mixed_rows(k)
        f = S.certificate(r1, r2, E, 0.85)
        assert f.sum() >= 1 and (~S.unmatched(nndr, 0.85)).sum() >= 1, MIXED[k]
    nndr, E, (r1, r2), _, _ = planted_rows(0.85)
    f = S.certificate(r1, r2, E, 0.85)
    assert (S.unmatched(nndr, 0.85) & ~f).any()


def test_certificate_edges():
    """+inf second distance (fewer than two targets), a non-finite bound, NaN, zero distances and a
    negative ratio: nothing is proven where the reference could still match."""
    f32 = np.float32
    one = lambda r1, r2, E, ratio: bool(S.certificate([r1], [r2], [E], ratio)[0])
    assert not one(0.3, np.inf, 2e-4, 0.85)
    assert not one(0.3, 0.31, np.inf, 0.85) and not one(0.3, 0.31, 2e38, 0.85)
    assert not one(np.nan, 0.31, 2e-4, 0.85) and not one(0.3, np.nan, 2e-4, 0.85)
    assert not one(0.0, 0.0, 2e-4, 0.85) and not one(-1e-5, 1e-5, 2e-4, 0.85)
    assert not one(0.3, 0.31, 2e-4, np.nan)
    assert one(0.3, 0.31, 2e-4, 0.85) and not one(0.3, 0.31, 2e-4, 1.0)
    assert one(0.0, 0.5, 2e-4, -1.0)      # nndr >= 0 > ratio whenever the second distance is positive
    assert not one(f32(3e38), f32(3.4e38), f32(1e38), 0.85)   # U overflows


def test_abi_declares_the_skip_read_back_with_the_headers_signature():
    res, args = header_prototype("sfm_debug_match_skips")
    assert _abi.MATCH_DEBUG_SIGNATURES["sfm_debug_match_skips"] == (res, args)
    assert _native.SIGNATURES["sfm_debug_match_skips"] == (res, args)
    fn = _native.load_library().sfm_debug_match_skips
    assert fn(*[None if a is ctypes.c_void_p else 0 for a in args]) == _abi.SFM_EINVAL
