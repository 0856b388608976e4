"""The sweep's "proven unmatched" certificate (csrc/match_mfma.hip proven_unmatched) restated in
numpy float32 on top of tests/match_ref.py, and tables whose rows' exact nndr sits in narrow
bands around the ratio threshold.

The certificate, per query row with a finite 2E: r1 <= r2 the row's two smallest d~ over every
target, E = 0.5 (2E);
    L = max(r1 - E, 0), one ulp toward zero if positive      (<= the exact smallest distance)
    U = r2 + E, one ulp up                                   (>= the exact second smallest)
    t = sqrt(L) / sqrt(U)                                    (float32, correctly rounded: monotone)
    proven unmatched  <=>  U > 0, U finite, t > ratio.
"""
from __future__ import annotations

import numpy as np

from tests import match_ref as R

f32 = np.float32
RATIOS = (0.5, 0.85, 1.0, 1.5)
DELTAS = (1e-6, 1e-4, 1e-3)     # half-widths of the bands of exact nndr around the ratio
PLANT_REPS = 3                  # planted rows per (band, side)


def certificate(r1, r2, E, ratio):
    """fires [n] bool for float32 arrays r1, r2 (two smallest d~) and E (match_ref.bound)."""
    r1, r2, E = (np.ascontiguousarray(x, f32) for x in (r1, r2, E))
    with np.errstate(all="ignore"):
        E2 = f32(2.0) * E
        Eh = f32(0.5) * E2
        L = np.maximum(r1 - Eh, f32(0.0))
        L = np.where(L > 0, (L.view(np.uint32) - np.uint32(1)).view(f32), L)
        U = r2 + Eh
        up = ((U.view(np.uint32) & np.uint32(0x7fffffff)) + np.uint32(1)).view(f32)   # +inf -> NaN
        U = np.where(U >= 0, up, U)
        t = np.sqrt(L) / np.sqrt(U)
        return (E2 <= f32(3.0e38)) & (U > 0) & (U < np.inf) & (t > f32(ratio))


def two_smallest(d):
    """Per row the two smallest of d [n1, n2 >= 2]."""
    p = np.partition(d, 1, axis=1)
    return p[:, 0], p[:, 1]


def nominal_top2(a):
    """r1, r2 of every row from match_ref's d~ (float64) rounded to float32."""
    return two_smallest(a["dt"].astype(f32))


def adversarial_top2(a):
    """The device forms d~ in float32 (MFMA accumulation, two fmas): each of its d~ lies within
    T2 + T3 (match_ref's docstring) of the float64 d~.  -> the largest r1 and the smallest r2
    any such evaluation can give, rounded outward to float32: where the certificate fires most
    readily."""
    t2, t3, _ = R.rounding_terms(a["qa"], a["tb"], a["d64"])
    s = t2 + t3
    hi1 = (a["dt"] + s).min(axis=1)
    lo2 = two_smallest(a["dt"] - s)[1]
    r1 = hi1.astype(f32)
    r1 = np.where(r1.astype(np.float64) < hi1, np.nextafter(r1, f32(np.inf)), r1)
    r2 = lo2.astype(f32)
    r2 = np.where(r2.astype(np.float64) > lo2, np.nextafter(r2, f32(-np.inf)), r2)
    return r1, r2


def reference_nndr(q, t):
    """The reference matcher's nndr of every query row (NaN where its second distance is 0): one
    run of match_ref.match with an infinite ratio keeps every row the `> 0` rule lets through."""
    m, c = R.match(q, t, np.inf)
    out = np.full(q.shape[0], np.nan, f32)
    out[m[:, 0]] = c
    return out


def unmatched(nndr, ratio):
    """Rows without a match at `ratio` given reference_nndr's output."""
    with np.errstate(invalid="ignore"):
        return ~(nndr <= f32(ratio))


def _rootsift_like(rng, n):
    h = rng.integers(0, 40, (n, 128)) * (rng.integers(0, 4, (n, 128)) == 0)
    h[h.sum(axis=1) == 0, 0] = 1
    return np.sqrt(h / h.sum(axis=1, keepdims=True))


def planted(ratio, seed=5):
    """-> queries [18, 128], targets [36 + 40, 128] (float32) and the aimed offsets [18]: query row
    i has its nearest target at distance (ratio + off_i) d and its second nearest at d = 0.2, far
    inside every other target's distance, with off_i = +-delta / 2 for delta in DELTAS (for
    ratio >= 1 both signs are planted below the ratio: nndr <= 1 always)."""
    rng = np.random.default_rng(seed)
    offs = np.array([s * 0.5 * dl for dl in DELTAS for s in (1.0, -1.0) for _ in range(PLANT_REPS)])
    if ratio >= 1.0:
        offs = -np.abs(offs)
    q = _rootsift_like(rng, len(offs))
    t = []
    for a, off in zip(q, offs):
        u, v = rng.standard_normal(128), rng.standard_normal(128)
        u /= np.linalg.norm(u)
        v -= (v @ u) * u
        v /= np.linalg.norm(v)
        t.append(a + (ratio + off) * 0.2 * u)
        t.append(a + 0.2 * v)
    t = np.concatenate([np.array(t), _rootsift_like(rng, 40)])
    return np.ascontiguousarray(q, f32), np.ascontiguousarray(t, f32), offs


def rootsift_mixed(n1, n2, seed):
    """RootSIFT-like tables (synth.make_descriptor_table, the generator of match_ref's `unit`
    cases) whose even query rows are near-duplicates of targets and whose odd query rows are
    fresh: matched and unmatched rows side by side.  (Every query row of the `unit` cases is a
    near-duplicate, so the reference matches all of them and no sound certificate can fire.)"""
    from sfmfromscratch_amd import synth
    t, hb = synth.make_descriptor_table(n2, seed)
    q, _ = synth.make_descriptor_table(n1, seed + 1, dup_of=hb, jitter=2)
    fresh, _ = synth.make_descriptor_table(n1, seed + 2)
    q = q.copy()
    q[1::2] = fresh[1::2]
    return np.ascontiguousarray(q, f32), np.ascontiguousarray(t, f32)


def analysis_of(q, t):
    """match_ref.analysis for a table outside match_ref.CASES."""
    qa, tb = R.operands(q), R.operands(t)
    return {"qa": qa, "tb": tb, "E": R.bound(qa, tb), "dt": R.dtilde(qa, tb), "d32": R.sqdist32(q, t),
            "d64": R.sqdist64(q, t)}
