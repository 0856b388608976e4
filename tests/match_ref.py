"""A plain restatement of the matcher that reads nothing of the library: the reference's
NN-ratio matcher written out literally, the prefilter's operands (csrc/match_mfma.hip
k_match_prep) bit for bit, its error bound E and approximate distance d~, and seeded case
generators that leave the RootSIFT family (non-negative, unit norm, well-separated neighbours)
every other matcher test stays in.

Everything here is numpy on the host.  Squared distances: `d_ref` is the reference's float32
`np.sum((a - b) ** 2, axis=2)` (numpy's pairwise order, which the library's re-rank restates),
`d64` the same in float64, `d~` the prefilter's approximation.

The bound and what it has to cover
----------------------------------
    E = 2^-15 |a| max|b|  +  4e-6 (|a|^2 + max|b|^2)  +  1.25e-4        (float32, per query row)

must bound |d~_device - d_ref| for every target of the pair.  With u = 2^-24 (float32 unit
roundoff, round to nearest) and gamma_k = k u / (1 - k u):

 1. |d~_f64 - d_ref|: d~ evaluated in float64 from the restated float16 operands and float32
    norms, against the actual reference value.  It holds the f16 hi / lo representation error,
    the dropped lo.lo product and the reference's own rounding; measured per (query, target).
 2. f32 accumulation of the three 128-term products.  Products of two f16 values are exact in
    float32; a chain of n products takes n - 1 rounded additions in some order, so its error is
    at most gamma_(n-1) sum|x_i y_i| whatever the order.  The hi.hi chain has 128 terms and
    enters d~ scaled by 2^-15; hi.lo and lo.hi share one chain of 256 terms scaled by 2^-26:
        T2 = 2^-15 gamma_127 sum|hi_a hi_b|  +  2^-26 gamma_255 sum(|hi_a lo_b| + |lo_a hi_b|)
 3. the roundings outside the MFMAs.  na, nb are float32 roundings of double sums (u |a|^2,
    u |b|^2; the double sum's own error, 7 2^-53 relative, is below the 1e-3 slack taken here);
    na + nb rounds once (u (na + nb)); each fma rounds once, and both results are at most
    na + nb + 2^-15 |ahh| + 2^-26 |ax| <= 2.01 (na + nb) in magnitude (2 |a.b| <= |a|^2 +
    |b|^2, and hi, lo exceed the element by at most 2^-11 relative):
        T3 = u (na + nb) (1 + 1 + 2.01 + 2.01) (1 + 1e-3)
 4. the reference's own float32 evaluation of sum((a - b)^2): the difference and the square
    round once each ((1 + u)^3 on the term), then 15 additions inside one of numpy's eight
    accumulators and 3 to combine them, all of non-negative terms:
        T4 = ((1 + u)^21 - 1) d64  +  150 * 2^-149   (the last for squares that underflow)
    (item 1 already holds the actual reference error; adding its worst case again only makes the
    check stricter.)

tests/test_match_ref_cpu.py asserts item 1 + T2 + T3 + T4 <= E for every (query, target) of
every case whose elements are inside the f16 range.
"""
from __future__ import annotations

import functools

import numpy as np

f32 = np.float32
U = 2.0 ** -24
F16_EDGE = 255.9375          # |x| * 2^8 >= 65520 rounds to +-inf in float16
CAND_CAP, HALF_CAP = 256, 128
PREP_ROWS = 16


# ---------------------------------------------------------------- the reference matcher
def sqdist32(a, b):
    """The reference's float32 squared distances [n1, n2] (NNRatioFeatureMatcher.py:31-34 before
    the sqrt), evaluated by the same numpy expression in blocks of query rows."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    out = np.empty((a.shape[0], b.shape[0]), f32)
    for i in range(0, a.shape[0], 32):
        out[i:i + 32] = np.sum((a[i:i + 32, np.newaxis] - b[np.newaxis, :]) ** 2, axis=2)
    return out


def sqdist64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]), np.float64)
    for i in range(0, a.shape[0], 32):
        out[i:i + 32] = np.sum((a[i:i + 32, np.newaxis] - b[np.newaxis, :]) ** 2, axis=2)
    return out


def match(f1, f2, ratio=0.85):
    """The reference's matcher, literally, with a stable argsort (ties: lowest index first).
    -> matches (k, 2) int64, confidences (k,) float32, in (nndr, row) order."""
    f1, f2 = np.ascontiguousarray(f1, f32), np.ascontiguousarray(f2, f32)
    if f1.shape[0] >= 1 and f2.shape[0] < 2:
        raise IndexError("index 1 is out of bounds")
    with np.errstate(over="ignore"):
        dists = np.sqrt(sqdist32(f1, f2))
    matches, confidences = [], []
    for d in range(dists.shape[0]):
        idx = np.argsort(dists[d], kind="stable")
        closest, second = idx[0], idx[1]
        if dists[d, second] > 0:
            nndr = dists[d, closest] / dists[d, second]
            if nndr <= f32(ratio):
                matches.append([d, closest])
                confidences.append(nndr)
    matches = np.array(matches, np.int64).reshape(-1, 2)
    confidences = np.array(confidences, f32)
    order = np.argsort(confidences, kind="stable")
    return matches[order], confidences[order]


# ---------------------------------------------------------------- operands, bit for bit
def operands(x, cap_rows=None):
    """k_match_prep of one slot: x [n, 128] float32 -> dict of hi, lo [capP, 128] float16,
    norm2, rnorm [capP] float32, pmax [capP / 16, 2] float32, flagged [n] bool.  capP: cap_rows
    (default n) rounded up to 128."""
    x = np.ascontiguousarray(x, f32).reshape(-1, 128)
    n = x.shape[0]
    capP = (max(cap_rows or n, 1) + 127) // 128 * 128
    with np.errstate(over="ignore", invalid="ignore"):
        xs = x * f32(256.0)                                   # exact: a power of two
        hi = xs.astype(np.float16)                            # round to nearest even
        lo = ((xs - hi.astype(f32)) * f32(2048.0)).astype(np.float16)   # exact difference and scaling
        flagged = ~(np.abs(hi.astype(f32)) <= f32(65504.0)).all(axis=1)
    hi[flagged] = 0
    lo[flagged] = 0
    # the squared norm in double, in the kernel's order: lane l adds x[l]^2 then x[l + 64]^2,
    # then the xor butterfly with offsets 32 .. 1 (every lane ends with the same sum; lane 0's)
    x64 = x.astype(np.float64)
    s = x64[:, :64] * x64[:, :64]
    s = s + x64[:, 64:] * x64[:, 64:]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[:, lanes ^ off]
    s = s[:, 0]
    with np.errstate(over="ignore"):
        n2 = s.astype(f32)
        rn = np.sqrt(s).astype(f32)
    rn[flagged] = np.inf
    H = np.zeros((capP, 128), np.float16)
    L = np.zeros((capP, 128), np.float16)
    N2 = np.full(capP, np.inf, f32)                           # padding rows: +inf
    RN = np.zeros(capP, f32)
    H[:n], L[:n], N2[:n], RN[:n] = hi, lo, n2, rn
    pm = np.zeros((capP // PREP_ROWS, 2), f32)
    for blk in range((n + PREP_ROWS - 1) // PREP_ROWS):
        r = slice(blk * PREP_ROWS, min((blk + 1) * PREP_ROWS, n))
        pm[blk] = (n2[r].max(), rn[r].max())
    return {"hi": H, "lo": L, "norm2": N2, "rnorm": RN, "pmax": pm, "flagged": flagged, "n": n}


def bound(qa, tb):
    """E of every query row of operands `qa` against the image `tb`, in float32 with the sweep's
    expression (no contraction): 2^-15 * ra * maxrn + 4e-6 * (na + maxn2) + 1.25e-4."""
    na, ra = qa["norm2"][:qa["n"]], qa["rnorm"][:qa["n"]]
    maxn2, maxrn = f32(tb["pmax"][:, 0].max()), f32(tb["pmax"][:, 1].max())
    with np.errstate(over="ignore", invalid="ignore"):
        return (f32(3.0517578125e-05) * ra * maxrn + f32(4e-6) * (na + maxn2)) + f32(1.25e-4)


def products(qa, tb):
    """float64 sums over the 128 elements from the restated operands: hh = sum hi_a hi_b,
    x = sum (hi_a lo_b + lo_a hi_b), and the same of absolute values."""
    ha, la = qa["hi"][:qa["n"]].astype(np.float64), qa["lo"][:qa["n"]].astype(np.float64)
    hb, lb = tb["hi"][:tb["n"]].astype(np.float64), tb["lo"][:tb["n"]].astype(np.float64)
    hh, x = ha @ hb.T, ha @ lb.T + la @ hb.T
    ahh = np.abs(ha) @ np.abs(hb).T
    ax = np.abs(ha) @ np.abs(lb).T + np.abs(la) @ np.abs(hb).T
    return hh, x, ahh, ax


def dtilde(qa, tb):
    """d~ [n1, n2] in float64 from the restated operands: na + nb - 2^-15 hh - 2^-26 x."""
    hh, x, _, _ = products(qa, tb)
    na = qa["norm2"][:qa["n"]].astype(np.float64)[:, None]
    nb = tb["norm2"][:tb["n"]].astype(np.float64)[None, :]
    return na + nb - 2.0 ** -15 * hh - 2.0 ** -26 * x


def gamma(k):
    return k * U / (1.0 - k * U)


def rounding_terms(qa, tb, d64):
    """T2, T3, T4 of the module docstring, [n1, n2] float64."""
    _, _, ahh, ax = products(qa, tb)
    na = qa["norm2"][:qa["n"]].astype(np.float64)[:, None]
    nb = tb["norm2"][:tb["n"]].astype(np.float64)[None, :]
    t2 = 2.0 ** -15 * gamma(127) * ahh + 2.0 ** -26 * gamma(255) * ax
    t3 = U * (na + nb) * (1 + 1 + 2.01 + 2.01) * (1 + 1e-3)
    t4 = ((1 + U) ** 21 - 1) * d64 + 150 * 2.0 ** -149
    return t2, t3, t4


def windows(dt, E):
    """Emulated window sizes: per row #{j : d~ <= b2~ + 2E}, b2~ the second smallest d~."""
    b2 = np.partition(dt, 1, axis=1)[:, 1]
    return (dt <= (b2 + 2.0 * E.astype(np.float64))[:, None]).sum(axis=1)


def bf16_down_value(word):
    """The stored d~ of a list word (its high 16 bits as a bfloat16) as float32."""
    return (np.asarray(word, np.uint32) & np.uint32(0xffff0000)).view(f32)


# ---------------------------------------------------------------- case generators
def _unit(n1, n2, seed):
    from sfmfromscratch_amd import synth
    t, hb = synth.make_descriptor_table(n2, seed)
    q, _ = synth.make_descriptor_table(n1, seed + 1, dup_of=hb, jitter=2)
    return q, t


def _u8(n1, n2, seed, rng=None):
    rng = rng or np.random.default_rng(seed)
    q = rng.integers(0, 256, (n1, 128))
    t = rng.integers(0, 256, (n2, 128))
    dup = rng.integers(0, n1, n2 // 2)                        # near-duplicates of queries (+-3)
    t[:n2 // 2] = np.clip(q[dup] + rng.integers(-3, 4, (n2 // 2, 128)), 0, 255)
    t[n2 - 1, 7] = 255                                       # one element exactly 255
    return q.astype(f32), t.astype(f32)


def _signed(n1, n2, seed):
    rng = np.random.default_rng(seed)
    q, t = 30 * rng.standard_normal((n1, 128)), 30 * rng.standard_normal((n2, 128))
    t[:n2 // 2] = q[rng.integers(0, n1, n2 // 2)] + 2 * rng.standard_normal((n2 // 2, 128))
    return q.astype(f32), t.astype(f32)


def _offset(amp):
    def gen(n1, n2, seed):
        rng = np.random.default_rng(seed)
        c = rng.random(128)
        q = c + amp * rng.standard_normal((n1, 128))
        t = c + amp * rng.standard_normal((n2, 128))
        src = rng.integers(0, n1, n2 // 2)                    # half: perturbed copies of queries
        t[::2][:n2 // 2] = q[src] + 0.25 * amp * rng.standard_normal((n2 // 2, 128))
        return q.astype(f32), t.astype(f32)
    return gen


def _tiny(s):
    def gen(n1, n2, seed):
        rng = np.random.default_rng(seed)
        q = (s * rng.random((n1, 128))).astype(f32)
        t = (s * rng.random((n2, 128))).astype(f32)
        t[:n2 // 2] = q[rng.integers(0, n1, n2 // 2)] * (1 + 0.05 * rng.standard_normal((n2 // 2, 128))).astype(f32)
        for tab in (q, t):                                    # a few float32-subnormal elements
            r, c = rng.integers(0, tab.shape[0], 6), rng.integers(0, 128, 6)
            tab[r, c] = (rng.integers(1, 2 ** 20, 6).astype(np.uint32)).view(f32)
        return q, t
    return gen


def _mixed(n1, n2, seed):
    rng = np.random.default_rng(seed)
    q = rng.random((n1, 128)) * 10.0 ** rng.integers(-4, 2, (n1, 1))
    t = rng.random((n2, 128)) * 10.0 ** rng.integers(-4, 2, (n2, 1))
    src = rng.integers(0, n1, n2 // 2)
    t[:n2 // 2] = q[src] * (1 + 0.02 * rng.standard_normal((n2 // 2, 128)))
    return q.astype(f32), t.astype(f32)


def _spike(n1, n2, seed):
    rng = np.random.default_rng(seed)
    q = 1e-2 * rng.standard_normal((n1, 128))
    t = 1e-2 * rng.standard_normal((n2, 128))
    q[np.arange(n1), rng.integers(0, 4, n1)] = 200.0          # four spike positions: near and far pairs
    t[np.arange(n2), rng.integers(0, 4, n2)] = 200.0
    src = rng.permutation(n1)[:min(n1, n2) // 4]              # perturbed copies, one per chosen query
    t[:len(src)] = q[src] + 1e-3 * rng.standard_normal((len(src), 128))
    return q.astype(f32), t.astype(f32)


def _zeros(n1, n2, seed):
    """Row 0 of the queries all zero; targets 0 and 1 all zero (row 0 then has d2 == 0: the `> 0`
    rule); query row 1 is a copy of target 2 with a lone zero target nearest but one."""
    q, t = _unit(n1, n2, seed)
    q, t = q.copy(), t.copy()
    q[0] = 0
    t[0] = 0
    if n2 > 2:
        t[1] = 0
    if n1 > 1 and n2 > 2:
        q[1] = t[2]
    return q, t


def _edge(v):
    def gen(n1, n2, seed):
        rng = np.random.default_rng(seed)
        q, t = _u8(n1, n2, seed, rng)
        q[n1 // 2, 5] = v
        t[n2 // 3, 9] = -v
        t[n2 - 2, 5] = v
        t[n2 - 2, 6:] = q[n1 // 2, 6:]                        # a near neighbour of the edge query row
        return q, t
    return gen


def _huge(n1, n2, seed):
    rng = np.random.default_rng(seed)
    q = 1000 * rng.standard_normal((n1, 128))
    t = 1000 * rng.standard_normal((n2, 128))
    t[:n2 // 2] = q[rng.integers(0, n1, n2 // 2)] + 20 * rng.standard_normal((n2 // 2, 128))
    return q.astype(f32), t.astype(f32)


GENERATORS = {
    "unit": _unit, "u8": _u8, "signed": _signed, "mixed": _mixed, "spike": _spike, "zeros": _zeros, "huge": _huge,
    "offset(0.03)": _offset(0.03), "offset(0.01)": _offset(0.01), "offset(0.006)": _offset(0.006),
    "offset(0.003)": _offset(0.003), "tiny(1e-3)": _tiny(1e-3), "tiny(1e-6)": _tiny(1e-6),
    "edge(255.9)": _edge(255.9), "edge(256)": _edge(256.0), "edge(1000)": _edge(1000.0), "edge(1e4)": _edge(1e4),
}

# (class, n1, n2, seed).  n2 over {2, 33, 65, 700}: below one 32-target sub-tile, one target over
# it, one over a 64-row stage, a ragged last stage; n1 over {1, 130, 260}: a partial second
# 128-row query block and a partial second 256-row block.  The offset / tiny(1e-6) cases keep
# 96 x 700, the size their window bands are stated for.
CASES = [
    ("unit", 130, 700, 11), ("unit", 1, 2, 12), ("unit", 260, 65, 13),
    ("u8", 130, 700, 21), ("u8", 260, 33, 22), ("u8", 1, 65, 23),
    ("signed", 260, 700, 31), ("signed", 130, 65, 32), ("signed", 1, 33, 33), ("signed", 130, 2, 34),
    ("offset(0.03)", 96, 700, 41), ("offset(0.01)", 96, 700, 42), ("offset(0.006)", 96, 700, 43),
    ("offset(0.003)", 96, 700, 47),
    ("tiny(1e-3)", 130, 700, 51), ("tiny(1e-6)", 96, 700, 52), ("tiny(1e-6)", 260, 33, 53),
    ("mixed", 260, 700, 61), ("mixed", 130, 33, 62),
    ("spike", 130, 700, 71), ("spike", 260, 65, 72),
    ("zeros", 130, 65, 81), ("zeros", 130, 700, 82), ("zeros", 1, 2, 83),
    ("edge(255.9)", 130, 700, 91), ("edge(256)", 130, 700, 92), ("edge(1000)", 130, 700, 93),
    ("edge(1e4)", 260, 65, 94),
    ("huge", 130, 700, 101), ("huge", 260, 33, 102),
]
CASE_IDS = ["%s-%dx%d" % c[:3] for c in CASES]
RATIO = 0.85


@functools.lru_cache(maxsize=None)
def case(i):
    """Case i of CASES -> (queries, targets), read-only float32 tables."""
    name, n1, n2, seed = CASES[i]
    q, t = GENERATORS[name](n1, n2, seed)
    q, t = np.ascontiguousarray(q, f32), np.ascontiguousarray(t, f32)
    assert q.shape == (n1, 128) and t.shape == (n2, 128) and np.isfinite(q).all() and np.isfinite(t).all()
    q.setflags(write=False)
    t.setflags(write=False)
    return q, t


def in_f16_range(*tables):
    return all(float(np.abs(t).max()) < F16_EDGE for t in tables)


def class_of(i):
    return CASES[i][0].split("(")[0]


@functools.lru_cache(maxsize=None)
def analysis(i):
    """Everything the tests need of case i, computed once: operands of both tables, E, d~ (f64),
    d_ref (float32 squared distances), d64, and D2 (the reference's second-smallest float32
    squared distance per row; +inf with fewer than two targets)."""
    q, t = case(i)
    qa, tb = operands(q), operands(t)
    d32, d64 = sqdist32(q, t), sqdist64(q, t)
    D2 = np.sort(d32, axis=1)[:, 1] if t.shape[0] >= 2 else np.full(q.shape[0], np.inf, f32)
    return {"qa": qa, "tb": tb, "E": bound(qa, tb), "dt": dtilde(qa, tb), "d32": d32, "d64": d64, "D2": D2}
