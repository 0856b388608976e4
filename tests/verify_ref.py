"""TEST INFRASTRUCTURE ONLY — numpy restatement of sfm_verify_matches_dev (include/sfmfeat.h has
the rule; verify.hip is the kernel): the counter-based sampler in Python integers masked to 64
bits, F per sample from ransac_ref.device_route_all, distances and counts from
ransac_ref.distances(..., np.float64), then rounds, early stop, winner, keep and stat.  The stop
table is an argument, so the device and the restatement read the same doubles.

It also builds the cases: correspondences of pose_ref.scene / pose_ref.random_pairs scattered by
a seeded permutation over the rows of a synthetic slot table, `matches` listing them in order.
Which properties the cases must have is asserted on the CPU by tests/test_verify_cpu.py.
Only tests/ import this module."""
from __future__ import annotations

import numpy as np

from tests import pose_ref as PR
from tests import ransac_ref as RR

ROUND = 256
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
ITERS = 700
SEED = 5
THRESHOLD = 1.0
CONFIDENCE = 0.98


# ---------------------------------------------------------------- the sampler
def mix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def pair_key(seed, a, b):
    return mix64(mix64(seed & M64) + ((a << 32) | b))


def sample(seed, a, b, it, n):
    """The eight indices of sample `it` of pair (a, b) with n matches."""
    key = pair_key(seed, a, b)
    moved = {}  # position -> value, the sparse part of the virtual arange(n)
    out = []
    for k in range(8):
        r = mix64(key + (8 * it + k + 1) * G) >> 32
        j = k + ((r * (n - k)) >> 32)
        vj, vk = moved.get(j, j), moved.get(k, k)
        out.append(vj)
        moved[j], moved[k] = vk, vj
    return out


def samples(seed, a, b, n, iters, first=0):
    return np.array([sample(seed, a, b, it, n) for it in range(first, iters)], np.int64).reshape(-1, 8)


def stop_ratios(confidence=CONFIDENCE, iters=ITERS):
    """The table sequence.verify_matches passes for `iters` samples (None: no early stop)."""
    from sfmfromscratch_amd import pose
    if not confidence:
        return None
    return pose.ransac_stop_ratios(confidence, min(64, (iters + ROUND - 1) // ROUND))


# ---------------------------------------------------------------- the rule
def correspondences(tab, p):
    """-> (attempted, n, valid [n], p1 [n, 2], p2 [n, 2] float64 with NaN rows where invalid)."""
    cap, nimg = tab["cap"], len(tab["count"])
    a, b = (int(v) for v in tab["pairs"][p])
    n = int(min(max(int(tab["nmatch"][p]), 0), cap))
    attempted = 0 <= a < nimg and 0 <= b < nimg and a != b and n >= 8
    if not attempted:
        return False, n, np.zeros(n, bool), np.zeros((n, 2)), np.zeros((n, 2))
    ca, cb = (int(min(max(int(tab["count"][s]), 0), cap)) for s in (a, b))
    m = tab["matches"][p, :n].astype(np.int64)
    valid = (m[:, 0] >= 0) & (m[:, 0] < ca) & (m[:, 1] >= 0) & (m[:, 1] < cb)
    p1 = np.full((n, 2), np.nan)
    p2 = np.full((n, 2), np.nan)
    p1[valid] = tab["xy"][a, m[valid, 0]]
    p2[valid] = tab["xy"][b, m[valid, 1]]
    return True, n, valid, p1, p2


_TABLES: dict = {}


def sample_table(tab, p, iters, seed=SEED):
    """(idx [iters, 8], F [iters, 3, 3], d [iters, n] float64) of pair p's first `iters` samples: F is
    NaN for a sample that contains an invalid match, d is NaN at invalid matches.  Cached by the
    table's name, so every test of a case shares one evaluation."""
    key = (tab["name"], p, seed)
    have = _TABLES.get(key)
    if have is not None and len(have[0]) >= iters:
        return tuple(v[:iters] for v in have)
    _, n, valid, p1, p2 = correspondences(tab, p)
    a, b = (int(v) for v in tab["pairs"][p])
    idx = samples(seed, a, b, n, iters)
    F = np.full((iters, 3, 3), np.nan)
    good = valid[idx].all(axis=1)
    if good.any():
        F[good] = RR.device_route_all(p1, p2, idx[good])[0]
    d = RR.distances(F, p1, p2, np.float64) if iters else np.zeros((0, n))
    _TABLES[key] = (idx, F, d)
    return idx, F, d


def decide(counts, n, iters, stop, min_inliers):
    """Rounds, early stop and winner over per-sample counts -> stat [4]."""
    if iters == 0:
        return np.array([0, -1, 0, 0], np.int32)
    n_stop = 0 if stop is None else len(stop)
    rounds = (iters + ROUND - 1) // ROUND
    best, win, done = -1, -1, 0
    for r in range(1, rounds + 1):
        lo, hi = ROUND * (r - 1), min(iters, ROUND * r)
        c = counts[lo:hi]
        k = int(np.argmax(c))  # the first of the largest
        if c[k] > best:
            best, win = int(c[k]), lo + k
        done = hi
        if r <= n_stop and np.float64(best) >= np.float64(stop[r - 1]) * np.float64(n):
            break
    return np.array([best, win, done, int(best > 0 and best >= min_inliers)], np.int32)


def verify(tab, iters=ITERS, threshold=THRESHOLD, min_inliers=16, seed=SEED, stop=None):
    """The whole call -> dict(keep [P, cap] uint8, F [P, 3, 3], stat [P, 4] int32, margin [P]): margin is
    the closest |d - threshold| over the evaluated samples' valid matches (inf where none)."""
    P, cap = len(tab["pairs"]), tab["cap"]
    keep = np.zeros((P, cap), np.uint8)
    F = np.full((P, 3, 3), np.nan)
    stat = np.zeros((P, 4), np.int32)
    margin = np.full(P, np.inf)
    for p in range(P):
        attempted, n, valid, _, _ = correspondences(tab, p)
        if not attempted:
            stat[p] = (-1, -1, 0, 0)
            continue
        _, Fs, d = sample_table(tab, p, iters, seed)
        with np.errstate(invalid="ignore"):
            inl = d < threshold  # NaN (an invalid match, a sample without a fit) is no inlier
        stat[p] = decide(inl.sum(axis=1), n, iters, stop, min_inliers)
        best, win, done, ok = (int(v) for v in stat[p])
        if best > 0:
            F[p] = Fs[win]
        if ok:
            keep[p, :n] = inl[win]
        if done and valid.any() and np.isfinite(threshold):
            with np.errstate(invalid="ignore"):
                gap = np.abs(d[:done][:, valid] - threshold)
            if np.isfinite(gap).any():
                margin[p] = float(np.nanmin(gap))
    return dict(keep=keep, F=F, stat=stat, margin=margin)


# ---------------------------------------------------------------- cases
def slot_table(name, sets, nimg=3, cap=None, seed=0):
    """A synthetic slot table holding the correspondence sets `sets` = [(a, b, p1, p2), ...], one pair
    each: set k's i-th correspondence sits in rows (perm_a[i], perm_b[i]) of slots a and b.  A slot
    used by several sets must get the same number of points from each (later sets overwrite)."""
    rng = np.random.default_rng(1000 + seed)
    nmax = max(len(s[2]) for s in sets)
    cap = cap or nmax + 3
    xy = rng.integers(0, 960, (nimg, cap, 2)).astype(np.int32)
    count = np.zeros(nimg, np.int32)
    pairs = np.zeros((len(sets), 2), np.int32)
    matches = np.zeros((len(sets), cap, 2), np.int32)
    nmatch = np.zeros(len(sets), np.int32)
    for k, (a, b, p1, p2) in enumerate(sets):
        n = len(p1)
        ra, rb = rng.permutation(n), rng.permutation(n)
        xy[a, ra], xy[b, rb] = p1, p2
        count[a], count[b] = max(count[a], n), max(count[b], n)
        pairs[k] = (a, b)
        matches[k, :n, 0], matches[k, :n, 1] = ra, rb
        nmatch[k] = n
    return dict(name=name, xy=xy, count=count, cap=cap, pairs=pairs, matches=matches, nmatch=nmatch)


# name -> (scene seed, n, outlier fraction).  Seeds 61-67 with these (n, fraction) are the issue's;
# n = 7 (not attempted) and the sizes around one and two staging chunks of 2560 are added here.
SINGLE = {
    "n7": (60, 7, 0.0),
    "n8": (61, 8, 0.0),
    "n9": (62, 9, 0.0),
    "n40": (63, 40, 0.2),
    "n255": (64, 255, 0.3),
    "n257": (65, 257, 0.5),
    "n2561": (66, 2561, 0.4),
    "n300": (67, 300, 0.7),
    "n2560": (68, 2560, 0.3),
    "n5121": (69, 5121, 0.6),
    "n2700_bad": (70, 2700, 0.1),
}
# cases whose match list gets rows outside [0, count): name -> how many of the matches.  n2700_bad is
# the multi-chunk case (n > 2560) whose samples, drawn from global memory, meet invalid matches and
# whose 0.98 table stops it between two restaged rounds.
BAD_ROWS = {"n2700_bad": 60}
# at confidence 0.98 and 700 samples (asserted by tests/test_verify_cpu.py): samples evaluated
STOPS_EARLY = {"n8": 256, "n9": 256, "n40": 256, "n255": 512, "n2700_bad": 256}
RUNS_ALL = ("n257", "n2561", "n300")
_CASES: dict = {}


def single(name):
    """One pair (slots 2 and 0 of three) holding the scene's correspondences, listed in the scene's
    order; the rows they sit in are scattered."""
    if name not in _CASES:
        seed, n, frac = SINGLE[name]
        p1, p2, _ = PR.scene(seed, n, frac)
        t = slot_table(name, [(2, 0, p1, p2)], seed=seed)
        if name in BAD_ROWS:
            rng = np.random.default_rng(4000 + seed)
            bad = rng.permutation(n)[:BAD_ROWS[name]]
            third = len(bad) // 3
            t["matches"][0, bad[:third], 0] = n + rng.integers(0, 3, third)              # >= count, below cap
            t["matches"][0, bad[third:2 * third], 1] = -1 - rng.integers(0, 3, third)   # negative
            t["matches"][0, bad[2 * third:], 1] = 1 << 24                                # far beyond cap
        _CASES[name] = t
    return _CASES[name]


MIXED_ITERS = 300
MIXED_RANDOM = 3   # the pure random_pairs pair of the mixed table


def mixed():
    """One table, one call: six slots of 120 keypoints (cap 131) — slots 0, 1 and 2, 3 hold two scenes,
    slots 4, 5 pure random_pairs — and nine pairs that cover every way a pair is not attempted or
    partly invalid.  Pair 0 (0, 1) clean; 1 (2, 3) with nmatch -1; 2 (2, 3) with nmatch > cap (all cap
    entries count; those beyond the 120 real ones point at rows >= count or below 0); 3 (4, 5) the
    random pair; 4 a == b; 5 and 6 a slot outside [0, nimg); 7 (0, 1) with rows >= count, negative rows
    and rows far beyond cap among the good ones; 8 (2, 3) with 7 matches."""
    if "mixed" in _CASES:
        return _CASES["mixed"]
    n = 120
    A, B, R = PR.scene(71, n, 0.2)[:2], PR.scene(72, n, 0.3)[:2], PR.random_pairs(75, n)
    base = slot_table("mixed_base", [(0, 1, *A), (2, 3, *B), (4, 5, *R)], nimg=6, cap=131, seed=7)
    cap = base["cap"]
    src = [0, 1, 1, 2, 0, 0, 0, 0, 1]
    t = dict(base, name="mixed", pairs=np.ascontiguousarray(base["pairs"][src]),
             matches=np.ascontiguousarray(base["matches"][src]), nmatch=np.ascontiguousarray(base["nmatch"][src]))
    rng = np.random.default_rng(3000)
    t["nmatch"][1] = -1
    t["nmatch"][2] = 1000
    t["matches"][2, n:] = np.column_stack((rng.integers(n, 200, cap - n), rng.integers(-5, 0, cap - n)))
    t["pairs"][4] = (1, 1)
    t["pairs"][5] = (6, 1)
    t["pairs"][6] = (0, -1)
    bad = rng.permutation(n)[:30]
    t["matches"][7, bad[:10], 0] = n + rng.integers(0, 11, 10)      # >= count, below cap
    t["matches"][7, bad[10:20], 1] = -1 - rng.integers(0, 3, 10)    # negative
    t["matches"][7, bad[20:], 0] = 1 << 20                          # far beyond cap
    t["nmatch"][8] = 7
    _CASES["mixed"] = t
    return t


def permuted_pairs(tab, seed):
    """The same table with its pairs in another order -> (table, order)."""
    order = np.random.default_rng(seed).permutation(len(tab["pairs"]))
    t = dict(tab, name=f"{tab['name']}_perm{seed}")
    for k in ("pairs", "matches", "nmatch"):
        t[k] = np.ascontiguousarray(tab[k][order])
    return t, order


def sub_table(tab, sel, name):
    t = dict(tab, name=name)
    for k in ("pairs", "matches", "nmatch"):
        t[k] = np.ascontiguousarray(tab[k][sel])
    return t
