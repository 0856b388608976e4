"""The keypoint selection (NaiveSIFT.py:77-120) restated in numpy, the select scan's bookkeeping
(kernels.h select_scan_plane), the route a plane takes through k_select, and the crafted planes
that take each route.

select_ref is written from the reference's lines, not from the kernel: the median is np.median,
the maxpool a padded maximum, the order a lexsort.  scan_ref and path_ref restate what the
library decides from a plane's histogram, so that a test can say which branch a plane must take
before it looks at the device's answer.  Path labels are tuples of strings:

  ("k0",)                                           k == 0: nothing runs
  ("certified", subset, form, ties)
  ("fallback_scan", *exact)                         the scan (or force_exact) sends the plane
  ("fallback_run", subset, form, ties, *exact)      the certified stage ran and did not certify
      subset  subset0 / subset1 / none              (topk_subset; none: the full top-k ran)
      form    whole / regs / global                 (topk_sorted), subset (sorted whole by
              topk_subset), short (fewer than k candidates: no top-k at all)
      ties    ties_lds / ties_global                (radix forms only), no_ties: no tie code ran
  exact = (loads, buckets, list, nms, form, ties)
      loads   vec / scalar            buckets  one_bucket / two_buckets
      list    list_lds / list_spill   nms      nms_vec4 / nms_scalar / nms_generic
      form    whole / regs / global (the plane's maximum is always a candidate: never none)
"""
from __future__ import annotations

import numpy as np

MED_BITS1 = 11                 # kernels.h kMedBits1: the scan's buckets are the keys' top 11 bits
SHIFT = 32 - MED_BITS1
HUGE_BUCKET = 0x7F4            # kernels.h kHugeBucket: buckets from 2^126 up never certify
# the library's branch sizes at k <= 2048 when it is not built (_native.select_constants)
FALLBACK_CONSTS = {"sel_cap": 2048, "topk_direct": 2048, "tie_lds_cap": 2048, "reg_keys": 8192, "med_cap": 8192}

ALL_LABELS = {"k0", "certified", "fallback_scan", "fallback_run", "subset0", "subset1", "none", "whole", "regs",
              "global", "subset", "short", "ties_lds", "ties_global", "no_ties", "vec", "scalar",
              "one_bucket", "two_buckets", "list_lds", "list_spill", "nms_vec4", "nms_scalar", "nms_generic"}


def consts_for(k: int, base: dict | None = None) -> dict:
    """The branch sizes at k from those at k <= 2048 (select.hip: sel_cap = max(kTopkDirect,
    next_pow2(k)); the median list lies over the sel and tie areas, two u32 per u64)."""
    c = dict(base or FALLBACK_CONSTS)
    p = c["topk_direct"]
    while p < k:
        p *= 2
    c["sel_cap"] = p
    c["med_cap"] = 2 * (p + c["tie_lds_cap"])
    return c


def fkey(a: np.ndarray) -> np.ndarray:
    """Order-preserving float32 -> uint32, -0 folded onto +0 (common.h fkey)."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def maxpool(R: np.ndarray, ksize: int) -> np.ndarray:
    """np.max over the ksize x ksize window clipped to the image (:85-88), by -inf padding."""
    H, W = R.shape
    h = ksize // 2
    P = np.full((H + 2 * h, W + 2 * h), -np.inf, np.float32)
    P[h:h + H, h:h + W] = R
    m = np.full((H, W), -np.inf, np.float32)
    for dy in range(2 * h + 1):
        for dx in range(2 * h + 1):
            m = np.maximum(m, P[dy:dy + H, dx:dx + W])
    return m


def ordered(R: np.ndarray, cand: np.ndarray, descending_index: bool = False):
    """Raster indices of the candidate mask ordered by confidence descending, then raster index
    ascending (descending_index: the other tie order, for the tests' own non-vacuity checks)."""
    idx = np.flatnonzero(cand.ravel())
    conf = R.ravel()[idx].astype(np.float64)
    return idx[np.lexsort((-idx if descending_index else idx, -conf))]


def exact_candidates(R: np.ndarray, ksize: int):
    med = np.float32(np.median(R))                                     # :91
    m = maxpool(R, ksize)
    return ((R >= med) & (R == m)) | ((R < med) & (R == 0)), med       # :92, :95


def select_ref(R: np.ndarray, k: int, ksize: int, hw: int, descending_index: bool = False):
    """-> x, y (int64), conf (float32), median (float32) of NaiveSIFT.py:77-120 on the plane R."""
    R = np.ascontiguousarray(R, np.float32)
    H, W = R.shape
    cand, med = exact_candidates(R, ksize)
    idx = ordered(R, cand, descending_index)[:max(int(k), 0)]           # :100
    y, x = idx // W, idx % W
    keep = (y >= hw) & (y < H - hw) & (x >= hw) & (x < W - hw)          # :108
    return x[keep], y[keep], R.ravel()[idx][keep], med


def scan_ref(R: np.ndarray, vmin: int, force_exact: bool) -> dict:
    """select_scan_plane: from the histogram of the keys' top 11 bits, the buckets holding the two
    middle ranks with the ranks inside them, the candidate threshold (the bucket of the vmin-th
    largest value, at least the lower median bucket), the two subset thresholds (the 3 vmin / 8-th
    and vmin / 2-th largest) and the certification threshold (the first key above the upper median
    bucket; none from kHugeBucket up, where the median's sum could overflow)."""
    keys = fkey(R).ravel()
    n = keys.size
    hist = np.bincount(keys >> SHIFT, minlength=1 << MED_BITS1)
    incl = np.cumsum(hist)

    def locate(r):  # the bucket holding 0-based rank r and the rank inside it
        b = int(np.searchsorted(incl, r, side="right"))
        return b, int(r - (incl[b] - hist[b]))

    (b1, r1), (b2, r2) = locate(n // 2 if n % 2 else n // 2 - 1), locate(n // 2)
    vs0, vs1 = 3 * vmin // 8, vmin // 2
    tb = max(locate(n - vmin)[0] if n > vmin else 0, b1)
    certifiable = (not force_exact) and b2 < HUGE_BUCKET
    return {"bucket0": b1, "bucket1": b2, "rank0": r1, "rank1": r2, "odd": n % 2,
            "tnms": tb << SHIFT,
            "tsub0": max(locate(n - vs0)[0] if n > vs0 else 0, tb) << SHIFT,
            "tsub1": max(locate(n - vs1)[0] if n > vs1 else 0, tb) << SHIFT,
            "tcert": (b2 + 1) << SHIFT if certifiable else 0xFFFFFFFF,
            "fallback": 0 if certifiable else 1}


def certified_candidates(R: np.ndarray, tnms: int, ksize: int) -> np.ndarray:
    """The certified NMS's candidate mask: window maxima whose key reaches tnms."""
    return (fkey(R) >= np.uint32(tnms)) & (R == maxpool(R, ksize))


def _topk_form(conf_keys: np.ndarray, kk: int, c: dict):
    """topk_sorted on a candidate list (descending-confidence keys as fkey values) for the kk best."""
    C = conf_keys.size
    if C <= c["sel_cap"]:
        return "whole", "no_ties"
    form = "regs" if C <= c["reg_keys"] else "global"
    kth = np.sort(conf_keys)[::-1][kk - 1]
    return form, "ties_lds" if int((conf_keys == kth).sum()) <= c["tie_lds_cap"] else "ties_global"


def path_ref(R: np.ndarray, k: int, ksize: int, vmin: int, force_exact: bool, consts: dict, r_offset: int = 0):
    """The route of plane R through k_select (module docstring).  consts: the library's branch
    sizes at this k; r_offset: the plane's first float counted from a 16-byte aligned address (the
    planes of a call are packed one after another)."""
    R = np.ascontiguousarray(R, np.float32)
    H, W = R.shape
    n = H * W
    if k <= 0:
        return ("k0",)
    s = scan_ref(R, vmin, force_exact)
    keys = fkey(R)
    head = ()
    if not s["fallback"]:
        ck = keys[certified_candidates(R, s["tnms"], ksize)]
        C = ck.size
        if C < k:
            head = ("fallback_run", "none", "short", "no_ties")
        else:
            subset = "none"
            if c_in(C, consts) and s["tsub0"] > s["tnms"]:
                n0, n1 = int((ck >= s["tsub0"]).sum()), int((ck >= s["tsub1"]).sum())
                if k <= n0 <= consts["sel_cap"]:
                    subset = "subset0"
                elif s["tsub1"] > s["tnms"] and k <= n1 <= consts["sel_cap"]:
                    subset = "subset1"
            form, ties = ("subset", "no_ties") if subset != "none" else _topk_form(ck, k, consts)
            kth = np.sort(ck)[::-1][k - 1]
            if kth >= s["tcert"]:
                return ("certified", subset, form, ties)
            head = ("fallback_run", subset, form, ties)
    else:
        head = ("fallback_scan",)
    aligned = r_offset % 4 == 0
    loads = "vec" if n % 4 == 0 and aligned else "scalar"
    buckets = "one_bucket" if s["bucket0"] == s["bucket1"] else "two_buckets"
    d = keys >> SHIFT
    m = int(((d == s["bucket0"]) | (d == s["bucket1"])).sum())
    lst = "list_lds" if m <= consts["med_cap"] else "list_spill"
    nms = "nms_generic" if ksize // 2 != 1 else "nms_vec4" if W % 4 == 0 and aligned else "nms_scalar"
    ek = keys[exact_candidates(R, ksize)[0]]
    assert ek.size >= 1   # (the plane's maximum, without NaN)
    form, ties = _topk_form(ek, min(k, ek.size), consts)
    return head + (loads, buckets, lst, nms, form, ties)


def c_in(C: int, c: dict) -> bool:
    """topk_subset looks at lists longer than sel_cap that fit the registers."""
    return c["sel_cap"] < C <= c["reg_keys"]


def ring_planes(H, W, kh):
    """Planes on which the outermost row and column of the window decide: over a flat -1
    background (below the threshold 0), sites of one pixel A (value 1 + site) and one larger
    pixel B (100 + site) at offset r x (sy, sx) from it, for the eight directions and r = kh
    (B is on the window's border: A is suppressed) and r = kh + 1 (just outside: A stays).
    Sites sit 2 kh + 3 columns apart, so no site's pixels lie in another's windows.  A random
    plane almost never notices a window one row or column short at ksize 31; this one must."""
    offs = [(sy * r, sx * r) for r in (kh, kh + 1)
            for sy, sx in ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))]
    per, ay = W // (2 * kh + 3), H // 2
    assert per >= 1 and ay - (kh + 1) >= 0 and ay + kh + 1 < H
    out = np.full((-(-len(offs) // per), H, W), -1.0, np.float32)
    for s, (dy, dx) in enumerate(offs):
        ax = kh + 1 + (s % per) * (2 * kh + 3)
        out[s // per, ay, ax] = 1.0 + s
        out[s // per, ay + dy, ax + dx] = 100.0 + s
    return out


# ------------------------------------------------------------------------------------------------
# Crafted planes.  Values that share sign, exponent and the top two mantissa bits share a bucket:
# [1, 1.25), [1.25, 1.5), [2, 2.25), [4, 4.25) and [8, 8.25) are five of them.  A layer is `count`
# pixels of one bucket: distinct values base + i ulp(base), or
# `count` copies of one value (a confidence tie).  With ksize = 1 every pixel is its own window
# maximum, so the certified candidates are exactly the pixels at or above the threshold's bucket.

def steps(base: float, count: int, first: int = 0) -> np.ndarray:
    """count distinct float32 values base + (first + i) ulp(base), all inside base's bucket."""
    assert first + count <= 1 << 21
    b = np.array([base], np.float32).view(np.uint32)[0]
    return (b + np.arange(first, first + count, dtype=np.uint32)).view(np.float32)


def layered(H: int, W: int, layers, seed: int, low: float = 1.0) -> np.ndarray:
    """A plane holding the concatenated `layers` (arrays of values), the rest filled with distinct
    values of `low`'s bucket, at positions shuffled by `seed`."""
    n = H * W
    vals = np.concatenate([np.asarray(v, np.float32).ravel() for v in layers] + [np.zeros(0, np.float32)])
    assert vals.size <= n
    rest = steps(low, n - vals.size)
    rng = np.random.default_rng(seed)
    return np.concatenate([vals, rest])[rng.permutation(n)].reshape(H, W).astype(np.float32)


class Case:
    """One plane with the call it belongs to and the route it claims."""

    def __init__(self, name, R, k, vmin, label, ksize=1, force_exact=False, hw=0):
        self.name, self.R, self.k, self.vmin, self.label = name, R, k, vmin, tuple(label)
        self.ksize, self.force_exact, self.hw = ksize, force_exact, hw

    def __repr__(self):
        return f"Case({self.name})"


SHAPE = (160, 160)   # n = 25600: up to 12799 pixels above the median's bucket
BIG = (192, 192)     # n = 36864
# the exact path of a plane whose pixels at or above the median number more than reg_keys
EX_GLOBAL = ("vec", "one_bucket", "list_spill", "nms_generic", "global", "ties_lds")


def topk_count_cases(c: dict):
    """k = 500, vmin = 400: C pixels in [4, 4.25), the rest in the median's bucket [1, 1.25); the
    400-th largest lies in [4, 4.25), so the certified candidates are those C (and both subset
    thresholds equal the candidate threshold: no subset)."""
    k, out = 500, []
    for C, lab in ((k - 1, ("fallback_run", "none", "short", "no_ties") + EX_GLOBAL),
                   (k, ("certified", "none", "whole", "no_ties")),
                   (c["sel_cap"], ("certified", "none", "whole", "no_ties")),
                   (c["sel_cap"] + 1, ("certified", "none", "regs", "ties_lds")),
                   (c["reg_keys"], ("certified", "none", "regs", "ties_lds")),
                   (c["reg_keys"] + 1, ("certified", "none", "global", "ties_lds"))):
        out.append(Case(f"count_{C}", layered(*SHAPE, [steps(4.0, C)], seed=C), k, 400, lab))
    return out


def tie_layers(nless: int, ntie: int, rest: int):
    """nless distinct values, ntie copies of one value below them, rest distinct values below
    that; all in the bucket [4, 4.25)."""
    return [steps(4.0, nless, first=rest + 1), np.full(ntie, steps(4.0, 1, first=rest)[0], np.float32),
            steps(4.0, rest)]


def tie_cases(c: dict):
    """Ties at the k-th confidence, in the register form (C <= reg_keys) and the global form:
    (name, nless, ntie, k).  vmin = 400 as above."""
    cap = c["tie_lds_cap"]
    out = []
    for form, C in (("regs", c["reg_keys"] - 100), ("global", c["reg_keys"] + 900)):
        for name, nless, ntie, k in (("cap", 100, cap, 500), ("cap1", 100, cap + 1, 500), ("last", 100, 400, 500),
                                     ("last_global", 100, cap + 352, 100 + cap + 352),
                                     ("first_lds", 0, 1000, 1), ("first_global", 0, cap + 952, 1)):
            rest = C - nless - ntie
            ties = "ties_lds" if ntie <= cap else "ties_global"
            ck = consts_for(k, c)
            lab = ("certified", "none", form if C > ck["sel_cap"] else "whole", ties if C > ck["sel_cap"] else "no_ties")
            out.append(Case(f"tie_{form}_{name}", layered(*SHAPE, tie_layers(nless, ntie, rest), seed=ntie + k),
                            k, 400, lab))
    return out


def k_cases(c: dict):
    """k in {0, 1, 2048, 2049, 2500, 8192} on planes of C candidates (vmin = 400): sel_cap is
    2048, 4096 (2049 and 2500) and 8192, where the register form cannot be reached."""
    cert = ("certified", "none")
    rows = [(0, 5000, ("k0",)), (1, 5000, cert + ("regs", "ties_lds")),
            (2048, 2048, cert + ("whole", "no_ties")), (2048, 5000, cert + ("regs", "ties_lds")),
            (2049, 4096, cert + ("whole", "no_ties")), (2049, 4097, cert + ("regs", "ties_lds")),
            (2500, 5000, cert + ("regs", "ties_lds")), (2500, 9000, cert + ("global", "ties_lds")),
            (8192, 8192, cert + ("whole", "no_ties")), (8192, 8193, cert + ("global", "ties_lds"))]
    return [Case(f"k{k}_C{C}", layered(*BIG, [steps(4.0, C)], seed=k + C), k, 400, lab) for k, C, lab in rows]


def subset_cases(c: dict):
    """sel_cap < C <= reg_keys with layers in [8, 8.25) (n8), [4, 4.25) (n4) and [2, 2.25) (n2), k =
    500: the candidate threshold is the bucket of the vmin-th largest value ([2, 2.25): C = n8 + n4
    + n2), tsub[0] that of the 3 vmin / 8-th and tsub[1] that of the vmin / 2-th largest.

    n0 == sel_cap + 1 does not "fall to tsub[1]": tsub[1] <= tsub[0], so n1 >= n0 and a subset too
    long at tsub[0] is too long at tsub[1].  topk_subset's tsub[1] arm is reached only with n0 < k
    (subset_subset1); n0_eq_cap1 must end in the full top-k."""
    k, cap = 500, c["sel_cap"]
    s0, s1, no = ("certified", "subset0", "subset", "no_ties"), ("certified", "subset1", "subset", "no_ties"), \
        ("certified", "none", "regs", "ties_lds")
    rows = [  # name, vmin, n8, n4, n2, label
        ("subset0", 4000, 1600, 1000, 2000, s0),            # the 1500-th largest in [8, 8.25): n0 = 1600
        ("n0_eq_cap", 4000, cap, 1000, 2000, s0),
        ("n0_eq_cap1", 4000, cap + 1, 1000, 2000, no),      # n0 = n1 = cap + 1: neither fits
        ("n1_gt_cap", 4000, 1400, cap, 2000, no),           # the 1500-th in [4, 4.25): n0 = n1 = 1400 + cap
        ("subset1", 1200, 460, 300, 2000, s1),              # 450-th in [8, 8.25): n0 = 460 < k; 600-th: n1 = 760
        ("n0_eq_k", 1200, k, 300, 2000, s0),
        ("both_below_k", 900, 340, 115, 2000, no),          # n0 = 340, n1 = 455
    ]
    return [Case(f"subset_{name}", layered(*SHAPE, [steps(8.0, n8), steps(4.0, n4), steps(2.0, n2)], seed=n8 + n4),
                 k, vmin, lab) for name, vmin, n8, n4, n2, lab in rows]


def certify_edge_cases(c: dict):
    """64 x 64, vmin = n (the candidate threshold is the median's bucket [1, 1.25), so every pixel
    is a candidate: 4096 of them, the register form), k = 500 with 499 values above 1.25: the k-th
    is 1.25 itself, the first key of the bucket above the median's (certifies), or the last key of
    the median's bucket (must fall back)."""
    H = W = 64
    top = steps(1.25, 499, first=1)
    last = np.nextafter(np.float32(1.25), np.float32(0))
    # (its exact path: the 2048 pixels at or above the median, sorted whole)
    ex = ("vec", "one_bucket", "list_lds", "nms_generic", "whole", "no_ties")
    return [Case("kth_first_key_above", layered(H, W, [top, [np.float32(1.25)]], seed=1), 500, H * W,
                 ("certified", "none", "regs", "ties_lds")),
            Case("kth_last_key_of_bucket", layered(H, W, [top, [last]], seed=2), 500, H * W,
                 ("fallback_run", "none", "regs", "ties_lds") + ex)]


def huge_case(c: dict):
    """Every value in [2^126, 2^126 (1 + 2^-11)): the median's bucket is kHugeBucket, the largest
    sum of two stays finite."""
    H, W = 40, 50
    R = layered(H, W, [], seed=3, low=2.0 ** 126)
    return [Case("huge_bucket", R, 50, 400, ("fallback_scan", "vec", "one_bucket", "list_lds", "nms_generic", "whole",
                                             "no_ties"))]


def median_planes(H: int, W: int):
    """(name, plane, buckets) for the exact median at one shape: contents by construction."""
    n = H * W
    rng = np.random.default_rng(n)
    lo, hi = n // 2, n - n // 2
    out = [("normal", rng.standard_normal(n).astype(np.float32), None)]
    # the lower half in [1, 1.25), the upper in [1.25, 1.5): for even n the middle pair straddles
    out.append(("two_buckets", np.concatenate([steps(1.0, lo), steps(1.25, hi)]), "two_buckets" if n % 2 == 0 else None))
    # the middle pair -0.75 ulp-steps and +1.0: one negative, one positive
    out.append(("straddle_zero", np.concatenate([-steps(0.75, lo), steps(1.0, hi)]),
                "two_buckets" if n % 2 == 0 else None))
    out.append(("all_equal", np.full(n, 3.5, np.float32), "one_bucket"))
    nz = n // 3
    out.append(("median_zero", np.concatenate([-steps(1.0, (n - nz) // 2), np.zeros(nz, np.float32),
                                               steps(1.0, n - nz - (n - nz) // 2)]), "one_bucket"))
    out.append(("negative", np.concatenate([-steps(2.0, n - n // 4), steps(1.0, n // 4)]), "one_bucket"))
    # the middle pair 1 + 2^-23 and 1.5: their sum 2.5 + 2^-23 is not a float32
    out.append(("sum_rounds", np.concatenate([steps(0.5, lo - 1), steps(1.0, 1, first=1), [np.float32(1.5)],
                                              steps(2.0, hi - 1)]), "two_buckets" if n % 2 == 0 else None))
    # ... and within one bucket: 1.75 + 2^-23 and 1.75 + 2^-22 sum to 3.5 + 3 2^-23
    out.append(("sum_rounds_one_bucket", np.concatenate([steps(0.5, lo - 1), steps(1.75, 2, first=1),
                                                         steps(2.0, hi - 1)]), "one_bucket"))
    # a single -0.0 just below the middle, between negatives and positives: a candidate (R == 0
    # below the median) whose confidence the device reports as +0 (compared by value)
    out.append(("minus_zero", np.concatenate([-steps(1.0, lo - 1), [np.float32(-0.0)], steps(1.0, hi)]), None))
    return [(name, np.asarray(v, np.float32)[rng.permutation(n)].reshape(H, W), b) for name, v, b in out]


def median_list_shapes(c: dict):
    """(m, H, W): collected-list lengths around med_cap, twice and four times it (256 x 256 where
    192 x 192 cannot hold four times); 129 x 127 is odd, so one spilling list is collected with
    scalar loads."""
    cap = c["med_cap"]
    return [(cap - 1, *BIG), (cap, *BIG), (cap + 1, *BIG), (cap + 1, 129, 127) if cap < 129 * 127 - 2 else
            (cap + 1, 191, 191), (2 * cap + 5, *BIG),
            (4 * cap, *BIG) if 4 * cap + 4 <= BIG[0] * BIG[1] else (4 * cap, 256, 256)]


def median_list_plane(H: int, W: int, m: int, seed: int) -> np.ndarray:
    """m pixels in the median's bucket [1, 1.25), the others split evenly between [0.5, 0.625) and
    [2, 2.25): the collected median list holds exactly m keys."""
    n = H * W
    below = (n - m) // 2
    assert m > 2 and below >= 1
    return layered(H, W, [steps(0.5, below), steps(2.0, n - m - below)], seed=seed)


# ------------------------------------------------------------------------------------------------
# Probe calls.  A spec is one sfm_debug_select call: its levels, parameters and what each plane
# claims about its route - a full label, or the atoms it must show.  Built here so that the CPU
# test holds every claim to path_ref; tests/test_gpu_select_planes.py runs them on the device.

def planes(B, H, W, seed):
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((B, H, W)).astype(np.float32)
    R[0] = np.round(R[0] * 2) / 2           # plateaus: many equal neighbours
    if B > 1:
        R[1] = np.abs(R[1]) * 1e3           # positive, large
    if B > 2:
        R[2, :, : W // 2] = 0.0             # a flat half (R == 0 plateaus)
    return R


def spec(name, levels, k, ksize=1, hw=0, vmin=400, force_exact=False, labels=None, needs=None, by_value=()):
    """One probe call: levels [B, H, W] arrays (or one), per-plane full labels [l][b] and / or the
    label atoms each plane must show, and the (l, b) whose confidences are compared by value."""
    if isinstance(levels, np.ndarray):
        levels = [levels]
    levels = [np.ascontiguousarray(R, np.float32) for R in levels]
    hw = [hw] * len(levels) if np.isscalar(hw) else list(hw)
    return dict(name=name, levels=levels, k=k, ksize=ksize, hw=hw, vmin=vmin, force_exact=force_exact,
                labels=labels, needs=needs, by_value=set(by_value))


def route_labels(sp, base, asserted=None):
    """path_ref of every plane of the call, held to what the case claims.  asserted (a set): gets
    the atoms the claims name - all of a full label, the atoms of `needs`."""
    c = consts_for(sp["k"], base)
    B = sp["levels"][0].shape[0]
    out, off = [], 0
    for l, R in enumerate(sp["levels"]):
        row = []
        for b in range(B):
            lab = path_ref(R[b], sp["k"], sp["ksize"], sp["vmin"], sp["force_exact"], c, r_offset=off)
            assert set(lab) <= ALL_LABELS
            if sp["labels"] is not None and sp["labels"][l][b] is not None:
                assert lab == tuple(sp["labels"][l][b]), (sp["name"], l, b, lab)
                if asserted is not None:
                    asserted |= set(lab)
            if sp["needs"] is not None:
                assert set(sp["needs"][l][b]) <= set(lab), (sp["name"], l, b, lab)
                if asserted is not None:
                    asserted |= set(sp["needs"][l][b])
            row.append(lab)
            off += R[b].size
        out.append(row)
    return out


def grouped(cases):
    """The cases of a generator as probe calls: planes of one (shape, k, vmin, ...) share a call."""
    groups = {}
    for case in cases:
        key = (case.R.shape, case.k, case.vmin, case.ksize, case.force_exact, case.hw)
        groups.setdefault(key, []).append(case)
    return [spec(f"{sh[0]}x{sh[1]}_k{k}_vmin{vmin}", np.stack([c.R for c in g]), k, ksize, hw, vmin, fx,
                 labels=[[c.label for c in g]]) for (sh, k, vmin, ksize, fx, hw), g in groups.items()]


_SPECS = {}


def cached(fn):
    """The case lists are built once per set of branch sizes and shared, unchanged, by the tests."""
    def wrap(base):
        key = (fn.__name__, tuple(sorted(base.items())))
        if key not in _SPECS:
            _SPECS[key] = fn(base)
        return _SPECS[key]
    wrap.__name__ = fn.__name__
    return wrap


def pick(specs, name):
    """The spec of that name.  Test ids are enumerated with FALLBACK_CONSTS; a library whose
    branch sizes regroup the cases fails here, by name, instead of running another case."""
    byname = {sp["name"]: sp for sp in specs}
    assert len(byname) == len(specs), "spec names repeat"
    assert name in byname, f"no case {name} at the library's branch sizes: {sorted(byname)}"
    return byname[name]


@cached
def topk_specs(base):
    return grouped(topk_count_cases(base) + tie_cases(base) + k_cases(base) + subset_cases(base) +
                   certify_edge_cases(base) + huge_case(base))


MEDIAN_SHAPES = [(36, 53), (38, 53), (37, 53)]   # n % 4 == 0; even with n % 4 == 2; odd


@cached
def median_specs(base):
    out = []
    for H, W in MEDIAN_SHAPES:
        ps = median_planes(H, W)
        loads = "vec" if (H * W) % 4 == 0 else "scalar"
        needs = [[{"fallback_scan", loads, "list_lds", "nms_generic"} | ({b} if b else set()) for _, _, b in ps]]
        zero = [(0, i) for i, (name, _, _) in enumerate(ps) if name == "minus_zero"]
        # k = 1100: above every plane's candidate count but the all-equal one's, so the -0.0 pixel is kept
        out.append(spec(f"contents_{H}x{W}", np.stack([R for _, R, _ in ps]), 1100, 1, 0, H * W, True, needs=needs,
                        by_value=zero))
    for k in (20, 2500):   # med_cap 8192 and 12288
        c = consts_for(k, base)
        by_shape = {}
        for m, H, W in median_list_shapes(c):
            by_shape.setdefault((H, W), []).append(m)
        for (H, W), ms in by_shape.items():
            needs = [[{"fallback_scan", "vec" if (H * W) % 4 == 0 else "scalar", "one_bucket",
                       "list_lds" if m <= c["med_cap"] else "list_spill"} for m in ms]]
            out.append(spec(f"lists_k{k}_{H}x{W}", np.stack([median_list_plane(H, W, m, seed=m) for m in ms]), k, 1, 0,
                            H * W, True, needs=needs))
    return out


def nms_contents(H, W, seed):
    """The three kinds of `planes`, zeros below a positive median, zeros above a negative one."""
    rng = np.random.default_rng(seed)
    R = planes(3, H, W, seed) + np.float32(0.0)   # (the rounded plane's -0.0 become +0.0: bits are compared)
    pos = (1 + np.abs(rng.standard_normal((H, W)))).astype(np.float32)
    pos[rng.random((H, W)) < 0.35] = 0.0
    neg = (-1 - np.abs(rng.standard_normal((H, W)))).astype(np.float32)
    neg[rng.random((H, W)) < 0.35] = 0.0
    return np.concatenate([R, pos[None], neg[None]])


def ring_fits(H, W, kh):
    """ring_planes needs kh + 1 rows above and below the middle row and one site's 2 kh + 3 columns."""
    return W >= 2 * kh + 3 and H // 2 - (kh + 1) >= 0 and H // 2 + kh + 1 < H


def nms_spec(name, P, ksize, form):
    """force_exact, k large enough to keep every candidate of every plane (500 beyond 8192).  A
    width that is a multiple of 4 takes the scalar rows when its planes are not 16-byte aligned:
    a level of 1 x 1 planes in front of them sees to that (their number is no multiple of 4)."""
    most = max(int(exact_candidates(R, ksize)[0].sum()) for R in P)
    k = most if most <= 8192 else 500
    needs = [[{"fallback_scan", form}] * len(P)]
    if form == "nms_scalar" and P.shape[2] % 4 == 0:
        assert len(P) % 4
        return spec(name, [np.arange(len(P), dtype=np.float32).reshape(-1, 1, 1), P], k, ksize, 0, P[0].size, True,
                    needs=[[{"fallback_scan"}] * len(P)] + needs)
    return spec(name, P, k, ksize, 0, P[0].size, True, needs=needs)


# (form, H, W, ksize).  ksize 3: the ring planes (window half 1) join wherever they fit, H >= 5
# and W >= 5; they do not fit W = 4, W = 1 and H in {1, 2, 3}, which run on the contents alone.
NMS_ROWS = ([("nms_vec4", 7, W, 3) for W in (4, 64, 256, 260, 516)] +
            [("nms_scalar", 7, W, 3) for W in (1, 5, 53, 63, 64, 65, 127, 129, 130)] +
            [(form, H, W, 3) for form, W in (("nms_vec4", 8), ("nms_scalar", 5))
             for H in (1, 2, 3, 32, 33, 47, 48, 49)] +
            [("nms_generic", H, W, ks) for ks in (1, 5, 7, 31) for H, W in ((45, 120), (33, 102))])
NMS_NAMES = [f"{f}_{H}x{W}_ksize{ks}" for f, H, W, ks in NMS_ROWS]
RING_LESS = [(H, W) for _, H, W, ks in NMS_ROWS if ks == 3 and not ring_fits(H, W, 1)]


@cached
def nms_specs(base):
    out = []
    for name, (form, H, W, ks) in zip(NMS_NAMES, NMS_ROWS):
        P = nms_contents(H, W, seed=1000 * H + W + ks)
        if ks > 1 and ring_fits(H, W, ks // 2):
            P = np.concatenate([P, ring_planes(H, W, ks // 2)])
        out.append(nms_spec(name, P, ks, form))
    return out


def emit_spec():
    R = np.random.default_rng(11).standard_normal((1, 20, 30)).astype(np.float32)
    return spec("emit", [R] * 4, 200, 3, [0, 1, 8, 10], 600, True, needs=[[{"fallback_scan", "nms_scalar"}]] * 4)


def batch_spec():
    H = W = 64
    ex = ("vec", "one_bucket", "list_lds", "nms_generic")
    P = np.stack([layered(H, W, [steps(4.0, 400)], seed=21), layered(H, W, [], seed=22),
                  np.zeros((H, W), np.float32)])
    labels = [[("certified", "none", "whole", "no_ties"),
               ("fallback_run", "none", "regs", "ties_lds") + ex + ("whole", "no_ties"),
               ("fallback_run", "none", "regs", "ties_global") + ex + ("regs", "ties_global")]]
    return spec("batch", P, 100, 1, 0, 300, False, labels=labels)


def level_specs():
    rng = np.random.default_rng(31)
    lv = [rng.standard_normal((2, H, W)).astype(np.float32) for H, W in ((37, 53), (40, 64), (18, 26))]
    cert = ("certified", "none", "whole", "no_ties")
    # levels 1 and 2 start 2 floats past a 16-byte boundary: 40 x 64 planes read with scalar loads
    needs = [[set(), set()], [{"scalar"}, {"scalar"}], [set(), set()]]
    return [spec("levels_certified", lv, 30, 3, [2, 1, 0], 600, False, labels=[[cert, cert]] * 3),
            spec("levels_forced_exact", lv, 30, 3, [2, 1, 0], 600, True,
                 needs=[[a | {"fallback_scan", "nms_scalar"} for a in r] for r in needs])]


def all_specs(base):
    return topk_specs(base) + median_specs(base) + nms_specs(base) + [emit_spec(), batch_spec()] + level_specs()
