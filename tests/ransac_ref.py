"""TEST INFRASTRUCTURE ONLY — the per-sample side of the 8-point RANSAC (ransac.hip):

* `device_route`: a float64 numpy restatement of k_ransac_F — Hartley normalisation, the 8 x 9
  system, Gaussian elimination with partial pivoting (first row of largest magnitude; a column
  whose candidates are all below 1e-300 is free), the last free column set to 1 and the others
  to 0, back-substitution over the pivots found, unit norm, rank 2 by removing the smallest
  singular direction, un-normalisation.  It reports the pivot columns, so a test can name the
  branch of the elimination that a sample takes.
* `distances`: the kernels' expression d = |l . p2| / sqrt(l0^2 + l1^2), l = F p1, for every
  (sample, point), in the precision asked for.
* the cases of tests/golden/ransac_fits.npz and `fixture_arrays`, which computes the
  reference's definition of every sample's F (Hartley normalisation, smallest right singular
  vector, rank 2 by dropping sigma3, un-normalisation) in 60 digits with mpmath.
  tools/gen_golden.py writes the file; GPU tests read it and never import mpmath.

Only tests/ and tools/gen_golden.py import this module."""
from __future__ import annotations

import io
import zipfile

import numpy as np

from oracle import ransac as OR
from tests import pose_ref as PR

THRESHOLD = 1.0
# F per sample is compared where the fit is well conditioned:
S18_MAX = 1e6    # sigma1 / sigma8 of the normalised 8 x 9 system
GAP_MAX = 1e3    # sigma2 / (sigma2 - sigma3) of the normalised F before the rank-2 step
MP_DIGITS = 60

K_4K = np.diag([4.0, 4.0, 1.0]) @ PR.K_SCENE  # the scene's camera on a 3840 x 2160 frame


# ---------------------------------------------------------------- the device's route, float64
def hartley8(x):
    """normalise8 of ransac.hip: x [8, 2] -> (normalised [8, 2], s, cx, cy), sums in index order."""
    mx = my = 0.0
    for i in range(8):
        mx += x[i, 0]
        my += x[i, 1]
    mx /= 8.0
    my /= 8.0
    md = 0.0
    for i in range(8):
        md += np.sqrt((x[i, 0] - mx) * (x[i, 0] - mx) + (x[i, 1] - my) * (x[i, 1] - my))
    md /= 8.0
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(2.0) / md
        return np.column_stack((s * x[:, 0] + (-s * mx), s * x[:, 1] + (-s * my))), s, mx, my


def system(a, b):
    u1, v1, u2, v2 = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    return np.stack([u1 * u2, v1 * u2, u2, u1 * v2, v1 * v2, v2, u1, v1, np.ones(8)], -1)


def null_vector(A, free="last"):
    """The elimination of null_vector_8x9 (null_vector_8x9_regs takes the same steps when the
    pivots are columns 0..7) -> (f [9], pivot columns).  free="first" is the mutant that sets
    the first unused column to 1."""
    A = np.array(A, np.float64)
    piv = []
    r = 0
    with np.errstate(all="ignore"):
        for c in range(9):
            if r >= 8:
                break
            best = r + int(np.argmax(np.abs(A[r:, c])))  # the first row of largest |A[., c]|
            if not abs(A[best, c]) >= 1e-300:
                continue
            A[[r, best]] = A[[best, r]]
            for i in range(r + 1, 8):
                A[i, c:] -= (A[i, c] / A[r, c]) * A[r, c:]
            piv.append(c)
            r += 1
        unused = [c for c in range(9) if c not in piv]
        f = np.zeros(9)
        f[unused[-1] if free == "last" else unused[0]] = 1.0
        for i in range(r - 1, -1, -1):
            c = piv[i]
            acc = 0.0
            for k in range(c + 1, 9):
                acc += A[i, k] * f[k]
            f[c] = -acc / A[i, c]
    return f, piv


def device_route(s1, s2, free="last"):
    """k_ransac_F for one sample: s1, s2 [8, 2] -> (F [3, 3], pivot columns)."""
    s1 = np.asarray(s1, np.float64)
    s2 = np.asarray(s2, np.float64)
    a, sa, ax, ay = hartley8(s1)
    b, sb, bx, by = hartley8(s2)
    f, piv = null_vector(system(a, b), free)
    with np.errstate(all="ignore"):
        f = f * (1.0 / np.sqrt(np.sum(f * f)))
        Fn = f.reshape(3, 3)
        if np.isfinite(Fn).all():
            w, V = np.linalg.eigh(Fn.T @ Fn)  # ascending: V[:, 0] is the smallest direction
            v3 = V[:, 0]
            Fn = Fn - np.outer(Fn @ v3, v3)
        T1 = np.array([[sa, 0, -sa * ax], [0, sa, -sa * ay], [0, 0, 1]])
        T2 = np.array([[sb, 0, -sb * bx], [0, sb, -sb * by], [0, 0, 1]])
        return T2.T @ (Fn @ T1), piv


def device_route_all(p1, p2, idx):
    Fs, pivs = [], []
    for s in idx:
        F, piv = device_route(p1[s], p2[s])
        Fs.append(F)
        pivs.append(tuple(piv))
    return np.stack(Fs), pivs


def oracle_route_all(p1, p2, idx):
    return OR.fundamental(p1[idx].astype(np.float64), p2[idx].astype(np.float64))


def distances(F, p1, p2, dtype=np.longdouble):
    """d [samples, points] of the kernels' expression, F [samples, 3, 3] (or a (hi, lo) pair of
    float64 arrays that is summed in `dtype`)."""
    if isinstance(F, tuple):
        F = F[0].astype(dtype) + F[1].astype(dtype)
    F = np.asarray(F, dtype).reshape(-1, 3, 3)
    x1, y1 = (np.asarray(p1)[:, k].astype(dtype) for k in (0, 1))
    x2, y2 = (np.asarray(p2)[:, k].astype(dtype) for k in (0, 1))
    with np.errstate(all="ignore"):
        l = [F[:, r, 0, None] * x1 + F[:, r, 1, None] * y1 + F[:, r, 2, None] for r in range(3)]
        return np.abs(l[0] * x2 + l[1] * y2 + l[2]) / np.sqrt(l[0] * l[0] + l[1] * l[1])


def line_strength(F, p1, dtype=np.longdouble):
    """|(l0, l1)| / |(a0, a1)| [samples, points], a_r = (|F_r0| + |F_r1|) L + |F_r2| with L the largest
    coordinate of the pair: the size of the terms that l_r cancels from.  0 where p1 is the
    epipole of F.  The distance of such a point is 0 / 0 in
    exact arithmetic, so no evaluation of it can be compared with another; tests leave out
    (sample, point) entries below LINE_MIN."""
    if isinstance(F, tuple):
        F = F[0].astype(dtype) + F[1].astype(dtype)
    F = np.asarray(F, dtype).reshape(-1, 3, 3)
    x1, y1 = (np.asarray(p1)[:, k].astype(dtype) for k in (0, 1))
    with np.errstate(all="ignore"):
        l = [F[:, r, 0, None] * x1 + F[:, r, 1, None] * y1 + F[:, r, 2, None] for r in range(2)]
        L = max(1, np.abs(np.asarray(p1)).max())
        a = [(np.abs(F[:, r, 0, None]) + np.abs(F[:, r, 1, None])) * L + np.abs(F[:, r, 2, None]) for r in range(2)]
        return np.sqrt(l[0] * l[0] + l[1] * l[1]) / np.sqrt(a[0] * a[0] + a[1] * a[1])


# float64 rounding leaves about 1e-16 of the cancelled sum in a line that is exactly zero; the
# epipolar line of a point one pixel from the epipole of a 4K frame keeps about 1 / 4000 of it
LINE_MIN = 1e-9


def counts_and_band(d, thr, band):
    """(#(d < thr) per sample, in-band mask): comparisons with NaN are false, as on the device."""
    with np.errstate(invalid="ignore"):
        return (d < thr).sum(axis=1), np.abs(d - thr) <= band


# ---------------------------------------------------------------- cases
GENERAL_ITERS = 400


def general_cases():
    """name -> (p1, p2, iterations): general motion, the fixture holds every sample's F."""
    out = {}
    p1, p2, _ = PR.scene(3, 300, 0.3)
    out["g300"] = (p1, p2, GENERAL_ITERS)
    p1, p2, _ = PR.scene(4, 1000, 0.5, K1=K_4K, K2=K_4K)  # coordinates of a 4K frame
    out["g1000_4k"] = (p1, p2, GENERAL_ITERS)
    p1, p2, _ = PR.scene(5, 8, 0.0)
    out["n8"] = (p1, p2, GENERAL_ITERS)
    p1, p2, _ = PR.scene(6, 9, 0.0)
    out["n9"] = (p1, p2, GENERAL_ITERS)
    return out


def _with_outliers(rng, p1, p2, frac):
    """The planted mask (True = follows the motion) with about `frac` of p2 redrawn."""
    p2 = p2.copy()
    out = rng.random(len(p1)) < frac
    p2[out] = np.column_stack((rng.integers(0, 1900, int(out.sum())), rng.integers(0, 1000, int(out.sum()))))
    return p2, ~out


DEGENERATE_ITERS = 300


def degenerate_cases():
    """name -> (p1, p2, planted mask, iterations): motions whose 8 x 9 systems have a null space
    of more than one dimension (numerically or exactly).  No per-sample F is held for them."""
    out = {}
    n = 200
    for k, (t, frac) in enumerate([((5, -3), 0.3), ((1, 0), 0.3), ((64, 32), 0.3)]):
        rng = np.random.default_rng(100 + k)
        p1 = np.column_stack((rng.integers(0, 1900, n), rng.integers(0, 1000, n))).astype(np.int64)
        p2, mask = _with_outliers(rng, p1, p1 + np.array(t), frac)
        out[f"trans_{t[0]}_{t[1]}"] = (p1, p2, mask, DEGENERATE_ITERS)
    for k, frac in enumerate([0.0, 0.1, 0.3]):
        rng = np.random.default_rng(110 + k)
        p1 = np.column_stack((rng.integers(0, 1900, n), rng.integers(0, 1000, n))).astype(np.int64)
        p2, mask = _with_outliers(rng, p1, p1, frac)
        out[f"same_{int(100 * frac)}"] = (p1, p2, mask, DEGENERATE_ITERS)
    # a planar scene: a homography with integer entries (an affine map), so that the planted
    # points follow it exactly, as the translations do — rounded projections of a plane would
    # leave every planted point half a pixel of noise, and no null-space member is then bound to
    # keep it under the threshold
    rng = np.random.default_rng(120)
    p1 = np.column_stack((rng.integers(0, 900, n), rng.integers(0, 500, n))).astype(np.int64)
    p2 = np.column_stack((2 * p1[:, 0] + p1[:, 1] + 7, p1[:, 0] + 3 * p1[:, 1] + 40))
    p2, mask = _with_outliers(rng, p1, p2, 0.2)
    out["planar"] = (p1, p2, mask, DEGENERATE_ITERS)
    # eight points on one line of the first image: every null vector is a l^T, so F p1 = 0 and
    # the distance is 0 / 0 — no point is guaranteed to any null-space member (empty planted mask)
    rng = np.random.default_rng(121)
    x = rng.permutation(np.arange(20, 900, 37))[:8]
    p1 = np.column_stack((x, 2 * x + 3)).astype(np.int64)
    p2 = np.column_stack((rng.integers(0, 960, 8), rng.integers(0, 540, 8))).astype(np.int64)
    out["collinear8"] = (p1, p2, np.zeros(8, bool), 40)
    return out


BRANCH_ITERS = 64
BRANCH_SEARCH_SEED = 2024
BRANCH_SEARCH_TRIES = 40000
BRANCH_MIN_S81 = 1e-6
BRANCH_SCALE = 64


def search_free_column_samples(want=3):
    """Seeded search over eight correspondences in {0..hi-1}^2 for systems of exact rank 8 whose
    elimination (in input order) leaves a column below 8 free.  -> [(p1, p2, pivot columns)]."""
    rng = np.random.default_rng(BRANCH_SEARCH_SEED)
    found, seen = [], set()
    for _ in range(BRANCH_SEARCH_TRIES):
        hi = int(rng.integers(2, 5))
        s1 = rng.integers(0, hi, (8, 2))
        s2 = rng.integers(0, hi, (8, 2))
        a, sa, _, _ = hartley8(s1.astype(np.float64))
        b, sb, _, _ = hartley8(s2.astype(np.float64))
        if not (np.isfinite(sa) and np.isfinite(sb)):
            continue
        A = system(a, b)
        _, piv = null_vector(A)
        if len(piv) != 8 or piv == list(range(8)) or tuple(piv) in seen:
            continue
        sv = np.linalg.svd(A, compute_uv=False)
        if sv[7] / sv[0] < 100 * BRANCH_MIN_S81:  # (the 60-digit run admits at 1e-6; margin for float64)
            continue
        seen.add(tuple(piv))
        found.append((s1.astype(np.int64), s2.astype(np.int64), tuple(piv)))
        if len(found) == want:
            break
    return found


def branch_cases():
    """name -> (p1, p2, iterations, kind): n = 8 pairs, so every iteration is a permutation of the
    same eight rows.  kind "free": rank 8 with a free column below 8 (the fixture holds F);
    "rank7": two identical correspondences; "const_x2": every second-image x equal (three
    zero columns, rank <= 6).  Every free-column sample found on such a grid has a first-image
    point paired with three second-image points: that point is the epipole, F p1 = 0 there and
    its distance is 0 / 0 by the reference's own definition (see `line_strength`)."""
    out = {}
    for k, (p1, p2, piv) in enumerate(search_free_column_samples()):
        # times 64: a power of two scales every step of the normalisation exactly, so the system
        # and its pivots are bit for bit those of the small grid, while the distances leave the
        # grid's exact multiples of the threshold
        out[f"free{k}"] = (BRANCH_SCALE * p1, BRANCH_SCALE * p2, BRANCH_ITERS, "free")
    p1, p2, _ = PR.scene(7, 8, 0.0)
    p1[5], p2[5] = p1[2], p2[2]
    out["rank7"] = (p1, p2, BRANCH_ITERS, "rank7")
    p1, p2, _ = PR.scene(8, 8, 0.0)
    p2[:, 0] = 417
    out["const_x2"] = (p1, p2, BRANCH_ITERS, "const_x2")
    return out


# ---------------------------------------------------------------- the reference's definition, 60 digits
def _mp_fit(s1, s2):
    """(F [9] unit Frobenius norm as (hi, lo) float64, sigma8 / sigma1, sigma2 / (sigma2 - sigma3))."""
    from mpmath import mp
    mp.dps = MP_DIGITS

    def norm(pts):
        xs = [mp.mpf(int(p[0])) for p in pts]
        ys = [mp.mpf(int(p[1])) for p in pts]
        cx, cy = mp.fsum(xs) / 8, mp.fsum(ys) / 8
        md = mp.fsum(mp.sqrt((x - cx) ** 2 + (y - cy) ** 2) for x, y in zip(xs, ys)) / 8
        s = mp.sqrt(2) / md
        T = mp.matrix([[s, 0, -s * cx], [0, s, -s * cy], [0, 0, 1]])
        return [(s * (x - cx), s * (y - cy)) for x, y in zip(xs, ys)], T

    a, T1 = norm(s1)
    b, T2 = norm(s2)
    A = mp.matrix(8, 9)
    for i in range(8):
        (u1, v1), (u2, v2) = a[i], b[i]
        for j, v in enumerate((u1 * u2, v1 * u2, u2, u1 * v2, v1 * v2, v2, u1, v1, mp.mpf(1))):
            A[i, j] = v
    _, S, V = mp.svd_r(A, full_matrices=True)
    F = mp.matrix(3, 3)
    for k in range(9):
        F[k // 3, k % 3] = V[8, k]
    U, D, Vt = mp.svd_r(F)
    gap = D[1] / (D[1] - D[2])
    F2 = U * mp.diag([D[0], D[1], 0]) * Vt
    Fu = T2.T * F2 * T1
    nrm = mp.sqrt(mp.fsum(Fu[i, j] ** 2 for i in range(3) for j in range(3)))
    hi, lo = np.zeros(9), np.zeros(9)
    for k in range(9):
        v = Fu[k // 3, k % 3] / nrm
        hi[k] = float(v)
        lo[k] = float(v - mp.mpf(hi[k]))
    return hi, lo, float(S[7] / S[0]), float(gap)


def fixture_arrays(progress=None):
    """Every array of tests/golden/ransac_fits.npz, in the file's order.  Needs mpmath."""
    out = {}

    def fits(name, p1, p2, iters):
        idx = OR.samples(len(p1), iters)
        cache = {}
        hi, lo = np.zeros((iters, 9)), np.zeros((iters, 9))
        s81, gap = np.zeros(iters), np.zeros(iters)
        for it, s in enumerate(idx):
            key = tuple(sorted(int(v) for v in s))  # F does not depend on the order of the eight rows
            if key not in cache:
                cache[key] = _mp_fit(p1[list(key)], p2[list(key)])
            hi[it], lo[it], s81[it], gap[it] = cache[key]
        out[f"{name}_F_hi"], out[f"{name}_F_lo"], out[f"{name}_s81"], out[f"{name}_gap"] = hi, lo, s81, gap
        if progress:
            progress(f"{name}: {len(cache)} fits, min s8/s1 {s81.min():.3e}, max gap {gap.max():.3e}")

    for name, (p1, p2, iters) in general_cases().items():
        out[f"{name}_p1"], out[f"{name}_p2"], out[f"{name}_iters"] = p1, p2, np.int64(iters)
        fits(name, p1, p2, iters)
    for name, (p1, p2, mask, iters) in degenerate_cases().items():
        out[f"{name}_p1"], out[f"{name}_p2"], out[f"{name}_iters"] = p1, p2, np.int64(iters)
        out[f"{name}_planted"] = mask
    for name, (p1, p2, iters, kind) in branch_cases().items():
        out[f"{name}_p1"], out[f"{name}_p2"], out[f"{name}_iters"] = p1, p2, np.int64(iters)
        if kind == "free":
            fits(name, p1, p2, iters)
            assert out[f"{name}_s81"].min() >= BRANCH_MIN_S81, name
    out["general"] = np.array(list(general_cases()))
    out["degenerate"] = np.array(list(degenerate_cases()))
    out["branch"] = np.array(list(branch_cases()))
    out["branch_kind"] = np.array([v[3] for v in branch_cases().values()])
    return out


def fixture_bytes(arrays):
    """The .npz container with a constant member timestamp: equal arrays give equal bytes."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key, val in arrays.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with zf.open(info, "w", force_zip64=False) as fid:
                np.lib.format.write_array(fid, np.asanyarray(val), allow_pickle=False)
    return buf.getvalue()


# ---------------------------------------------------------------- what the tests share
# The largest |d - d_ref| of the two float64 routes (LAPACK SVD, the elimination restatement)
# against the 60-digit F over the admitted samples of the fixture, measured on the CPU by
# tests/test_ransac_ref_cpu.py: 2.5e-7 px (the 4K case, a point 57,000 px from its line; 1.5e-8 px
# on the 960 x 540 case).  100 x that is the project's margin for float64 results whose operation
# order differs; the cap of 1e-6 px is the lower of the two and so the bound.
CPU_MEASURED = 2.5e-7
D_BOUND = min(1e-6, 100 * CPU_MEASURED)
MAX_LEFT_OUT = 0.05     # share of a case's samples outside S18_MAX / GAP_MAX
MAX_IN_BAND = 1e-4      # share of (sample, point) tests within D_BOUND of the threshold


def fit_cases(z):
    """The cases whose per-sample F the fixture holds: general motion and the free-column samples."""
    return [str(n) for n in z["general"]] + [str(n) for n, k in zip(z["branch"], z["branch_kind"]) if k == "free"]


def case_inputs(z, name):
    return z[f"{name}_p1"], z[f"{name}_p2"], int(z[f"{name}_iters"])


def reference_distances(z, name):
    """(d_ref [iters, n] longdouble, admitted [iters], defined [iters, n]) of a fit case."""
    p1, p2, _ = case_inputs(z, name)
    F = (z[f"{name}_F_hi"], z[f"{name}_F_lo"])
    admitted = (z[f"{name}_s81"] >= 1.0 / S18_MAX) & (z[f"{name}_gap"] <= GAP_MAX)
    return distances(F, p1, p2), admitted, line_strength(F, p1) >= LINE_MIN


def fit_error(z, name, F):
    """The largest |d(F) - d_ref| over the admitted samples' defined points, the share of samples
    left out, and the number of undefined (sample, point) entries."""
    p1, p2, _ = case_inputs(z, name)
    dref, admitted, defined = reference_distances(z, name)
    d = distances(F, p1, p2)
    use = admitted[:, None] & defined
    with np.errstate(invalid="ignore"):
        diff = np.abs(d - dref)
    diff = np.where(use, diff, 0)
    diff = np.where(np.isnan(diff), np.inf, diff)  # a NaN distance where the reference has one is an error
    return float(diff.max()), float((~admitted).mean()), int((~defined).sum())


def _fma(a, b, c):
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # one rounding, as the device's fma


def epi_inlier_exact(F, x1, y1, x2, y2, thr):
    """epi_inlier of ransac.hip operation by operation on finite inputs (Python floats are IEEE
    doubles; the fused multiply-adds are exact rationals rounded once) -> (the decision, whether
    the near-threshold branch — the reference's own expression — took it)."""
    import math
    F = [float(v) for v in np.asarray(F, np.float64).reshape(9)]
    x1, y1, x2, y2, thr = float(x1), float(y1), float(x2), float(y2), float(thr)
    l0 = _fma(F[0], x1, _fma(F[1], y1, F[2]))
    l1 = _fma(F[3], x1, _fma(F[4], y1, F[5]))
    l2 = _fma(F[6], x1, _fma(F[7], y1, F[8]))
    num = abs(_fma(l0, x2, _fma(l1, y2, l2)))
    den2 = _fma(l0, l0, l1 * l1)
    a = num * num
    t2 = thr * thr
    on = thr > 0.0
    lo = t2 * (1.0 - 2.0 ** -40) if on else -1.0
    hi = t2 * (1.0 + 2.0 ** -40) if on else -1.0
    if a < lo * den2:
        return True, False
    if a > hi * den2:
        return False, False
    return (num / math.sqrt(den2) < thr) if den2 > 0 else False, True
