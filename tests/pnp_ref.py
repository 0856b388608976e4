"""TEST INFRASTRUCTURE ONLY — this repository's numpy restatement of the PnP rule (DESIGN.md
§13D; include/sfmfeat.h sfm_pnp_ransac_dev / sfm_pnp_dev): 6-point DLT hypotheses from the
np.random.seed(5) sample stream, inlier counts under a reprojection threshold, the first
strict maximum, and a 6-parameter Levenberg-Marquardt refinement of the winner over its
inliers; `pnp` is the same DLT over all points followed by the same refinement.  Written
from the rule, not from OpenCV (whose outputs are not pinned anywhere in this repository).

The null vector of a sample's 11 x 12 system comes from the elimination the kernel runs (the
same pivot order); `route="svd"` takes numpy's SVD instead, for the admission check of
tests/test_pnp_cpu.py.  The sample stream is numpy's own (np.random.seed(5);
np.random.choice(n, 6, replace=False) per iteration).

The second half is apart from all that: rule 2 and the all-points DLT in 60 digits (mpmath;
`hypotheses_mp`, `dlt_all_mp`), the admission of a sample by the reference's own conditioning
figures, the degenerate scenes, and the arrays of tests/golden/pnp_fits.npz.

Only tests/ and tools/gen_golden_pnp.py, tools/bench_pnp.py import this module."""
from __future__ import annotations

import numpy as np

from tests.registry_ref import rodrigues_to_matrix

THRESHOLD = 8.0
MAX_ITER = 50
ST_CONVERGED, ST_LAMBDA, ST_NONFINITE, ST_MAXITER = 0, 1, 2, 3
MARGINAL = 1e-9   # tests/structure_ref.py: comparisons closer than this may go either way


def samples(n, iters, seed=5):
    """[iters, 6]: np.random.seed(seed); np.random.choice(n, 6, replace=False) per iteration."""
    st = np.random.RandomState(seed)
    return np.array([st.choice(n, 6, replace=False) for _ in range(iters)], np.int64).reshape(-1, 6)


def normalised_pixels(x, K):
    """K^-1 (u, v, 1) for upper-triangular K, by back substitution -> [n, 2]."""
    w = 1.0 / K[2, 2]
    vh = (x[:, 1] - K[1, 2] * w) / K[1, 1]
    uh = ((x[:, 0] - K[0, 1] * vh) - K[0, 2] * w) / K[0, 0]
    return np.column_stack([uh / w, vh / w])


def sample_systems(Xs, xs):
    """Xs [S, 6, 3] world points, xs [S, 6, 2] normalised pixels -> A [S, 11, 12], s [S], c [S, 3]."""
    c = Xs[:, 0]
    for i in range(1, 6):
        c = c + Xs[:, i]
    c = c / 6.0
    d = Xs - c[:, None]
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    md = dist[:, 0]
    for i in range(1, 6):
        md = md + dist[:, i]
    s = np.sqrt(3.0) / (md / 6.0)
    Y = s[:, None, None] * d
    S = len(Xs)
    A = np.zeros((S, 12, 12))
    Yh = np.concatenate([Y, np.ones((S, 6, 1))], axis=2)
    A[:, 0::2, 0:4] = Yh
    A[:, 0::2, 8:12] = -xs[:, :, 0:1] * Yh
    A[:, 1::2, 4:8] = Yh
    A[:, 1::2, 8:12] = -xs[:, :, 1:2] * Yh
    return A[:, :11], s, c


def null_elimination(A, last=False):
    """A [S, 11, 12] -> p [S, 12] with p[11] = 1 (NaN rows where a pivot is zero): Gaussian
    elimination with partial pivoting, the first row of the largest magnitude.  last=True takes
    the last such row instead: not the rule, but what tests/test_pnp_fits_cpu.py holds against
    it to show that the `lattice` scene can tell the two apart."""
    A = A.copy()
    S = len(A)
    ar = np.arange(S)
    ok = np.ones(S, bool)
    with np.errstate(all="ignore"):
        for c in range(11):
            col = np.abs(A[:, c:, c])
            piv = c + (col.shape[1] - 1 - np.argmax(col[:, ::-1], axis=1) if last else np.argmax(col, axis=1))
            rc, rp = A[ar, c].copy(), A[ar, piv].copy()
            A[ar, c], A[ar, piv] = rp, rc
            d = A[:, c, c]
            ok &= np.abs(d) >= 1e-300
            f = A[:, c + 1:, c] / d[:, None]
            A[:, c + 1:, c:] = A[:, c + 1:, c:] - f[:, :, None] * A[:, c:c + 1, c:]
        p = np.zeros((S, 12))
        p[:, 11] = 1.0
        for i in range(10, -1, -1):
            acc = np.zeros(S)
            for k in range(i + 1, 12):
                acc = acc + A[:, i, k] * p[:, k]
            p[:, i] = -acc / A[:, i, i]
    p[~ok] = np.nan
    return p


def null_svd(A):
    return np.linalg.svd(A)[2][:, -1, :]


def det3(M):
    return (M[..., 0, 0] * (M[..., 1, 1] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 1])
            - M[..., 0, 1] * (M[..., 1, 0] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 0])
            + M[..., 0, 2] * (M[..., 1, 0] * M[..., 2, 1] - M[..., 1, 1] * M[..., 2, 0]))


def pose_from_p(p, s, c):
    """p [S, 12] (normalised-frame projection matrices), s [S], c [S, 3] -> R [S, 3, 3], t [S, 3];
    NaN where anything is not finite."""
    with np.errstate(all="ignore"):
        P = p.reshape(-1, 3, 4).copy()
        bad = ~np.isfinite(P).all(axis=(1, 2))
        P[bad] = np.eye(3, 4)
        P = np.where((det3(P[:, :, :3]) < 0)[:, None, None], -P, P)
        M = P[:, :, :3]
        w, V = np.linalg.eigh(np.swapaxes(M, 1, 2) @ M)
        sq = np.sqrt(w)
        R = M @ ((V / sq[:, None, :]) @ np.swapaxes(V, 1, 2))
        sigma = ((sq[:, 0] + sq[:, 1]) + sq[:, 2]) / 3.0
        th = P[:, :, 3] / sigma[:, None]
        Rc = (R[:, :, 0] * c[:, None, 0] + R[:, :, 1] * c[:, None, 1]) + R[:, :, 2] * c[:, None, 2]
        t = (th - s[:, None] * Rc) / s[:, None]
    bad |= ~(np.isfinite(R).all(axis=(1, 2)) & np.isfinite(t).all(axis=1))
    R[bad] = np.nan
    t[bad] = np.nan
    return R, t


def hypotheses(X, x, K, idx, route="elim"):
    """One (R, t) per row of idx [S, 6]."""
    xn = normalised_pixels(x, K)
    A, s, c = sample_systems(X[idx], xn[idx])
    p = null_svd(A) if route == "svd" else null_elimination(A, last=route == "elim_last")
    return pose_from_p(p, s, c)


def elimination_cond_m(X, x, K, idx, last=False):
    """cond M [S] of the elimination route's projection matrices (inf where a pivot is zero)."""
    A, s, c = sample_systems(X[idx], normalised_pixels(x, K)[idx])
    p = null_elimination(A, last)
    M = np.where(np.isfinite(p).all(axis=1)[:, None, None], p.reshape(-1, 3, 4)[:, :, :3], np.zeros((3, 3)))
    sv = np.linalg.svd(M, compute_uv=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sv[:, 2] > 0, sv[:, 0] / sv[:, 2], np.inf)


def errors(X, x, K, R, t):
    """R [S, 3, 3], t [S, 3] -> (reprojection error [S, n], depth [S, n])."""
    with np.errstate(all="ignore"):
        Xc = [((R[:, k, 0, None] * X[None, :, 0] + R[:, k, 1, None] * X[None, :, 1]) + R[:, k, 2, None] * X[None, :, 2])
              + t[:, k, None] for k in range(3)]
        q0 = (K[0, 0] * Xc[0] + K[0, 1] * Xc[1]) + K[0, 2] * Xc[2]
        q1 = K[1, 1] * Xc[1] + K[1, 2] * Xc[2]
        q2 = K[2, 2] * Xc[2]
        dx, dy = q0 / q2 - x[None, :, 0], q1 / q2 - x[None, :, 1]
        return np.sqrt(dx * dx + dy * dy), Xc[2]


def inlier_mask(X, x, K, R, t, threshold=THRESHOLD):
    e, z = errors(X, x, K, R, t)
    with np.errstate(invalid="ignore"):
        return (z > 0) & (e < threshold)


def exp_so3(w):
    return rodrigues_to_matrix(w)


def residuals(X, x, K, R, t):
    """-> r [2n] (u0, v0, u1, v1, ...), J [2n, 6] (d omega, d t), cost."""
    with np.errstate(all="ignore"):
        Y = X @ R.T
        Xc = Y + t
        q = Xc @ K.T
        u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        r = np.column_stack([u - x[:, 0], v - x[:, 1]]).reshape(-1)
        g0 = (K[0][None, :] - u[:, None] * K[2][None, :]) / q[:, 2:3]
        g1 = (K[1][None, :] - v[:, None] * K[2][None, :]) / q[:, 2:3]
        J = np.empty((2 * len(X), 6))
        J[0::2, :3], J[0::2, 3:] = np.cross(Y, g0), g0   # g^T (-[Y]x) = Y x g
        J[1::2, :3], J[1::2, 3:] = np.cross(Y, g1), g1
        return r, J, float(r @ r)


def _solve6(H, g, lam):
    """(H + lam diag H) d = -g by Cholesky; a non-positive pivot gives NaN / inf (no exception)."""
    A = H + lam * np.diag(np.diag(H))
    L = np.zeros((6, 6))
    with np.errstate(all="ignore"):
        for j in range(6):
            L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
            for i in range(j + 1, 6):
                L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
        y = np.zeros(6)
        for i in range(6):
            y[i] = (-g[i] - L[i, :i] @ y[:i]) / L[i, i]
        d = np.zeros(6)
        for i in range(5, -1, -1):
            d[i] = (y[i] - L[i + 1:, i] @ d[i + 1:]) / L[i, i]
    return d


def refine(X, x, K, R, t, max_iter=MAX_ITER):
    """The LM of the rule over all rows of X, x -> dict(R, t, cost0, cost, iters (accepted steps),
    lm_iters (iterations run), status, firm, all_firm) — firm / all_firm as tests/structure_ref.py."""
    R, t = np.array(R, np.float64), np.array(t, np.float64).reshape(3)
    r, J, c = residuals(X, x, K, R, t)
    out = dict(R=R, t=t, cost0=c, cost=c, iters=0, lm_iters=0, status=ST_NONFINITE, firm=0, all_firm=True)
    if not np.isfinite(c):
        return out
    lam, acc, status, firm, all_firm, ran = 1e-3, 0, ST_MAXITER, 0, True, 0
    for _ in range(max_iter):
        ran += 1
        d = _solve6(J.T @ J, J.T @ r, lam)
        with np.errstate(all="ignore"):
            Rt, tt = exp_so3(d[:3]) @ R, t + d[3:]
        rt, Jt, ct = residuals(X, x, K, Rt, tt)
        if np.isfinite(ct) and abs(ct - c) <= MARGINAL * c:
            all_firm = False
        if ct < c:
            nd = np.sqrt(d @ d)
            bound = 1e-14 * max(1.0, np.sqrt(t @ t))
            if abs(nd - bound) <= MARGINAL * bound:
                all_firm = False
            R, t, r, J, c = Rt, tt, rt, Jt, ct
            lam = max(lam / 10.0, 1e-12)
            acc += 1
            if all_firm:
                firm = acc
            if nd <= bound:
                status = ST_CONVERGED
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                status = ST_LAMBDA
                break
    out.update(R=R, t=t, cost=c, iters=acc, lm_iters=ran, status=status, firm=firm, all_firm=all_firm)
    return out


def pnp_ransac(X, x, K, iters, threshold=THRESHOLD, route="elim", max_iter=MAX_ITER):
    """-> dict: found, iteration, counts [iters], inliers (ascending indices), R0, t0 (the winning
    hypothesis), and refine()'s entries; found False: no pose (n < 6, iters == 0, all counts 0)."""
    X, x, K = np.asarray(X, np.float64), np.asarray(x, np.float64), np.asarray(K, np.float64)
    n = len(X)
    out = dict(found=False, iteration=-1, counts=np.zeros(max(iters, 0), np.int32), inliers=np.empty(0, np.int32))
    if n < 6 or iters <= 0:
        return out
    R, t = hypotheses(X, x, K, samples(n, iters), route)
    mask = inlier_mask(X, x, K, R, t, threshold)
    counts = mask.sum(axis=1).astype(np.int32)
    out["counts"] = counts
    best = int(np.argmax(counts))  # the first maximum
    if counts[best] <= 0:
        return out
    inl = np.nonzero(mask[best])[0].astype(np.int32)
    out.update(found=True, iteration=best, inliers=inl, R0=R[best], t0=t[best])
    out.update(refine(X[inl], x[inl], K, R[best], t[best], max_iter))
    return out


def dlt_all(X, x, K):
    """Step 6's start: the DLT over all points -> (R, t)."""
    X, x, K = np.asarray(X, np.float64), np.asarray(x, np.float64), np.asarray(K, np.float64)
    xn = normalised_pixels(x, K)
    c = X.mean(axis=0)
    d = X - c
    s = np.sqrt(3.0) / np.sqrt((d * d).sum(axis=1)).mean()
    Yh = np.column_stack([s * d, np.ones(len(X))])
    A = np.zeros((2 * len(X), 12))
    A[0::2, 0:4], A[0::2, 8:12] = Yh, -xn[:, 0:1] * Yh
    A[1::2, 4:8], A[1::2, 8:12] = Yh, -xn[:, 1:2] * Yh
    w, V = np.linalg.eigh(A.T @ A)
    R, t = pose_from_p(V[:, 0][None], np.array([s]), c[None])
    return R[0], t[0]


def pnp(X, x, K, max_iter=MAX_ITER):
    """-> dict: found, R0, t0 (the DLT's pose) and refine()'s entries over all points."""
    X, x, K = np.asarray(X, np.float64), np.asarray(x, np.float64), np.asarray(K, np.float64)
    if len(X) < 6:
        return dict(found=False)
    R0, t0 = dlt_all(X, x, K)
    if not np.isfinite(R0).all():
        return dict(found=False)
    out = dict(found=True, R0=R0, t0=t0)
    out.update(refine(X, x, K, R0, t0, max_iter))
    return out


def scipy_minimum(X, x, K, R, t):
    """scipy's least_squares (method lm, xtol = ftol = gtol = 1e-15) from (R, t) over the update
    (omega, dt) of the rule -> (R, t, cost = sum of squared residuals)."""
    from scipy.optimize import least_squares

    def fun(p):
        return residuals(X, x, K, exp_so3(p[:3]) @ R, t + p[3:])[0]

    sol = least_squares(fun, np.zeros(6), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    return exp_so3(sol.x[:3]) @ R, t + sol.x[3:], float(2.0 * sol.cost)


# ---------------- the cases ----------------

K_SCENE = np.array([[800.0, 0, 480], [0, 800, 270], [0, 0, 1]])
K_SKEW = np.array([[810.0, 2.5, 470], [0, 790, 280], [0, 0, 1]])


def rot(yaw, pitch=0.0, roll=0.0):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    Rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def scene(seed, n, frac=0.0, K=K_SCENE, R=None, t=None, noise=0.6):
    """n camera-frame points of the box [-3,3] x [-2,2] x [4,12] seen by a 960 x 540 camera of
    pose (R, t) (world = R^T (camera - t)); world points rounded to float32 and pixels to
    integers (what Runner.py:258-259 hands over), sigma = `noise` Gaussian pixel noise, and
    floor(frac n) randomly chosen pixels replaced by uniform random ones
    -> (X [n, 3], x [n, 2], planted inlier mask, R, t)."""
    rng = np.random.default_rng(seed)
    R = rot(0.12, -0.05, 0.03) if R is None else R
    t = np.array([-1.0, 0.05, 0.1]) if t is None else t
    Xc = rng.uniform([-3, -2, 4], [3, 2, 12], (n, 3))
    X = ((Xc - t) @ R).astype(np.float32).astype(np.float64)
    q = (X @ R.T + t) @ K.T
    x = np.round(q[:, :2] / q[:, 2:] + rng.normal(0, noise, (n, 2)))
    planted = np.ones(n, bool)
    k = int(np.floor(frac * n))
    if k:
        idx = rng.choice(n, k, replace=False)
        x[idx] = np.column_stack((rng.integers(0, 960, k), rng.integers(0, 540, k))).astype(np.float64)
        planted[idx] = False
    return X, x, planted, R, t


def random_scene(seed, n):
    rng = np.random.default_rng(seed)
    X = rng.uniform([-3, -2, 4], [3, 2, 12], (n, 3)).astype(np.float32).astype(np.float64)
    x = np.column_stack((rng.integers(0, 960, n), rng.integers(0, 540, n))).astype(np.float64)
    return X, x, np.zeros(n, bool), np.eye(3), np.zeros(3)


CHUNK = 2560  # kRansacChunk (kernels.h): points staged in LDS at a time


def ransac_cases():
    """name -> (X, x, planted, R_true, t_true, K, iterations).  Seeds: the first from the listed
    base on for which the restatement meets the admission conditions of tests/test_pnp_cpu.py."""
    out = {}

    def add(name, sc, K=K_SCENE, iters=50):
        out[name] = sc + (K, iters)

    add("n5", scene(100, 5))
    # six or seven points leave the DLT no redundancy: only the pixel rounding as noise
    add("n6", scene(100, 6, noise=0.0))
    add("n7", scene(100, 7, noise=0.0))
    add("n12", scene(100, 12))
    add("n63", scene(100, 63, 0.1))
    add("n64", scene(101, 64, 0.1))
    add("n65", scene(101, 65, 0.1))
    add("n130", scene(100, 130, 0.3), iters=100)
    add("n2600", scene(103, CHUNK + 40, 0.2), iters=64)
    add("skew", scene(100, 40, 0.1, K=K_SKEW), K=K_SKEW)
    add("bigrot", scene(100, 40, 0.1, R=rot(2.4, 0.5, -1.0), t=np.array([0.5, -0.3, 1.5])))
    for it in (0, 1, 50, 300):
        add(f"it{it}", scene(101, 40, 0.2), iters=it)
    add("random", random_scene(25, 30))
    for n, seed in zip(LM_SIZES[1:], (100, 101, 100, 100)):
        add(f"lm{n}", scene(seed, n))
    return out


LM_SIZES = [6, 255, 256, 257, 513]   # the reduction edges of the refinement's 256-thread workgroup
LM_CASES = ["n6"] + [f"lm{n}" for n in LM_SIZES[1:]]   # every point is an inlier of the winner
NO_POSE = ["n5", "it0"]
# cases whose winner must hold every planted inlier: all but a single sample (its winner is
# that sample, whatever it is worth) and the all-random correspondences
HOLDS = [k for k in ransac_cases() if k not in NO_POSE + ["it1", "random"]]


# ---------------- the rule in 60 digits (mpmath), apart from the elimination route ----------------
# Only tools/gen_golden_pnp.py and the CPU tests call these; the GPU tests read their results
# from tests/golden/pnp_fits.npz and never import mpmath.

MP_DIGITS = 60
S_MAX = 1e4        # a sample is admitted when sigma_1 / sigma_11 of its 11 x 12 system <= S_MAX
CONDM_MAX = 1e3    # ... and cond M of its projection matrix's left 3 x 3 block <= CONDM_MAX
DLT_GAP_MIN = 10.0  # the all-points DLT is admitted when sigma_11 / sigma_12 >= DLT_GAP_MIN
MAX_LEFT_OUT = 0.05  # share of a case's samples that may fall outside the admission
MAX_IN_BAND = 1e-4   # share of (sample, point) tests that may stay undecided
BIG = 1e300        # what an infinite conditioning figure is stored as


def _mp_inputs(X, x, K):
    from mpmath import mp
    mp.dps = MP_DIGITS
    f = mp.mpf
    Kx = [[f(float(K[r, c])) for c in range(3)] for r in range(3)]
    Xm = [[f(float(v)) for v in row] for row in X]
    xn = []
    for u, v in x:
        q2 = 1 / Kx[2][2]
        q1 = (f(float(v)) - Kx[1][2] * q2) / Kx[1][1]
        q0 = (f(float(u)) - Kx[0][1] * q1 - Kx[0][2] * q2) / Kx[0][0]
        xn.append((q0 / q2, q1 / q2))
    return Xm, xn


def _mp_system(Xm, xn, rows, drop_last):
    """The DLT system of the points `rows` (Hartley-normalised among themselves) -> (A, s, c);
    drop_last leaves out the last point's second row (the 11 x 12 system of a sample)."""
    from mpmath import mp
    m = len(rows)
    c = [mp.fsum(Xm[j][k] for j in rows) / m for k in range(3)]
    d = [[Xm[j][k] - c[k] for k in range(3)] for j in rows]
    md = mp.fsum(mp.sqrt(mp.fsum(v * v for v in r)) for r in d) / m
    if md == 0:
        return None, None, c
    s = mp.sqrt(3) / md
    A = mp.zeros(2 * m - (1 if drop_last else 0), 12)
    for i, j in enumerate(rows):
        Yh = [s * d[i][0], s * d[i][1], s * d[i][2], mp.mpf(1)]
        u, v = xn[j]
        for k in range(4):
            A[2 * i, k] = Yh[k]
            A[2 * i, 8 + k] = -u * Yh[k]
            if not (drop_last and i == m - 1):
                A[2 * i + 1, 4 + k] = Yh[k]
                A[2 * i + 1, 8 + k] = -v * Yh[k]
    return A, s, c


def _mp_null(A):
    """The right singular vector of A's smallest singular value and all 12 singular values
    (descending; an 11-row system's twelfth is 0): the eigen-decomposition of A^T A, which in 60
    digits is that vector for every system admitted below (sigma_1 / sigma_11 <= 1e4 costs 8 of
    the 60 digits)."""
    from mpmath import mp
    E, Q = mp.eigsy(A.T * A)
    order = sorted(range(12), key=lambda k: E[k])
    sv = [mp.sqrt(max(E[k], 0)) for k in reversed(order)]
    return [Q[k, order[0]] for k in range(12)], sv


def _mp_pose(p, s, c):
    """P -> (R, t, cond M): the sign from det M, R = M (M^T M)^(-1/2), sigma the mean singular
    value of M, t = (P[:, 3] / sigma - s R c) / s.  None where M is singular."""
    from mpmath import mp
    M = mp.matrix(3, 3)
    for r in range(3):
        for k in range(3):
            M[r, k] = p[4 * r + k]
    p4 = [p[3], p[7], p[11]]
    if mp.det(M) < 0:
        M, p4 = -M, [-v for v in p4]
    w, V = mp.eigsy(M.T * M)
    if min(w) <= 0:
        return None
    q = [mp.sqrt(v) for v in w]
    B = V * mp.diag([1 / v for v in q]) * V.T
    R = M * B
    sigma = mp.fsum(q) / 3
    t = [(p4[r] / sigma - s * mp.fsum(R[r, k] * c[k] for k in range(3))) / s for r in range(3)]
    return R, t, max(q) / min(q)


def _mp_fit(Xm, xn, rows, drop_last):
    """-> (Rt [12] float64 (NaN without a pose), conditioning of the system, cond M); the
    conditioning is sigma_1 / sigma_11 of a sample's system, sigma_11 / sigma_12 of a full one."""
    from mpmath import mp
    nan = np.full(12, np.nan)
    A, s, c = _mp_system(Xm, xn, rows, drop_last)
    if A is None:
        return nan, BIG, BIG
    p, sv = _mp_null(A)
    if drop_last:
        fig = float(sv[0] / sv[10]) if sv[10] > mp.mpf(10) ** -50 * sv[0] else BIG
    else:
        fig = float(sv[10] / sv[11]) if sv[11] > 0 else BIG
    pose = _mp_pose(p, s, c)
    if pose is None:
        return nan, min(fig, BIG), BIG
    R, t, cm = pose
    Rt = np.array([float(R[r, k]) for r in range(3) for k in range(3)] + [float(v) for v in t])
    return Rt, min(fig, BIG), min(float(cm), BIG)


def hypotheses_mp(X, x, K, idx, cache=None):
    """Rule 2 of DESIGN.md §13D from the float64 inputs in 60 digits, one row of idx [S, 6] at a
    time -> (R [S, 3, 3], t [S, 3], sigma_1 / sigma_11 [S], cond M [S]).  cache: a dict shared
    between calls on the same (X, x, K)."""
    Xm, xn = _mp_inputs(np.asarray(X, np.float64), np.asarray(x, np.float64), np.asarray(K, np.float64))
    cache = {} if cache is None else cache
    S = len(idx)
    Rt, s111, cm = np.zeros((S, 12)), np.zeros(S), np.zeros(S)
    for k, row in enumerate(idx):
        key = tuple(int(v) for v in row)
        if key not in cache:
            cache[key] = _mp_fit(Xm, xn, list(key), True)
        Rt[k], s111[k], cm[k] = cache[key]
    return Rt[:, :9].reshape(S, 3, 3), Rt[:, 9:], s111, cm


def dlt_all_mp(X, x, K):
    """The all-points DLT in 60 digits -> (R [3, 3], t [3], sigma_11 / sigma_12)."""
    Xm, xn = _mp_inputs(np.asarray(X, np.float64), np.asarray(x, np.float64), np.asarray(K, np.float64))
    Rt, gap, _ = _mp_fit(Xm, xn, list(range(len(Xm))), False)
    return Rt[:9].reshape(3, 3), Rt[9:], gap


def admitted(s111, condM):
    return (s111 <= S_MAX) & (condM <= CONDM_MAX)


def dlt_all_svd(X, x, K):
    """`dlt_all` with the null vector from an SVD of A itself (the second float64 route)."""
    X, x, K = np.asarray(X, np.float64), np.asarray(x, np.float64), np.asarray(K, np.float64)
    xn = normalised_pixels(x, K)
    c = X.mean(axis=0)
    d = X - c
    s = np.sqrt(3.0) / np.sqrt((d * d).sum(axis=1)).mean()
    Yh = np.column_stack([s * d, np.ones(len(X))])
    A = np.zeros((2 * len(X), 12))
    A[0::2, 0:4], A[0::2, 8:12] = Yh, -xn[:, 0:1] * Yh
    A[1::2, 4:8], A[1::2, 8:12] = Yh, -xn[:, 1:2] * Yh
    R, t = pose_from_p(np.linalg.svd(A)[2][-1][None], np.array([s]), c[None])
    return R[0], t[0]


def pose_deviation(R, t, Rr, tr):
    """max |dR| [S] and |dt| / max(1, |t_ref|) [S]."""
    dR = np.abs(R - Rr).reshape(len(R), -1).max(axis=1)
    dt = np.linalg.norm(t - tr, axis=1) / np.maximum(1.0, np.linalg.norm(tr, axis=1))
    return dR, dt


def rotation_defect(R):
    """max |R R^T - I| [S] (NaN rows give NaN)."""
    with np.errstate(invalid="ignore"):
        return np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).reshape(len(R), -1).max(axis=1)


# ---------------- degenerate and near-degenerate scenes ----------------

DEG_N, DEG_ITERS = 60, 50


def _seen(X, K, rng, noise=0.6):
    R, t = rot(0.12, -0.05, 0.03), np.array([-1.0, 0.05, 0.1])
    q = (X @ R.T + t) @ K.T
    return np.round(q[:, :2] / q[:, 2:] + rng.normal(0, noise, (len(X), 2)))


def degenerate_cases():
    """name -> (X, x, K, iterations): world points for which rule 2's 11 x 12 systems lose rank
    exactly (plane, ident, dup), nearly (tilted, slab3, collinear), here and there (lattice) or
    not at all (slab1)."""
    out = {}
    K = K_SCENE
    rng = np.random.default_rng(300)
    # the exact plane z = 8, coordinates on a 1/4 grid: the centred z are exactly 0, so three
    # columns of every sample's system are exactly 0
    X = np.column_stack((rng.integers(-12, 13, DEG_N) / 4.0, rng.integers(-8, 9, DEG_N) / 4.0, np.full(DEG_N, 8.0)))
    out["plane"] = (X, _seen(X, K, rng), K, DEG_ITERS)
    # the same plane tilted and rounded to float32: nothing is exactly 0 any more
    Xt = (X @ rot(0.3, 0.2, 0.1).T + np.array([0.2, -0.1, 1.0])).astype(np.float32).astype(np.float64)
    out["tilted"] = (Xt, _seen(Xt, K, rng), K, DEG_ITERS)
    for name, half in (("slab3", 1e-3), ("slab1", 0.1)):
        Xs = np.column_stack((rng.uniform(-3, 3, DEG_N), rng.uniform(-2, 2, DEG_N), 8.0 + rng.uniform(-half, half, DEG_N)))
        Xs = Xs.astype(np.float32).astype(np.float64)
        out[name] = (Xs, _seen(Xs, K, rng), K, DEG_ITERS)
    # every correspondence twice: a sample that draws both copies has two identical pairs of rows
    # (seed 301: three samples share the largest count, 60 of 60)
    rd = np.random.default_rng(301)
    Xd = rd.uniform([-3, -2, 4], [3, 2, 12], (DEG_N // 2, 3)).astype(np.float32).astype(np.float64)
    xd = _seen(Xd, K, rd)
    out["dup"] = (np.repeat(Xd, 2, axis=0), np.repeat(xd, 2, axis=0), K, DEG_ITERS)
    # points of one line
    lam = rng.permutation(np.arange(-30, 30))[:DEG_N] / 8.0
    Xl = (np.array([0.3, -0.2, 8.0]) + lam[:, None] * np.array([0.6, 0.3, 0.5])).astype(np.float32).astype(np.float64)
    out["collinear"] = (Xl, _seen(Xl, K, rng), K, DEG_ITERS)
    # an integer lattice (z in steps of 1/8): many samples hold two rows of equal magnitude in a
    # pivot column and a coplanar or collinear subset, so which of the equal rows is taken decides
    # the bits, and for one sample whether a pivot is exactly 0
    rl = np.random.default_rng(310)
    Xg = np.column_stack((rl.integers(-3, 4, DEG_N).astype(np.float64), rl.integers(-2, 3, DEG_N).astype(np.float64),
                          8.0 + rl.integers(-2, 3, DEG_N) / 8.0))
    out["lattice"] = (Xg, _seen(Xg, K, rl), K, DEG_ITERS)
    # six identical points: the mean distance to the centroid is 0
    Xi = np.tile(np.array([[0.5, -0.25, 8.0]]), (6, 1))
    out["ident"] = (Xi, _seen(Xi, K, rng, noise=0.0), K, 9)
    return out


DEG_REFERENCED = ["slab1", "dup"]   # the degenerate-scene cases whose 60-digit hypotheses the fixture holds


def dlt_cases():
    """name -> (X, x, K) for the all-points DLT: n = 6, 7, one wave and one point more, the edges
    of the 256-thread reduction, and the skewed K.  Every point is planted: with the outliers of
    n64, n65 and skew the system has no null vector to speak of (sigma_11 / sigma_12 below 2.2)."""
    c = ransac_cases()
    out = {k: (c[k][0], c[k][1], c[k][5]) for k in ("n6", "n7")}
    out["dlt64"] = scene(100, 64)[:2] + (K_SCENE,)
    out["dlt65"] = scene(101, 65)[:2] + (K_SCENE,)
    out.update({k: (c[k][0], c[k][1], c[k][5]) for k in LM_CASES[1:]})
    out["dltskew"] = scene(100, 40, K=K_SKEW)[:2] + (K_SKEW,)
    return out


DLT_CASES_N = [k for k in dlt_cases() if k != "dltskew"]   # the sizes; dltskew is the skewed K


def fits_cases():
    """name -> (X, x, K, iterations) of every case with a 60-digit reference per sample: the
    fixture cases of pnp.npz that run samples, and DEG_REFERENCED."""
    out = {k: (v[0], v[1], v[5], v[6]) for k, v in ransac_cases().items() if len(v[0]) >= 6 and v[6] > 0}
    deg = degenerate_cases()
    out.update({k: deg[k] for k in DEG_REFERENCED})
    return out


# The largest deviation of the two float64 routes of this module (the elimination restatement,
# LAPACK's SVD; for the all-points DLT eigh of A^T A and the SVD of A) from the 60-digit
# reference over the admitted samples of every case, measured by tests/test_pnp_cpu.py, which
# holds these constants to the measurement (they may not be below it, nor above twice it).
# 100 x the constant, capped at 1e-8, bounds the device (tests/test_gpu_pnp_fits.py).
CPU_MEASURED_R, CPU_MEASURED_T = 5e-11, 3.5e-11            # measured 4.001e-11 (n65, SVD), 2.852e-11 (n63)
CPU_MEASURED_DLT_R, CPU_MEASURED_DLT_T = 5.5e-13, 4.5e-12  # measured 4.400e-13, 3.458e-12 (n6, eigh of A^T A)
FIT_CAP = 1e-8


def fit_bounds():
    return {"bound_R": min(FIT_CAP, 100 * CPU_MEASURED_R), "bound_t": min(FIT_CAP, 100 * CPU_MEASURED_T),
            "bound_dlt_R": min(FIT_CAP, 100 * CPU_MEASURED_DLT_R), "bound_dlt_t": min(FIT_CAP, 100 * CPU_MEASURED_DLT_T)}


def fixture_arrays(progress=None):
    """Every array of tests/golden/pnp_fits.npz, in the file's order.  Needs mpmath."""
    out = {}
    caches = {}
    for name, (X, x, K, iters) in fits_cases().items():
        # (it1, it50 and it300 are one scene and prefixes of one stream)
        cache = caches.setdefault((X.tobytes(), x.tobytes(), K.tobytes()), {})
        R, t, s111, cm = hypotheses_mp(X, x, K, samples(len(X), iters), cache)
        out[f"{name}_R"], out[f"{name}_t"] = R, t
        f32 = lambda a: np.minimum(a, 3e38).astype(np.float32)   # (the figures are for reading; the flag decides)
        out[f"{name}_s111"], out[f"{name}_condM"] = f32(s111), f32(cm)
        out[f"{name}_admitted"] = admitted(s111, cm)
        if progress:
            a = out[f"{name}_admitted"]
            progress(f"{name}: {iters} samples, {int((~a).sum())} left out, worst admitted s1/s11 "
                     f"{s111[a].max():.3e} cond M {cm[a].max():.3e}")
    for name, (X, x, K, iters) in degenerate_cases().items():
        out[f"{name}_X"], out[f"{name}_x"], out[f"{name}_K"], out[f"{name}_iters"] = X, x, K, np.int32(iters)
    for name, (X, x, K) in dlt_cases().items():
        if name.startswith("dlt"):
            out[f"{name}_X"], out[f"{name}_x"], out[f"{name}_K"] = X, x, K
        R, t, gap = dlt_all_mp(X, x, K)
        out[f"{name}_dlt_R"], out[f"{name}_dlt_t"], out[f"{name}_dlt_gap"] = R, t, np.float64(gap)
        if progress:
            progress(f"dlt {name}: n {len(X)} sigma11/sigma12 {gap:.3e}")
    out["fits"] = np.array(list(fits_cases()))
    out["degenerate"] = np.array(list(degenerate_cases()))
    out["dlt"] = np.array(list(dlt_cases()))
    for k, v in fit_bounds().items():
        out[k] = np.float64(v)
    return out


def fixture_bytes(arrays):
    """The .npz container with a constant member timestamp: equal arrays give equal bytes."""
    import io
    import zipfile
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key, val in arrays.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with zf.open(info, "w", force_zip64=False) as fid:
                np.lib.format.write_array(fid, np.asanyarray(val), allow_pickle=False)
    return buf.getvalue()
