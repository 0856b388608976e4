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


def null_elimination(A):
    """A [S, 11, 12] -> p [S, 12] with p[11] = 1 (NaN rows where a pivot is zero): Gaussian
    elimination with partial pivoting, the first row of the largest magnitude."""
    A = A.copy()
    S = len(A)
    ar = np.arange(S)
    ok = np.ones(S, bool)
    with np.errstate(all="ignore"):
        for c in range(11):
            piv = c + np.argmax(np.abs(A[:, c:, c]), axis=1)
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
    p = null_elimination(A) if route == "elim" else null_svd(A)
    return pose_from_p(p, s, c)


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
