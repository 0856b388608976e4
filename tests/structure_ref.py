"""TEST INFRASTRUCTURE ONLY — this repository's numpy restatement of the structure stage
(DESIGN.md §13B): the per-point Levenberg-Marquardt that stands in for
CameraPose.non_linear_triangulation (SFM.py:255-289), the error norms of
Util.print_reprojection_error (Util.py:65-82) and the 2D -> 3D association loop of
Runner.py:241-250.  Written from the rule the kernels implement (include/sfmfeat.h), not
from the reference's code: the reference solves one joint problem with scipy, this solves
each point's own.  tools/gen_golden_structure.py pins it to the reference's outputs in
tests/golden/structure.npz.

The link step is inline code in SFMRunner.perform and cannot be called, so its fixtures are
this restatement's outputs; `link` is written with numpy's own calls (np.linalg.norm(...,
axis=1), np.argmin, <) on the caller's integer arrays, the reference's arithmetic.

Only tests/ and tools/gen_golden_structure.py import this module."""
from __future__ import annotations

import numpy as np

from tests import pose_ref as PR

MAX_ITER = 50
ST_CONVERGED, ST_LAMBDA, ST_NONFINITE, ST_MAXITER = 0, 1, 2, 3
# A comparison the iteration's path depends on is "marginal" when its two sides differ by less
# than this, relatively.  A cost is evaluated to about 500 eps ~ 1e-13 relative (a residual of
# about a pixel is the difference of two numbers of about 500), and two correct
# implementations' steps differ by about eps cond(J^T J) ~ 1e-12 relative, so differences above
# 1e-9 are decided the same way by both with three orders of margin.
MARGINAL = 1e-9

# Against the reference (measured on the CPU with this restatement, tests/test_structure_cpu.py):
# largest ||X_ref - X_rest|| / ||X_rest|| over the clean cases, and the bound 100 x that, capped
X_REF_MEASURED = 3.874e-8
X_REF_TOL = min(1e-6, 100 * X_REF_MEASURED)
# largest positive relative excess of a point's cost over the reference's cost for that point,
# all cases; the bound 100 x that, floored at 1e-12 and capped at 1e-9
COST_EXCESS_MEASURED = 1.664e-12  # c64, a point whose cost is 8.9e-4
COST_DELTA = min(1e-9, max(1e-12, 100 * COST_EXCESS_MEASURED))


def _camera(P, X, p):
    h = P[:, :3] @ X + P[:, 3]
    u, v = h[0] / h[2], h[1] / h[2]
    r = np.array([p[0] - u, p[1] - v])
    J = -np.array([P[0, :3] - u * P[2, :3], P[1, :3] - v * P[2, :3]]) / h[2]
    return r, J


def _evaluate(X, a, b, P1, P2):
    r1, J1 = _camera(P1, X, a)
    r2, J2 = _camera(P2, X, b)
    r = np.concatenate([r1, r2])
    return r, np.vstack([J1, J2]), float(r @ r)


def _solve(H, g, lam):
    """(H + lam diag H) d = -g by Cholesky; a non-positive pivot gives NaN / inf (no exception)."""
    a00, a11, a22 = H[0, 0] + lam * H[0, 0], H[1, 1] + lam * H[1, 1], H[2, 2] + lam * H[2, 2]
    l00 = np.sqrt(a00)
    l10, l20 = H[0, 1] / l00, H[0, 2] / l00
    l11 = np.sqrt(a11 - l10 * l10)
    l21 = (H[1, 2] - l20 * l10) / l11
    l22 = np.sqrt(a22 - l20 * l20 - l21 * l21)
    y0 = -g[0] / l00
    y1 = (-g[1] - l10 * y0) / l11
    y2 = (-g[2] - l20 * y0 - l21 * y1) / l22
    d2 = y2 / l22
    d1 = (y1 - l21 * d2) / l11
    d0 = (y0 - l10 * d1 - l20 * d2) / l00
    return np.array([d0, d1, d2])


def refine_point(X0, a, b, P1, P2, max_iter=MAX_ITER):
    """One point's LM -> (X, cost, accepted steps, status, firm, all_firm): `firm` is the number
    of accepted steps before the first marginal comparison, `all_firm` says none was marginal."""
    X = np.array(X0, np.float64)
    with np.errstate(all="ignore"):
        r, J, c = _evaluate(X, a, b, P1, P2)
        if not np.isfinite(c):
            return X, c, 0, ST_NONFINITE, 0, True
        lam, acc, status, firm, all_firm = 1e-3, 0, ST_MAXITER, 0, True
        for _ in range(max_iter):
            d = _solve(J.T @ J, J.T @ r, lam)
            Xt = X + d
            rt, Jt, ct = _evaluate(Xt, a, b, P1, P2)
            if np.isfinite(ct) and abs(ct - c) <= MARGINAL * c:
                all_firm = False
            if ct < c:
                nd, nx = np.sqrt(d @ d), np.sqrt(X @ X)
                if abs(nd - 1e-14 * nx) <= MARGINAL * 1e-14 * nx:
                    all_firm = False
                X, r, J, c = Xt, rt, Jt, ct
                lam = max(lam / 10.0, 1e-12)
                acc += 1
                if all_firm:
                    firm = acc
                if nd <= 1e-14 * nx:
                    status = ST_CONVERGED
                    break
            else:
                lam *= 10.0
                if lam > 1e12:
                    status = ST_LAMBDA
                    break
    return X, c, acc, status, firm, all_firm


def refine(X0, p1, p2, P1, P2, max_iter=MAX_ITER):
    """-> dict of X [n, 3], cost [n], iters, status, firm [n] int32, all_firm [n] bool."""
    X0 = np.asarray(X0, np.float64)
    p1, p2 = np.asarray(p1, np.float64), np.asarray(p2, np.float64)
    P1, P2 = np.asarray(P1, np.float64).reshape(3, 4), np.asarray(P2, np.float64).reshape(3, 4)
    res = [refine_point(X0[i], p1[i], p2[i], P1, P2, max_iter) for i in range(len(X0))]
    return {"X": np.array([r[0] for r in res]).reshape(-1, 3), "cost": np.array([r[1] for r in res], np.float64),
            "iters": np.array([r[2] for r in res], np.int32), "status": np.array([r[3] for r in res], np.int32),
            "firm": np.array([r[4] for r in res], np.int32), "all_firm": np.array([r[5] for r in res], bool)}


def point_costs(X, p1, p2, P1, P2):
    """Sum of the four squared residuals of SFM.py:262-273 per point."""
    Xh = np.column_stack([X, np.ones(len(X))])
    with np.errstate(all="ignore"):
        h1, h2 = Xh @ np.asarray(P1).reshape(3, 4).T, Xh @ np.asarray(P2).reshape(3, 4).T
        e1 = p1 - h1[:, :2] / h1[:, 2:]
        e2 = p2 - h2[:, :2] / h2[:, 2:]
    return (e1 ** 2).sum(1) + (e2 ** 2).sum(1)


def reprojection_error(X, p1, p2, P1, P2):
    """(mean, errors [n, 2]) of Util.py:65-82."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    Xh = np.column_stack([X, np.ones(len(X))])
    h1, h2 = Xh @ np.asarray(P1).reshape(3, 4).T, Xh @ np.asarray(P2).reshape(3, 4).T
    e1 = np.linalg.norm(p1 - h1[:, :2] / h1[:, 2:], axis=1)
    e2 = np.linalg.norm(p2 - h2[:, :2] / h2[:, 2:], axis=1)
    err = np.column_stack([e1, e2])
    return (float(np.mean(np.mean(err, axis=1))) if len(X) else float("nan")), err


def link(tgt, qry, threshold):
    """Runner.py:241-250 -> (target indices, query indices) of the kept pairs, in query order."""
    ti, qi = [], []
    for q in range(qry.shape[0]):
        dist = np.linalg.norm(tgt - qry[q:q + 1], axis=1)
        k = np.argmin(dist)
        if dist[k] < threshold:
            ti.append(int(k))
            qi.append(q)
    return np.array(ti, np.int32), np.array(qi, np.int32)


def link_results(tgt, p3d, qry, nxt, threshold):
    """(result_prev, result_next, ti, qi) as Runner.py:249-250 builds the first two."""
    ti, qi = link(tgt, qry, threshold)
    return np.array([p3d[k] for k in ti]), np.array([nxt[q] for q in qi]), ti, qi


# ---------------- the cases ----------------

K2_ALT = np.array([[820.0, 0, 470], [0, 815, 275], [0, 0, 1]])
BASE = (PR.yaw(0.02), np.array([0.05, -0.02, 0.1]))
T2 = np.array([-1.0, 0.05, 0.1])


def refine_scene(seed, n, integer=True, K1=PR.K_SCENE, K2=PR.K_SCENE, base=None, wild=0.0, noise=0.7):
    """n points of the box [-3,3] x [-2,2] x [4,12] in front of the first camera (960 x 540,
    f = 800), a second camera turned by 0.12 rad and moved by (-1, 0.05, 0.1) relative to it;
    pixels with sigma = `noise` Gaussian noise, rounded when `integer`; floor(wild n) randomly
    chosen second-image points replaced by uniform random pixels -> (p1, p2, P1, P2)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-3, -2, 4], [3, 2, 12], (n, 3))
    Rb, Tb = base if base is not None else (np.eye(3), np.zeros(3))
    R2 = PR.yaw(0.12)
    P1 = K1 @ np.hstack([Rb, Tb[:, None]])
    P2 = K2 @ np.hstack([R2 @ Rb, (R2 @ Tb + T2)[:, None]])
    a = X @ K1.T
    b = (X @ R2.T + T2) @ K2.T
    p1 = a[:, :2] / a[:, 2:] + rng.normal(0, noise, (n, 2))
    p2 = b[:, :2] / b[:, 2:] + rng.normal(0, noise, (n, 2))
    if integer:
        p1, p2 = np.round(p1), np.round(p2)
    k = int(np.floor(wild * n))
    if k:
        idx = rng.choice(n, k, replace=False)
        p2[idx] = np.column_stack((rng.integers(0, 960, k), rng.integers(0, 540, k))).astype(np.float64)
    return p1, p2, P1, P2


CLEAN_SIZES = [1, 12, 63, 64, 65, 129, 200]  # around the wave and the 128-thread workgroup
BATCH = ["b0", "b1", "b2"]                   # one launch, three camera pairs


def refine_cases():
    """name -> (p1, p2, P1, P2); the linear triangulation that starts the refinement is the
    reference's own, stored in the fixture."""
    out = {}
    for n in CLEAN_SIZES:
        out[f"c{n}"] = refine_scene(100 + n, n)
    out["float40"] = refine_scene(301, 40, integer=False)
    out["k1k2base"] = refine_scene(302, 40, K2=K2_ALT, base=BASE)
    out["wild10"] = refine_scene(303, 60, wild=0.1)
    out["wild30"] = refine_scene(304, 60, wild=0.3)
    out["b0"] = refine_scene(311, 12)
    out["b1"] = refine_scene(312, 65, K2=K2_ALT)
    out["b2"] = refine_scene(313, 40, base=BASE)
    return out


WILD = ["wild10", "wild30"]
CLEAN = [k for k in refine_cases() if k not in WILD]

LINK_CHUNK = 2560  # kRansacChunk (kernels.h): targets staged in LDS at a time
OFFSETS = [(0, 0), (3, 4), (2, 4), (1, 1), (0, 5), (3, 3), (40, -25), (4, 3), (-2, -4), (6, 0), (-3, 3)]


def link_scene(seed, m, nq, dtype=np.int32):
    """m target pixels, nq queries: a target plus one of OFFSETS (several of them at exactly
    d = 5 and at d^2 = 20, 18), every seventh a uniform random pixel."""
    rng = np.random.default_rng(seed)
    tgt = np.column_stack((rng.integers(0, 960, m), rng.integers(0, 540, m)))
    pick = rng.integers(0, m, nq)
    qry = tgt[pick] + np.array([OFFSETS[i % len(OFFSETS)] for i in range(nq)])
    rnd = np.arange(nq) % 7 == 6
    qry[rnd] = np.column_stack((rng.integers(0, 960, nq), rng.integers(0, 540, nq)))[rnd]
    p3d = rng.uniform([-3, -2, 4], [3, 2, 12], (m, 3))
    nxt = np.column_stack((rng.integers(0, 960, nq), rng.integers(0, 540, nq)))
    return tgt.astype(dtype), p3d, qry.astype(dtype), nxt.astype(dtype)


def link_cases():
    """name -> (points_2d_prev, p3d, prev_frame_2d, next_frame_2d, dist_threshold)."""
    out = {}
    for i, (m, nq) in enumerate([(1, 1), (64, 65), (130, 129), (LINK_CHUNK + 1, 300)]):
        out[f"l{m}_{nq}"] = link_scene(400 + i, m, nq) + (5.0,)
    # duplicate targets and distinct targets at equal distance: the first index wins
    tgt = np.array([[10, 10], [20, 20], [10, 10], [12, 10], [8, 10], [20, 20]], np.int32)
    qry = np.array([[10, 10], [11, 10], [9, 10], [20, 21], [10, 12], [300, 300]], np.int32)
    out["dups"] = (tgt, np.arange(18, dtype=np.float64).reshape(6, 3), qry, qry + 100, 5.0)
    # (3, 4): d = 5.0 exactly, not < 5.0; (2, 4): d^2 = 20, kept
    tgt = np.array([[100, 100]], np.int32)
    qry = np.array([[103, 104], [102, 104], [100, 105], [96, 97]], np.int32)
    out["edge5"] = (tgt, np.array([[1.0, 2.0, 3.0]]), qry, qry * 2, 5.0)
    # no sum of two squares lies in (20, 25), so 4.5 keeps what 5.0 keeps; 4.4 drops d^2 = 20
    out["thr4_5"] = link_scene(410, 64, 65) + (4.5,)
    out["thr4_4"] = link_scene(410, 64, 65) + (4.4,)
    t, p, q, nx = link_scene(411, 40, 30)
    out["nothing"] = (t, p, q + 2000, nx, 5.0)
    out["int64"] = link_scene(412, 70, 66, dtype=np.int64) + (5.0,)
    return out
