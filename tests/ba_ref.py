"""TEST INFRASTRUCTURE ONLY — this repository's numpy restatement of the bundle-adjustment rule
(include/sfmfeat.h sfm_bundle_adjust_dev): Levenberg-Marquardt over every
camera's (R, t) and every point's X with Marquardt damping, strict acceptance, and the rows
that do not move replaced by the identity.  Two forms of one step:

* `step_schur`: the block form the kernels run — U_c, V_j, W_cj (merged over duplicate
  observations of one (c, j)), S = U* - sum W V*^-1 W^T, S d_c = b, back-substitution;
* `step_dense`: (J^T J + lambda diag J^T J) d = -J^T r over all unknowns at once.

Written from the rule, not from scipy (whose iterates are not pinned anywhere in this
repository).  Also the planted scenes the tests and tools/gen_golden_ba.py share.

Only tests/ and tools/gen_golden_ba.py, tools/bench_ba.py import this module."""
from __future__ import annotations

import numpy as np

from tests.registry_ref import rodrigues_to_matrix, rodrigues_to_vector

MAX_ITER = 200
ST_CONVERGED, ST_LAMBDA, ST_NONFINITE, ST_MAXITER = 0, 1, 2, 3
MARGINAL = 1e-9   # tests/structure_ref.py: comparisons closer than this may go either way


class Rejected(Exception):
    """A factorisation met a pivot that is not positive and finite."""


def linearise(sc, R, t, X, jac=True):
    """-> r [M, 2], Jc [M, 2, 6], Jp [M, 2, 3] at the state (R [n_cam, 3, 3], t, X)."""
    c, j = sc["cam_idx"], sc["pt_idx"]
    Rc, K = R[c], sc["K"][c]
    Y = np.einsum("mab,mb->ma", Rc, X[j])
    q = np.einsum("mab,mb->ma", K, Y + t[c])
    pu = q[:, :2] / q[:, 2:3]
    r = pu - sc["obs"]
    if not jac:
        return r, None, None
    g = (K[:, :2, :] - pu[:, :, None] * K[:, 2:3, :]) / q[:, 2, None, None]      # [M, 2, 3]
    Jc = np.concatenate([np.cross(Y[:, None, :], g), g], axis=2)
    Jp = np.einsum("mak,mkb->mab", g, Rc)
    return r, Jc, Jp


def active(sc):
    """(camera moves [n_cam], point moves [n_pts])."""
    ca = np.bincount(sc["cam_idx"], minlength=sc["n_cam"]) > 0
    ca &= ~sc["fixed"].astype(bool)
    return ca, np.bincount(sc["pt_idx"], minlength=sc["n_pts"]) > 0


def _chol(A):
    if not np.isfinite(A).all():
        raise Rejected
    try:
        return np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        raise Rejected


def step_dense(sc, r, Jc, Jp, lam):
    """-> (d_c [n_cam, 6], d_X [n_pts, 3]); raises Rejected."""
    nc, npt, M = sc["n_cam"], sc["n_pts"], len(r)
    n = 6 * nc + 3 * npt
    J = np.zeros((2 * M, n))
    for a in range(2):
        rows = 2 * np.arange(M) + a
        for k in range(6):
            J[rows, 6 * sc["cam_idx"] + k] += Jc[:, a, k]
        for k in range(3):
            J[rows, 6 * nc + 3 * sc["pt_idx"] + k] += Jp[:, a, k]
    H, g = J.T @ J, J.T @ r.reshape(-1)
    A = H + lam * np.diag(np.diag(H))
    ca, pa = active(sc)
    still = np.concatenate([np.repeat(~ca, 6), np.repeat(~pa, 3)])
    A[still, :] = 0.0
    A[:, still] = 0.0
    A[still, still] = 1.0
    g[still] = 0.0
    L = _chol(A)
    d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
    return d[:6 * nc].reshape(nc, 6), d[6 * nc:].reshape(npt, 3)


def step_schur(sc, r, Jc, Jp, lam):
    """The block form -> (d_c, d_X); raises Rejected."""
    nc, npt = sc["n_cam"], sc["n_pts"]
    c, j = sc["cam_idx"], sc["pt_idx"]
    ca, pa = active(sc)
    U = np.zeros((nc, 6, 6))
    V = np.zeros((npt, 3, 3))
    gc, gj = np.zeros((nc, 6)), np.zeros((npt, 3))
    np.add.at(U, c, np.einsum("mak,mal->mkl", Jc, Jc))
    np.add.at(V, j, np.einsum("mak,mal->mkl", Jp, Jp))
    np.add.at(gc, c, np.einsum("mak,ma->mk", Jc, r))
    np.add.at(gj, j, np.einsum("mak,ma->mk", Jp, r))
    pairs, inv = np.unique(c.astype(np.int64) * npt + j, return_inverse=True)   # duplicates of (c, j) merge
    W = np.zeros((len(pairs), 6, 3))
    np.add.at(W, inv.reshape(-1), np.einsum("mak,mal->mkl", Jc, Jp))
    pc, pj = pairs // npt, pairs % npt
    eye6, eye3 = np.eye(6), np.eye(3)
    Us = U + lam * U * eye6
    Vs = V + lam * V * eye3
    Us[~ca], gc[~ca] = eye6, 0.0
    Vs[~pa], gj[~pa] = eye3, 0.0
    W[~ca[pc]] = 0.0
    if not np.isfinite(Vs).all():
        raise Rejected
    try:
        Lv = np.linalg.cholesky(Vs)
    except np.linalg.LinAlgError:
        raise Rejected
    Vi = np.linalg.inv(Lv)
    Vi = np.einsum("nka,nkb->nab", Vi, Vi)
    S = np.zeros((6 * nc, 6 * nc))
    b = -gc.copy()
    for a in range(nc):
        S[6 * a:6 * a + 6, 6 * a:6 * a + 6] = Us[a]
    Yp = np.einsum("pab,pbc->pac", W, Vi[pj])
    order = np.argsort(pj, kind="stable")
    start = np.searchsorted(pj[order], np.arange(npt + 1))
    for jj in range(npt):
        ps = order[start[jj]:start[jj + 1]]
        for p1 in ps:
            if not ca[pc[p1]]:
                continue
            a = pc[p1]
            b[a] += Yp[p1] @ gj[jj]
            for p2 in ps:
                if ca[pc[p2]]:
                    bb = pc[p2]
                    S[6 * a:6 * a + 6, 6 * bb:6 * bb + 6] -= Yp[p1] @ W[p2].T
    L = _chol(S)
    dc = np.linalg.solve(L.T, np.linalg.solve(L, b.reshape(-1))).reshape(nc, 6)
    acc = np.zeros((npt, 3))
    np.add.at(acc, pj, np.einsum("pab,pa->pb", W, dc[pc]))
    dX = -np.einsum("nab,nb->na", Vi, gj + acc)
    return dc, dX


def exp_so3(w):
    return rodrigues_to_matrix(w)


def solve(sc, ftol=1e-2, max_iter=MAX_ITER, form="schur"):
    """The whole rule -> dict(cams [n_cam, 6], X, cost0, cost, status, iters (accepted steps),
    lm_iters (iterations run), rejected (iterations with a rejected factorisation), costs (the
    cost after each accepted step), firm (accepted steps before the first marginal comparison),
    all_firm)."""
    nc = sc["n_cam"]
    cams0, X = sc["cams"].copy(), sc["X"].copy()
    R = np.array([rodrigues_to_matrix(cams0[k, :3]) for k in range(nc)])
    t = cams0[:, 3:].copy()
    ca, _ = active(sc) if len(sc["cam_idx"]) else (np.zeros(nc, bool), None)
    out = dict(cams=cams0, X=X, cost0=0.0, cost=0.0, status=ST_CONVERGED, iters=0, lm_iters=0, rejected=0,
               costs=np.zeros(0), firm=0, all_firm=True)
    if len(sc["cam_idx"]) == 0:
        return out
    step = step_schur if form == "schur" else step_dense
    with np.errstate(all="ignore"):
        r, Jc, Jp = linearise(sc, R, t, X)
        c = float((r * r).sum())
        out.update(cost0=c, cost=c, status=ST_NONFINITE)
        if not np.isfinite(c):
            return out
        lam, acc, status, firm, all_firm, ran, rej, costs = 1e-3, 0, ST_MAXITER, 0, True, 0, 0, []
        for _ in range(max_iter):
            ran += 1
            ct = np.inf
            try:
                dc, dX = step(sc, r, Jc, Jp, lam)
                Rn = np.array([exp_so3(dc[k, :3]) @ R[k] for k in range(nc)])
                tn, Xn = t + dc[:, 3:], X + dX
                rn, _, _ = linearise(sc, Rn, tn, Xn, jac=False)
                ct = float((rn * rn).sum())
            except Rejected:
                rej += 1
            if np.isfinite(ct) and abs(ct - c) <= MARGINAL * c:
                all_firm = False
            if np.isfinite(ct) and ct < c:
                rel = (c - ct) / c
                nd = np.sqrt((dc * dc).sum() + (dX * dX).sum())
                bound = 1e-14 * max(1.0, np.sqrt((t * t).sum() + (X * X).sum()))
                if abs(rel - ftol) <= MARGINAL or abs(nd - bound) <= MARGINAL * bound:
                    all_firm = False
                R, t, X, c = Rn, tn, Xn, ct
                r, Jc, Jp = linearise(sc, R, t, X)
                lam = max(lam / 10.0, 1e-12)
                acc += 1
                costs.append(c)
                if all_firm:
                    firm = acc
                if rel <= ftol or nd <= bound:
                    status = ST_CONVERGED
                    break
            else:
                lam *= 10.0
                if lam > 1e12:
                    status = ST_LAMBDA
                    break
    cams = cams0.copy()
    if acc:
        for k in range(nc):
            if ca[k]:
                cams[k, :3] = rodrigues_to_vector(R[k]).reshape(3)
                cams[k, 3:] = t[k]
    out.update(cams=cams, X=X if acc else sc["X"].copy(), cost=c, status=status, iters=acc, lm_iters=ran,
               rejected=rej, costs=np.array(costs), firm=firm, all_firm=all_firm)
    return out


def cost_of(sc, cams, X):
    R = np.array([rodrigues_to_matrix(cams[k, :3]) for k in range(sc["n_cam"])])
    r, _, _ = linearise(sc, R, np.asarray(cams)[:, 3:], np.asarray(X), jac=False)
    return float((r * r).sum())


# ---------------- planted scenes ----------------

def scene(seed, n_cam, n_pts, views, fixed=(), noise=0.5, pert=0.02, dup=0, idle_cam=False, idle_pt=False,
          exact_cam=None, M=None, heavy_cam=None, arc=0.5, tilt=1.0):
    """A ring of cameras looking at a point cloud.  views(j, rng) -> the cameras that see point j.
    arc: the cameras turn about y by angles spread over [-arc, arc] (pi: a whole orbit); tilt scales
    the x and z components of their rotation vectors (0: pure y rotations).
    noise: pixels; pert: the start's offset from the planted model.  dup: that many observations
    repeated (a second measurement of the same (c, j)); idle_cam / idle_pt append a camera / a
    point nothing observes; exact_cam: a camera whose observations are the start's own
    projections (r = 0 there); M: cut to exactly M observations; heavy_cam = (c, k): keep exactly k
    observations of camera c."""
    rng = np.random.RandomState(seed)
    Xt = rng.uniform(-1.0, 1.0, (n_pts, 3))
    cams_t = np.zeros((n_cam, 6))
    K = np.zeros((n_cam, 3, 3))
    for c in range(n_cam):
        ang = arc * (c - (n_cam - 1) / 2.0) / max(n_cam - 1, 1) * 2.0
        w = np.array([tilt * 0.1 * np.sin(3.0 * c), ang, tilt * 0.05 * np.cos(2.0 * c)])
        Rm = rodrigues_to_matrix(w)
        centre = np.array([4.0 * np.sin(ang), 0.3 * np.cos(c), -4.0 * np.cos(ang)])
        cams_t[c, :3], cams_t[c, 3:] = w, -Rm @ centre
        f = 700.0 + 15.0 * c
        K[c] = [[f, 0.3, 320.0 + c], [0.0, f + 5.0, 240.0 - c], [0.0, 0.0, 1.0]]
    ci, pi = [], []
    for j in range(n_pts):
        for c in views(j, rng):
            ci.append(c)
            pi.append(j)
    ci, pi = np.array(ci, np.int64), np.array(pi, np.int64)
    if heavy_cam is not None:
        c, k = heavy_cam
        own = np.flatnonzero(ci == c)
        assert len(own) >= k, (len(own), k)
        keep = np.ones(len(ci), bool)
        keep[own[k:]] = False
        ci, pi = ci[keep], pi[keep]
    if dup:
        pick = rng.choice(len(ci), dup, replace=False)
        ci, pi = np.concatenate([ci, ci[pick]]), np.concatenate([pi, pi[pick]])
    if M is not None:
        assert len(ci) >= M, (len(ci), M)
        ci, pi = ci[:M], pi[:M]
    sc = dict(n_cam=n_cam, n_pts=n_pts, cam_idx=ci, pt_idx=pi, K=K, fixed=np.zeros(n_cam, np.uint8))
    Rt = np.array([rodrigues_to_matrix(cams_t[c, :3]) for c in range(n_cam)])
    sc["obs"] = np.zeros((len(ci), 2))
    r, _, _ = linearise(sc, Rt, cams_t[:, 3:], Xt, jac=False)
    sc["obs"] = r + noise * rng.standard_normal(r.shape)
    cams = cams_t + pert * rng.standard_normal(cams_t.shape) * np.array([0.2, 0.2, 0.2, 1, 1, 1])
    for c in fixed:
        cams[c] = cams_t[c]
        sc["fixed"][c] = 1
    sc["cams"], sc["X"] = cams, Xt + pert * rng.standard_normal(Xt.shape)
    if exact_cam is not None:
        R0 = np.array([rodrigues_to_matrix(cams[c, :3]) for c in range(n_cam)])
        keep = sc["obs"].copy()
        sc["obs"] = np.zeros_like(keep)
        r0, _, _ = linearise(sc, R0, cams[:, 3:], sc["X"], jac=False)
        sc["obs"] = np.where((ci == exact_cam)[:, None], r0, keep)
    if idle_cam:
        sc["n_cam"] += 1
        sc["cams"] = np.vstack([sc["cams"], [[0.3, -0.2, 0.1, 1.0, 2.0, 3.0]]])
        sc["K"] = np.concatenate([K, K[:1]])
        sc["fixed"] = np.append(sc["fixed"], 0).astype(np.uint8)
    if idle_pt:
        sc["n_pts"] += 1
        sc["X"] = np.vstack([sc["X"], [[9.0, 8.0, 7.0]]])
    return sc


def _all(n_cam):
    return lambda j, rng: range(n_cam)


def _mixed(n_cam):
    """points seen by 1, 2, .. n_cam cameras in turn."""
    def v(j, rng):
        k = j % n_cam + 1
        return sorted(rng.choice(n_cam, k, replace=False).tolist())
    return v


def _half_once(n_cam):
    """the reference's situation: half the points observed once."""
    def v(j, rng):
        if j % 2:
            return [int(rng.randint(n_cam))]
        return sorted(rng.choice(n_cam, min(n_cam, 2 + j % 2 + (j // 2) % 2), replace=False).tolist())
    return v


TILE = 64  # the trailing update of k_ba_solve sweeps a row 64 columns at a time; 6 n_cam crosses it at 11


def cases():
    """name -> scene.  Sizes are the smallest at which each kernel takes another path."""
    c = {}
    c["one_fixed_cam"] = scene(1, 1, 40, _all(1), fixed=(0,))                       # points only
    c["two_cams"] = scene(2, 2, 30, _all(2), fixed=(0,))
    c["three_cams_2fixed"] = scene(3, 3, 24, _mixed(3), fixed=(0, 1))               # no gauge freedom
    c["three_cams_free"] = scene(4, 3, 40, _half_once(3))                           # the reference's situation
    c["four_cams_1fixed"] = scene(5, 4, 30, _mixed(4), fixed=(0,), dup=5)           # duplicated (c, j)
    c["idle_rows"] = scene(6, 3, 24, _mixed(3), fixed=(0, 1), idle_cam=True, idle_pt=True)
    c["exact_cam"] = scene(7, 3, 24, _all(3), fixed=(0, 1), exact_cam=2)            # a camera with r = 0
    for n in (TILE // 6, TILE // 6 + 1, TILE // 6 + 2):                             # 6 n = 60, 66, 72 around 64
        c[f"tile_{n}"] = scene(10 + n, n, 36, _mixed(n), fixed=(0, 1))
    for M in (255, 256, 257):
        c[f"obs_{M}"] = scene(20 + M % 10, 3, 90, _all(3), fixed=(0, 1), M=M)
    for k in (255, 256, 257):                                                       # one camera's list
        c[f"camlist_{k}"] = scene(30 + k % 10, 2, 260, _all(2), fixed=(0,), heavy_cam=(1, k))
    c["obs_2000"] = scene(40, 4, 500, _all(4), fixed=(0, 1))                        # M = 2,000
    return c


RING_SEED = 80


def _ring(n_cam):
    """each point seen by cameras j, j + 1, j + 2 and j + 4 (mod n_cam)."""
    return lambda j, rng: sorted({j % n_cam, (j + 1) % n_cam, (j + 2) % n_cam, (j + 4) % n_cam})


NONPRINCIPAL_CAMS = {1: -1, 7: +1}   # ring9_nonprincipal: camera -> whole turns added to its start angle


def ring_cases():
    """name -> scene: cameras that orbit the cloud, so that their rotations pass pi / 2 and come
    close to pi (cases() stays within 0.52 rad).  Apart from cases(): the fixture holds none of
    them; the restatement solves them at test time, as for many_cameras."""
    c = {}
    c["ring9"] = scene(RING_SEED, 9, 48, _ring(9), fixed=(4, 5), arc=np.pi)
    c["ring9_flat"] = scene(RING_SEED, 9, 48, _ring(9), fixed=(4, 5), arc=np.pi, tilt=0.0)   # pure y rotations
    c["ring8"] = scene(RING_SEED, 8, 48, _ring(8), fixed=(3, 4), arc=7.0 * np.pi / 8.0)
    c["ring5_quarter"] = scene(RING_SEED, 5, 48, _ring(5), fixed=(2, 3), arc=np.pi / 2.0, tilt=0.0)
    sc = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c["ring9"].items()}
    for cam, turns in NONPRINCIPAL_CAMS.items():     # the same rotations, one turn below and one above
        w = sc["cams"][cam, :3]
        th = np.sqrt(w @ w)
        sc["cams"][cam, :3] = w / th * (th + turns * 2.0 * np.pi)
    c["ring9_nonprincipal"] = sc
    return c


def rotation_angles(cams):
    """(c [n], theta [n]) of the cameras' rotations as rodrigues_inv sees them: c = (trace - 1) / 2,
    whose sign chooses the branch, and theta = atan2(s, c) in [0, pi]."""
    R = np.array([rodrigues_to_matrix(w) for w in np.asarray(cams)[:, :3]])
    c = (np.trace(R, axis1=1, axis2=2) - 1.0) / 2.0
    v = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1) / 2.0
    return c, np.arctan2(np.sqrt((v * v).sum(1)), c)


def nonfinite_case():
    sc = scene(50, 2, 12, _all(2), fixed=(0,))
    sc["X"][3, 1] = np.nan
    return sc


def empty_case():
    sc = scene(51, 2, 12, _all(2))
    sc["cam_idx"], sc["pt_idx"], sc["obs"] = sc["cam_idx"][:0], sc["pt_idx"][:0], sc["obs"][:0]
    return sc


LDS_EDGE = 228  # cameras from which k_ba_schur's row of S, (36 n_cam + 6) * 8 bytes, exceeds 64 KiB


def many_cameras(n_cam):
    """n_cam cameras, 3 n_cam points, each seen by cameras j, j + 37 and j + 101 (mod n_cam): nine
    observations per camera, wide baselines and a well-connected camera graph.  (A chain of near
    neighbours, j, j + 1, j + 7, leaves the reduced system so ill-conditioned at 256 cameras that
    the two numpy forms of this file already differ by 1.5e-11 in the final cost.)  Built and
    solved at test time: too large for the fixture."""
    return scene(70 + n_cam % 7, n_cam, 3 * n_cam,
                 lambda j, rng: sorted({j % n_cam, (j + 37) % n_cam, (j + 101) % n_cam}), fixed=(0, 1))


def bench_scene(n_cam=16, n_pts=20000, per_point=3, seed=60):
    """tools/bench_ba.py's workload: every point seen by `per_point` cameras."""
    def v(j, rng):
        return sorted(rng.choice(n_cam, per_point, replace=False).tolist())
    return scene(seed, n_cam, n_pts, v, fixed=(0, 1))
