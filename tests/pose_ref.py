"""TEST INFRASTRUCTURE ONLY — numpy restatement of CameraPose.ransac_camera_motion
(SFM.py:38-124), triangulate_point (:239-253) and triangulate_points (:292-305), vectorised
over iterations, candidates and points: np.random.RandomState(5) samples and the
fundamental matrices of oracle/ransac.py, LAPACK SVDs (np.linalg.svd on a stack runs the
same routine per matrix), and the validity of every (iteration, candidate) in full — no
early exit, so the table also shows iterations with more than one valid candidate.
Pinned to tests/golden/pose.npz, which tools/gen_golden_pose.py makes by calling the
reference's own methods.  `route="eig"` swaps both SVDs for eigen-decompositions of
E^T E / A^T A, and `f_noise` perturbs every F: the admission checks of tests/test_pose_cpu.py.
Only tests/ and tools/gen_golden_pose.py import this module."""
from __future__ import annotations

import numpy as np

from oracle import ransac as OR

K_SCENE = np.array([[800.0, 0, 480], [0, 800, 270], [0, 0, 1]])
W_MAT = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])

# (seed, n, outlier fraction, iterations): the golden cases.  The third was planned with seed 3;
# with this scene generator that seed's winner has 3 inliers, two of them with sigma3 / sigma4
# < 10 in the triangulation system (above the 2 % such points the X comparison may leave
# out), so it got the next seed from 103 on whose winner meets that rule and the admission
# condition of tests/test_pose_cpu.py.
GOLDEN = [(1, 24, 0.0, 60), (2, 40, 0.0, 60), (106, 40, 0.05, 60), (4, 120, 0.0, 40), (5, 300, 0.03, 200)]


def yaw(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def scene(seed, n, frac, K1=K_SCENE, K2=K_SCENE, base=None):
    """Integer correspondences of n points in [-3,3] x [-2,2] x [4,12] seen by a 960 x 540
    camera at `base` (default the origin) and one turned by 0.12 rad and moved by
    (-1, 0.05, 0.1) relative to it; the first floor(frac n) second-image points are uniform
    random pixels."""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-3, -2, 4], [3, 2, 12], (n, 3))
    R2, t2 = yaw(0.12), np.array([-1.0, 0.05, 0.1])
    if base is not None:  # world points such that the first camera still sees the box
        Rb, Tb = base
        Xw = (X - Tb) @ Rb  # Rb^T (X - Tb)
    else:
        Xw = X
    a = X @ K1.T
    b = (X @ R2.T + t2) @ K2.T
    p1 = np.round(a[:, :2] / a[:, 2:]).astype(np.int64)
    p2 = np.round(b[:, :2] / b[:, 2:]).astype(np.int64)
    k = int(np.floor(frac * n))
    if k:
        p2[:k] = np.column_stack((rng.integers(0, 960, k), rng.integers(0, 540, k)))
    return p1, p2, Xw


def random_pairs(seed, n):
    rng = np.random.default_rng(seed)
    return (np.column_stack((rng.integers(0, 960, n), rng.integers(0, 540, n))).astype(np.int64),
            np.column_stack((rng.integers(0, 960, n), rng.integers(0, 540, n))).astype(np.int64))


def null_vectors(A, route="svd"):
    """Smallest right singular vector of each matrix of the stack, and sigma[-2] / sigma[-1]."""
    if route == "svd":
        _, s, Vt = np.linalg.svd(A)
        return Vt[..., -1, :], s[..., -2] / s[..., -1]
    w, V = np.linalg.eigh(np.swapaxes(A, -1, -2) @ A)  # ascending
    with np.errstate(divide="ignore", invalid="ignore"):
        return V[..., :, 0], np.sqrt(np.abs(w[..., 1]) / np.abs(w[..., 0]))


def dlt_system(x1, x2, P1, P2):
    """The 4 x 4 systems of SFM.py:241-246: x1, x2 [n, 2], P1, P2 [..., 3, 4] -> [..., n, 4, 4]."""
    P1 = np.asarray(P1)[..., None, :, :]
    P2 = np.asarray(P2)[..., None, :, :]
    rows = [x1[:, 0, None] * P1[..., 2, :] - P1[..., 0, :], x1[:, 1, None] * P1[..., 2, :] - P1[..., 1, :],
            x2[:, 0, None] * P2[..., 2, :] - P2[..., 0, :], x2[:, 1, None] * P2[..., 2, :] - P2[..., 1, :]]
    shape = np.broadcast_shapes(*[r.shape for r in rows])
    return np.stack([np.broadcast_to(r, shape) for r in rows], axis=-2)


def triangulate(x1, x2, P1, P2, route="svd"):
    """triangulate_point over the rows of x1, x2 -> (X [n, 3], sigma3 / sigma4 [n])."""
    x1 = np.asarray(x1, np.float64)
    x2 = np.asarray(x2, np.float64)
    v, gap = null_vectors(dlt_system(x1, x2, np.asarray(P1, np.float64), np.asarray(P2, np.float64)), route)
    with np.errstate(divide="ignore", invalid="ignore"):
        return v[..., :3] / v[..., 3:], gap


def hartley(x):  # CameraPose.normalize_points (SFM.py:163-178)
    x = np.asarray(x, np.float64)
    cu, cv = x[:, 0].mean(), x[:, 1].mean()
    s = np.sqrt(2) / np.sqrt((x[:, 0] - cu) ** 2 + (x[:, 1] - cv) ** 2).mean()
    T = np.array([[s, 0, -s * cu], [0, s, -s * cv], [0, 0, 1]])
    return np.column_stack((x[:, :2], np.ones(len(x)))) @ T.T, T


def triangulate_points(x1, x2, P1, P2, route="svd"):
    a, T1 = hartley(x1)
    b, T2 = hartley(x2)
    return triangulate(a, b, T1 @ P1, T2 @ P2, route)


def essential_svd(E, route="svd"):
    """U, V^T of the stack E ([I, 3, 3]); route "eig": V from E^T E, u_i = E v_i / sigma_i,
    u3 = u1 x u2 (what the device does)."""
    if route == "svd":
        U, _, Vt = np.linalg.svd(E)
        return U, Vt
    w, V = np.linalg.eigh(np.swapaxes(E, -1, -2) @ E)
    V = V[..., ::-1]
    u = E @ V[..., :2]
    u = u / np.linalg.norm(u, axis=-2, keepdims=True)
    u3 = np.cross(u[..., 0], u[..., 1])
    return np.concatenate([u, u3[..., None]], -1), np.swapaxes(V, -1, -2)


def candidates(F, K1, K2, route="svd"):
    """R [I, 4, 3, 3], T [I, 4, 3]: (R1, T), (R1, -T), (R2, T), (R2, -T) of SFM.py:58-81."""
    U, Vt = essential_svd(K2.T @ F @ K1, route)
    R1 = U @ W_MAT @ Vt
    R2 = U @ W_MAT.T @ Vt
    R1 = np.where(np.linalg.det(R1)[:, None, None] < 0, -R1, R1)
    R2 = np.where(np.linalg.det(R2)[:, None, None] < 0, -R2, R2)
    T = U[..., :, 2]
    return np.stack([R1, R1, R2, R2], 1), np.stack([T, -T, T, -T], 1)


def table(p1, p2, K1, K2, R_base, T_base, threshold, iters, route="svd", f_noise=0.0, chunk=64):
    """Everything ransac_camera_motion decides from, for every iteration: counts [I], masks
    [I, n], valid [I, 4] (the candidate passes _check_valid_pose), nan_depth (any NaN depth),
    R [I, 4, 3, 3], T [I, 4, 3], dist [I, n]."""
    p1 = np.asarray(p1)
    p2 = np.asarray(p2)
    n = len(p1)
    K1, K2 = np.asarray(K1, np.float64), np.asarray(K2, np.float64)
    Rb, Tb = np.asarray(R_base, np.float64), np.asarray(T_base, np.float64).reshape(3)
    out = {"counts": np.zeros(iters, np.int64), "masks": np.zeros((iters, n), bool),
           "valid": np.zeros((iters, 4), bool), "nan_depth": False, "R": np.zeros((iters, 4, 3, 3)),
           "T": np.zeros((iters, 4, 3)), "dist": np.zeros((iters, n))}
    if iters == 0:
        return out
    idx = OR.samples(n, iters)
    F = OR.fundamental(p1[idx].astype(np.float64), p2[idx].astype(np.float64))
    if f_noise:
        F = F * (1.0 + f_noise * np.random.default_rng(99).standard_normal(F.shape))
    a_h = np.column_stack((p1, np.ones(n)))
    b_h = np.column_stack((p2, np.ones(n)))
    lb = np.einsum("kij,nj->kni", F, a_h)
    out["dist"] = np.abs(np.sum(lb * b_h[None], axis=2)) / np.sqrt(lb[..., 0] ** 2 + lb[..., 1] ** 2)
    out["masks"] = out["dist"] < threshold
    out["counts"] = out["masks"].sum(axis=1)
    R, T = candidates(F, K1, K2, route)
    out["R"], out["T"] = R, T
    P1 = K1 @ np.hstack([Rb, Tb[:, None]])
    x1 = p1.astype(np.float64)
    x2 = p2.astype(np.float64)
    for c0 in range(0, iters, chunk):
        Rc, Tc = R[c0:c0 + chunk], T[c0:c0 + chunk]
        P2 = K2 @ np.concatenate([Rc, Tc[..., None]], -1)          # [i, 4, 3, 4]
        X, _ = triangulate(x1, x2, P1, P2, route)                   # [i, 4, n, 3]
        zb = X @ Rb[2] + Tb[2]
        zc = np.einsum("icnk,ick->icn", X, Rc[:, :, 2, :]) + Tc[:, :, 2, None]
        out["nan_depth"] = bool(out["nan_depth"] or np.isnan(zb).any() or np.isnan(zc).any())
        out["valid"][c0:c0 + chunk] = ~((zb < 1e-6) | (zc < 1e-6)).any(axis=-1)
    return out


def winner(tab):
    """(iteration, candidate) the reference's loop ends with, or (-1, -1): strict > over the
    valid candidates in order (SFM.py:81-101)."""
    best, bi, bc = 0, -1, -1
    for it in range(len(tab["counts"])):
        v = np.flatnonzero(tab["valid"][it])
        if len(v) and tab["counts"][it] > best:
            best, bi, bc = int(tab["counts"][it]), it, int(v[0])
    return bi, bc


def ransac_camera_motion(p1, p2, K1, K2, R_base, T_base, threshold=1.0, max_iterations=1000, route="svd"):
    """-> (R, t, in1, in2) with the reference's conventions, plus (winning iteration, table)."""
    p1 = np.asarray(p1)
    p2 = np.asarray(p2)
    if len(p1) < 8:
        return None, None, None, None, -1, None
    tab = table(p1, p2, K1, K2, R_base, T_base, threshold, max_iterations, route)
    it, c = winner(tab)
    if it < 0:
        return None, None, np.array([]), np.array([]), -1, tab
    m = tab["masks"][it]
    return tab["R"][it, c], tab["T"][it, c], p1[m], p2[m], it, tab


def cases():
    """name -> (p1, p2, K1, K2, R_base, T_base, threshold, iterations): the golden scenes,
    their variations and the planted sizes of tests/test_gpu_pose.py (n around the wave
    size, above the 2560-point LDS chunk; iterations 1 and above one 256-sample workgroup)."""
    I3, Z = np.eye(3), np.zeros(3)
    out = {}
    for i, (seed, n, frac, iters) in enumerate(GOLDEN):
        p1, p2, _ = scene(seed, n, frac)
        out[f"g{i}"] = (p1, p2, K_SCENE, K_SCENE, I3, Z, 1.0, iters)
    K2 = np.array([[820.0, 0, 470], [0, 815, 275], [0, 0, 1]])
    p1, p2, _ = scene(11, 60, 0.0, K2=K2)
    out["k1k2"] = (p1, p2, K_SCENE, K2, I3, Z, 1.0, 60)
    base = (yaw(0.02), np.array([0.05, -0.02, 0.1]))
    p1, p2, _ = scene(12, 60, 0.0, base=base)
    out["base"] = (p1, p2, K_SCENE, K_SCENE, base[0], base[1], 1.0, 60)
    p1, p2 = random_pairs(13, 40)
    out["random"] = (p1, p2, K_SCENE, K_SCENE, I3, Z, 1.0, 60)
    p1, p2, _ = scene(14, 7, 0.0)
    out["n7"] = (p1, p2, K_SCENE, K_SCENE, I3, Z, 1.0, 60)
    p1, p2, _ = scene(15, 30, 0.0)
    out["iters0"] = (p1, p2, K_SCENE, K_SCENE, I3, Z, 1.0, 0)
    for n, iters, seed in [(8, 60, 21), (65, 60, 22), (130, 60, 23), (2600, 48, 24), (50, 1, 25), (50, 300, 26)]:
        p1, p2, _ = scene(seed, n, 0.0)
        out[f"n{n}_i{iters}"] = (p1, p2, K_SCENE, K_SCENE, I3, Z, 1.0, iters)
    return out


def triangulation_inputs():
    """1000 integer correspondences of the golden scene and its true projection matrices."""
    p1, p2, _ = scene(31, 1000, 0.0)
    P1 = K_SCENE @ np.hstack([np.eye(3), np.zeros((3, 1))])
    P2 = K_SCENE @ np.hstack([yaw(0.12), np.array([[-1.0], [0.05], [0.1]])])
    return p1, p2, P1, P2


TRI_SIZES = [1, 63, 64, 65, 1000]
