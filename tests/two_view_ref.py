"""TEST INFRASTRUCTURE ONLY — numpy restatement of sfm_homography_matches_dev and
sfm_two_view_pose_dev (include/sfmfeat.h has both rules; twoview.hip the kernels).

Homography: verify_ref's counter stream at sample size 4 under the H key, in Python integers; the
fit in the device's operation order (Hartley over four points, the 8 x 9 DLT system, the null
vector through ransac_ref.null_vector — the route ransac_ref.device_route_all uses — and the
un-normalisation written out); the division-free transfer test; verify_ref.decide for rounds, stop
and winner.  `fit_H_solve` is a second float64 route (LAPACK's LU on the 8 x 8 system), against
which tests/test_two_view_cpu.py measures how far two float64 fits of one sample move a decision.

Pose: the four candidates by pose_ref.candidates(route="eig"), put into the device's order (the
sign of each eigenvector is the Jacobi iteration's, restated by linalg_ref.jacobi_eig3; a flipped
sign permutes the four and leaves them the same as a set); X by pose_ref's SVD triangulation; the
front and parallax counts.

Every decision comes with its relative gap from equality, so the CPU test can assert that no case
sits close enough to a threshold for the last bits of a fit to decide it.  It also builds the
cases: scenes of four kinds on pose_ref.K_SCENE scattered into verify_ref.slot_table.
Only tests/ import this module."""
from __future__ import annotations

import numpy as np

from tests import linalg_ref as LR
from tests import pose_ref as PR
from tests import ransac_ref as RR
from tests import verify_ref as VR

H_XOR = 0x486F6D6F67726170   # "Homograp": xor-ed into the seed, so the H stream is not verify's
ITERS = 600
SEED = 5
THRESHOLD = 2.0
CONFIDENCE = 0.98
DEPTH_MIN = 1e-6
COS2_MIN = float(np.cos(np.radians(2.0)) ** 2)


# ---------------------------------------------------------------- the sampler
def sample(seed, a, b, it, n):
    """The four indices of sample `it` of pair (a, b) with n matches."""
    key = VR.pair_key((seed & VR.M64) ^ H_XOR, a, b)
    moved = {}
    out = []
    for k in range(4):
        r = VR.mix64(key + (4 * it + k + 1) * VR.G) >> 32
        j = k + ((r * (n - k)) >> 32)
        vj, vk = moved.get(j, j), moved.get(k, k)
        out.append(vj)
        moved[j], moved[k] = vk, vj
    return out


def samples(seed, a, b, n, iters):
    return np.array([sample(seed, a, b, it, n) for it in range(iters)], np.int64).reshape(-1, 4)


def stop_ratios(confidence=CONFIDENCE, iters=ITERS):
    """The table sequence.two_view_geometry passes for `iters` samples (None: no early stop)."""
    from sfmfromscratch_amd import pose
    if not confidence:
        return None
    return pose.ransac_stop_ratios(confidence, min(64, (iters + VR.ROUND - 1) // VR.ROUND), 4)


# ---------------------------------------------------------------- the fit
def hartley4(x):
    """normalise_sample<4>: x [4, 2] -> (normalised [4, 2], s, cx, cy), sums in index order."""
    mx = my = 0.0
    for i in range(4):
        mx += x[i, 0]
        my += x[i, 1]
    mx /= 4.0
    my /= 4.0
    md = 0.0
    for i in range(4):
        md += np.sqrt((x[i, 0] - mx) * (x[i, 0] - mx) + (x[i, 1] - my) * (x[i, 1] - my))
    md /= 4.0
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(2.0) / md
        return np.column_stack((s * x[:, 0] + (-s * mx), s * x[:, 1] + (-s * my))), s, mx, my


def system(a, b):
    """The 8 x 9 DLT system: two rows per point, in point order."""
    A = np.zeros((8, 9))
    for i in range(4):
        u1, v1, u2, v2 = a[i, 0], a[i, 1], b[i, 0], b[i, 1]
        A[2 * i] = [-u1, -v1, -1.0, 0.0, 0.0, 0.0, u2 * u1, u2 * v1, u2]
        A[2 * i + 1] = [0.0, 0.0, 0.0, -u1, -v1, -1.0, v2 * u1, v2 * v1, v2]
    return A


def unnormalise(h, s1, c1x, c1y, s2, c2x, c2y):
    """T2^-1 Hn T1 in the device's order."""
    with np.errstate(all="ignore"):
        t1x, t1y, i2 = -s1 * c1x, -s1 * c1y, 1.0 / s2
        M = np.empty(9)
        for r in range(3):
            M[3 * r] = h[3 * r] * s1
            M[3 * r + 1] = h[3 * r + 1] * s1
            M[3 * r + 2] = (h[3 * r] * t1x + h[3 * r + 1] * t1y) + h[3 * r + 2]
        H = np.empty(9)
        for c in range(3):
            H[c] = M[c] * i2 + c2x * M[6 + c]
            H[3 + c] = M[3 + c] * i2 + c2y * M[6 + c]
            H[6 + c] = M[6 + c]
    return H.reshape(3, 3)


def fit_H(s1, s2):
    """ransac_fit_H for one sample: s1, s2 [4, 2] -> (H [3, 3], pivot columns)."""
    a, sa, ax, ay = hartley4(np.asarray(s1, np.float64))
    b, sb, bx, by = hartley4(np.asarray(s2, np.float64))
    h, piv = RR.null_vector(system(a, b))
    return unnormalise(h, sa, ax, ay, sb, bx, by), piv


def fit_H_solve(s1, s2):
    """A second float64 route: h8 = 1 and LAPACK's solve of the 8 x 8 system (NaN where singular)."""
    a, sa, ax, ay = hartley4(np.asarray(s1, np.float64))
    b, sb, bx, by = hartley4(np.asarray(s2, np.float64))
    A = system(a, b)
    try:
        h = np.append(np.linalg.solve(A[:, :8], -A[:, 8]), 1.0)
    except np.linalg.LinAlgError:
        h = np.full(9, np.nan)
    return unnormalise(h, sa, ax, ay, sb, bx, by)


# ---------------------------------------------------------------- the inlier test
def adjugate(H):
    """adj(H) of a stack [S, 3, 3]: the transposed cofactors, each a difference of two products."""
    h = H.reshape(-1, 9).T
    with np.errstate(all="ignore"):
        g = [h[4] * h[8] - h[5] * h[7], h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
             h[5] * h[6] - h[3] * h[8], h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
             h[3] * h[7] - h[4] * h[6], h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]
    return np.stack(g, -1).reshape(-1, 3, 3)


def transfer_terms(M, x, y, xp, yp):
    """M [S, 3, 3], points [n] -> (lhs, w2) [S, n]: (x' w - u)^2 + (y' w - v)^2 and w^2."""
    m = M.reshape(-1, 9)
    with np.errstate(all="ignore"):
        u = (m[:, 0, None] * x + m[:, 1, None] * y) + m[:, 2, None]
        v = (m[:, 3, None] * x + m[:, 4, None] * y) + m[:, 5, None]
        w = (m[:, 6, None] * x + m[:, 7, None] * y) + m[:, 8, None]
        du, dv = xp * w - u, yp * w - v
        return du * du + dv * dv, w * w


def thr2_of(threshold):
    return np.float64(threshold) * np.float64(threshold) if threshold > 0 else np.float64(-1.0)


def inliers_of(terms, threshold):
    lf, wf, lb, wb = terms
    t2 = thr2_of(threshold)
    with np.errstate(all="ignore"):
        return (lf < t2 * wf) & (lb < t2 * wb)


_TABLES: dict = {}


def correspondences(tab, p):
    """verify_ref.correspondences with the homography's minimum of four matches."""
    cap, nimg = tab["cap"], len(tab["count"])
    a, b = (int(v) for v in tab["pairs"][p])
    n = int(min(max(int(tab["nmatch"][p]), 0), cap))
    attempted = 0 <= a < nimg and 0 <= b < nimg and a != b and n >= 4
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


def sample_table(tab, p, iters, seed=SEED):
    """(idx [iters, 4], H [iters, 3, 3], terms = (lhs_fwd, w2_fwd, lhs_bwd, w2_bwd) each [iters, n]) of
    pair p's first `iters` samples; H is NaN for a sample that contains an invalid match.  Cached by
    the table's name."""
    key = (tab["name"], p, seed)
    have = _TABLES.get(key)
    if have is not None and len(have[0]) >= iters:
        return have[0][:iters], have[1][:iters], tuple(t[:iters] for t in have[2])
    _, n, valid, p1, p2 = correspondences(tab, p)
    a, b = (int(v) for v in tab["pairs"][p])
    idx = samples(seed, a, b, n, iters)
    H = np.full((iters, 3, 3), np.nan)
    for it in np.flatnonzero(valid[idx].all(axis=1)):
        H[it] = fit_H(p1[idx[it]], p2[idx[it]])[0]
    terms = (*transfer_terms(H, p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]),
             *transfer_terms(adjugate(H), p2[:, 0], p2[:, 1], p1[:, 0], p1[:, 1]))
    _TABLES[key] = (idx, H, terms)
    return idx, H, terms


def relative_gap(lhs, rhs):
    """|lhs - rhs| / max(lhs, rhs) where both are finite and rhs > 0 (inf elsewhere)."""
    with np.errstate(all="ignore"):
        g = np.abs(lhs - rhs) / np.maximum(np.abs(lhs), np.abs(rhs))
    return np.where(np.isfinite(g), g, np.inf)


def homography(tab, iters=ITERS, threshold=THRESHOLD, seed=SEED, stop=None, attempt=None):
    """The whole call -> dict(H [P, 3, 3], hkeep [P, cap] uint8, hstat [P, 4] int32, gap [P]): gap is
    the closest relative distance of either transfer inequality from equality over the evaluated
    samples' valid matches (inf where none)."""
    P, cap = len(tab["pairs"]), tab["cap"]
    hkeep = np.zeros((P, cap), np.uint8)
    H = np.full((P, 3, 3), np.nan)
    hstat = np.zeros((P, 4), np.int32)
    gap = np.full(P, np.inf)
    for p in range(P):
        attempted, n, valid, _, _ = correspondences(tab, p)
        if not attempted or (attempt is not None and not attempt[p]):
            hstat[p] = (-1, -1, 0, 0)
            continue
        _, Hs, terms = sample_table(tab, p, iters, seed)
        inl = inliers_of(terms, threshold)
        hstat[p] = VR.decide(inl.sum(axis=1), n, iters, stop, 0)
        hstat[p, 3] = 0
        best, win, done = (int(v) for v in hstat[p, :3])
        if best > 0:
            H[p] = Hs[win]
            hkeep[p, :n] = inl[win]
        if done and valid.any() and threshold > 0 and np.isfinite(threshold):
            t2 = thr2_of(threshold)
            g = np.minimum(relative_gap(terms[0][:done][:, valid], t2 * terms[1][:done][:, valid]),
                           relative_gap(terms[2][:done][:, valid], t2 * terms[3][:done][:, valid]))
            gap[p] = float(g.min())
    return dict(H=H, hkeep=hkeep, hstat=hstat, gap=gap)


def transfer_residuals(H, p1, p2):
    """The symmetric transfer distances [n, 2] (pixels) of a 3 x 3 H on valid correspondences: what
    the GPU test compares the device's winning H through (scale and sign drop out)."""
    with np.errstate(all="ignore"):
        def one(M, a, b):
            q = np.column_stack((a, np.ones(len(a)))) @ M.T
            return np.hypot(q[:, 0] / q[:, 2] - b[:, 0], q[:, 1] / q[:, 2] - b[:, 1])
        return np.column_stack((one(H, p1, p2), one(adjugate(np.asarray(H, np.float64))[0], p2, p1)))


# ---------------------------------------------------------------- the pose
def device_candidates(F, K1, K2):
    """R [4, 3, 3], t [4, 3] of pose_ref.candidates(route="eig") in the device's order, and how far the
    device's construction (Jacobi signs, the compare-exchange order of the eigenvalues) is from the
    candidate it was matched with."""
    R, T = (v[0] for v in PR.candidates(F[None], K1, K2, route="eig"))
    E = K2.T @ F @ K1
    lam, V, _ = LR.jacobi_eig3(E.T @ E)
    for i, j in ((0, 1), (1, 2), (0, 1)):
        if lam[i] < lam[j]:
            lam[[i, j]] = lam[[j, i]]
            V[:, [i, j]] = V[:, [j, i]]
    u = E @ V[:, :2]
    u = u / np.linalg.norm(u, axis=0)
    U = np.column_stack((u, np.cross(u[:, 0], u[:, 1])))
    R1, R2 = U @ PR.W_MAT @ V.T, U @ PR.W_MAT.T @ V.T
    R1 = -R1 if np.linalg.det(R1) < 0 else R1
    R2 = -R2 if np.linalg.det(R2) < 0 else R2
    dev = [(R1, U[:, 2]), (R1, -U[:, 2]), (R2, U[:, 2]), (R2, -U[:, 2])]
    order, worst = [], 0.0
    for Rd, td in dev:
        dist = [max(np.abs(Rd - R[k]).max(), np.abs(td - T[k]).max()) for k in range(4)]
        order.append(int(np.argmin(dist)))
        worst = max(worst, min(dist))
    return R[order], T[order], worst, order


def two_view_pose(tab, keep, F, K, attempt=None, cos2_min=COS2_MIN, perturb=None):
    """The whole call -> dict(pose [P, 12], pstat [P, 4] int32, depth_gap, wide_gap, w_gap, order_err [P]).
    depth_gap: the closest relative distance of a depth from 1e-6 over every (candidate, point);
    w_gap: the smallest |v_w| / |v| of a triangulated homogeneous point (its sign is the depth's);
    wide_gap: the closest relative distance of the parallax inequality from equality (and of d from 0)
    over the winner's front points.  perturb (rng, size): move every candidate's R and t by that much,
    to measure how far candidates that differ in their last bits move a decision."""
    P, cap, nimg = len(tab["pairs"]), tab["cap"], len(tab["count"])
    K = np.broadcast_to(np.asarray(K, np.float64), (nimg, 3, 3)) if np.ndim(K) == 2 else np.asarray(K, np.float64)
    pose = np.full((P, 12), np.nan)
    pstat = np.zeros((P, 4), np.int32)
    gaps = {k: np.full(P, np.inf) for k in ("depth_gap", "wide_gap", "w_gap")}
    order_err = np.zeros(P)
    z_all, q_all = {}, {}
    for p in range(P):
        a, b = (int(v) for v in tab["pairs"][p])
        ok = 0 <= a < nimg and 0 <= b < nimg and a != b and (attempt is None or attempt[p]) \
            and np.isfinite(F[p]).all()
        if not ok:
            pstat[p] = (-1, -1, 0, 0)
            continue
        n = int(min(max(int(tab["nmatch"][p]), 0), cap))
        ca, cb = (int(min(max(int(tab["count"][s]), 0), cap)) for s in (a, b))
        m = tab["matches"][p, :n].astype(np.int64)
        sel = (keep[p, :n] != 0) & (m[:, 0] >= 0) & (m[:, 0] < ca) & (m[:, 1] >= 0) & (m[:, 1] < cb)
        x1 = tab["xy"][a, m[sel, 0]].astype(np.float64)
        x2 = tab["xy"][b, m[sel, 1]].astype(np.float64)
        R, T, order_err[p], _ = device_candidates(np.asarray(F[p], np.float64).reshape(3, 3), K[a], K[b])
        if perturb is not None:
            rng, size = perturb
            R = R + size * rng.uniform(-1, 1, R.shape)
            T = T + size * rng.uniform(-1, 1, T.shape)
        P1 = K[a] @ np.hstack((np.eye(3), np.zeros((3, 1))))
        P2 = K[b] @ np.concatenate((R, T[:, :, None]), axis=2)          # [4, 3, 4]
        with np.errstate(all="ignore"):
            v, _ = PR.null_vectors(PR.dlt_system(x1, x2, P1, P2), "svd")  # [4, n, 4]
            X = v[..., :3] / v[..., 3:]
            z1 = X[..., 2]
            z2 = np.einsum("ck,cnk->cn", R[:, 2, :], X) + T[:, 2, None]
            front = (z1 >= DEPTH_MIN) & (z2 >= DEPTH_MIN)
            counts = front.sum(axis=1)
            win = int(np.argmax(counts)) if counts.max() > 0 else -1   # argmax: the lowest on a tie
            n_wide = 0
            if len(x1):
                zz = np.stack((z1, z2))
                gaps["depth_gap"][p] = float(relative_gap(zz, np.full_like(zz, DEPTH_MIN)).min())
                gaps["w_gap"][p] = float((np.abs(v[..., 3]) / np.linalg.norm(v, axis=-1)).min())
            if win >= 0:
                Xf = X[win][front[win]]
                C = -R[win].T @ T[win]
                e = Xf - C
                d = (Xf * e).sum(axis=1)
                rhs = (cos2_min * (Xf * Xf).sum(axis=1)) * (e * e).sum(axis=1)
                wide = (d <= 0) | (d * d < rhs)
                n_wide = int(wide.sum())
                gaps["wide_gap"][p] = float(min(relative_gap(d * d, rhs).min(),
                                                (np.abs(d) / np.sqrt(rhs / cos2_min)).min()))
                pose[p, :9], pose[p, 9:] = R[win].ravel(), T[win]
                q_all[p] = d * d / rhs
            z_all[p] = np.stack((z1, z2))
        pstat[p] = (int(counts[win]) if win >= 0 else 0, win, n_wide, int(sel.sum()))
    return dict(pose=pose, pstat=pstat, order_err=order_err, z=z_all, q=q_all, **gaps)


# ---------------------------------------------------------------- scenes and cases
R_TRUE = PR.yaw(0.12)
T_TRUE = np.array([-1.0, 0.05, 0.1])


def scene(kind, seed, n, frac, K1=PR.K_SCENE, K2=PR.K_SCENE):
    """Integer correspondences (p1, p2) of n points: "general" is pose_ref.scene; "planar" puts its
    points on z = 8 + 0.3 x - 0.2 y; "rotation" keeps the box and sets t = 0; "random" is
    pose_ref.random_pairs.  The first floor(frac n) second-image points are uniform random pixels."""
    if kind == "general":
        return PR.scene(seed, n, frac, K1, K2)[:2]
    if kind == "random":
        return PR.random_pairs(seed, n)
    rng = np.random.default_rng(seed)
    X = rng.uniform([-3, -2, 4], [3, 2, 12], (n, 3))
    t = T_TRUE
    if kind == "planar":
        X[:, 2] = 8 + 0.3 * X[:, 0] - 0.2 * X[:, 1]
    elif kind == "rotation":
        t = np.zeros(3)
    else:
        raise ValueError(kind)
    a = X @ K1.T
    b = (X @ R_TRUE.T + t) @ K2.T
    p1 = np.round(a[:, :2] / a[:, 2:]).astype(np.int64)
    p2 = np.round(b[:, :2] / b[:, 2:]).astype(np.int64)
    k = int(np.floor(frac * n))
    if k:
        p2[:k] = np.column_stack((rng.integers(0, 960, k), rng.integers(0, 540, k)))
    return p1, p2


# name -> (kind, scene seed, n, outlier fraction): the homography call's single-pair cases
SINGLE = {
    "n3": ("planar", 80, 3, 0.0),
    "n4": ("planar", 81, 4, 0.0),
    "n5": ("rotation", 82, 5, 0.0),
    "n40": ("planar", 83, 40, 0.2),
    "n255": ("rotation", 84, 255, 0.3),
    "n257": ("general", 85, 257, 0.3),
    "n2560": ("planar", 86, 2560, 0.3),
    "n2561": ("rotation", 87, 2561, 0.4),
    "n2700_bad": ("planar", 88, 2700, 0.1),
    "n300_random": ("random", 89, 300, 0.0),
}
BAD_ROWS = {"n2700_bad": 60}
# with the 0.98 table at 600 samples (asserted on the CPU): samples evaluated
STOPS_EARLY = {"n4": 256, "n5": 256, "n40": 256, "n255": 256, "n2560": 256, "n2561": 256, "n2700_bad": 256}
RUNS_ALL = ("n257", "n300_random")
_CASES: dict = {}


def single(name):
    """One pair (slots 2 and 0 of three), as verify_ref.single builds it."""
    if name not in _CASES:
        kind, seed, n, frac = SINGLE[name]
        p1, p2 = scene(kind, seed, n, frac)
        t = VR.slot_table("tv_" + name, [(2, 0, p1, p2)], seed=seed)
        if name in BAD_ROWS:
            rng = np.random.default_rng(4000 + seed)
            bad = rng.permutation(n)[:BAD_ROWS[name]]
            third = len(bad) // 3
            t["matches"][0, bad[:third], 0] = n + rng.integers(0, 3, third)
            t["matches"][0, bad[third:2 * third], 1] = -1 - rng.integers(0, 3, third)
            t["matches"][0, bad[2 * third:], 1] = 1 << 24
        _CASES[name] = t
    return _CASES[name]


def mixed():
    """verify_ref.mixed's table and its nine kinds of pair under another name (the caches are keyed
    by name and hold different things)."""
    if "mixed" not in _CASES:
        _CASES["mixed"] = dict(VR.mixed(), name="tv_mixed")
    return _CASES["mixed"]


VERIFY_ITERS = 300
# name -> (kind, scene seed, n, outlier fraction): the pose call's cases and the classes (general 1,
# planar and rotation-only 2, random 0) asserted on the restatement.  The noise-free general scenes
# are the ones compared with the planted motion.
POSE = {
    "g8": ("general", 123, 8, 0.0),   # (of seeds 110-139 the first third mostly leave fewer than 8 inliers)
    "g64": ("general", 91, 64, 0.0),
    "g65": ("general", 92, 65, 0.0),
    "g300": ("general", 93, 300, 0.0),
    "g300_out": ("general", 94, 300, 0.3),
    "p40": ("planar", 95, 40, 0.2),
    "p300": ("planar", 96, 300, 0.3),
    "r255": ("rotation", 97, 255, 0.3),
    "x120": ("random", 98, 120, 0.0),
}
PLANTED = ("g8", "g64", "g65", "g300")
CLASS = {"general": 1, "planar": 2, "rotation": 2, "random": 0}
K_OTHER = np.array([[640.0, 0, 500], [0, 660, 250], [0, 0, 1]])


def pose_case(name, K2=PR.K_SCENE):
    """(table, verify's restated result) of one pair in slots 2 and 0; K2 other than K_SCENE gives the
    second camera (slot 0) its own intrinsics."""
    key = ("pose", name, K2 is PR.K_SCENE)
    if key not in _CASES:
        kind, seed, n, frac = POSE[name]
        p1, p2 = scene(kind, seed, n, frac, PR.K_SCENE, K2)
        t = VR.slot_table(f"tvp_{name}_{key[2]}", [(2, 0, p1, p2)], seed=seed)
        min_inl = 8 if n < 16 else 16
        v = VR.verify(t, iters=VERIFY_ITERS, min_inliers=min_inl, stop=None)
        _CASES[key] = (t, v)
    return _CASES[key]


def classify(vstat, hstat, pstat, planar_ratio=0.8):
    """TwoView.config on host arrays."""
    out = np.zeros(len(vstat), np.int8)
    ok = vstat[:, 3] != 0
    planar = ok & (hstat[:, 0] >= planar_ratio * vstat[:, 0])
    out[ok] = 1
    out[ok & ~planar & (pstat[:, 1] < 0)] = 3
    out[planar] = 2
    return out


def pipeline_table():
    """The 6-slot table of the end-to-end test: pairs (0, 1) general, (2, 3) planar, (4, 5)
    rotation-only, (1, 2) random (rows i <-> i of two unrelated scenes), (0, 1) again with only its
    first 60 matches — a general pair with fewer points — and (4, 5) with three matches."""
    if "pipeline" not in _CASES:
        n = 120
        sets = [(0, 1, *scene("general", 101, n, 0.2)), (2, 3, *scene("planar", 102, n, 0.2)),
                (4, 5, *scene("rotation", 103, n, 0.2))]
        base = VR.slot_table("tv_pipeline_base", sets, nimg=6, cap=131, seed=11)
        src = [0, 1, 2, 0, 0, 2]
        t = dict(base, name="tv_pipeline", pairs=np.ascontiguousarray(base["pairs"][src]),
                 matches=np.ascontiguousarray(base["matches"][src]),
                 nmatch=np.ascontiguousarray(base["nmatch"][src]))
        t["pairs"][3] = (1, 2)
        t["matches"][3, :n] = np.column_stack((np.arange(n), np.arange(n)))
        t["nmatch"][4] = 60
        t["nmatch"][5] = 3
        _CASES["pipeline"] = t
    return _CASES["pipeline"]
