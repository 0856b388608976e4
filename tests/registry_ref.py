"""numpy restatement of the global point registry and of the bundle-adjustment input score
(SFMRunner.add_points / is_new_point / find_existing_point, Runner.py:361-385;
prepare_for_ba and total_reprojection_error, Runner.py:311-334, :387-401), the case generators
of tests/golden/registry.npz (tools/gen_golden_registry.py runs the reference's own methods on
them), and the Rodrigues formulas in any float type.

Two forms of the registry rule:
* `add_sequential`: the reference's loop, one point at a time against the whole registry.
* `add_two_phase`: the decomposition registry.hip runs — every point against the registry as
  it stood before the call, every point against the earlier points of the call, a serial
  walk over the contested points only, then an exclusive scan for the new slots.
  strict=True marks a point contested when any earlier point of the call is within the
  threshold; strict=False (the kernel's rule) only when such a point is strictly nearer than
  the hit in the old registry — a tie goes to the old registry, so nothing else can change
  the answer.  All three give the same indices and registry (tests/test_registry_cpu.py).
"""
from __future__ import annotations

import numpy as np

THRESHOLD = 1e-6
CHUNK = 256           # registry.hip's kRegChunk (pose.REGISTRY_CHUNK)
REG_SIZES = (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
BATCH_SIZES = (1, 63, 64, 65, 257)


def _dist(G, p):
    """np.linalg.norm(G - p, axis=1) on 3 columns: sqrt((dx*dx + dy*dy) + dz*dz)."""
    d = G - p
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def add_sequential(G, pts, thr=THRESHOLD):
    """G: list of float64 3-vectors (extended in place) -> indices [n]."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    out = np.empty(len(pts), np.int64)
    m = len(G)
    Ga = np.empty((m + len(pts), 3))  # np.array(self.global_points_3D), kept instead of rebuilt
    if m:
        Ga[:m] = np.array(G)
    for i, p in enumerate(pts):
        if m:
            d = np.linalg.norm(Ga[:m] - p[np.newaxis], axis=1)
            if np.min(d) < thr:
                out[i] = np.argmin(d)
                continue
        Ga[m] = p
        G.append(p)
        m += 1
        out[i] = m - 1
    return out


def add_two_phase(G, pts, thr=THRESHOLD, strict=False, info=None):
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    n, count = len(pts), len(G)
    old_d = np.full(n, np.inf)
    old_j = np.full(n, -1, np.int64)
    if count:
        Ga = np.array(G)
        for i in range(n):
            d = _dist(Ga, pts[i])
            j = int(np.argmin(d))
            if d[j] < thr:
                old_d[i], old_j[i] = d[j], j
    contested = np.zeros(n, bool)
    for i in range(1, n):
        m = _dist(pts[:i], pts[i]).min()
        contested[i] = m < thr and (strict or m < old_d[i])
    res = old_j.copy()  # >= 0 old index, -1 new, <= -3 point -(r + 3) of the call
    for i in np.flatnonzero(contested):
        ks = np.flatnonzero(res[:i] == -1)
        best, bk = np.inf, -1
        if len(ks):
            d = _dist(pts[ks], pts[i])
            q = int(np.argmin(d))
            if d[q] < thr:
                best, bk = d[q], int(ks[q])
        res[i] = -(bk + 3) if best < old_d[i] else old_j[i]
    new = res == -1
    slot = count + np.cumsum(new) - new
    out = np.where(new, slot, res)
    ref = res <= -3
    out[ref] = slot[-(res[ref] + 3)]
    G.extend(list(pts[new]))
    if info is not None:
        info["contested"] = int(contested.sum())
    return out.astype(np.int64)


def replay(calls, add=add_sequential, thr=THRESHOLD):
    """calls: [(p3d, p2d, frame)] -> (point_indices, frame_indices, G [m, 3], points_2D)."""
    G, pi, fi, p2 = [], [], [], []
    for p3d, p2d, f in calls:
        idx = add(G, p3d, thr) if len(p3d) else np.empty(0, np.int64)
        pi.extend(idx.tolist())
        fi.extend([f] * len(idx))
        p2.extend(list(p2d))
    return (np.array(pi, np.int64), np.array(fi, np.int64), np.array(G, np.float64).reshape(-1, 3),
            np.array(p2))


# ---------------- cases ----------------

def _p2(rng, n):
    return rng.randint(0, 2000, size=(n, 2)).astype(np.int64)


def boundary_indices(R):
    """The registry's first and last entries and those either side of every chunk boundary."""
    s = {0, R - 1}
    for b in range(CHUNK, R + 1, CHUNK):
        s.update((b - 1, b, b + 1))
    return sorted(i for i in s if 0 <= i < R)


def chunk_case(R, seed):
    """A registry of R points, then batches of BATCH_SIZES: exact copies of the boundary entries,
    copies of random entries, points 0.3e-6 beside an entry; the last batch also fresh points."""
    rng = np.random.RandomState(seed)
    base = rng.uniform(-10, 10, size=(R, 3))
    calls = [(base, _p2(rng, R), 0)]
    bi = boundary_indices(R)
    for f, B in enumerate(BATCH_SIZES, start=1):
        rows = []
        for k in range(B):
            m = k % 4
            if k < len(bi):
                rows.append(base[bi[(k + f) % len(bi)]].copy())
            elif m == 0:
                rows.append(base[rng.randint(R)].copy())
            elif m == 1:
                rows.append(base[rng.randint(R)] + np.array([0.3e-6, 0.0, 0.0]))
            elif m == 2 and B == BATCH_SIZES[-1]:
                rows.append(rng.uniform(-10, 10, size=3))
            else:
                rows.append(base[bi[rng.randint(len(bi))]].copy())
        calls.append((np.array(rows), _p2(rng, B), f))
    return calls


LATTICE_OFFSETS = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [-5.0, 0.5, 7.0]])


def lattice_points(rng, n, pitch=0.4e-6, sites=6):
    o = LATTICE_OFFSETS[rng.randint(len(LATTICE_OFFSETS), size=n)]
    return o + pitch * rng.randint(sites, size=(n, 3))


def contested_case(seed=11):
    rng = np.random.RandomState(seed)
    calls = []
    for f in range(3):
        p = lattice_points(rng, 200)
        if f == 2:
            G = replay(calls)[2]
            p = np.concatenate([p, G[rng.randint(len(G), size=50)]])
            p = p[rng.permutation(len(p))]
        calls.append((p, _p2(rng, len(p)), f))
    return calls


def sequence_case(seed=21, n=300, frames=4):
    """The calls SFMRunner.perform issues (Runner.py:217, :269, :280)."""
    rng = np.random.RandomState(seed)
    off = np.array([0.0, 0.0, 10.0])  # in front of the cameras of sequence_poses
    p3d = rng.uniform(-4, 4, size=(n, 3)) + off
    calls = [(p3d, _p2(rng, n), 0)]
    for f in range(1, frames):
        prev = p3d[rng.randint(len(p3d), size=n - 7 * f)]  # exact copies, repeats included
        calls.append((prev, _p2(rng, len(prev)), f))
        p3d = rng.uniform(-4, 4, size=(n + f, 3)) + off
        p3d[::17] = prev[:len(p3d[::17])]  # a few re-triangulated onto known points
        calls.append((p3d, _p2(rng, len(p3d)), f))
    return calls


def split_points(seed=31):
    rng = np.random.RandomState(seed)
    p = np.concatenate([rng.uniform(-2, 2, size=(150, 3)), lattice_points(rng, 107)])
    return p[rng.permutation(len(p))], _p2(rng, 257)


def cases():
    e = 2.0 ** -20
    order = np.array([[0, 0, 0], [0.6e-6, 0, 0], [1.2e-6, 0, 0], [5, 5, 5], [5 + 2 * e, 5, 5], [5 + e, 5, 5],
                      [0, 0, 0]], np.float64)
    rng = np.random.RandomState(1)
    z = np.zeros((1, 3))
    one = np.array([[0.25, -1.5, 3.0]])
    sp, sp2 = split_points()
    c = {
        "order_ties": [(order, _p2(rng, 7), 0)],
        "threshold_edge": [(z, _p2(rng, 1), 0), (np.array([[1e-6, 0, 0]]), _p2(rng, 1), 1),
                           (np.array([[0, np.nextafter(1e-6, 0), 0]]), _p2(rng, 1), 2)],
        "empty_tiny": [(one, _p2(rng, 1), 0), (np.empty((0, 3)), np.empty((0, 2), np.int64), 1),
                       (one.copy(), _p2(rng, 1), 2)],
        "contested": contested_case(),
        "sequence": sequence_case(),
        "split_whole": [(sp, sp2, 0)],
        "split_parts": [(sp[:100], sp2[:100], 0), (sp[100:], sp2[100:], 0)],
    }
    for k, R in enumerate(REG_SIZES):
        c[f"chunk_{R}"] = chunk_case(R, 100 + k)
    return c


# ---------------- Rodrigues, prepare_for_ba, total_reprojection_error ----------------

def rodrigues_to_matrix(r, dtype=np.float64):
    r = np.asarray(r, dtype).reshape(3)
    th = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if th < np.finfo(np.float64).eps:
        return np.eye(3, dtype=dtype)
    k = r / th
    c, s = np.cos(th), np.sin(th)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype)
    return c * np.eye(3, dtype=dtype) + (1 - c) * np.outer(k, k) + s * Kx


def rodrigues_to_vector(R, dtype=np.float64):
    """Axis from the antisymmetric part, angle from atan2(sin, cos); beyond pi / 2 the axis comes
    from the symmetric part (R_ii = c + (1 - c) k_i^2), its sign from what is left of the other."""
    R = np.asarray(R, dtype).reshape(3, 3)
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dtype) / 2
    s = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    th = np.arctan2(s, c)
    if c >= 0:
        return a.copy() if s == 0 else a * (th / s)
    k2 = np.maximum((np.diag(R) - c) / (1 - c), 0)
    i = int(np.argmax(k2))
    k = np.zeros(3, dtype)
    k[i] = np.sqrt(k2[i])
    if a[i] < 0:
        k[i] = -k[i]
    for j in range(3):
        if j != i:
            k[j] = (R[i, j] + R[j, i]) / 2 / ((1 - c) * k[i])
    return k / np.sqrt((k[0] * k[0] + k[1] * k[1]) + k[2] * k[2]) * th


def prepare_for_ba(point_indices, frame_indices, G, points_2D, global_poses, global_K):
    cams = np.array([np.hstack((np.asarray(p[0]).flatten(), np.asarray(p[1]).flatten())) for p in global_poses])
    return (len(set(np.asarray(frame_indices).tolist())), len(G), frame_indices, point_indices, np.array(points_2D),
            cams, np.array(G), np.array(global_K))


def reprojection_errors(num_points, camera_indices, point_indices, points_2D, camera_params, points_3D, K_list,
                        dtype=np.float64):
    """e_o = |pi(K (R X + t)) - obs| for the first num_points observations (Runner.py:316)."""
    cp = np.asarray(camera_params, dtype)
    X, K, obs = np.asarray(points_3D, dtype), np.asarray(K_list, dtype), np.asarray(points_2D, dtype)
    e = np.empty(num_points, dtype)
    for o in range(num_points):
        c, p = int(camera_indices[o]), int(point_indices[o])
        R = rodrigues_to_matrix(cp[c, :3], dtype)
        q = K[c] @ (R @ X[p] + cp[c, 3:6])
        d = q[:2] / q[2] - obs[o]
        e[o] = np.sqrt(d[0] * d[0] + d[1] * d[1])
    return e


def score_case(seed=41, n_cam=4, n_pts=300, M=900):
    rng = np.random.RandomState(seed)
    X = np.column_stack([rng.uniform(-2, 2, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4, 8, n_pts)])
    cp = np.column_stack([rng.uniform(-0.2, 0.2, size=(n_cam, 3)), rng.uniform(-0.5, 0.5, size=(n_cam, 3))])
    cp[1, :3] = 0.0  # the identity branch
    K = np.array([[[800.0 + 10 * c, 0, 480], [0, 805.0 + 10 * c, 270], [0, 0, 1]] for c in range(n_cam)])
    cam = rng.randint(n_cam, size=M).astype(np.int64)
    pt = np.concatenate([np.arange(n_pts), rng.randint(n_pts, size=M - n_pts)]).astype(np.int64)
    obs = np.empty((M, 2))
    for o in range(M):
        q = K[cam[o]] @ (rodrigues_to_matrix(cp[cam[o], :3]) @ X[pt[o]] + cp[cam[o], 3:6])
        obs[o] = q[:2] / q[2]
    obs = np.round(obs + rng.normal(0, 0.7, size=obs.shape))
    return cam, pt, obs, cp, X, K


def sequence_poses(n=4, seed=51):
    """(Rodrigues vector [3, 1], t [3]) per frame and K per frame, as perform collects them."""
    rng = np.random.RandomState(seed)
    poses = [(rng.uniform(-0.1, 0.1, size=(3, 1)), rng.uniform(-1, 1, size=3)) for _ in range(n)]
    Ks = [np.array([[800.0, 0, 480], [0, 800.0, 270], [0, 0, 1]]) for _ in range(n)]
    return poses, Ks
