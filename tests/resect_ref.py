"""TEST INFRASTRUCTURE ONLY — this repository's numpy restatement of the resection rule
(include/sfmfeat.h sfm_resect_tracks_dev) and of the reconstruction loop of
sequence.reconstruct, with the cases the CPU and GPU tests share.

The link list and the sampler (Python integers; a dense Fisher-Yates to hold it against) are
written here from the rule; the hypotheses (routes "elim" and "svd"), the errors, the inlier mask
and the refinement are tests/pnp_ref.py's, the tracks and their triangulation tests/tracks_ref.py's.
Nothing here reads the library.

Only tests/ and tools/bench_resect.py import this module."""
from __future__ import annotations

import functools

import numpy as np

from tests import pnp_ref as PR
from tests import tracks_ref as TR

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEED_XOR = 0x526573656374696F   # "Resectio"
SEED = 5
ITERS = 248                     # pose.calculate_num_ransac_iterations(0.98, 6, 0.5)
MIN_INLIERS = 12
THRESHOLDS = (8.0, 2.0, 0.5)
ITER_EDGES = (0, 1, 7, 8, 9, 63, 64, 65, 129, 248)
MARGIN = 1e-6                   # px: every decided error lies farther than this from the threshold


def mix64(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def slot_key(seed, s):
    return mix64(mix64((seed ^ SEED_XOR) & M64) + (s & 0xFFFFFFFF))


def draws(seed, s, it):
    key = slot_key(seed, s)
    return [mix64(key + (6 * it + k + 1) * G) >> 32 for k in range(6)]


def sample(seed, s, it, n):
    """The six link numbers of sample `it` of slot s with n links: the virtual Fisher-Yates."""
    moved = {}   # position -> value, the sparse part of the virtual arange(n)
    out = []
    for k, r in enumerate(draws(seed, s, it)):
        j = k + ((r * (n - k)) >> 32)
        vj, vk = moved.get(j, j), moved.get(k, k)
        out.append(vj)
        moved[j], moved[k] = vk, vj
    return out


def sample_dense(seed, s, it, n):
    """The same six steps on an actual arange(n)."""
    a = list(range(n))
    for k, r in enumerate(draws(seed, s, it)):
        j = k + ((r * (n - k)) >> 32)
        a[k], a[j] = a[j], a[k]
    return a[:6]


def samples(seed, s, n, iters):
    return np.array([sample(seed, s, it, n) for it in range(iters)], np.int64).reshape(-1, 6)


def links(tab, s):
    """-> (rows [n] ascending, X [n, 3], x [n, 2] float64) of slot s."""
    cap, T = tab["cap"], tab["n_tracks"]
    c = min(max(int(tab["count"][s]), 0), cap)
    nt = tab["node_track"][s, :c].astype(np.int64)
    ok = (nt >= 0) & (nt < T)
    fin = np.zeros(c, bool)
    fin[ok] = np.isfinite(tab["X"][nt[ok]]).all(axis=1)
    rows = np.flatnonzero(ok & fin)
    return rows, tab["X"][nt[rows]].reshape(-1, 3).astype(np.float64), tab["xy"][s, rows].astype(np.float64).reshape(-1, 2)


def k_ok(K):
    K = np.asarray(K, np.float64).reshape(9)
    return bool(np.isfinite(K).all() and K[3] == 0 and K[6] == 0 and K[7] == 0 and K[0] != 0 and K[4] != 0
                and K[8] != 0)


def slot_fits(tab, s, iters, seed=SEED, route="elim"):
    """-> (rows, X, x, idx [iters, 6], R [iters, 3, 3], t [iters, 3]) of an attempted slot."""
    rows, X, x = links(tab, s)
    idx = samples(seed, s, len(rows), iters)
    if iters:
        R, t = PR.hypotheses(X, x, tab["K"][s], idx, route)
    else:
        R, t = np.zeros((0, 3, 3)), np.zeros((0, 3))
    return rows, X, x, idx, R, t


def resect(tab, iters=ITERS, threshold=PR.THRESHOLD, min_inliers=MIN_INLIERS, seed=SEED, attempt=None,
           route="elim", max_iter=PR.MAX_ITER, refine=True):
    """The call, slot by slot -> dict(pose [nimg, 12], rstat [nimg, 8], rcost [nimg, 2],
    rkeep [nimg, cap], counts [nimg, iters], hyp [nimg, iters, 12], fit: {slot: pnp_ref.refine's
    dict}).  refine=False leaves the refinement out (pose = the winning hypothesis, rstat[5..7] and
    rcost unset): the integer outputs do not depend on it."""
    nimg, cap = len(tab["count"]), tab["cap"]
    pose = np.full((nimg, 12), np.nan)
    rstat = np.zeros((nimg, 8), np.int32)
    rcost = np.full((nimg, 2), np.nan)
    rkeep = np.zeros((nimg, cap), np.uint8)
    counts = np.zeros((nimg, iters), np.int32)
    hyp = np.full((nimg, iters, 12), np.nan)
    fit = {}
    for s in range(nimg):
        rows, X, x = links(tab, s)
        n = len(rows)
        go = (attempt is None or attempt[s] != 0) and n >= 6 and k_ok(tab["K"][s])
        if not go:
            rstat[s] = (-1, -1, 0, n, 0, -1, 0, 0)
            continue
        if iters == 0:
            rstat[s] = (0, -1, 0, n, 0, -1, 0, 0)
            continue
        K = tab["K"][s]
        R, t = PR.hypotheses(X, x, K, samples(seed, s, n, iters), route)
        mask = PR.inlier_mask(X, x, K, R, t, threshold)
        cnt = mask.sum(axis=1).astype(np.int32)
        counts[s] = cnt
        hyp[s, :, :9], hyp[s, :, 9:] = R.reshape(-1, 9), t
        best = int(np.argmax(cnt))   # the first maximum
        posed = cnt[best] > 0 and cnt[best] >= min_inliers
        rstat[s] = (cnt[best], best, iters, n, int(posed), -1, 0, 0)
        if not posed:
            continue
        inl = np.flatnonzero(mask[best])
        rkeep[s, rows[inl]] = 1
        if refine:
            f = PR.refine(X[inl], x[inl], K, R[best], t[best], max_iter)
            fit[s] = f
            pose[s, :9], pose[s, 9:] = f["R"].reshape(9), f["t"]
            rstat[s, 5:] = (f["status"], f["iters"], f["lm_iters"])
            rcost[s] = (f["cost0"], f["cost"])
        else:
            pose[s] = hyp[s, best]
    return dict(pose=pose, rstat=rstat, rcost=rcost, rkeep=rkeep, counts=counts, hyp=hyp, fit=fit)


# ---------------- the conditions a slot's scene must meet (tests/test_resect_cpu.py asserts them) ----------------

def system_figures(X, x, K, idx):
    """sigma_1 / sigma_11 of every sample's 11 x 12 system and cond M of its projection matrix, in
    float64 (numpy's SVD): the figures pnp_ref.admitted takes."""
    A, _, _ = PR.sample_systems(X[idx], PR.normalised_pixels(x, K)[idx])
    sv = np.linalg.svd(A, compute_uv=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        s111 = np.where(sv[:, 10] > 0, sv[:, 0] / sv[:, 10], PR.BIG)
    return s111, np.minimum(PR.elimination_cond_m(X, x, K, idx), PR.BIG)


def slot_margins(X, x, K, idx):
    """What the GPU test relies on for one slot's links and samples -> dict(same_masks, margin (px:
    the nearest decided error of an admitted sample to any of THRESHOLDS), left_out (share of
    samples outside pnp_ref.admitted), dR, dt (the two routes' largest difference on admitted
    samples), defect (the elimination route's largest |R R^T - I| on them))."""
    Re, te = PR.hypotheses(X, x, K, idx, "elim")
    Rs, ts = PR.hypotheses(X, x, K, idx, "svd")
    adm = PR.admitted(*system_figures(X, x, K, idx)) & np.isfinite(Re).all(axis=(1, 2))
    ee, ze = PR.errors(X, x, K, Re, te)
    same = all(np.array_equal(PR.inlier_mask(X, x, K, Re, te, thr), PR.inlier_mask(X, x, K, Rs, ts, thr))
               for thr in THRESHOLDS)
    with np.errstate(invalid="ignore"):
        dec = ee[adm][ze[adm] > 0]
        margin = min((float(np.abs(dec - thr).min()) for thr in THRESHOLDS), default=np.inf) if dec.size else np.inf
    dR, dt = (PR.pose_deviation(Re[adm], te[adm], Rs[adm], ts[adm]) if adm.any() else (np.zeros(1), np.zeros(1)))
    defect = float(PR.rotation_defect(Re[adm]).max()) if adm.any() else 0.0
    return dict(same_masks=same, margin=margin, left_out=float(1.0 - adm.mean()) if len(idx) else 0.0,
                dR=float(dR.max()), dt=float(dt.max()), defect=defect, admitted=adm)


def margins_ok(m):
    return m["same_masks"] and m["margin"] > MARGIN and m["left_out"] <= PR.MAX_LEFT_OUT


# ---------------- the cases ----------------

def slot_pose(s):
    """A pose of its own for every slot (the camera still sees pnp_ref.scene's box)."""
    return PR.rot(0.12 + 0.07 * s, -0.05 + 0.03 * (s % 4), 0.03 * (s % 3) - 0.03), \
        np.array([-1.0 + 0.3 * (s % 5), 0.05 * s - 0.2, 0.1 + 0.05 * (s % 3)])


FRACS = (0.0, 0.1, 0.2, 0.3, 0.4)


def build_table(name, sizes, cap, base_seed):
    """A slot table whose slot s has sizes[s] links from pnp_ref.scene (the first seed from
    base_seed + 10 s on that meets margins_ok at ITERS samples), scattered in ascending order among
    rows that are not links: node_track -1, -2, -3, node_track >= n_tracks, X rows with a NaN and
    with an inf, and rows at and beyond count that would be links otherwise.  One slot in three
    has K_SKEW.  -> dict(name, count, cap, xy, node_track, X, n_tracks, K, R, t (planted), seeds)."""
    nimg = len(sizes)
    rng = np.random.default_rng(base_seed)
    xy = rng.integers(0, 540, (nimg, cap, 2)).astype(np.int32)
    node_track = np.full((nimg, cap), -1, np.int32)
    count = np.zeros(nimg, np.int32)
    Xs, Ks, Rs, ts, seeds = [np.array([[np.nan, 1.0, 2.0], [0.5, np.inf, 8.0], [np.nan] * 3])], [], [], [], []
    T = 3
    for s, n in enumerate(sizes):
        K = PR.K_SKEW if s % 3 == 2 else PR.K_SCENE
        R, t = slot_pose(s)
        frac = FRACS[s % len(FRACS)] if n >= 12 else 0.0
        noise = 0.6 if n >= 12 else 0.0   # six or seven points leave the DLT no redundancy
        for seed in range(base_seed + 10 * s, base_seed + 10 * s + 10):
            X, x, _, _, _ = PR.scene(seed, n, frac, K=K, R=R, t=t, noise=noise)
            if n < 6 or margins_ok(slot_margins(X, x, K, samples(SEED, s, n, ITERS))):
                break
        else:
            raise AssertionError(f"{name}: no seed of slot {s} meets the margins")
        seeds.append(seed)
        decoys = min(cap - n - 4, 24 + s)
        c = n + decoys
        pos = np.sort(rng.choice(c, n, replace=False))
        node_track[s, pos] = T + np.arange(n)
        xy[s, pos] = x.astype(np.int32)
        other = np.setdiff1d(np.arange(c), pos)
        kinds = [-1, -2, -3, None, 0, 1, 2]   # None: beyond the table; 0, 1, 2: the NaN / inf rows of X
        for k, r in enumerate(other):
            v = kinds[k % len(kinds)]
            node_track[s, r] = (10 ** 6 + k) if v is None else v
        node_track[s, c:] = T + rng.integers(0, max(n, 1), cap - c)   # at and beyond count: not links
        count[s] = c
        Xs.append(X)
        T += n
        Ks.append(K), Rs.append(R), ts.append(t)
    X = np.concatenate(Xs)
    node_track[node_track >= 10 ** 6] = T + 5   # (>= n_tracks)
    return dict(name=name, count=count, cap=cap, xy=xy, node_track=node_track, X=X, n_tracks=T, K=np.array(Ks),
                R=np.array(Rs), t=np.array(ts), seeds=seeds, sizes=list(sizes))


SMALL_SIZES = (5, 6, 7, 12, 63, 64, 65, 255, 256, 257)
TABLES = {"small": (SMALL_SIZES, 320, 100), "big0": ((2559, 2560), 2700, 300), "big1": ((2561, 12), 2700, 400)}


@functools.lru_cache(maxsize=None)
def table(name):
    """Built once per process; treat the arrays as read-only."""
    sizes, cap, base = TABLES[name]
    return build_table(name, sizes, cap, base)


# (table, iterations, threshold): every size at every threshold.  The iteration edges are ITER_EDGES:
# prefixes of one stream, which tests/test_gpu_resect.py runs one by one on table "small" at 8 px
# against slices of the 248-sample restatement
CASES = [("small", 248, 8.0), ("small", 129, 2.0), ("small", 65, 0.5), ("big0", 64, 8.0), ("big0", 9, 0.5),
         ("big1", 63, 2.0)]


@functools.lru_cache(maxsize=None)
def expected(name, iters, threshold, refine=True):
    return resect(table(name), iters, threshold, refine=refine)


# ---------------- the reconstruction loop on tracks_ref.planted_scene() ----------------

def planted_tracks(seed=11):
    """tracks_ref.planted_scene(seed=seed) with its tracks -> (scene, tracks)."""
    sc = TR.planted_scene(seed=seed)
    return sc, TR.build_tracks(sc["count"], sc["cap"], sc["pairs"], sc["matches"], sc["nmatch"], sc["keep"], 2)


def relative_pose(sc, a, b):
    """(R, t) of slot b relative to slot a, |t| = 1: the planted seed pair."""
    R = sc["R"][b] @ sc["R"][a].T
    t = sc["t"][b] - R @ sc["t"][a]
    return R, t / np.linalg.norm(t)


def reconstruct(sc, tr, seed_pair, per_round=None, iters=ITERS, threshold=PR.THRESHOLD, min_inliers=MIN_INLIERS,
                seed=SEED):
    """The loop of sequence.reconstruct -> dict(rounds, posed, R, t, X, n_links (per round))."""
    a, b, R01, t01 = seed_pair
    nimg = len(sc["count"])
    K = np.broadcast_to(sc["K"], (nimg, 3, 3))
    R, t = np.full((nimg, 3, 3), np.nan), np.full((nimg, 3), np.nan)
    posed = np.zeros(nimg, bool)
    R[a], t[a], R[b], t[b] = np.eye(3), 0.0, R01, t01
    posed[[a, b]] = True
    rounds, n_links = [[a, b]], []

    def tri():
        P = np.where(posed[:, None, None], K @ np.concatenate([R, t[:, :, None]], axis=2), 0.0)
        return TR.triangulate_tracks(tr["offsets"], tr["obs_slot"], tr["obs_row"], sc["xy"], P, posed)[0]

    X = tri()
    while True:
        tab = dict(count=sc["count"], cap=sc["cap"], xy=sc["xy"], node_track=tr["node_track"], X=X,
                   n_tracks=len(X), K=K)
        e = resect(tab, iters, threshold, min_inliers, seed, attempt=(~posed).astype(np.uint8))
        n_links.append(e["rstat"][:, 3].copy())
        order = np.flatnonzero(e["rstat"][:, 4] != 0)
        order = order[np.argsort(-e["rstat"][order, 0].astype(np.int64), kind="stable")]
        if per_round is not None:
            order = order[:per_round]
        rounds.append([int(s) for s in order])
        if not len(order):
            break
        for s in order:
            R[s], t[s] = e["pose"][s, :9].reshape(3, 3), e["pose"][s, 9:]
        posed[order] = True
        X = tri()
    return dict(rounds=rounds, posed=posed, R=R, t=t, X=X, n_links=n_links)


def gauge_error(R, t, sc, a=0, b=1):
    """The poses against the planted ones in the gauge of slot a with |t_ab| = 1 -> (max |dR|, max |dt|)
    over the posed slots."""
    Ra, ta = sc["R"][a], sc["t"][a]
    scale = np.linalg.norm(relative_pose_unscaled(sc, a, b))
    dR = dt = 0.0
    for s in range(len(R)):
        if not np.isfinite(R[s]).all():
            continue
        Rw = sc["R"][s] @ Ra.T
        tw = (sc["t"][s] - Rw @ ta) / scale
        dR = max(dR, float(np.abs(R[s] - Rw).max()))
        dt = max(dt, float(np.linalg.norm(t[s] - tw)))
    return dR, dt


def relative_pose_unscaled(sc, a, b):
    R = sc["R"][b] @ sc["R"][a].T
    return sc["t"][b] - R @ sc["t"][a]


# ---------------- what the CPU test measured (tests/test_resect_cpu.py holds these to the measurement:
# not below it, not above twice it); the GPU test's bounds are 100 x (hypotheses, refinement) and
# 2 x (planted poses) these ----------------
# the two routes' largest mutual difference on admitted samples: measured 1.075e-10 (small, slot 7), 7.832e-11 (slot 6)
CPU_ROUTES_R, CPU_ROUTES_T = 1.3e-10, 9e-11
# the refinement's distance from scipy_minimum over CASES: measured 9.465e-7, 1.0034e-5 (big0 at 0.5 px, slot 1:
# 101 inliers, the refinement ends on lambda); 3e-10 to 2e-7 where it converges
CPU_SCIPY_R, CPU_SCIPY_T = 1.2e-6, 1.3e-5
# the loop's error against the planted poses of tracks_ref.planted_scene(): measured 6.497e-3, 4.130e-2
# (per_round=None; 5.504e-3, 3.719e-2 at per_round=1)
CPU_PLANTED_R, CPU_PLANTED_T = 7e-3, 4.5e-2
HYP_CAP = 1e-8


def hyp_bounds():
    return min(HYP_CAP, 100 * CPU_ROUTES_R), min(HYP_CAP, 100 * CPU_ROUTES_T)
