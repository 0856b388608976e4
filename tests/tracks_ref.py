"""numpy restatement of the feature-track rules (include/sfmfeat.h sfm_build_tracks_dev,
sfm_triangulate_tracks_dev) and the cases the CPU and GPU tests share.

build_tracks: a plain union-find over the edges, then the definitions, word for word.
triangulate_tracks: np.linalg.svd of the stacked rows.  Nothing here reads the library."""
from __future__ import annotations

import functools

import numpy as np

STATS = ("n_tracks", "n_obs", "inconsistent", "short", "skipped_edges", "max_len")


def graph_edges(count, cap, pairs, matches, nmatch, keep=None):
    """-> (edges [E, 2] node ids, skipped): the edges of the definition, in input order."""
    count = np.clip(np.asarray(count, np.int64), 0, cap)
    nimg = len(count)
    edges, skipped = [], 0
    for p in range(len(pairs)):
        s0, s1 = int(pairs[p][0]), int(pairs[p][1])
        for m in range(min(max(int(nmatch[p]), 0), cap)):
            if keep is not None and keep[p][m] == 0:
                continue
            r0, r1 = int(matches[p][m][0]), int(matches[p][m][1])
            if not (0 <= s0 < nimg and 0 <= s1 < nimg) or s0 == s1 or not (0 <= r0 < count[s0]) \
                    or not (0 <= r1 < count[s1]):
                skipped += 1
                continue
            edges.append((s0 * cap + r0, s1 * cap + r1))
    return np.array(edges, np.int64).reshape(-1, 2), skipped


def component_labels(count, cap, edges):
    """label [nimg * cap]: the smallest node id of each node's component (its own id when it has no
    edge), -1 for rows at or beyond count.  Plain union-find."""
    count = np.clip(np.asarray(count, np.int64), 0, cap)
    N = len(count) * cap
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edges.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.full(N, -1, np.int64)
    for n in range(N):
        if n % cap < count[n // cap]:
            label[n] = find(n)   # (linking the larger root under the smaller: the root is the minimum)
    members = {}
    for n in np.nonzero(label >= 0)[0].tolist():
        members.setdefault(int(label[n]), []).append(n)
    for root, mem in members.items():
        assert root == min(mem)
    return label


def build_tracks(count, cap, pairs, matches, nmatch, keep=None, min_len=2):
    """-> dict(offsets [T + 1], obs_slot, obs_row [n_obs], node_track [nimg, cap], out_n [6], label)
    all int32 (label int64), as sfm_build_tracks_dev defines them."""
    nimg = len(count)
    edges, skipped = graph_edges(count, cap, pairs, matches, nmatch, keep)
    label = component_labels(count, cap, edges)
    members = {}
    for n in np.nonzero(label >= 0)[0].tolist():
        members.setdefault(int(label[n]), []).append(n)
    node_track = np.full(nimg * cap, -1, np.int32)
    offsets, obs = [0], []
    bad = short = longest = 0
    for root in sorted(members):
        mem = sorted(members[root])
        if len(mem) < 2:
            continue
        slots = [n // cap for n in mem]
        if len(set(slots)) != len(slots):
            node_track[mem] = -2
            bad += 1
        elif len(mem) < min_len:
            node_track[mem] = -3
            short += 1
        else:
            node_track[mem] = len(offsets) - 1
            obs += mem            # ascending id = ascending slot
            offsets.append(len(obs))
            longest = max(longest, len(mem))
    obs = np.array(obs, np.int64)
    return dict(offsets=np.array(offsets, np.int32), obs_slot=(obs // cap).astype(np.int32),
                obs_row=(obs % cap).astype(np.int32), node_track=node_track.reshape(nimg, cap),
                out_n=np.array([len(offsets) - 1, len(obs), bad, short, skipped, longest], np.int32), label=label)


def track_rows(offsets, obs_slot, obs_row, xy, P, cam_valid, t, dtype=np.float64):
    """The stacked rows of track t ([2 V, 4]) and V: x P[2] - P[0], y P[2] - P[1] per valid view."""
    P = np.asarray(P, dtype).reshape(-1, 3, 4)
    rows = []
    for o in range(int(offsets[t]), int(offsets[t + 1])):
        s, r = int(obs_slot[o]), int(obs_row[o])
        if s >= len(P) or (cam_valid is not None and not cam_valid[s]):
            continue
        x, y = dtype(xy[s, r, 0]), dtype(xy[s, r, 1])
        rows.append(x * P[s, 2] - P[s, 0])
        rows.append(y * P[s, 2] - P[s, 1])
    return np.array(rows, dtype).reshape(-1, 4), len(rows) // 2


def triangulate_tracks(offsets, obs_slot, obs_row, xy, P, cam_valid=None):
    """-> (X [T, 3] float64, views [T] int32): the right singular vector of the smallest singular
    value of each track's stacked rows over its fourth component; NaN below 2 valid views."""
    T = len(offsets) - 1
    X = np.full((T, 3), np.nan)
    views = np.zeros(T, np.int32)
    for t in range(T):
        A, v = track_rows(offsets, obs_slot, obs_row, xy, P, cam_valid, t)
        views[t] = v
        if v >= 2:
            h = np.linalg.svd(A)[2][-1]
            X[t] = h[:3] / h[3]
    return X, views


# ---------------- cases ----------------

def _pad(per_pair, cap, nmatch=None):
    """Lists of (r0, r1) per pair -> matches [P, cap, 2] int32 (zeros past each pair's list) and
    nmatch [P] (the lists' lengths, then the overrides of `nmatch`)."""
    P = len(per_pair)
    mm = np.full((max(P, 1), cap, 2), 0, np.int32)
    nm = np.zeros(max(P, 1), np.int32)
    for p, lst in enumerate(per_pair):
        assert len(lst) <= cap
        if lst:
            mm[p, :len(lst)] = np.array(lst, np.int32)
        nm[p] = len(lst)
    if nmatch is not None:
        for p, v in nmatch.items():
            nm[p] = v
    return mm, nm


def hand_case():
    """nimg = 4, cap = 8 (the issue's hand graph).  Rows 0: a 4-view chain, given with duplicate
    edges.  Rows 1-2: a component reaching rows 1 and 2 of slot 2 (inconsistent).  Rows 3: a
    3-node component that keep cuts into a 2-node one and an isolated node.  Row 7 of slot 1 is
    beyond its count (7): skipped.  A pair (3, 3): skipped.  A pair with nmatch -1 and one with 0,
    both with rows that would be edges.  Rows 4-6 stay isolated."""
    cap = 8
    count = np.array([8, 7, 8, 6], np.int32)
    pairs = np.array([[0, 1], [1, 2], [2, 3], [0, 2], [0, 3], [3, 3], [1, 3], [0, 1]], np.int32)
    per = [
        [(0, 0), (1, 1), (0, 0), (3, 3), (5, 7)],      # (0,1): chain, bad start, duplicate, keep-split, row >= count
        [(0, 0), (1, 1), (1, 2), (3, 3)],              # (1,2): chain; row 1 of slot 1 reaches rows 1 and 2 of slot 2
        [(0, 0)],                                      # (2,3): chain's end
        [(0, 0), (1, 1)],                              # (0,2): duplicates by another route
        [(4, 4), (5, 5)],                              # (0,3): nmatch 0 below: no edge
        [(2, 3)],                                      # (3,3): equal slots
        [(6, 5), (6, 4)],                              # (1,3): nmatch -1 below: no edge
        [(0, 0)],                                      # (0,1) again: a duplicate edge from a duplicate pair
    ]
    mm, nm = _pad(per, cap, {4: 0, 6: -1})
    keep = np.ones((len(per), cap), np.uint8)
    keep[1, 3] = 0                                      # cuts (1,3)-(2,3): {(0,3),(1,3)} stays, (2,3) isolated
    return dict(count=count, cap=cap, pairs=pairs, matches=mm, nmatch=nm, keep=keep)


def long_path_case(nimg=300, cap=4):
    """One chain through all slots, its pairs listed in descending order."""
    rng = np.random.default_rng(7)
    rows = rng.integers(0, cap, nimg)
    pairs = np.array([[s, s + 1] for s in range(nimg - 2, -1, -1)], np.int32)
    per = [[(int(rows[s]), int(rows[s + 1]))] for s in range(nimg - 2, -1, -1)]
    mm, nm = _pad(per, cap)
    return dict(count=np.full(nimg, cap, np.int32), cap=cap, pairs=pairs, matches=mm, nmatch=nm, keep=None)


def giant_case(nimg=64, cap=65):
    """Row 0 of every slot linked to every other's (one consistent track of nimg nodes, every edge
    on one root) and rows 1..cap-1 of all slots chained into one inconsistent component."""
    i, j = np.triu_indices(nimg, k=1)
    pairs = np.stack([i, j], 1).astype(np.int32)
    per = []
    for a, b in pairs.tolist():
        lst = [(0, 0)]
        if b == a + 1:      # row r of every slot in one chain ...
            lst += [(r, r) for r in range(1, cap)]
        elif (a, b) == (0, 2):  # ... and the chains of rows r and r + 1 joined in slot 2
            lst += [(r, r % (cap - 1) + 1) for r in range(1, cap)]
        per.append(lst)
    mm, nm = _pad(per, cap)
    return dict(count=np.full(nimg, cap, np.int32), cap=cap, pairs=pairs, matches=mm, nmatch=nm, keep=None)


def random_case(nimg, cap, seed, window=None, n_tracks=None, noise=0.15, with_keep=True):
    """Planted tracks plus noise edges.  Counts just below cap (one slot empty when nimg > 3); all
    pairs (or a window); each planted track visits 2..6 slots with a row of its own per slot and
    appears in a pair's matches with probability 0.7; noise matches take any row in [-1, cap],
    so some fall outside their table; matches are shuffled within a pair; one pair has nmatch -1
    and one 0 when there are enough of them; keep drops one match in ten."""
    rng = np.random.default_rng(seed)
    count = rng.integers(max(cap - 2, 0), cap + 1, nimg).astype(np.int32)
    if nimg > 3:
        count[rng.integers(0, nimg)] = 0
    i, j = np.triu_indices(nimg, k=1)
    if window is not None:
        sel = (j - i) <= window
        i, j = i[sel], j[sel]
    pairs = np.stack([i, j], 1).astype(np.int32)
    order = rng.permutation(len(pairs))
    pairs = pairs[order]
    swap = rng.random(len(pairs)) < 0.3     # some pairs listed (j, i)
    pairs[swap] = pairs[swap][:, ::-1]
    pidx = {(int(a), int(b)): p for p, (a, b) in enumerate(pairs.tolist())}
    per = [[] for _ in pairs]
    free = [list(rng.permutation(int(c))) for c in count]
    n_tracks = n_tracks if n_tracks is not None else max(2, (nimg * cap) // 6)
    for _ in range(n_tracks):
        L = int(rng.integers(2, min(nimg, 6) + 1))
        slots = sorted(rng.choice(nimg, L, replace=False).tolist())
        slots = [s for s in slots if free[s]]
        rows = {s: int(free[s].pop()) for s in slots}
        for a in slots:
            for b in slots:
                if a < b and rng.random() < 0.7:
                    if (a, b) in pidx:
                        per[pidx[(a, b)]].append((rows[a], rows[b]))
                    elif (b, a) in pidx:
                        per[pidx[(b, a)]].append((rows[b], rows[a]))
    for p, (a, b) in enumerate(pairs.tolist()):
        for _ in range(int(rng.binomial(cap, noise)) if cap > 1 else int(rng.random() < 0.5)):
            per[p].append((int(rng.integers(-1, cap + 1)), int(rng.integers(-1, cap + 1))))
        rng.shuffle(per[p])
        per[p] = per[p][:cap]
    special = {}
    if len(pairs) >= 4:
        special = {int(len(pairs) // 2): -1, int(len(pairs) // 3): 0}
    mm, nm = _pad(per, cap, special)
    keep = (rng.random((max(len(pairs), 1), cap)) >= 0.1).astype(np.uint8) if with_keep else None
    return dict(count=count, cap=cap, pairs=pairs, matches=mm, nmatch=nm, keep=keep)


RANDOM_SEED = 20           # tests/test_tracks_cpu.py asserts what this seed must contain
SIZE_CAPS = (1, 63, 64, 65, 257)
SIZE_NIMGS = (2, 3, 65)


def size_case(nimg, cap):
    """The size-edge cases: all pairs up to nimg = 3, a window of 2 at nimg = 65."""
    return random_case(nimg, cap, 1000 * nimg + cap, window=None if nimg <= 3 else 2,
                       n_tracks=max(2, min(nimg * cap // 6, 400)), noise=0.05)


def empty_cases():
    """P = 0, and a table whose counts are all zero (every edge skipped)."""
    c = random_case(3, 5, 3)
    none = dict(c, pairs=np.zeros((0, 2), np.int32), matches=np.zeros((1, 5, 2), np.int32),
                nmatch=np.zeros(1, np.int32), keep=None)
    zero = dict(c, count=np.zeros(3, np.int32))
    return {"no_pairs": none, "zero_counts": zero}


@functools.lru_cache(maxsize=None)
def case(name):
    """Every named case (built once per process; treat the arrays as read-only)."""
    if name == "hand":
        return hand_case()
    if name == "long_path":
        return long_path_case()
    if name == "giant":
        return giant_case()
    if name == "random":
        return random_case(12, 257, RANDOM_SEED, noise=0.01)
    if name in ("no_pairs", "zero_counts"):
        return empty_cases()[name]
    if name.startswith("size_"):
        _, nimg, cap = name.split("_")
        return size_case(int(nimg), int(cap))
    raise KeyError(name)


CASE_NAMES = ["hand", "long_path", "giant", "random", "no_pairs", "zero_counts"] + \
    [f"size_{n}_{c}" for n in SIZE_NIMGS for c in SIZE_CAPS]


@functools.lru_cache(maxsize=None)
def expected(name, min_len=2):
    c = case(name)
    return build_tracks(c["count"], c["cap"], c["pairs"], c["matches"], c["nmatch"], c["keep"], min_len)


def permuted(c, seed):
    """The same graph with the pairs permuted and the matches permuted within each pair."""
    rng = np.random.default_rng(seed)
    P, cap = len(c["pairs"]), c["cap"]
    order = rng.permutation(P)
    mm, nm = c["matches"][:P][order].copy(), c["nmatch"][:P][order].copy()
    keep = None if c["keep"] is None else c["keep"][:P][order].copy()
    for p in range(P):
        k = min(max(int(nm[p]), 0), cap)
        q = rng.permutation(k)
        mm[p, :k] = mm[p, :k][q]
        if keep is not None:
            keep[p, :k] = keep[p, :k][q]
    return dict(c, pairs=c["pairs"][order].copy(), matches=mm, nmatch=nm, keep=keep)


# ---------------- the planted scene of the triangulation tests ----------------

def planted_scene(n_cam=6, n_pts=200, seed=11, wrong=0.05):
    """6 cameras on an arc looking at 200 points, pixels rounded to integers; consecutive-plus-
    window-2 pairs matched from ground truth, 5 % of the matches pointed at a wrong row.  Every
    point is seen by a contiguous run of 2, 3 or all 6 cameras (a third each).
    -> dict(count, cap, xy [n_cam, cap, 2] int32, P [n_cam, 3, 4], K, Rt (Rodrigues-free R, t lists),
            Xw [n_pts, 3], pairs, matches, nmatch)."""
    rng = np.random.default_rng(seed)
    K = np.array([[900.0, 0, 640], [0, 900.0, 360], [0, 0, 1]])
    Xw = np.column_stack([rng.uniform(-2, 2, n_pts), rng.uniform(-1.2, 1.2, n_pts), rng.uniform(-1.0, 1.0, n_pts)])
    Ps, Rs, ts = [], [], []
    for c in range(n_cam):
        a = np.deg2rad(-25 + 10 * c)
        C = np.array([8 * np.sin(a), 0.3 * np.cos(3 * a), -8 * np.cos(a)])
        z = -C / np.linalg.norm(C)
        x = np.cross([0, 1.0, 0], z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        t = -R @ C
        Rs.append(R)
        ts.append(t)
        Ps.append(K @ np.column_stack([R, t]))
    P = np.array(Ps)
    cap = n_pts + 8
    xy = np.zeros((n_cam, cap, 2), np.int32)
    count = np.zeros(n_cam, np.int32)
    row_of = -np.ones((n_cam, n_pts), np.int64)
    span = []
    for j in range(n_pts):
        L = (2, 3, n_cam)[j % 3]
        lo = int(rng.integers(0, n_cam - L + 1))
        span.append((lo, lo + L))
    for c in range(n_cam):
        seen = [j for j in range(n_pts) if span[j][0] <= c < span[j][1]]
        seen = [seen[k] for k in rng.permutation(len(seen))]
        for r, j in enumerate(seen):
            q = P[c] @ np.append(Xw[j], 1.0)
            xy[c, r] = np.rint(q[:2] / q[2]).astype(np.int32)
            row_of[c, j] = r
        count[c] = len(seen)
    pairs, per = [], []
    for a in range(n_cam):
        for b in range(a + 1, min(a + 3, n_cam)):
            lst = []
            for j in range(n_pts):
                if row_of[a, j] >= 0 and row_of[b, j] >= 0:
                    rb = int(row_of[b, j])
                    if rng.random() < wrong:
                        rb = int(rng.integers(0, count[b]))
                    lst.append((int(row_of[a, j]), rb))
            pairs.append((a, b))
            per.append(lst)
    mm, nm = _pad(per, cap)
    return dict(count=count, cap=cap, xy=xy, P=P, K=K, R=np.array(Rs), t=np.array(ts), Xw=Xw,
                pairs=np.array(pairs, np.int32), matches=mm, nmatch=nm, keep=None)
