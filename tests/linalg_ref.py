"""TEST INFRASTRUCTURE ONLY — plain numpy forms of the float64 helpers the geometry kernels share
(csrc/linalg3.h, linalg4.h, f64_dev.h) and the edge inputs the probe
sfm_debug_geom (`_native.debug_geom`) is run on.  Every restatement takes a `dtype`, so the same
function runs in float64 and in np.longdouble (80-bit on the test hosts): the longdouble run is
the reference, the float64 run measures what rounding alone costs (tests/test_linalg_ref_cpu.py),
and the device is held to a multiple of that (tests/test_gpu_linalg.py).  Rodrigues comes from
tests/registry_ref.py: there is one copy.

Only tests/ imports this module."""
from __future__ import annotations

import numpy as np

from tests.registry_ref import rodrigues_to_matrix, rodrigues_to_vector

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
PI = float(np.pi)
SEED = 1307


# ---------------- restatements, one row at a time unless said otherwise ----------------

def rodrigues(r, dtype=np.float64):
    """rows r [n, 3] -> [n, 9]."""
    return np.array([rodrigues_to_matrix(v, dtype).reshape(9) for v in np.asarray(r, np.float64).reshape(-1, 3)], dtype)


def rodrigues_inv(R, dtype=np.float64):
    """rows R [n, 9] -> [n, 3]."""
    with np.errstate(all="ignore"):
        return np.array([rodrigues_to_vector(m, dtype).reshape(3) for m in np.asarray(R, np.float64).reshape(-1, 9)],
                        dtype)


def compose3(E, R, dtype=np.float64):
    """Rn = E R on rows [n, 9], each entry (E[3r] R[k] + E[3r + 1] R[3 + k]) + E[3r + 2] R[6 + k]."""
    E, R = np.asarray(E, dtype).reshape(-1, 9), np.asarray(R, dtype).reshape(-1, 9)
    out = np.empty_like(E)
    for r in range(3):
        for k in range(3):
            out[:, 3 * r + k] = (E[:, 3 * r] * R[:, k] + E[:, 3 * r + 1] * R[:, 3 + k]) + E[:, 3 * r + 2] * R[:, 6 + k]
    return out


def rotate3(R, x, dtype=np.float64):
    """Y = R x on rows, each entry (R[3r] x + R[3r + 1] y) + R[3r + 2] z."""
    R, x = np.asarray(R, dtype).reshape(-1, 9), np.asarray(x, dtype).reshape(-1, 3)
    return np.stack([(R[:, 3 * r] * x[:, 0] + R[:, 3 * r + 1] * x[:, 1]) + R[:, 3 * r + 2] * x[:, 2] for r in range(3)],
                    axis=1)


def wave_sum(row, dtype=np.float64):
    """The xor butterfly over 64 lanes, offsets 32 .. 1 -> each lane's own result [64]."""
    v = np.asarray(row, dtype).reshape(64).copy()
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[lane ^ off]
    return v


def block_sum(row, dtype=np.float64):
    """The halving tree over 256 slots: thread t adds slot t + off for off = 128 .. 1 -> the sum."""
    s = np.asarray(row, dtype).reshape(256).copy()
    with np.errstate(all="ignore"):
        for off in (128, 64, 32, 16, 8, 4, 2, 1):
            s[:off] = s[:off] + s[off:2 * off]
    return s[0]


def left_to_right(row):
    t = np.float64(0.0)
    for v in np.asarray(row, np.float64).reshape(-1):
        t = t + v
    return t


def jacobi_eig3(S, dtype=np.float64):
    """Cyclic Jacobi as linalg3.h runs it -> (diagonal [3], V [3, 3], rotations applied)."""
    S = np.array(S, dtype).reshape(3, 3)
    V = np.eye(3, dtype=dtype)
    one, rot = dtype(1.0), 0
    with np.errstate(all="ignore"):
        for _ in range(16):
            off = abs(S[0, 1]) + abs(S[0, 2]) + abs(S[1, 2])
            dia = abs(S[0, 0]) + abs(S[1, 1]) + abs(S[2, 2])
            if off <= dtype(1e-18) * dia:
                break
            for p in range(2):
                for q in range(p + 1, 3):
                    if abs(S[p, q]) < 1e-300:
                        continue
                    theta = (S[q, q] - S[p, p]) / (2 * S[p, q])
                    t = (one if theta >= 0 else -one) / (abs(theta) + np.sqrt(theta * theta + one))
                    c = one / np.sqrt(t * t + one)
                    s = t * c
                    S = _rot_sym(S, p, q, c, s)      # S = J^T S J: the columns, then the rows
                    V = _rot_cols(V, p, q, c, s)
                    rot += 1
    return np.array([S[0, 0], S[1, 1], S[2, 2]], dtype), V, rot


def _rot_cols(M, p, q, c, s):
    M = M.copy()
    mp, mq = M[:, p].copy(), M[:, q].copy()
    M[:, p], M[:, q] = c * mp - s * mq, s * mp + c * mq
    return M


def _rot_sym(S, p, q, c, s):
    S = _rot_cols(S, p, q, c, s)
    sp, sq = S[p, :].copy(), S[q, :].copy()
    S[p, :], S[q, :] = c * sp - s * sq, s * sp + c * sq
    return S


def null_vector_4x4(A, dtype=np.float64):
    """One-sided Jacobi as linalg4.h runs it -> (v [4], the rotated columns' squared norms [4]).
    (The helper's fmas are not restated: in longdouble the difference is below 1e-19.)"""
    A = np.array(A, dtype).reshape(4, 4)
    V = np.eye(4, dtype=dtype)
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        for _ in range(30):
            rotated = False
            for p in range(3):
                for q in range(p + 1, 4):
                    al, be, ga = A[:, p] @ A[:, p], A[:, q] @ A[:, q], A[:, p] @ A[:, q]
                    if not ga * ga > dtype(2.0) ** -104 * (al * be):
                        continue
                    rotated = True
                    zeta = (be - al) / (2 * ga)
                    t = (one if zeta >= 0 else -one) / (abs(zeta) + np.sqrt(zeta * zeta + one))
                    c = one / np.sqrt(t * t + one)
                    s = c * t
                    A, V = _rot_cols(A, p, q, c, s), _rot_cols(V, p, q, c, s)
            if not rotated:
                break
        nn = (A * A).sum(0)
    mi, mv = 0, nn[0]
    for c in range(1, 4):
        if nn[c] < mv:
            mv, mi = nn[c], c
    return V[:, mi].copy(), nn


def sigma4(A):
    """sigma_4(A) to longdouble accuracy: the smallest column norm the longdouble Jacobi ends with."""
    _, nn = null_vector_4x4(A, LD)
    return np.sqrt(nn.min())


# ---------------- residuals, evaluated in longdouble ----------------

def eig_residuals(S, lam, V):
    """(|S V - V diag(lam)|_max / |S|_max, |V^T V - I|_max) in longdouble; a zero S counts as scale 1."""
    S, lam, V = np.asarray(S, LD).reshape(3, 3), np.asarray(lam, LD).reshape(3), np.asarray(V, LD).reshape(3, 3)
    scale = np.abs(S).max()
    Sn = S / scale if scale > 0 else S      # the quotient first: 1e+-150 squared leaves the range of no type here
    r = np.abs(Sn @ V - V * (lam / scale if scale > 0 else lam)[None, :]).max()
    return float(r), float(np.abs(V.T @ V - np.eye(3, dtype=LD)).max())


def null_residual(A, v):
    """(|A v|_2 - sigma_4(A)) / |A|_F in longdouble; a zero A counts as |A|_F = 1."""
    A, v = np.asarray(A, LD).reshape(4, 4), np.asarray(v, LD).reshape(4)
    fro = np.sqrt((A * A).sum())
    Av = A @ v
    return float((np.sqrt(Av @ Av) - sigma4(A)) / (fro if fro > 0 else LD(1.0)))


# ---------------- input tables ----------------

def angles(principal=True):
    h = PI / 2
    a = [1e-17, np.nextafter(EPS, 0), EPS, 2.3e-16, 1e-12, 1e-9, 1e-8, 1e-5, 1e-3, 0.5,
         h - 1e-3, h + 1e-3, h - 1e-9, h + 1e-9, np.nextafter(h, 0), h, np.nextafter(h, 4), 2.0, 3.0,
         PI - 1e-3, PI - 1e-6, PI - 1e-9, PI - 1e-12, np.nextafter(PI, 0), PI]
    if not principal:
        a = [PI + 1e-3, 4.0, 2 * PI - 1e-9, 2 * PI, 2 * PI + 0.5, 40.0]
    return np.array(a, np.float64)


def axes():
    """The coordinate axes and their negatives, ties between two k2 entries ((1, 1, 0) / sqrt 2: the first
    maximum wins; (1, -1, 1) / sqrt 3: all three tie), a nearly pure y axis, (0.6, 0, -0.8), 20 random."""
    a = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 0], [1, -1, 1], [1e-8, 1, 0],
         [0.6, 0, -0.8]]
    rng = np.random.RandomState(SEED)
    a = np.concatenate([np.array(a, np.float64), rng.standard_normal((20, 3))])
    return a / np.sqrt((a * a).sum(1))[:, None]


def rotation_vectors(principal=True):
    """-> (r [n, 3], theta [n], axis [n, 3]): every axis at every angle, the angle varying fastest."""
    th, ax = angles(principal), axes()
    T, A = np.tile(th, len(ax)), np.repeat(ax, len(th), axis=0)
    return A * T[:, None], T, A


def principal_form(r):
    """The principal rotation vector of r, worked in longdouble and rounded once -> float64 [n, 3]."""
    r = np.asarray(r, LD).reshape(-1, 3)
    th = np.sqrt((r * r).sum(1))
    two_pi = 2 * np.arctan2(LD(0.0), LD(-1.0))
    thp = th - two_pi * np.round(th / two_pi)      # in [-pi, pi]: a negative angle turns the axis over
    return np.asarray(r / th[:, None] * thp[:, None], np.float64)


def rotation_matrices():
    """name -> rows [n, 9] for rodrigues_inv.
    table: the float64 matrices of the principal vectors; exact: the three half turns about the
    coordinate axes (s == 0 exactly and c < 0) and the identity; noisy: every seventh table matrix
    with 1e-15 noise on each entry, as a product of many compose3 steps carries."""
    r, _, _ = rotation_vectors(True)
    tab = rodrigues(r)
    exact = np.array([np.diag(d).reshape(9) for d in ([1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, 1])], np.float64)
    rng = np.random.RandomState(SEED + 1)
    noisy = tab[::7] + 1e-15 * rng.standard_normal(tab[::7].shape)
    return {"table": tab, "exact": exact, "noisy": noisy}


def _sym(rows):
    return np.array(rows, np.float64)


def symmetric3():
    """-> (S [n, 3, 3], names [n]).  The unit rows, the same scaled by 1e-150 and 1e+150, then the
    rows that stand alone (a sub-1e-300 off-diagonal entry, random ones, one NaN)."""
    rng = np.random.RandomState(SEED + 2)
    v = np.array([0.3, -0.5, 0.81])
    w = np.array([0.7, 0.1, -0.2])
    # an exact essential matrix [t]x R: its E^T E has the spectrum (|t|^2, |t|^2, 0)
    t = np.array([0.6, -0.3, 0.74])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ rodrigues_to_matrix(np.array([0.2, -0.4, 0.1]))
    Q = rodrigues_to_matrix(np.array([0.5, 0.3, -0.7]))
    unit = {"zero": np.zeros((3, 3)), "identity": np.eye(3), "diag221": np.diag([2.0, 2.0, 1.0]),
            "diag122": np.diag([1.0, 2.0, 2.0]), "rank1": np.outer(v, v), "rank2": np.outer(v, v) + np.outer(w, w),
            "essential": E.T @ E, "near_pair": Q @ np.diag([1.0, 1.0 + 1e-12, 3.0]) @ Q.T,
            "rotated221": Q @ np.diag([2.0, 2.0, 1.0]) @ Q.T}
    S, names = [], []
    for tag, sc in (("", 1.0), ("_1e-150", 1e-150), ("_1e+150", 1e150)):
        for k, m in unit.items():
            S.append((m + m.T) / 2 * sc)
            names.append(k + tag)
    tiny = np.diag([1.0, 2.0, 3.0])
    tiny[0, 1] = tiny[1, 0] = 1e-305
    tiny[1, 2] = tiny[2, 1] = 0.25
    S.append(tiny)
    names.append("tiny_offdiagonal")
    for k in range(12):
        B = rng.standard_normal((3, 3))
        S.append(B @ B.T if k % 2 == 0 else (B + B.T) / 2)
        names.append(("spd" if k % 2 == 0 else "indefinite") + str(k // 2))
    bad = np.eye(3)
    bad[0, 2] = bad[2, 0] = np.nan
    S.append(bad)
    names.append("nan")
    return np.array(S), names


def upper6(S):
    """[n, 3, 3] -> the probe's rows s00 s01 s02 s11 s12 s22."""
    S = np.asarray(S)
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)


def _camera(rng, ang):
    R = rodrigues_to_matrix(np.array([0.05, ang, -0.03]))
    K = np.array([[800.0, 0.0, 480.0], [0.0, 805.0, 270.0], [0.0, 0.0, 1.0]])
    return K @ np.hstack([R, rng.uniform(-0.5, 0.5, (3, 1)) + np.array([[0.0], [0.0], [6.0]])])


def _dlt(P1, P2, X):
    rows = []
    for P in (P1, P2):
        q = P @ np.append(X, 1.0)
        x, y = q[0] / q[2], q[1] / q[2]
        rows += [x * P[2] - P[0], y * P[2] - P[1]]
    return np.array(rows)


def matrices4():
    """-> (A [n, 4, 4], names [n], rank [n]): rank 3 where the null vector is determined (compared
    with numpy's), 2 for the two-dimensional null space, 4 / 0 / -1 (NaN) where only the call and
    the residual are looked at."""
    rng = np.random.RandomState(SEED + 3)
    A, names, rank = [], [], []

    def add(m, n, r):
        A.append(np.array(m, np.float64))
        names.append(n)
        rank.append(r)

    for k in range(6):
        P1, P2 = _camera(rng, -0.2), _camera(rng, 0.15 + 0.05 * k)
        X = rng.uniform(-1.0, 1.0, 3)
        D = _dlt(P1, P2, X)
        add(D, f"dlt{k}", 3)
        if k < 2:
            add(np.triu(np.linalg.qr(D)[1]), f"dlt{k}_triangular", 3)     # as tracks.hip hands over
            add(D * np.array([1.0, 1e3, 1e6, 1e-6]), f"dlt{k}_columns_scaled", 3)
    P1 = _camera(rng, 0.1)
    add(_dlt(P1, P1, np.array([0.2, -0.4, 0.3])), "same_camera", 2)
    Q = np.linalg.qr(rng.standard_normal((4, 4)))[0]
    add(Q, "orthogonal", 4)
    add(Q * np.array([4.0, 3.0, 2.0, 1.0]), "orthogonal_columns", 4)
    for k in range(3):
        add(np.triu(rng.standard_normal((4, 4))), f"triangular{k}", 4)
    add(np.zeros((4, 4)), "zero", 0)
    bad = rng.standard_normal((4, 4))
    bad[1, 2] = np.nan
    add(bad, "nan", -1)
    return np.array(A), names, np.array(rank)


def sum_rows(n):
    """-> (rows [m, n] float64, names [m]) for n = 64 (one wave) or 256 (one workgroup)."""
    rng = np.random.RandomState(SEED + n)
    rows, names = [], []

    def add(r, name):
        rows.append(np.asarray(r, np.float64))
        names.append(name)

    add(np.resize([1e16, 1.0, -1e16, 3.0, 1e-3, 2.0 ** 53, -7.0, 1e8], n), "mixed_magnitudes")
    add(np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * (1.0 + np.arange(n) * 2.0 ** -30) * 10.0 ** (np.arange(n) % 5),
        "alternating_signs")
    add(rng.randint(1, 1 << 20, n) * 5e-324 * np.where(rng.rand(n) < 0.5, -1.0, 1.0), "subnormals")
    add(np.where(np.arange(n) == n // 3, 1.0, 0.0) * 2.0 ** -1040 + rng.randint(0, 9, n) * 5e-324, "subnormal_and_tiny")
    add(rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n), "random")
    add(np.arange(n, dtype=np.float64), "integers")
    inf = rng.standard_normal(n)
    inf[n - 5] = np.inf
    add(inf, "inf")
    nan = rng.standard_normal(n)
    nan[7] = np.nan
    add(nan, "nan")
    return np.array(rows), names


# ---------------- measures shared by the CPU and the GPU tests ----------------

NEAR_PI = 1e-6   # closer to pi than this the sign of the vector is rounding: vectors are compared up to sign


def rodrigues_error(fn, principal=True):
    """max |fn(r) - R_ld(r)| over the table of vectors; fn: rows [n, 3] -> [n, 9]."""
    r, _, _ = rotation_vectors(principal)
    return float(np.abs(np.asarray(fn(r), LD) - rodrigues(r, LD)).max())


def rodrigues_inv_errors(fn, R):
    """fn: rows [n, 9] -> [n, 3], against the longdouble restatement on the same rows ->
    (max |r - r_ld| where pi - theta >= NEAR_PI, the same up to sign where it is nearer,
    max |R_ld(r) - R| over every row, max |r|, the number of rows with c < 0)."""
    got = np.asarray(fn(R), np.float64)
    ref = rodrigues_inv(R, LD)
    near = PI - np.sqrt((ref * ref).sum(1)).astype(np.float64) < NEAR_PI
    d = np.abs(got - ref).max(1)
    far_err = float(d[~near].max()) if (~near).any() else 0.0
    near_err = float(np.minimum(d, np.abs(got + ref).max(1))[near].max()) if near.any() else 0.0
    back = float(np.abs(rodrigues(got, LD) - np.asarray(R, LD)).max())
    c = (R[:, 0] + R[:, 4] + R[:, 8] - 1.0) / 2.0
    return far_err, near_err, back, float(np.sqrt((got * got).sum(1)).max()), int((c < 0).sum())


def eig_errors(lam, V, S, names):
    """The worst residual and the worst |V^T V - I| over the rows but the NaN one."""
    rs = [eig_residuals(S[k], lam[k], V[k]) for k in range(len(S)) if names[k] != "nan"]
    return max(r[0] for r in rs), max(r[1] for r in rs)


def rodrigues_bound(fig):
    """What the device's rodrigues / rodrigues_inv are held to: 8 x the float64 restatement's own
    error on the same table (the device's sin, cos, atan2 and sqrt need not round as the host's),
    with a floor of 16 eps."""
    return max(8.0 * fig, 16.0 * EPS)


def eig_bound(fig):
    """jacobi_eig3: 8 x LAPACK's residual on the same table, with a floor of 64 eps (up to 48 rotations)."""
    return max(8.0 * fig, 64.0 * EPS)


# The float64 restatements' and LAPACK's own figures on the tables above, as measured by
# tests/test_linalg_ref_cpu.py (which holds each to its measurement: not above twice the record,
# not below a quarter of it).  Every device bound of tests/test_gpu_linalg.py comes from these.
RECORDED = {
    "rodrigues_principal": 5.340e-16,       # |R - R_ld|, 750 vectors up to theta = pi
    "rodrigues_nonprincipal": 3.897e-15,    # the same, 180 vectors from pi + 1e-3 to 40 rad
    "inv_vector_table": 5.876e-16,          # |r - r_ld|, either sign within NEAR_PI of pi
    "inv_vector_exact": 1.225e-16,
    "inv_vector_noisy": 5.840e-16,
    "inv_rebuilt_table": 7.051e-16,         # |R_ld(r) - R|
    "inv_rebuilt_exact": 1.225e-16,
    "inv_rebuilt_noisy": 4.311e-15,
    "eigh_residual": 6.060e-16,             # np.linalg.eigh: |S V - V L|_max / |S|_max
    "eigh_orthogonality": 7.510e-16,        # |V^T V - I|_max
    "svd_residual": 1.998e-16,              # np.linalg.svd: (|A v|_2 - sigma_4) / |A|_F
}
