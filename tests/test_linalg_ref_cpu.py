"""CPU: the references of tests/linalg_ref.py by themselves, because every bound that
tests/test_gpu_linalg.py holds the device helpers to comes from here (LR.RECORDED).  Each figure
is printed before its assertion and must lie between a quarter of its record and twice it: a
record cannot be inflated to widen a device bound, and another host's libm may move it a little.
Measured on the development host (x86-64, 80-bit long double):
  rodrigues, float64 restatement against longdouble, |R - R_ld|: 5.340e-16 (750 vectors up to pi),
    3.897e-15 (180 non-principal vectors up to 40 rad, where |r| itself carries ulp(40) / 2)
  rodrigues_inv, |r - r_ld| (either sign within 1e-6 of pi) and |R_ld(r) - R|: table (750 matrices,
    334 with c < 0) 5.876e-16 / 7.051e-16, exact half turns and identity 1.225e-16 / 1.225e-16,
    1e-15 noise (108 matrices) 5.840e-16 / 4.311e-15; no angle of the table stands out
  np.linalg.eigh on the symmetric table (40 matrices): residual 6.060e-16, |V^T V - I| 7.510e-16;
    the Jacobi restatement 1.182e-15 / 1.290e-15, its eigenvalues 9.745e-16 of |S| from eigh's, five
    sweeps at most
  np.linalg.svd on the 4 x 4 table (17 matrices): (|A v| - sigma_4) / |A|_F 1.998e-16, sigma_4 from
    the longdouble Jacobi (5.6e-17 of |A|_F from svd's own); the Jacobi restatement 1.536e-16
The restatements of the two Jacobi helpers are held here to the bounds the device gets, so a
fault in a restatement, or a bound that the algorithm cannot meet, shows without a GPU."""
from __future__ import annotations

import math

import numpy as np
import pytest

from sfmfromscratch_amd import pose
from tests import linalg_ref as LR
from tests.test_gpu_triangulate_tracks import X_TOL

EPS, LD = LR.EPS, LR.LD


def held(name, fig):
    rec = LR.RECORDED[name]
    print(f"MEASURED {name}: {fig:.3e} (recorded {rec:.3e})")
    assert rec / 4 <= fig <= 2 * rec, name


def test_longdouble_is_wider_than_float64():
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_tables_hold_what_they_promise():
    th, ax = LR.angles(), LR.axes()
    assert len(th) == 25 and len(LR.angles(False)) == 6 and len(ax) == 30
    assert th[1] < EPS == th[2] and th[-1] == np.pi and th[-2] < np.pi
    h = np.pi / 2
    assert (np.sort(th[14:17]) == [np.nextafter(h, 0), h, np.nextafter(h, 4)]).all()
    assert np.abs(np.sqrt((ax * ax).sum(1)) - 1).max() <= 2 * EPS
    # every `best` index of the symmetric branch wins somewhere, and two k2 entries tie
    R = LR.rotation_matrices()
    tab = R["table"]
    c = (tab[:, 0] + tab[:, 4] + tab[:, 8] - 1) / 2
    neg = tab[c < 0]
    k2 = np.maximum((neg[:, [0, 4, 8]] - c[c < 0, None]) / (1 - c[c < 0, None]), 0)
    assert set(np.argmax(k2, axis=1).tolist()) == {0, 1, 2}
    srt = np.sort(k2, axis=1)
    assert (srt[:, 2] == srt[:, 1]).any()
    print(f"rodrigues_inv table: {len(tab)} matrices, {(c < 0).sum()} with c < 0; exact {len(R['exact'])}, "
          f"noisy {len(R['noisy'])}")
    assert (c < 0).sum() >= 250
    ex = R["exact"]
    v = np.stack([ex[:, 7] - ex[:, 5], ex[:, 2] - ex[:, 6], ex[:, 3] - ex[:, 1]], 1)
    assert not v.any() and ((ex[:3, 0] + ex[:3, 4] + ex[:3, 8] - 1) / 2 == -1).all()
    S, names = LR.symmetric3()
    assert len(set(names)) == len(names) == len(S) and np.isnan(S[names.index("nan")]).any()
    assert np.abs(S[names.index("diag221_1e+150")]).max() == 2e150
    assert 0 < abs(S[names.index("tiny_offdiagonal")][0, 1]) < 1e-300
    lam = np.linalg.eigvalsh(S[names.index("essential")])
    assert abs(lam[0]) < 4 * EPS * lam[2] and abs(lam[2] - lam[1]) < 4 * EPS * lam[2]      # (s, s, 0)
    lam = np.linalg.eigvalsh(S[names.index("near_pair")])
    assert 0.5e-12 < lam[1] - lam[0] < 2e-12
    A, names4, rank = LR.matrices4()
    sv = np.array([np.linalg.svd(a, compute_uv=False) for a in A[rank >= 0]])
    r = rank[rank >= 0]
    assert (sv[r == 3, 3] < 1e-12 * sv[r == 3, 0]).all() and (sv[r == 3, 2] > 1e-9 * sv[r == 3, 0]).all()
    assert (sv[r == 2, 2] < 1e-12 * sv[r == 2, 0]).all() and (sv[r == 4, 3] > 1e-3 * sv[r == 4, 0]).all()
    assert any(n.endswith("triangular") for n in names4) and not np.tril(A[names4.index("dlt0_triangular")], -1).any()


@pytest.mark.parametrize("principal", [True, False])
def test_rodrigues_restatement_against_longdouble(principal):
    held("rodrigues_principal" if principal else "rodrigues_nonprincipal", LR.rodrigues_error(LR.rodrigues, principal))
    r, th, _ = LR.rotation_vectors(principal)
    R = LR.rodrigues(r)
    # no bad angle anywhere: each matrix is a rotation to rounding
    RtR = np.einsum("nab,nac->nbc", R.reshape(-1, 3, 3), R.reshape(-1, 3, 3))
    assert np.abs(RtR - np.eye(3)).max() <= 16 * EPS * (1 if principal else 40)
    if not principal:   # and a non-principal vector gives the matrix of its principal form
        d = float(np.abs(LR.rodrigues(LR.principal_form(r), LD) - LR.rodrigues(r, LD)).max())
        print(f"MEASURED principal form against the vector itself, longdouble: {d:.3e}")
        assert d <= 4 * EPS   # the principal form is rounded to float64 once: |r| <= pi, so half an ulp of pi
    # NaN or inf in gives NaN out
    for bad in (np.nan, np.inf, -np.inf):
        with np.errstate(all="ignore"):
            assert np.isnan(LR.rodrigues(np.array([[0.1, bad, 0.2]]))).all()


@pytest.mark.parametrize("table", ["table", "exact", "noisy"])
def test_rodrigues_inv_restatement_against_longdouble(table):
    R = LR.rotation_matrices()[table]
    far, near, back, rmax, neg = LR.rodrigues_inv_errors(LR.rodrigues_inv, R)
    print(f"MEASURED rodrigues_inv {table}: {len(R)} rows, {neg} with c < 0; |r - r_ld| {far:.3e}, within 1e-6 of pi "
          f"up to sign {near:.3e}; rebuilt {back:.3e}; max |r| - pi {rmax - np.pi:.3e}")
    held(f"inv_vector_{table}", max(far, near))
    held(f"inv_rebuilt_{table}", back)
    assert rmax <= np.pi + 1e-15
    # the host stand-in is the same formula
    host = np.array([pose.rodrigues(m.reshape(3, 3))[0].reshape(3) for m in R])
    assert host.tobytes() == LR.rodrigues_inv(R).tobytes()
    if table == "exact":
        assert LR.rodrigues_inv(R).tolist() == [[np.pi, 0, 0], [0, np.pi, 0], [0, 0, np.pi], [0, 0, 0]]
    bad = R[:1].copy()
    bad[0, 5] = np.nan
    assert np.isnan(LR.rodrigues_inv(bad)).all()


def test_compose_and_rotate_are_the_written_parenthesisation():
    rng = np.random.RandomState(3)
    E, R, x = rng.standard_normal((50, 9)), rng.standard_normal((50, 9)), rng.standard_normal((50, 3))
    C, Y = LR.compose3(E, R), LR.rotate3(R, x)
    for n in range(50):
        for r in range(3):
            assert Y[n, r] == (R[n, 3 * r] * x[n, 0] + R[n, 3 * r + 1] * x[n, 1]) + R[n, 3 * r + 2] * x[n, 2]
            for k in range(3):
                assert C[n, 3 * r + k] == (E[n, 3 * r] * R[n, k] + E[n, 3 * r + 1] * R[n, 3 + k]) + E[n, 3 * r + 2] * R[n, 6 + k]
    assert np.abs(C - (E.reshape(-1, 3, 3) @ R.reshape(-1, 3, 3)).reshape(-1, 9)).max() < 1e-14


def test_lapack_yardstick_and_the_jacobi_restatement_on_the_symmetric_table():
    S, names = LR.symmetric3()
    ok = [k for k in range(len(S)) if names[k] != "nan"]
    lam, V = np.zeros((len(S), 3)), np.zeros((len(S), 3, 3))
    for k in ok:
        lam[k], V[k] = np.linalg.eigh(S[k])
    res, orth = LR.eig_errors(lam, V, S, names)
    held("eigh_residual", res)
    held("eigh_orthogonality", orth)
    bound = LR.eig_bound(LR.RECORDED["eigh_residual"])
    jl, jV, rots = np.zeros_like(lam), np.zeros_like(V), []
    for k in range(len(S)):
        jl[k], jV[k], r = LR.jacobi_eig3(S[k])      # the NaN row returns too
        rots.append(r)
    jres, jorth = LR.eig_errors(jl, jV, S, names)
    worst = max(float(np.abs(np.sort(jl[k]) - lam[k]).max() / max(np.abs(S[k]).max(), 1e-300)) for k in ok)
    print(f"MEASURED jacobi restatement: residual {jres:.3e}, |V^T V - I| {jorth:.3e}, eigenvalues against eigh "
          f"{worst:.3e} (bound {bound:.3e}); rotations {min(rots)} to {max(rots)} of 48")
    assert jres <= bound and jorth <= bound and worst <= bound
    # five sweeps at most where the input is finite; the NaN row never meets the stopping rule and ends with the sweeps
    assert max(rots[k] for k in ok) <= 15 and rots[names.index("nan")] <= 48 and rots[names.index("zero")] == 0
    z = names.index("zero")
    assert not jl[z].any() and np.array_equal(jV[z], np.eye(3))
    for k in ok:   # the scaled rows are the unit rows scaled
        if "_1e" in names[k]:
            base, sc = names[k].split("_1e")
            u = names.index(base)
            assert np.isfinite(jl[k]).all() and np.isfinite(jV[k]).all()
            assert np.abs(np.sort(jl[k]) / float("1e" + sc) - np.sort(jl[u])).max() <= bound * max(np.abs(S[u]).max(), 1.0)


def test_lapack_yardstick_and_the_jacobi_restatement_on_the_4x4_table():
    A, names, rank = LR.matrices4()
    ok = [k for k in range(len(A)) if rank[k] >= 0]
    figs, jfigs, s4 = [], [], []
    for k in ok:
        _, s, Vt = np.linalg.svd(A[k])
        figs.append(LR.null_residual(A[k], Vt[3]))
        fro = np.sqrt((A[k] * A[k]).sum())
        s4.append(abs(float(LR.sigma4(A[k])) - s[3]) / (fro if fro > 0 else 1.0))
        v, _ = LR.null_vector_4x4(A[k])
        jfigs.append(LR.null_residual(A[k], v))
        assert abs(np.sqrt(v @ v) - 1) <= 16 * EPS
        if rank[k] == 3:
            d = min(np.abs(v - Vt[3]).max(), np.abs(v + Vt[3]).max())
            assert d <= X_TOL / (s[2] / s[0]), names[k]
    print("per row (svd, jacobi restatement): " + ", ".join(f"{names[k]} {a:.1e} {b:.1e}" for k, a, b in zip(ok, figs, jfigs)))
    print(f"MEASURED longdouble sigma_4 against svd's: {max(s4):.3e} of |A|_F")
    assert max(s4) <= 4 * EPS
    held("svd_residual", max(figs))
    bound = 8 * LR.RECORDED["svd_residual"]
    print(f"MEASURED jacobi restatement: (|A v| - sigma_4) / |A|_F {max(jfigs):.3e} (bound {bound:.3e})")
    assert max(jfigs) <= bound
    LR.null_vector_4x4(A[names.index("nan")])   # returns


@pytest.mark.parametrize("n", [64, 256])
def test_sum_restatements_are_order_sensitive(n):
    rows, names = LR.sum_rows(n)
    fn = (lambda r: LR.wave_sum(r)[0]) if n == 64 else LR.block_sum
    differs_fsum = differs_ltr = 0
    for row, name in zip(rows, names):
        got = fn(row)
        if name in ("inf", "nan"):
            assert (np.isinf(got) and got > 0) if name == "inf" else np.isnan(got)
            continue
        exact = math.fsum(row.tolist())
        ltr = LR.left_to_right(row)
        differs_fsum += np.float64(got).tobytes() != np.float64(exact).tobytes()
        differs_ltr += np.float64(got).tobytes() != np.float64(ltr).tobytes()
        wide = fn(row.astype(LD)) if n == 256 else LR.wave_sum(row, LD)[0]
        print(f"{name} [{n}]: restatement {got!r} fsum {exact!r} left to right {ltr!r} longdouble {float(wide)!r}")
        if n == 64:
            assert len(set(LR.wave_sum(row).tobytes()[8 * k:8 * k + 8] for k in range(64))) == 1   # every lane
    assert differs_fsum >= 1 and differs_ltr >= 1
    assert fn(rows[names.index("integers")]) == n * (n - 1) / 2
    sub = rows[names.index("subnormals")]
    assert (np.abs(sub) < 2.3e-308).all() and sub.any() and fn(sub) == math.fsum(sub.tolist())   # exact: no flushing


def test_rodrigues_inv_restatement_on_an_inf_is_not_always_nan():
    """What tests/test_gpu_linalg.py compares the device with entry by entry: a NaN anywhere gives
    NaN, but an inf need not.  +inf on the diagonal makes c = +inf and theta = atan2(s, inf) = 0 (a
    zero vector); an off-diagonal inf that the symmetric branch's chosen row does not hold leaves
    theta = pi / 2 about a finite axis.  k_ba_finish only sees the matrices of a finite state."""
    R = LR.rotation_matrices()["table"]
    pick = R[[7 * 25 + 9, 9 * 25 + 17, 12 * 25 + 18, 20 * 25 + 11]]   # theta = 0.5, 2, 3, pi / 2 + 1e-3
    rows, entry = np.arange(36), np.tile(np.arange(9), 4)
    diag = np.isin(entry, (0, 4, 8))
    for v, with_nan in ((np.inf, 18), (-np.inf, 30)):
        bad = np.repeat(pick, 9, axis=0)
        bad[rows, entry] = v
        out = LR.rodrigues_inv(bad)
        assert not np.isinf(out).any() and np.isnan(out).any(axis=1).sum() == with_nan
        if v > 0:
            assert not out[diag].any()
        else:
            assert np.isnan(out[diag]).all()
