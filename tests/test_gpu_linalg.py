"""GPU: the float64 helpers the geometry kernels share (csrc/linalg3.h, linalg4.h, f64_dev.h;
DESIGN.md §13G), each run by itself through the probe sfm_debug_geom on the inputs of
tests/linalg_ref.py: rotations up to and beyond pi, both branches of rodrigues_inv, degenerate
and badly scaled spectra, sums whose order shows in the bits, non-finite input.  No stage reaches
these: the BA scenes of the fixture stay within 0.52 rad.

References and bounds (none comes from the device's own output; tests/test_linalg_ref_cpu.py pins
every recorded figure):
  bit-exact   compose3, rotate3 (numpy with the parenthesisation linalg3.h writes down), wave_sum_f64
              and block_sum256_tree (the butterfly and the halving tree restated), the identity
              branch of rodrigues, rodrigues_inv of the identity
  rodrigues, rodrigues_inv   against the longdouble restatement: 8 x the float64 restatement's own
              error on the same table, floor 16 eps (LR.rodrigues_bound)
  jacobi_eig3 residuals in longdouble: 8 x LAPACK's on the same table, floor 64 eps (LR.eig_bound)
  null_vector_4x4   | |v| - 1 | <= 16 eps; |A v| <= sigma_4 + 8 x svd's figure x |A|_F; rank 3: numpy's
              vector up to sign within test_gpu_triangulate_tracks.X_TOL / (sigma_3 / sigma_1)
Every figure is printed before its assertion.  Measured on the MI355X (figure / bound):
  rodrigues      750 vectors up to pi 5.745e-16 / 4.272e-15; 180 non-principal ones up to 40 rad
                 4.008e-15 / 3.118e-14, and 4.108e-15 from the device's matrix of their principal form
  rodrigues_inv  table: 750 matrices, 334 through the c < 0 branch: vectors 5.319e-16 / 4.701e-15
                 (within 1e-6 of pi, up to sign, 6.165e-16), rebuilt matrix 7.051e-16 / 5.641e-15,
                 max |r| - pi 4.4e-16, pose.rodrigues 2.220e-16; exact half turns (3 with c < 0) and
                 identity: 0 / 3.553e-15, rebuilt 1.225e-16; 1e-15 noise, 108 matrices, 50 with c < 0:
                 6.041e-16 / 4.672e-15, rebuilt 4.311e-15 / 3.449e-14
  jacobi_eig3    40 matrices: residual 1.182e-15, |V^T V - I| 1.290e-15, eigenvalues 1.364e-15 of |S|
                 from eigvalsh's / 1.421e-14 (LAPACK's own residual 6.060e-16)
  null_vector_4x4  17 matrices: | |v| - 1 | 4.441e-16 / 3.553e-15; (|A v| - sigma_4) / |A|_F
                 1.554e-16 / 1.598e-15 (svd's own 1.998e-16); rank 3 against numpy's vector, times
                 sigma_3 / sigma_1, 1.201e-16 / 1.568e-12
An inf in a matrix does not always reach rodrigues_inv's output as a NaN (see the test); a NaN does."""
from __future__ import annotations

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native, pose
from tests import linalg_ref as LR
from tests.test_gpu_triangulate_tracks import X_TOL

pytestmark = pytest.mark.gpu

EPS, LD = LR.EPS, LR.LD


def probe(op, rows):
    return _native.debug_geom(op, np.ascontiguousarray(rows, np.float64))


def dev_rodrigues(r):
    return probe(_abi.SFM_GEOM_RODRIGUES, r)


def dev_rodrigues_inv(R):
    return probe(_abi.SFM_GEOM_RODRIGUES_INV, R)


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


# ---------------- bit-exact ----------------

def test_compose_and_rotate_bits():
    rng = np.random.RandomState(LR.SEED + 10)
    tab = LR.rotation_matrices()["table"]
    n = 333                                       # more than one workgroup of 64, not a multiple of it
    E = np.concatenate([tab[rng.randint(len(tab), size=n - 40)], rng.standard_normal((40, 9)) * 10.0 ** rng.uniform(-6, 6, (40, 9))])
    R = np.concatenate([tab[rng.randint(len(tab), size=n - 40)], rng.standard_normal((40, 9)) * 10.0 ** rng.uniform(-6, 6, (40, 9))])
    x = rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 3))
    got = probe(_abi.SFM_GEOM_COMPOSE, np.hstack([E, R]))
    assert same_bits(got, LR.compose3(E, R))
    got = probe(_abi.SFM_GEOM_ROTATE, np.hstack([R, x]))
    assert same_bits(got, LR.rotate3(R, x))


def test_wave_sum_bits_in_every_lane():
    rows, names = LR.sum_rows(64)
    got = probe(_abi.SFM_GEOM_WAVE_SUM, rows)
    for k, name in enumerate(names):
        want = LR.wave_sum(rows[k])
        if name == "nan":
            assert np.isnan(got[k]).all() and np.isnan(want).all()
            continue
        assert same_bits(got[k], want), name                                  # each lane against its own restatement
        assert len({got[k, j].tobytes() for j in range(64)}) == 1, name       # and all 64 alike
        if name == "inf":
            assert np.isposinf(got[k]).all()


def test_two_block_sums_in_a_row_on_one_lds_array():
    rows, names = LR.sum_rows(256)
    m = len(rows)
    first = np.concatenate([rows, rows])
    second = np.concatenate([rows[(np.arange(m) + 3) % m], rows[(np.arange(m) + 5) % m]])   # never its own first half
    got = probe(_abi.SFM_GEOM_BLOCK_SUM, np.hstack([first, second]))
    assert got.shape == (2 * m, 512)
    for k in range(2 * m):
        for half, src in ((got[k, :256], first[k]), (got[k, 256:], second[k])):
            want = LR.block_sum(src)
            if np.isnan(want):
                assert np.isnan(half).all()
                continue
            # all 256 threads hold the restatement's bits: the second sum is the sum of its own inputs,
            # whatever the first left in the array (an inf, a NaN)
            assert same_bits(half, np.full(256, want)), (names[k % m], k)
    inf, nan = names.index("inf"), names.index("nan")
    assert np.isposinf(got[inf, :256]).all() and np.isfinite(got[inf, 256:]).all()
    assert np.isnan(got[nan, :256]).all() and np.isfinite(got[nan, 256:]).all()


def test_rodrigues_identity_switch_and_inverse_of_the_identity():
    eye = np.eye(3).reshape(9)
    ax = np.eye(3)
    below = np.concatenate([ax * 1e-17, ax * np.nextafter(EPS, 0), -ax * np.nextafter(EPS, 0), np.zeros((1, 3))])
    got = dev_rodrigues(below)
    assert all(same_bits(g, eye) for g in got)            # the exact identity, +0 off the diagonal
    at = dev_rodrigues(np.concatenate([ax * EPS, -ax * EPS]))     # !(th < eps): the first value past the switch
    for k in range(6):
        assert not same_bits(at[k], eye)
        a, sgn = k % 3, 1.0 if k < 3 else -1.0
        want = eye.copy()                                 # cos(eps) = 1, sin(eps) = eps, (1 - cos) = 0
        i, j = (a + 1) % 3, (a + 2) % 3
        want[3 * j + i], want[3 * i + j] = sgn * EPS, -sgn * EPS
        assert np.abs(at[k] - want).max() <= 2 * EPS * EPS, k     # sin(eps) to 2 ulp of eps
    assert same_bits(dev_rodrigues_inv(eye[None]), np.zeros((1, 3)))


# ---------------- rodrigues, rodrigues_inv against the longdouble restatement ----------------

@pytest.mark.parametrize("principal", [True, False])
def test_rodrigues_against_longdouble(principal):
    name = "rodrigues_principal" if principal else "rodrigues_nonprincipal"
    bound = LR.rodrigues_bound(LR.RECORDED[name])
    r, th, _ = LR.rotation_vectors(principal)
    err = LR.rodrigues_error(dev_rodrigues, principal)
    print(f"MEASURED {name}: {len(r)} vectors, theta {th.min():.3g} to {th.max():.6g}: |R - R_ld| {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    if not principal:   # the same matrix as the principal form of the vector
        d = float(np.abs(dev_rodrigues(r) - dev_rodrigues(LR.principal_form(r))).max())
        print(f"MEASURED {name}: against the device's matrix of the principal form {d:.3e} (bound {bound:.3e})")
        assert d <= bound


def test_rodrigues_of_non_finite_vectors_is_nan():
    bad = np.array([[0.1, np.nan, 0.2], [np.inf, 0.0, 0.0], [0.3, 0.1, -np.inf], [np.nan, np.nan, np.nan]])
    assert np.isnan(dev_rodrigues(bad)).all()
    with np.errstate(all="ignore"):
        assert np.isnan(LR.rodrigues(bad)).all()


@pytest.mark.parametrize("table", ["table", "exact", "noisy"])
def test_rodrigues_inv_against_longdouble(table):
    R = LR.rotation_matrices()[table]
    bv, bb = LR.rodrigues_bound(LR.RECORDED[f"inv_vector_{table}"]), LR.rodrigues_bound(LR.RECORDED[f"inv_rebuilt_{table}"])
    far, near, back, rmax, neg = LR.rodrigues_inv_errors(dev_rodrigues_inv, R)
    print(f"MEASURED rodrigues_inv {table}: {len(R)} rows, {neg} through the c < 0 branch: |r - r_ld| {far:.3e} where "
          f"pi - theta >= 1e-6 (bound {bv:.3e}; nearer pi, up to sign, {near:.3e}); matrix rebuilt in longdouble "
          f"{back:.3e} (bound {bb:.3e}); max |r| - pi {rmax - np.pi:.3e}")
    assert neg >= (3 if table == "exact" else 50)
    assert far <= bv and back <= bb
    assert rmax <= np.pi + 1e-15
    # and the host stand-in pose.rodrigues, by the same measure
    host = np.array([pose.rodrigues(m.reshape(3, 3))[0].reshape(3) for m in R])
    got = dev_rodrigues_inv(R)
    near_pi = np.pi - np.sqrt((host * host).sum(1)) < LR.NEAR_PI
    d = np.abs(got - host).max(1)
    d_far = float(d[~near_pi].max())
    d_near = float(np.minimum(d, np.abs(got + host).max(1))[near_pi].max()) if near_pi.any() else 0.0
    print(f"MEASURED rodrigues_inv {table}: against pose.rodrigues {d_far:.3e} (nearer pi, up to sign, {d_near:.3e})")
    assert d_far <= bv


def test_rodrigues_inv_of_nan_is_nan_and_inf_goes_as_the_restatement():
    R = LR.rotation_matrices()["table"]
    pick = R[[7 * 25 + 9, 9 * 25 + 17, 12 * 25 + 18, 20 * 25 + 11]]   # theta = 0.5, 2, 3, pi / 2 + 1e-3: both branches
    c = (pick[:, 0] + pick[:, 4] + pick[:, 8] - 1) / 2
    assert (c < 0).any() and (c >= 0).any()
    bad = np.repeat(pick, 9, axis=0)
    bad[np.arange(36), np.tile(np.arange(9), 4)] = np.nan     # a NaN in each entry in turn
    assert np.isnan(dev_rodrigues_inv(bad)).all() and np.isnan(LR.rodrigues_inv(bad)).all()
    # an inf in each entry in turn: NaN exactly where the restatement gives NaN, and its values elsewhere.
    # An inf does not always end as a NaN, in either: +inf on the diagonal makes c = +inf and theta =
    # atan2(s, inf) = 0, so the vector is zero; an off-diagonal inf that the chosen row of the symmetric
    # part does not hold leaves theta = pi / 2 about a finite axis (tests/test_linalg_ref_cpu.py pins this).
    # k_ba_finish only sees matrices of a state whose cost was finite.
    for v in (np.inf, -np.inf):
        bad = np.repeat(pick, 9, axis=0)
        bad[np.arange(36), np.tile(np.arange(9), 4)] = v
        got, want = dev_rodrigues_inv(bad), LR.rodrigues_inv(bad)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
        fin = np.isfinite(want)
        assert np.abs(got - want)[fin].max() <= LR.rodrigues_bound(LR.RECORDED["inv_vector_table"])


# ---------------- jacobi_eig3 ----------------

def test_jacobi_eig3_on_degenerate_and_scaled_spectra():
    S, names = LR.symmetric3()
    out = probe(_abi.SFM_GEOM_EIG3, LR.upper6(S))
    lam, V = out[:, :3], out[:, 3:].reshape(-1, 3, 3)
    bound = LR.eig_bound(LR.RECORDED["eigh_residual"])
    res, orth = LR.eig_errors(lam, V, S, names)
    ok = [k for k in range(len(S)) if names[k] != "nan"]
    worst = max(float(np.abs(np.sort(lam[k]) - np.linalg.eigvalsh(S[k])).max() / max(np.abs(S[k]).max(), 1e-300)) for k in ok)
    print(f"MEASURED jacobi_eig3: {len(ok)} matrices: |S V - V L| / |S| {res:.3e}, |V^T V - I| {orth:.3e}, eigenvalues "
          f"against eigvalsh {worst:.3e} of |S| (bound {bound:.3e}; LAPACK's own {LR.RECORDED['eigh_residual']:.3e}, "
          f"{LR.RECORDED['eigh_orthogonality']:.3e})")
    assert np.isfinite(out[ok]).all()
    assert res <= bound and orth <= LR.eig_bound(LR.RECORDED["eigh_orthogonality"]) and worst <= bound
    z = names.index("zero")
    assert same_bits(lam[z], np.zeros(3)) and same_bits(V[z], np.eye(3))
    for k in ok:   # the 1e+-150 rows are the unit rows scaled: nothing overflows in theta * theta
        if "_1e" in names[k]:
            base, sc = names[k].split("_1e")
            u = names.index(base)
            d = float(np.abs(np.sort(lam[k]) / float("1e" + sc) - np.sort(lam[u])).max())
            assert d <= bound * max(np.abs(S[u]).max(), 1.0), names[k]
    # the NaN row came back with the others: the sweeps end


# ---------------- null_vector_4x4 ----------------

def test_null_vector_4x4_on_rank_deficient_and_scaled_matrices():
    A, names, rank = LR.matrices4()
    v = probe(_abi.SFM_GEOM_NULL4, A.reshape(-1, 16))
    ok = [k for k in range(len(A)) if rank[k] >= 0]      # but the NaN row, which only has to return
    norm = max(abs(float(np.sqrt((v[k].astype(LD) ** 2).sum())) - 1.0) for k in ok)
    figs = [LR.null_residual(A[k], v[k]) for k in ok]
    bound = 8 * LR.RECORDED["svd_residual"]
    print(f"MEASURED null_vector_4x4: {len(ok)} matrices: | |v| - 1 | {norm:.3e} (bound {16 * EPS:.3e}); "
          f"(|A v| - sigma_4) / |A|_F {max(figs):.3e} (bound {bound:.3e}; svd's own {LR.RECORDED['svd_residual']:.3e})")
    assert np.isfinite(v[ok]).all()
    assert norm <= 16 * EPS
    assert max(figs) <= bound
    worst = 0.0
    for k in ok:
        if rank[k] == 3:
            _, s, Vt = np.linalg.svd(A[k])
            d = min(np.abs(v[k] - Vt[3]).max(), np.abs(v[k] + Vt[3]).max()) * (s[2] / s[0])
            worst = max(worst, float(d))
    print(f"MEASURED null_vector_4x4: rank 3 against numpy's vector, times sigma_3 / sigma_1: {worst:.3e} (bound {X_TOL:.3e})")
    assert worst <= X_TOL
    assert same_bits(v[names.index("zero")], [1.0, 0.0, 0.0, 0.0])     # nothing to rotate: the first column
