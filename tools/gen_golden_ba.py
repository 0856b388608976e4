#!/usr/bin/env python3
"""Makes tests/golden/ba.npz: the bundle-adjustment cases of tests/ba_ref.py (the scenes), the
numpy restatement's outputs for each at ftol = 1e-2 and ftol = 0 (cameras, points where a test
compares them, costs with the cost after every accepted step, status, accepted steps,
iterations run, rejected factorisations, the marginal-comparison flags) and, for the scenes
small enough, scipy's least_squares(method="trf", jac="3-point", ftol = xtol = gtol = 1e-15)
minimum over the same unknowns (Rodrigues vector, t, X of the rows that move) from the same
start.

For the scene REFERENCE_CASE it also records the REFERENCE's own
BundleAdjustment.sparse_bundle_adjustment result (SFM.py:405-464) with the scores
SFMRunner.total_reprojection_error prints before and after it (Runner.py:291-306).  Those are
obtained on the generating machine only, by importing the reference with oracle/cv2_standin.py
in place of cv2 (plus the Rodrigues closed form of tests/registry_ref.py, as
tools/gen_golden_registry.py does); without a reference checkout the committed values are kept.

    PYTHONDONTWRITEBYTECODE=1 SFM_REFERENCE=<checkout> python tools/gen_golden_ba.py [--check]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SFM_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
OUT = os.path.join(ROOT, "tests", "golden", "ba.npz")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

from tests import ba_ref as BR  # noqa: E402
from tests import registry_ref as RR  # noqa: E402

REFERENCE_CASE = "three_cams_free"
SCIPY_MAX_POINTS = 100
SCENE_KEYS = ("cam_idx", "pt_idx", "obs", "cams", "K", "X", "fixed")
REST_KEYS = ("cams", "cost0", "cost", "status", "iters", "lm_iters", "rejected", "costs", "firm", "all_firm")
REF_KEYS = ("ref_cams", "ref_X", "ref_score_before", "ref_score_after", "ref_cost_after", "ref_seconds")


def scipy_minimum(sc):
    """The tight-tolerance minimum of the cost over the rows that move -> cost."""
    from scipy.optimize import least_squares
    ca, pa = BR.active(sc)
    nc, npt = int(ca.sum()), int(pa.sum())

    def unpack(x):
        cams, X = sc["cams"].copy(), sc["X"].copy()
        cams[ca] = x[:6 * nc].reshape(nc, 6)
        X[pa] = x[6 * nc:].reshape(npt, 3)
        return cams, X

    def fun(x):
        cams, X = unpack(x)
        R = np.array([RR.rodrigues_to_matrix(cams[k, :3]) for k in range(sc["n_cam"])])
        r, _, _ = BR.linearise(sc, R, cams[:, 3:], X, jac=False)
        return r.reshape(-1)

    x0 = np.concatenate([sc["cams"][ca].reshape(-1), sc["X"][pa].reshape(-1)])
    res = least_squares(fun, x0, method="trf", jac="3-point", ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000)
    return float(2.0 * res.cost)


def reference_run(sc):
    """The reference's BundleAdjustment on the scene -> dict of REF_KEYS, or None without a checkout."""
    if not os.path.isdir(REF):
        return None
    from oracle import cv2_standin

    def _rodrigues(a):
        a = np.asarray(a, np.float64)
        if a.size == 3:
            return RR.rodrigues_to_matrix(a), None
        return RR.rodrigues_to_vector(a).reshape(3, 1), None

    cv2_standin.Rodrigues = _rodrigues
    sys.modules["cv2"] = cv2_standin
    sys.path.insert(0, REF)
    from Runner import SFMRunner
    from SFM import BundleAdjustment
    r = object.__new__(SFMRunner)
    args = (sc["n_pts"], sc["cam_idx"], sc["pt_idx"], sc["obs"])
    before = r.total_reprojection_error(*args, sc["cams"], sc["X"], sc["K"])
    ba = BundleAdjustment(sc["n_cam"], sc["n_pts"], sc["cam_idx"], sc["pt_idx"], sc["obs"], sc["cams"].copy(),
                          sc["X"].copy(), sc["K"])
    t0 = time.time()
    with contextlib.redirect_stdout(io.StringIO()):  # verbose=2
        cams, X = ba.sparse_bundle_adjustment()
    dt = time.time() - t0
    after = r.total_reprojection_error(*args, cams, X, sc["K"])
    return dict(ref_cams=cams, ref_X=X, ref_score_before=np.float64(before), ref_score_after=np.float64(after),
                ref_cost_after=np.float64(BR.cost_of(sc, cams, X)), ref_seconds=np.float64(dt))


def build():
    out = {}
    cases = BR.cases()
    out["names"] = np.array(list(cases.keys()))
    for name, sc in cases.items():
        p = name + "_"
        out[p + "n_cam"], out[p + "n_pts"] = np.int32(sc["n_cam"]), np.int32(sc["n_pts"])
        for k in SCENE_KEYS:
            out[p + k] = sc[k].astype(np.int32) if k in ("cam_idx", "pt_idx") else sc[k]
        line = f"{name}: n_cam {sc['n_cam']} n_pts {sc['n_pts']} M {len(sc['cam_idx'])}"
        for tag, ftol in (("f2", 1e-2), ("f0", 0.0)):
            r = BR.solve(sc, ftol=ftol)
            out.update({f"{p}{tag}_{k}": np.asarray(r[k]) for k in REST_KEYS})
            if int(sc["fixed"].sum()) >= 2 and sc["n_pts"] <= SCIPY_MAX_POINTS:  # no gauge freedom: points compared too
                out[f"{p}{tag}_X"] = r["X"]
            line += (f" | ftol {ftol:g}: {r['cost0']:.4f} -> {r['cost']:.8f} status {r['status']} accepted "
                     f"{r['iters']} (firm {r['firm']}{'' if r['all_firm'] else ', marginal'}) ran {r['lm_iters']}")
        if sc["n_pts"] <= SCIPY_MAX_POINTS:
            cs = scipy_minimum(sc)
            out[p + "sp_cost"] = np.float64(cs)
            c0 = float(out[p + "f0_cost"])
            line += f" | scipy {cs:.8f} (restatement excess {(c0 - cs) / max(cs, 1e-300):.2e})"
        print(line, flush=True)
    sc = cases[REFERENCE_CASE]
    ref = reference_run(sc)
    if ref is None and os.path.exists(OUT):
        z = np.load(OUT, allow_pickle=False)
        ref = {k: z[k] for k in REF_KEYS if k in z.files}
        print("no reference checkout: the committed reference values are kept")
    if ref:
        out.update(ref)
        out["ref_case"] = np.array(REFERENCE_CASE)
        print(f"reference on {REFERENCE_CASE}: score {float(ref['ref_score_before']):.6f} -> "
              f"{float(ref['ref_score_after']):.6f}, cost after {float(ref['ref_cost_after']):.8f} "
              f"(restatement at ftol 0: {float(out[REFERENCE_CASE + '_f0_cost']):.8f}), "
              f"{float(ref['ref_seconds']):.1f} s in scipy")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    out = build()
    if args.check:
        z = np.load(OUT, allow_pickle=False)
        same = lambda a, b: np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
        bad = [k for k in out if k != "ref_seconds" and (k not in z.files or not same(np.asarray(out[k]), z[k]))]
        print("differs:", bad if bad else "nothing")
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
