"""Makes tests/golden/pnp.npz: the PnP cases of tests/pnp_ref.py (inputs and planted truth),
the numpy restatement's outputs for each (per-sample counts, winner, inliers, the pose before
and after the Levenberg-Marquardt refinement, costs, status, accepted steps, iterations run,
the marginal-comparison flags) and scipy's least_squares(method="lm", xtol = ftol = gtol =
1e-15) minimum from the same start over the same inliers; for the LM sizes also `pnp` (the DLT
over all points) with its own scipy minimum.  Nothing here comes from OpenCV or from the
reference project: the fixture holds data of this repository's restatement and of scipy only.

With --fits: tests/golden/pnp_fits.npz instead — rule 2 of DESIGN.md §13D in 60 digits (mpmath,
tests/pnp_ref.py hypotheses_mp / dlt_all_mp): the (R, t) of every sample of every sampled case,
its conditioning figures and admission flag, the all-points DLT's pose at the reduction edges,
the inputs of the degenerate scenes, and the device bounds that follow from the float64
routes' own deviation (tests/pnp_ref.py fit_bounds).  The arithmetic is mpmath's and the
container has constant timestamps: the same bytes every run.

usage: python tools/gen_golden_pnp.py [--fits] [--check]   (--check: compare with the committed file)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pnp_ref as PR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pnp.npz")
OUT_FITS = os.path.join(ROOT, "tests", "golden", "pnp_fits.npz")
REFINE_KEYS = ("R", "t", "cost0", "cost", "iters", "lm_iters", "status", "firm", "all_firm")


def build():
    out = {}
    for name, (X, x, planted, Rt, tt, K, iters) in PR.ransac_cases().items():
        p = f"{name}_"
        out.update({p + "X": X, p + "x": x, p + "planted": planted, p + "R_true": Rt, p + "t_true": tt, p + "K": K,
                    p + "iters": np.int32(iters), p + "thr": np.float64(PR.THRESHOLD)})
        r = PR.pnp_ransac(X, x, K, iters)
        out.update({p + "found": np.bool_(r["found"]), p + "iteration": np.int32(r["iteration"]),
                    p + "counts": r["counts"], p + "inliers": r["inliers"]})
        line = f"{name}: n {len(X)} iters {iters} found {r['found']}"
        if r["found"]:
            out.update({p + "R0": r["R0"], p + "t0": r["t0"]})
            out.update({p + "rest_" + k: np.asarray(r[k]) for k in REFINE_KEYS})
            inl = r["inliers"]
            line += (f" winner {r['iteration']} inliers {len(inl)} status {r['status']} accepted {r['iters']} "
                     f"(firm {r['firm']}) cost {r['cost0']:.4f} -> {r['cost']:.6f}")
            if len(inl) >= 6:  # scipy's lm needs as many residuals as unknowns
                Rs, ts, cs = PR.scipy_minimum(X[inl], x[inl], K, r["R0"], r["t0"])
                out.update({p + "sp_R": Rs, p + "sp_t": ts, p + "sp_cost": np.float64(cs)})
                line += f"; scipy cost {cs:.6f} (restatement excess {(r['cost'] - cs) / cs:.2e})"
        print(line, flush=True)
    for name in PR.LM_CASES:
        X, x, planted, Rt, tt, K, iters = PR.ransac_cases()[name]
        r = PR.pnp(X, x, K)
        p = f"{name}_pnp_"
        out.update({p + "R0": r["R0"], p + "t0": r["t0"]})
        out.update({p + "rest_" + k: np.asarray(r[k]) for k in REFINE_KEYS})
        Rs, ts, cs = PR.scipy_minimum(X, x, K, r["R0"], r["t0"])
        out.update({p + "sp_R": Rs, p + "sp_t": ts, p + "sp_cost": np.float64(cs)})
        print(f"pnp {name}: status {r['status']} accepted {r['iters']} cost {r['cost0']:.4f} -> {r['cost']:.6f}; "
              f"scipy {cs:.6f} (restatement excess {(r['cost'] - cs) / cs:.2e})", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--fits", action="store_true")
    args = ap.parse_args()
    if args.fits:
        data = PR.fixture_bytes(PR.fixture_arrays(progress=lambda line: print(line, flush=True)))
        if args.check:
            same = open(OUT_FITS, "rb").read() == data
            print("pnp_fits.npz:", "the same bytes" if same else "differs")
            sys.exit(0 if same else 1)
        with open(OUT_FITS, "wb") as f:
            f.write(data)
        print(f"wrote {OUT_FITS}: {len(data)} bytes")
        return
    out = build()
    if args.check:
        z = np.load(OUT, allow_pickle=False)
        bad = [k for k in out if k not in z.files or not np.array_equal(np.asarray(out[k]), z[k], equal_nan=True)]
        print("differs:", bad if bad else "nothing")
        sys.exit(1 if bad else 0)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
