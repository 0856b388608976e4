#!/usr/bin/env python3
"""Generate tests/golden/structure.npz: the REFERENCE's own CameraPose.triangulate_point,
CameraPose.non_linear_triangulation (SFM.py) and Util.print_reprojection_error (Util.py,
stdout captured) on the refine cases of tests/structure_ref.py, next to the restatement's
outputs (X, cost, iters, status and its marginal-comparison bookkeeping) from the same
linear points.

The link step (Runner.py:241-250) is inline code in SFMRunner.perform and cannot be called:
its fixtures are the restatement's outputs (tests/structure_ref.py `link_results`, numpy's own
norm / argmin / < on the same arrays).

Like tools/gen_golden_pose.py this runs only where the reference checkout is present
(SFM_REFERENCE, by default a `reference` directory beside the repository); its cv2 import is
served by oracle/cv2_standin.py.

    PYTHONDONTWRITEBYTECODE=1 SFM_REFERENCE=<checkout> python tools/gen_golden_structure.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SFM_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
OUT = os.path.join(ROOT, "tests", "golden")

sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
from oracle import cv2_standin  # noqa: E402
from tests import structure_ref as SR  # noqa: E402

sys.modules["cv2"] = cv2_standin
sys.path.insert(0, REF)
from SFM import CameraPose  # noqa: E402
from Util import print_reprojection_error  # noqa: E402


def main():
    cases = SR.refine_cases()
    out = {"names": np.array(list(cases.keys()))}
    for name, (p1, p2, P1, P2) in cases.items():
        X0 = np.array([CameraPose.triangulate_point(a, b, P1, P2) for a, b in zip(p1, p2)])[:, :3]
        t0 = time.time()
        Xr = CameraPose.non_linear_triangulation(X0.copy(), p1, p2, P1, P2)
        dt = time.time() - t0
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            print_reprojection_error(Xr, p1, p2, P1, P2)
        r = SR.refine(X0, p1, p2, P1, P2)
        pre = name + "_"
        out[pre + "p1"], out[pre + "p2"], out[pre + "P1"], out[pre + "P2"] = p1, p2, P1, P2
        out[pre + "X0"], out[pre + "Xref"] = X0, Xr
        out[pre + "line"] = np.array(buf.getvalue().strip())
        for k, v in r.items():
            out[pre + "rest_" + k] = v
        rel = np.linalg.norm(Xr - r["X"], axis=1) / np.linalg.norm(r["X"], axis=1)
        print(f"  {name}: n={len(p1)} reference {dt:.2f} s; '{buf.getvalue().strip()}'; restatement vs reference "
              f"max rel {rel.max():.3e}; accepted steps <= {r['iters'].max()}; "
              f"{int(r['all_firm'].sum())} points without a marginal comparison")
    links = SR.link_cases()
    out["link_names"] = np.array(list(links.keys()))
    for name, (tgt, p3d, qry, nxt, thr) in links.items():
        rp, rn, ti, qi = SR.link_results(tgt, p3d, qry, nxt, thr)
        pre = "link_" + name + "_"
        out[pre + "tgt"], out[pre + "p3d"], out[pre + "qry"], out[pre + "nxt"] = tgt, p3d, qry, nxt
        out[pre + "thr"] = np.float64(thr)
        out[pre + "prev"], out[pre + "next"], out[pre + "ti"], out[pre + "qi"] = rp, rn, ti, qi
        print(f"  link {name}: m={len(tgt)} nq={len(qry)} threshold {thr} -> {len(ti)} kept")
    path = os.path.join(OUT, "structure.npz")
    np.savez_compressed(path, **out)
    print(f"wrote structure.npz ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
