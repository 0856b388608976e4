#!/usr/bin/env python3
"""Generate tests/golden/pose.npz by running the REFERENCE's own CameraPose.ransac_camera_motion,
triangulate_point and triangulate_points (SFM.py) on the cases of tests/pose_ref.py.

Like tools/gen_golden.py this runs only where the reference checkout is present; its cv2
import is served by oracle/cv2_standin.py.  Per case the fixture holds the inputs, the
reference's R, t and inliers, and — after the restatement (tests/pose_ref.py) has reproduced
those outputs — the restatement's winning iteration and per-iteration (count, valid) table,
which the reference does not expose.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_pose.py
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("SFM_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
from oracle import cv2_standin  # noqa: E402
from tests import pose_ref as PR  # noqa: E402

sys.modules["cv2"] = cv2_standin
sys.path.insert(0, REF)
from SFM import CameraPose  # noqa: E402


def main():
    out = {"names": np.array(list(PR.cases().keys()))}
    for name, (p1, p2, K1, K2, Rb, Tb, thr, iters) in PR.cases().items():
        t0 = time.time()
        R, t, in1, in2 = CameraPose(p1, p2, K1, K2).ransac_camera_motion(Rb, Tb, threshold=thr, max_iterations=iters)
        dt = time.time() - t0
        r = PR.ransac_camera_motion(p1, p2, K1, K2, Rb, Tb, thr, iters)
        pre = name + "_"
        out[pre + "p1"], out[pre + "p2"] = p1, p2
        out[pre + "K1"], out[pre + "K2"], out[pre + "Rb"], out[pre + "Tb"] = K1, K2, Rb, Tb
        out[pre + "thr"], out[pre + "iters"] = np.float64(thr), np.int64(iters)
        if in1 is None:
            assert r[:4] == (None, None, None, None)
            out[pre + "state"] = np.array("none")
            print(f"  {name}: n={len(p1)} -> four Nones")
            continue
        tab = r[5]
        out[pre + "counts"], out[pre + "valid"] = tab["counts"].astype(np.int32), tab["valid"]
        out[pre + "win"] = np.int64(r[4])
        if R is None:
            assert r[0] is None and len(in1) == 0 and len(r[2]) == 0
            out[pre + "state"] = np.array("empty")
            print(f"  {name}: n={len(p1)} iters={iters} -> no pose ({dt:.1f} s)")
            continue
        # the restatement reproduces the reference before its table is recorded
        assert np.array_equal(r[2], in1) and np.array_equal(r[3], in2), name
        assert np.abs(r[0] - R).max() <= 1e-12 and np.abs(r[1] - t).max() <= 1e-12, name
        out[pre + "state"] = np.array("pose")
        out[pre + "R"], out[pre + "t"], out[pre + "in1"], out[pre + "in2"] = R, t, in1, in2
        # the winner's inliers triangulated with its pose (Runner.py:202-208)
        Pa = CameraPose.calculate_projection_matrix(Rb, Tb, K1)
        Pb = CameraPose.calculate_projection_matrix(R, t, K2)
        if name.startswith("n"):  # the planted sizes: pose only
            print(f"  {name}: n={len(p1)} iters={iters} -> iteration {r[4]}, {len(in1)} inliers, "
                  f"{int(tab['valid'].any(1).sum())} iterations with a valid pose (reference {dt:.2f} s)")
            continue
        out[pre + "X"] = np.array([CameraPose.triangulate_point(a, b, Pa, Pb) for a, b in zip(in1, in2)])
        out[pre + "Xn"] = CameraPose.triangulate_points(in1, in2, Pa, Pb)
        print(f"  {name}: n={len(p1)} iters={iters} -> iteration {r[4]}, {len(in1)} inliers, "
              f"{int(tab['valid'].any(1).sum())} iterations with a valid pose (reference {dt:.2f} s)")
    p1, p2, P1, P2 = PR.triangulation_inputs()
    out["tri_p1"], out["tri_p2"], out["tri_P1"], out["tri_P2"] = p1, p2, P1, P2
    out["tri_X"] = np.array([CameraPose.triangulate_point(a, b, P1, P2) for a, b in zip(p1, p2)])
    for N in PR.TRI_SIZES[1:]:  # the Hartley transforms depend on the set; one point has no
        out[f"tri_Xn{N}"] = CameraPose.triangulate_points(p1[:N], p2[:N], P1, P2)  # scale (LinAlgError)
    path = os.path.join(OUT, "pose.npz")
    np.savez_compressed(path, **out)
    print(f"wrote pose.npz ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
