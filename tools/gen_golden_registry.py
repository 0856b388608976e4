#!/usr/bin/env python3
"""Generate tests/golden/registry.npz: the REFERENCE's own SFMRunner.add_points (with
is_new_point / find_existing_point), prepare_for_ba and total_reprojection_error
(Runner.py:311-334, :361-401) on the cases of tests/registry_ref.py.

The methods are pure numpy and are driven without constructing a runner:
object.__new__(SFMRunner) plus the list attributes they touch.  The reference's cv2 import is
served by oracle/cv2_standin.py; total_reprojection_error reaches cv2.Rodrigues through
CameraPose.project_point, which the stand-in lacks, so this tool sets a `Rodrigues` attribute
on the stand-in module at run time (the closed form of tests/registry_ref.py; parity with real
OpenCV is unpinned).  Only inputs the generators cannot rebuild and recorded
outputs are written.

    PYTHONDONTWRITEBYTECODE=1 SFM_REFERENCE=<checkout> python tools/gen_golden_registry.py
"""
from __future__ import annotations

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
from tests import registry_ref as RR  # noqa: E402


def _rodrigues(a):
    a = np.asarray(a, np.float64)
    if a.size == 3:
        return RR.rodrigues_to_matrix(a), None
    return RR.rodrigues_to_vector(a).reshape(3, 1), None


cv2_standin.Rodrigues = _rodrigues
sys.modules["cv2"] = cv2_standin
sys.path.insert(0, REF)
from Runner import SFMRunner  # noqa: E402


def runner():
    r = object.__new__(SFMRunner)
    r.global_points_3D, r.global_points_2D, r.frame_indices, r.point_indices = [], [], [], []
    r.global_poses, r.global_K = [], []
    return r


def main():
    out = {}
    cases = RR.cases()
    out["names"] = np.array(list(cases.keys()))
    for name, calls in cases.items():
        r = runner()
        t0 = time.time()
        for p3d, p2d, f in calls:
            r.add_points(p3d, p2d, f)
        dt = time.time() - t0
        pre = name + "_"
        out[pre + "pt_idx"] = np.array(r.point_indices, np.int64)
        out[pre + "frame_idx"] = np.array(r.frame_indices, np.int64)
        out[pre + "p3d"] = np.array(r.global_points_3D, np.float64).reshape(-1, 3)
        info = {}
        G = []
        for p3d, _, _ in calls:
            RR.add_two_phase(G, p3d, info=info) if len(p3d) else None
        print(f"  {name}: {len(calls)} calls, {len(r.point_indices)} points -> {len(r.global_points_3D)} registered "
              f"({dt:.2f} s in the reference; {info.get('contested', 0)} contested in the last call)")
        if name == "sequence":
            r.global_poses, r.global_K = RR.sequence_poses()
            ba = r.prepare_for_ba()
            out["ba_num_cameras"], out["ba_num_points"] = np.int64(ba[0]), np.int64(ba[1])
            out["ba_camera_indices"], out["ba_point_indices"] = np.array(ba[2], np.int64), np.array(ba[3], np.int64)
            out["ba_points_2D"], out["ba_camera_params"], out["ba_points_3D"], out["ba_K"] = ba[4], ba[5], ba[6], ba[7]
            out["ba_mean"] = np.float64(r.total_reprojection_error(*ba[1:]))
    cam, pt, obs, cp, X, K = RR.score_case()
    r = runner()
    for k in (300, 900):
        out[f"score_mean_{k}"] = np.float64(r.total_reprojection_error(k, cam, pt, obs, cp, X, K))
        e = RR.reprojection_errors(k, cam, pt, obs, cp, X, K)
        print(f"  score num_points {k}: reference mean {out[f'score_mean_{k}']:.12g}, restatement {e.mean():.12g}")
    # the reference's cost at the size the issue quotes: 2,000 fresh points, then 1,000 duplicates
    rng = np.random.RandomState(7)
    fresh = rng.uniform(-5, 5, size=(2000, 3))
    r = runner()
    t0 = time.time()
    r.add_points(fresh, np.zeros((2000, 2)), 0)
    r.add_points(fresh[:1000], np.zeros((1000, 2)), 1)
    print(f"  reference add_points, 2,000 fresh + 1,000 duplicates: {time.time() - t0:.2f} s")
    path = os.path.join(OUT, "registry.npz")
    np.savez_compressed(path, **out)
    print(f"wrote registry.npz ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
