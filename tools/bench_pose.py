"""Initial-pair pose RANSAC timing (diagnostic, not part of bench.py): a planted two-view
scene (960 x 540, f = 800, yaw 0.12 rad, integer pixels, `--outliers` of the second image's
points replaced by random pixels) through sfm_ransac_camera_motion_dev, for one pair at
n = 2500, iters = 1000 and for 32 pairs batched.  Reports the cold call (host replay of the
sampling stream included), warm calls and the device time between HIP events on the call's
stream, and the triangulation of the pair's points.  With no outliers nearly every sample
has a valid candidate, which then runs all n points: the kernel's most expensive input.

--cpu times the numpy restatement (tests/pose_ref.py) and --reference DIR the reference's own
CameraPose.ransac_camera_motion (where that checkout exists; no GPU needed) on a smaller
case, --cpu-n points and --cpu-iters iterations."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_scene(n, frac, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    K = np.array([[800.0, 0, 480], [0, 800, 270], [0, 0, 1]])
    X = rng.uniform([-3, -2, 4], [3, 2, 12], (n, 3))
    c, s = np.cos(0.12), np.sin(0.12)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    a = X @ K.T
    b = (X @ R.T + np.array([-1.0, 0.05, 0.1])) @ K.T
    p1 = np.round(a[:, :2] / a[:, 2:]).astype(np.int64)
    p2 = np.round(b[:, :2] / b[:, 2:]).astype(np.int64)
    k = int(frac * n)
    if k:
        p2[:k] = np.column_stack((rng.integers(0, 960, k), rng.integers(0, 540, k)))
    return p1, p2, K


def time_device(P, n, iters, frac, reps):
    import numpy as np
    import torch
    from sfmfromscratch_amd import _abi, _native, pose
    sets = [make_scene(n, frac, 100 + p) for p in range(P)]
    K = sets[0][2]
    pts = np.zeros((P, n, 4), np.int32)
    for p, (a, b, _) in enumerate(sets):
        pts[p, :, :2] = a
        pts[p, :, 2:] = b
    npts = np.full(P, n, np.int32)
    Kh = np.ascontiguousarray(np.tile(np.concatenate([K.ravel(), K.ravel()]), (P, 1)))
    bh = np.ascontiguousarray(np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (P, 1)))
    oR, ot = np.zeros((P, 9)), np.zeros((P, 3))
    ctx = _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))
    d_pts = torch.from_numpy(pts).cuda()
    d_n = torch.from_numpy(npts).cuda()
    o_pts = torch.zeros_like(d_pts)
    o_n = torch.zeros(P, dtype=torch.int32, device="cuda")
    o_it = torch.zeros(P, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dp = ctypes.POINTER(ctypes.c_double)

    def call():
        _native.check(ctx.lib.sfm_ransac_camera_motion_dev(
            ctx.handle, d_pts.data_ptr(), d_n.data_ptr(), npts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), P, n,
            iters, ctypes.c_double(1.0), Kh.ctypes.data_as(dp), bh.ctypes.data_as(dp), o_pts.data_ptr(),
            o_n.data_ptr(), o_it.data_ptr(), oR.ctypes.data_as(dp), ot.ctypes.data_as(dp), st or None), ctx.handle)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    cold = time.perf_counter() - t0
    warm, dev = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        warm.append(time.perf_counter() - t0)
        dev.append(e0.elapsed_time(e1))
    cand = ctx.pose_candidates(P, iters)
    on = o_n.cpu().numpy()
    print(f"pose {P} pair(s), n {n}, iters {iters}, outliers {frac}: cold {cold * 1e3:.1f} ms, warm "
          f"{np.median(warm) * 1e3:.2f} ms, events {np.median(dev):.3f} ms (min {min(dev):.3f}); "
          f"{(cand >= 0).mean() * 100:.0f} % of samples with a valid pose, inliers mean {on.mean():.0f}", flush=True)
    if P == 1 and on[0] > 0:
        a, b, _ = sets[0]
        Pa = pose.calculate_projection_matrix(np.eye(3), np.zeros(3), K)
        Pb = pose.calculate_projection_matrix(oR[0].reshape(3, 3), ot[0], K)
        x1 = torch.from_numpy(a.astype(np.float64)).cuda()
        x2 = torch.from_numpy(b.astype(np.float64)).cuda()
        A, B = torch.from_numpy(Pa).cuda(), torch.from_numpy(Pb).cuda()
        for fn in (pose.triangulate, pose.triangulate_points):
            fn(x1, x2, A, B)
            ts = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(x1, x2, A, B)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            print(f"{fn.__name__} n {n}: events {np.median(ts):.3f} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2500)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--outliers", type=float, nargs="*", default=[0.0, 0.02])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-device", action="store_true", help="only the CPU timings")
    ap.add_argument("--cpu", action="store_true", help="time the numpy restatement on the smaller case")
    ap.add_argument("--reference", default="", help="reference checkout: time its own call on the smaller case")
    ap.add_argument("--cpu-n", type=int, default=300)
    ap.add_argument("--cpu-iters", type=int, default=100)
    args = ap.parse_args()
    import numpy as np
    if not args.no_device:
        for frac in args.outliers:
            time_device(1, args.n, args.iters, frac, args.reps)
            time_device(args.pairs, args.n, args.iters, frac, args.reps)
    if args.cpu or args.reference:
        p1, p2, K = make_scene(args.cpu_n, 0.0, 100)
        if args.cpu:
            from tests import pose_ref as PR
            t0 = time.perf_counter()
            PR.ransac_camera_motion(p1, p2, K, K, np.eye(3), np.zeros(3), 1.0, args.cpu_iters)
            print(f"restatement (numpy, vectorised, no early exit) n {args.cpu_n}, iters {args.cpu_iters}: "
                  f"{time.perf_counter() - t0:.2f} s", flush=True)
        if args.reference:
            from oracle import cv2_standin
            sys.modules["cv2"] = cv2_standin
            sys.path.insert(0, args.reference)
            from SFM import CameraPose
            t0 = time.perf_counter()
            r = CameraPose(p1, p2, K, K).ransac_camera_motion(np.eye(3), np.zeros(3), 1.0, args.cpu_iters)
            print(f"reference CameraPose.ransac_camera_motion n {args.cpu_n}, iters {args.cpu_iters}: "
                  f"{time.perf_counter() - t0:.2f} s ({len(r[2])} inliers)", flush=True)


if __name__ == "__main__":
    main()
