"""Bundle-adjustment timing (diagnostic, not part of bench.py): device time between HIP events
of one sfm_bundle_adjust_dev call on the planted scene of tests/ba_ref.py — 16 cameras, 20,000
points, 60,000 observations (every point seen by three cameras), two cameras fixed, ftol = 1e-2,
max_iter = 50 — after one warm-up call (which also sizes the workspace).  Inputs and outputs are
device tensors; nothing is copied inside the timed span.

--reference times the REFERENCE's scipy path (SFM.py:405-464, least_squares with a 2-point
Jacobian and one Python loop over the observations per column) on a scene small enough to
finish; it needs a reference checkout (SFM_REFERENCE) and imports it with oracle/cv2_standin.py
in place of cv2, as tools/gen_golden_ba.py does.  It runs on the host only."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=16)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--views", type=int, default=3, help="cameras per point")
    ap.add_argument("--ftol", type=float, default=1e-2)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--reference", action="store_true", help="time the reference's scipy path on a small scene")
    ap.add_argument("--ref-cams", type=int, default=4)
    ap.add_argument("--ref-points", type=int, default=100)
    args = ap.parse_args()
    import numpy as np
    from tests import ba_ref as BR
    if not args.no_device:
        import torch
        from sfmfromscratch_amd import _native, pose
        sc = BR.bench_scene(args.cams, args.points, args.views)
        dev = torch.device("cuda", 0)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        ci, pi, obs = t(sc["cam_idx"], np.int32), t(sc["pt_idx"], np.int32), t(sc["obs"], np.float64)
        cams, K, X, fixed = t(sc["cams"], np.float64), t(sc["K"], np.float64), t(sc["X"], np.float64), t(sc["fixed"], np.uint8)
        oc, oX = torch.empty_like(cams), torch.empty_like(X)
        cost = torch.empty(2, dtype=torch.float64, device=dev)
        status = torch.empty(4, dtype=torch.int32, device=dev)
        ctx, stream = pose._structure_ctx(dev)
        M = int(obs.shape[0])

        def call():
            _native.check(ctx.lib.sfm_bundle_adjust_dev(
                ctx.handle, ci.data_ptr(), pi.data_ptr(), obs.data_ptr(), M, cams.data_ptr(), sc["n_cam"], K.data_ptr(),
                X.data_ptr(), sc["n_pts"], fixed.data_ptr(), args.ftol, args.max_iter, oc.data_ptr(), oX.data_ptr(),
                cost.data_ptr(), status.data_ptr(), stream or None), ctx.handle)

        call()  # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        st, c = status.cpu().numpy(), cost.cpu().numpy()
        print(f"bundle adjustment {sc['n_cam']} cameras {sc['n_pts']} points {M} observations ftol {args.ftol:g}: events "
              f"{float(np.median(ts)):.3f} ms (min {min(ts):.3f}, {args.reps} calls); status {int(st[0])} accepted "
              f"{int(st[1])} iterations {int(st[2])} rejected factorisations {int(st[3])}, cost {c[0]:.2f} -> {c[1]:.4f} "
              f"({ts[0] / max(int(st[2]), 1):.3f} ms per iteration with the plan and the idle rounds)", flush=True)
    if args.reference:
        from tools import gen_golden_ba as G
        sc = BR.bench_scene(args.ref_cams, args.ref_points, min(args.views, args.ref_cams), seed=61)
        sc["fixed"][:] = 0  # the reference fixes nothing
        sc = dict(sc)
        t0 = time.perf_counter()
        r = BR.solve(sc, ftol=args.ftol, max_iter=args.max_iter)
        dt = time.perf_counter() - t0
        ref = G.reference_run(sc)
        if ref is None:
            print("no reference checkout (SFM_REFERENCE)")
            return
        print(f"reference (scipy trf, 2-point Jacobian) {sc['n_cam']} cameras {sc['n_pts']} points {len(sc['obs'])} "
              f"observations: {float(ref['ref_seconds']):.2f} s, cost {r['cost0']:.2f} -> {float(ref['ref_cost_after']):.4f}; "
              f"the numpy restatement of the library's rule: {dt:.2f} s, cost -> {r['cost']:.4f}", flush=True)


if __name__ == "__main__":
    main()
