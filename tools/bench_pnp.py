"""PnP timing (diagnostic, not part of bench.py): device time between HIP events of
sfm_pnp_ransac_dev at n = 2,500 links with 5,967 iterations (the runner's count,
calculate_num_ransac_iterations(0.98, 8, 0.4)) and of sfm_pnp_dev over the same points, after
warm-up calls (the first call also uploads the sample stream).  The scene is the planted
960 x 540, f = 800 family of tests/pnp_ref.py with sigma = 0.6 pixel noise, rounded, 20 % random
image points.

--cpu times the numpy restatement (tests/pnp_ref.py) of the same call on the host."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def events(fn, warmup, reps):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2500)
    ap.add_argument("--iters", type=int, default=5967)
    ap.add_argument("--outliers", type=float, default=0.2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--cpu", action="store_true", help="time the numpy restatement on the host")
    args = ap.parse_args()
    import numpy as np
    from tests import pnp_ref as PR
    X, x, planted, Rt, tt = PR.scene(900, args.n, args.outliers)
    K = PR.K_SCENE
    if not args.no_device:
        import torch
        from sfmfromscratch_amd import _native, pose
        dev = torch.device("cuda", 0)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
        dX, dx, dK = t(X), t(x), t(K).reshape(-1)
        out = {}

        def ransac():
            out.update(pose._pnp_ransac_dev(dX, dx, dK, args.iters, pose.PNP_THRESHOLD, pose.REFINE_MAX_ITER, dev))

        med, lo = events(ransac, args.warmup, args.reps)
        k = int(out["n"].cpu()[0])
        st = out["status"].cpu().numpy()
        c = out["cost"].cpu().numpy()
        inl = out["inliers"][:max(k, 0)].cpu().numpy()
        print(f"pnp ransac n {args.n} iters {args.iters}: events {med:.3f} ms (min {lo:.3f}); winner "
              f"{int(out['iteration'].cpu()[0])}, {k} inliers ({int(planted[inl].sum())} of {int(planted.sum())} planted), "
              f"LM status {int(st[1])} accepted {int(st[2])} iterations {int(st[3])}, cost {c[0]:.2f} -> {c[1]:.4f}",
              flush=True)
        # the refinement's share: the same call with the sampling reduced to the winner's prefix is
        # not the same problem, so time PnP (DLT + refinement) over the planted inliers instead
        Xi, xi = t(X[planted]), t(x[planted])
        R = torch.empty(9, dtype=torch.float64, device=dev)
        tv = torch.empty(3, dtype=torch.float64, device=dev)
        status = torch.empty(4, dtype=torch.int32, device=dev)
        cost = torch.empty(2, dtype=torch.float64, device=dev)
        ctx, stream = pose._structure_ctx(dev)

        def pnp():
            _native.check(ctx.lib.sfm_pnp_dev(ctx.handle, Xi.data_ptr(), xi.data_ptr(), dK.data_ptr(), int(Xi.shape[0]),
                                              pose.REFINE_MAX_ITER, R.data_ptr(), tv.data_ptr(), status.data_ptr(),
                                              cost.data_ptr(), stream or None), ctx.handle)

        med, lo = events(pnp, args.warmup, args.reps)
        st = status.cpu().numpy()
        c = cost.cpu().numpy()
        print(f"pnp (DLT over all + refinement) n {int(Xi.shape[0])}: events {med:.3f} ms (min {lo:.3f}); LM status "
              f"{int(st[1])} accepted {int(st[2])} iterations {int(st[3])}, cost {c[0]:.2f} -> {c[1]:.4f}", flush=True)
    if args.cpu:
        t0 = time.perf_counter()
        r = PR.pnp_ransac(X, x, K, args.iters)
        dt = time.perf_counter() - t0
        print(f"restatement (numpy, vectorised over samples) n {args.n} iters {args.iters}: {dt:.2f} s; winner "
              f"{r['iteration']}, {len(r['inliers'])} inliers, cost {r['cost0']:.2f} -> {r['cost']:.4f}", flush=True)


if __name__ == "__main__":
    main()
