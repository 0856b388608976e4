"""Point-registry timing (diagnostic, not part of bench.py): device time between HIP events of
one sfm_registry_add_dev of --n points against registries of 10^3, 10^4 and 10^5 points, after
warm-up calls, for three batches: all fresh points, all exact copies of registered points
(perform's result_prev, Runner.py:269), and half copies with --contested points of a 0.4e-6
lattice (the serial walk).  The count is restored before every call, so each call sees the
same registry.  Then the total reprojection error of --obs observations.

--cpu times the reference's rule restated in numpy (tests/registry_ref.py add_sequential: the
same arithmetic per point, without the reference's rebuild of the array from a Python list) on
2,000 fresh points followed by 1,000 duplicates; --reference times the reference's own add_points
at that size (where its checkout is present; driven as in tools/gen_golden_registry.py)."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2500)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000, 10000, 100000])
    ap.add_argument("--contested", type=int, default=200)
    ap.add_argument("--obs", type=int, default=200000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--reference", action="store_true",
                    help="time the reference's own add_points (needs the checkout, SFM_REFERENCE)")
    args = ap.parse_args()
    import numpy as np
    from tests import registry_ref as RR
    rng = np.random.RandomState(3)
    if not args.no_device:
        import torch
        from sfmfromscratch_amd import _abi, _native
        dev = torch.device("cuda", 0)
        ctx = _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))
        st = torch.cuda.current_stream(dev).cuda_stream
        t = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        n = args.n
        for R in args.sizes:
            base = rng.uniform(-10, 10, size=(R, 3))
            cap = R + n
            table = torch.empty((cap, 3), dtype=torch.float64, device=dev)
            table[:R] = t(base)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            idx = torch.empty(n, dtype=torch.int32, device=dev)
            new = torch.empty(n, dtype=torch.int32, device=dev)
            mixed = np.concatenate([base[rng.randint(R, size=n - n // 2 - args.contested)],
                                    rng.uniform(-10, 10, size=(n // 2, 3)),
                                    20.0 + RR.lattice_points(rng, args.contested)])
            batches = {"fresh": rng.uniform(-10, 10, size=(n, 3)), "copies": base[rng.randint(R, size=n)],
                       "mixed": mixed[rng.permutation(n)]}
            for name, pts in batches.items():
                d_pts = t(pts)
                ts = []
                for k in range(args.warmup + args.reps):
                    count.fill_(R)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _native.check(ctx.lib.sfm_registry_add_dev(ctx.handle, table.data_ptr(), count.data_ptr(), cap,
                                                               d_pts.data_ptr(), n, ctypes.c_double(1e-6),
                                                               idx.data_ptr(), new.data_ptr(), st or None), ctx.handle)
                    e1.record()
                    torch.cuda.synchronize()
                    if k >= args.warmup:
                        ts.append(e0.elapsed_time(e1))
                print(f"registry {R} + {n} {name}: events {np.median(ts):.3f} ms (min {min(ts):.3f}); "
                      f"{int(new.sum())} new, count {int(count.cpu()[0])}", flush=True)
        cam, pt, obs, cp, X, K = RR.score_case(M=900)
        M = args.obs
        sel = rng.randint(900, size=M)
        d_cam, d_pt, d_obs = t(cam[sel], np.int32), t(pt[sel], np.int32), t(obs[sel])
        d_cp, d_X, d_K = t(cp), t(X), t(K)
        err = torch.empty(M, dtype=torch.float64, device=dev)
        mean = torch.empty(1, dtype=torch.float64, device=dev)
        ts = []
        for k in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _native.check(ctx.lib.sfm_total_reprojection_error_dev(
                ctx.handle, d_cam.data_ptr(), d_pt.data_ptr(), d_obs.data_ptr(), M, d_cp.data_ptr(), len(cp),
                d_K.data_ptr(), d_X.data_ptr(), len(X), err.data_ptr(), mean.data_ptr(), st or None), ctx.handle)
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                ts.append(e0.elapsed_time(e1))
        print(f"total reprojection error, {M} observations: events {np.median(ts):.3f} ms (min {min(ts):.3f}); "
              f"mean {float(mean.cpu()[0]):.6f}", flush=True)
    if args.cpu:
        fresh = rng.uniform(-5, 5, size=(2000, 3))
        G = []
        t0 = time.perf_counter()
        RR.add_sequential(G, fresh)
        RR.add_sequential(G, fresh[:1000])
        print(f"restatement (numpy, sequential) 2,000 fresh + 1,000 duplicates: {time.perf_counter() - t0:.2f} s",
              flush=True)
    if args.reference:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gen_golden_registry as GG
        fresh = rng.uniform(-5, 5, size=(2000, 3))
        r = GG.runner()
        t0 = time.perf_counter()
        r.add_points(fresh, np.zeros((2000, 2)), 0)
        r.add_points(fresh[:1000], np.zeros((1000, 2)), 1)
        print(f"reference add_points 2,000 fresh + 1,000 duplicates: {time.perf_counter() - t0:.2f} s "
              f"({len(r.global_points_3D)} registered)", flush=True)


if __name__ == "__main__":
    main()
