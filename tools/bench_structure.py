"""Structure-stage timing (diagnostic, not part of bench.py): device time between HIP events of
the refinement (sfm_refine_points_dev), the reprojection error (sfm_reprojection_error_dev) and
the 2D -> 3D association (sfm_link_points_dev) at n = 2500 points — one camera pair, and 32
segments of n points with 32 camera pairs in one refinement launch — after warm-up calls.
The scene is the 960 x 540, f = 800, yaw 0.12 rad family with sigma = 0.7 pixel noise, rounded.

--cpu times the numpy restatement (tests/structure_ref.py) on --cpu-n points; the reference's
own CameraPose.non_linear_triangulation is timed by tools/gen_golden_structure.py, which prints
its time per fixture case."""
import argparse
import ctypes
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
    ap.add_argument("--segments", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--cpu", action="store_true", help="time the numpy restatement on --cpu-n points")
    ap.add_argument("--cpu-n", type=int, default=200)
    args = ap.parse_args()
    import numpy as np
    from tests import pose_ref as PR
    from tests import structure_ref as SR
    if not args.no_device:
        import torch
        from sfmfromscratch_amd import _abi, _native, pose
        dev = torch.device("cuda", 0)
        ctx = _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))
        st = torch.cuda.current_stream(dev).cuda_stream
        t = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        for S in (1, args.segments):
            scenes = [SR.refine_scene(500 + s, args.n) for s in range(S)]
            N = S * args.n
            a, b = t(np.concatenate([c[0] for c in scenes])), t(np.concatenate([c[1] for c in scenes]))
            Pm = t(np.concatenate([np.concatenate([c[2].ravel(), c[3].ravel()]) for c in scenes]))
            seg = t(np.repeat(np.arange(S), args.n), np.int32)
            X0 = torch.cat([pose.triangulate(a[s * args.n:(s + 1) * args.n], b[s * args.n:(s + 1) * args.n],
                                             Pm[24 * s:24 * s + 12], Pm[24 * s + 12:24 * s + 24]) for s in range(S)])
            X = torch.empty_like(X0)
            cost = torch.empty(N, dtype=torch.float64, device=dev)
            it = torch.empty(N, dtype=torch.int32, device=dev)

            def refine():
                _native.check(ctx.lib.sfm_refine_points_dev(
                    ctx.handle, X0.data_ptr(), a.data_ptr(), b.data_ptr(), N, Pm.data_ptr(), S,
                    seg.data_ptr() if S > 1 else None, 50, X.data_ptr(), cost.data_ptr(), it.data_ptr(), st or None),
                    ctx.handle)

            med, lo = events(refine, args.warmup, args.reps)
            itn = it.cpu().numpy()
            print(f"refine {S} segment(s) x {args.n} points: events {med:.3f} ms (min {lo:.3f}); accepted steps "
                  f"mean {(itn & 0xFFFFFF).mean():.1f} max {(itn & 0xFFFFFF).max()}, status counts "
                  f"{np.bincount(itn >> 24, minlength=4).tolist()}", flush=True)
        # error and link on one pair's points
        n = args.n
        p1, p2, P1, P2 = SR.refine_scene(500, n)
        a, b, A, B = t(p1), t(p2), t(P1.ravel()), t(P2.ravel())
        X = pose.non_linear_triangulation(pose.triangulate(a, b, A, B), a, b, A, B)
        err = torch.empty((n, 2), dtype=torch.float64, device=dev)
        mean = torch.empty(1, dtype=torch.float64, device=dev)

        def reproj():
            _native.check(ctx.lib.sfm_reprojection_error_dev(ctx.handle, X.data_ptr(), a.data_ptr(), b.data_ptr(), n,
                                                             A.data_ptr(), B.data_ptr(), err.data_ptr(),
                                                             mean.data_ptr(), st or None), ctx.handle)

        med, lo = events(reproj, args.warmup, args.reps)
        print(f"reprojection error n {n}: events {med:.3f} ms (min {lo:.3f}); mean {float(mean.cpu()[0]):.4f}",
              flush=True)
        tgt, _, qry, _ = SR.link_scene(600, n, n)
        d_t, d_q = t(tgt, np.int32), t(qry, np.int32)
        o_t = torch.empty(n, dtype=torch.int32, device=dev)
        o_q = torch.empty(n, dtype=torch.int32, device=dev)
        o_n = torch.zeros(1, dtype=torch.int32, device=dev)

        def link():
            _native.check(ctx.lib.sfm_link_points_dev(ctx.handle, d_t.data_ptr(), n, d_q.data_ptr(), n,
                                                      ctypes.c_double(5.0), o_t.data_ptr(), o_q.data_ptr(),
                                                      o_n.data_ptr(), st or None), ctx.handle)

        med, lo = events(link, args.warmup, args.reps)
        print(f"link m {n} nq {n}: events {med:.3f} ms (min {lo:.3f}); {int(o_n.cpu()[0])} kept", flush=True)
    if args.cpu:
        p1, p2, P1, P2 = SR.refine_scene(500, args.cpu_n)
        X0, _ = PR.triangulate(p1, p2, P1, P2)
        t0 = time.perf_counter()
        SR.refine(X0, p1, p2, P1, P2)
        print(f"restatement (numpy, one point at a time) n {args.cpu_n}: {time.perf_counter() - t0:.2f} s", flush=True)


if __name__ == "__main__":
    main()
