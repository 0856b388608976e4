"""Two-view geometry timing (diagnostic, not part of bench.py).  The job is bench_verify.py's: N
synthetic frames (synth.py) extracted and matched on the device, all N (N - 1) / 2 pairs (256
frames: 32,640 pairs, cap 2,500), the match tensors resident, then verify_matches once for keep, F
and stat.  Timed between HIP events after warm-up, the three calls alternating run by run on the
same box, each on preallocated outputs (what sequence.two_view_geometry enqueues, without its
allocations):

  verify      sfm_verify_matches_dev at --verify-iters samples, confidence 0.98 (its own time, for
              scale: DESIGN.md §13H measured 180 ms)
  homography  sfm_homography_matches_dev at --iters samples over the verified pairs, with the
              0.98 table for four-point samples and with the early stop off
  pose        sfm_two_view_pose_dev over the verified pairs

Each window repeats its call --inner times, so that it holds enough work for the event clock.
The parent commit has no route to these results, so there is nothing to compare against and
nothing is asserted.  Writes profiles/two_view_bench.txt (or --out)."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P_OCT = {"num_interest_points": 2500, "ksize": 3, "gaussian_size": 7, "sigma": 6, "alpha": 0.05,
         "feature_width": 18, "pyramid_level": 4, "pyramid_scale_factor": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--verify-iters", type=int, default=5967)
    ap.add_argument("--iters", type=int, default=150)
    ap.add_argument("--threshold", type=float, default=2.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_bench.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from sfmfromscratch_amd import pose, sequence as S, synth
    from sfmfromscratch_amd.pipeline import BatchMatcher
    if not torch.cuda.is_available():
        raise SystemExit("bench_two_view.py measures on the device: no GPU found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N = args.frames
    t0 = time.perf_counter()
    frames = [synth.u8_to_gray(synth.make_frame_u8(args.height, args.width, 1234 + 1000 * (i // 32), i % 32))
              for i in range(N)]
    cache = S.FeatureCache(frames, P_OCT, batch=32)
    del frames
    slots = cache.slots
    dev, cap = slots.desc.device, cache.cap
    ctx = cache.extractor.ctx
    say(f"{N} frames {args.height}x{args.width} extracted in {time.perf_counter() - t0:.1f} s, cap {cap}")
    matcher = BatchMatcher(0.85, device=dev.index, ctx=ctx)
    pairs = S.pair_schedule(N, "all")
    P = len(pairs)
    pt = torch.from_numpy(pairs).to(dev)
    mm = torch.zeros((P, cap, 2), dtype=torch.int32, device=dev)
    cc = torch.zeros((P, cap), dtype=torch.float32, device=dev)
    nm = torch.zeros(P, dtype=torch.int32, device=dev)
    matcher.prep(slots)
    for a in range(0, P, 4096):
        matcher.match(slots, pt[a:a + 4096], out=(mm[a:a + 4096], cc[a:a + 4096], nm[a:a + 4096]), prepped=True)
    torch.cuda.synchronize()
    nmh = nm.cpu().numpy()
    say(f"{P} pairs matched; matches per pair min {nmh.min()} mean {nmh.mean():.0f} max {nmh.max()}")

    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
    keep, F, stat = z((P, cap), torch.uint8), z((P, 9), torch.float64), z((P, 4), torch.int32)
    H, hkeep, hstat = z((P, 9), torch.float64), z((P, cap), torch.uint8), z((P, 4), torch.int32)
    rt, pstat = z((P, 12), torch.float64), z((P, 4), torch.int32)
    K = torch.tensor([[1600.0, 0, args.width / 2], [0, 1600.0, args.height / 2], [0, 0, 1]], dtype=torch.float64,
                     device=dev).reshape(1, 9).expand(N, 9).contiguous()
    vstop = pose.ransac_stop_ratios(0.98, min(64, (args.verify_iters + 255) // 256))
    hstop = pose.ransac_stop_ratios(0.98, min(64, (args.iters + 255) // 256), 4)
    cos2 = math.cos(math.radians(2.0)) ** 2
    stream = torch.cuda.current_stream(dev).cuda_stream

    def verify():
        ctx.verify_matches_dev(slots.xy, slots.count, pt, mm, nm, args.verify_iters, 1.0, 16, 5, vstop, keep, F, stat,
                               stream)

    verify()
    att = stat[:, 3].contiguous()

    def homography(stop):
        return lambda: ctx.homography_matches_dev(slots.xy, slots.count, pt, mm, nm, att, args.iters, args.threshold, 5,
                                                  stop, H, hkeep, hstat, stream)

    def two_view_pose():
        ctx.two_view_pose_dev(slots.xy, slots.count, pt, mm, nm, keep, F, K, att, cos2, rt, pstat, stream)

    routes = {"verify": verify, "homography_stop": homography(hstop), "homography_fixed": homography(None),
              "pose": two_view_pose}
    runs = {k: [] for k in routes}
    for r in range(args.warmup + args.reps):
        for k, fn in routes.items():   # alternating: one window of each call per round
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                runs[k].append(e0.elapsed_time(e1) / args.inner)
    homography(hstop)()
    torch.cuda.synchronize()
    vs, hs, ps = stat.cpu().numpy(), hstat.cpu().numpy(), pstat.cpu().numpy()
    ok = vs[:, 3] != 0
    planar = ok & (hs[:, 0] >= 0.8 * vs[:, 0])
    res = {"frames": N, "pairs": P, "cap": int(cap), "verify_iters": args.verify_iters, "iters": args.iters,
           "threshold": args.threshold, "reps": args.reps, "inner": args.inner,
           "events_ms_per_call": {k: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3),
                                      "max": round(max(v), 3)} for k, v in runs.items()},
           "verified_pairs": int(ok.sum()), "matches_kept": int(vs[ok, 0].sum()),
           "homography_samples_mean": float(hs[ok, 2].mean()) if ok.any() else 0.0,
           "planar_or_panoramic": int(planar.sum()), "with_pose": int((ps[:, 1] >= 0).sum()),
           "wide_points": int(ps[ps[:, 1] >= 0, 2].sum())}
    for k, v in res["events_ms_per_call"].items():
        say(f"{k}: {v['median']:.3f} ms per call (min {v['min']:.3f}, max {v['max']:.3f}; HIP events, {args.reps} "
            f"windows of {args.inner} calls)")
    say(json.dumps({"bench_two_view": res}))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
