"""Geometric-verification timing (diagnostic, not part of bench.py).  The job is bench_tracks.py's:
N synthetic frames (synth.py) extracted and matched on the device, all N (N - 1) / 2 pairs (256
frames: 32,640 pairs), the match tensors resident.  Timed, interleaved run by run after warm-up:

  new/fixed   sequence.verify_matches at --iters samples, early stop off
  new/stop    the same with confidence 0.98
  parent      the only route to the same mask without the call: download the match tensors and the
              table's pixels, gather each pair's correspondences on the host (the
              convert_matches_to_coords step), pose.find_inliers_batch at the same iteration count,
              find each pair's inlier rows again in its match list (find_inliers returns compacted
              points, not a mask), upload keep [P][cap]

Every span is wall-clock time around the route with a device synchronisation at both ends (the
parent route is mostly host work); the new call's span between HIP events is printed too.  The
parent route stores every sample's F (P x iters x 72 B) and replays numpy's sample stream on one
host thread for every distinct match count, so it is timed on a SUBSET of the pairs: every
(P // --subset)-th pair of the schedule, the same subset for all three routes, and scaled by
P / subset for the full job.  The new call is then also run on the whole schedule, unless its
subset time predicts more than --full-budget seconds per run.

Also printed, without a bar: matching the same pairs, and build_tracks with the mask."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P_OCT = {"num_interest_points": 2500, "ksize": 3, "gaussian_size": 7, "sigma": 6, "alpha": 0.05,
         "feature_width": 18, "pyramid_level": 4, "pyramid_scale_factor": 2}


def parent_route(torch, pose, slots, pairs, mm, nm, iters, threshold, dev):
    """-> (keep [P, cap] uint8 on the device, seconds by phase)."""
    import numpy as np
    t0 = time.perf_counter()
    m, n, xy = mm.cpu().numpy(), nm.cpu().numpy(), slots.xy.cpu().numpy()
    t1 = time.perf_counter()
    P, cap = len(pairs), m.shape[1]
    sets = []
    for p in range(P):
        k = max(int(n[p]), 0)
        sets.append((xy[pairs[p, 0], m[p, :k, 0]].astype(np.int64), xy[pairs[p, 1], m[p, :k, 1]].astype(np.int64)))
    t2 = time.perf_counter()
    res = pose.find_inliers_batch(sets, threshold=threshold, max_iterations=iters, device=dev.index or 0)
    t3 = time.perf_counter()
    keep = np.zeros((P, cap), np.uint8)
    for p, r in enumerate(res):
        if len(r) != 2 or len(r[0]) == 0:
            continue
        # equal coordinates get equal decisions, so a row is kept exactly when it is among the inliers
        # (pixel coordinates are below 2^16: the four of a row packed into one int64 key)
        key = lambda a, b: (a[:, 0] << 48) | (a[:, 1] << 32) | (b[:, 0] << 16) | b[:, 1]  # noqa: E731
        rows = key(*sets[p])
        keep[p, :len(rows)] = np.isin(rows, key(np.asarray(r[0], np.int64), np.asarray(r[1], np.int64)))
    t4 = time.perf_counter()
    kd = torch.from_numpy(keep).to(dev)
    torch.cuda.synchronize()
    t5 = time.perf_counter()
    return kd, {"download": t1 - t0, "gather": t2 - t1, "find_inliers_batch": t3 - t2, "mask": t4 - t3,
                "upload": t5 - t4, "total": t5 - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=5967)
    ap.add_argument("--threshold", type=float, default=1.0)
    ap.add_argument("--subset", type=int, default=2048, help="pairs the three routes are timed on")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--full-budget", type=float, default=60.0, help="seconds one full-schedule run may take")
    ap.add_argument("--no-parent", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from sfmfromscratch_amd import pose, sequence as S, synth
    from sfmfromscratch_amd.pipeline import BatchMatcher
    N = args.frames
    t0 = time.perf_counter()
    frames = [synth.u8_to_gray(synth.make_frame_u8(args.height, args.width, 1234 + 1000 * (i // 32), i % 32))
              for i in range(N)]
    cache = S.FeatureCache(frames, P_OCT, batch=32)
    del frames
    dev, cap = cache.slots.desc.device, cache.cap
    print(f"{N} frames {args.height}x{args.width} extracted in {time.perf_counter() - t0:.1f} s, cap {cap}, "
          f"mean count {float(cache.slots.count.float().mean()):.0f}", flush=True)
    matcher = BatchMatcher(0.85, device=dev.index, ctx=cache.extractor.ctx)
    pairs = S.pair_schedule(N, "all")
    P = len(pairs)
    pt = torch.from_numpy(pairs).to(dev)
    mm = torch.zeros((P, cap, 2), dtype=torch.int32, device=dev)
    cc = torch.zeros((P, cap), dtype=torch.float32, device=dev)
    nm = torch.zeros(P, dtype=torch.int32, device=dev)

    def match_all():
        matcher.prep(cache.slots)
        for a in range(0, P, 4096):
            matcher.match(cache.slots, pt[a:a + 4096], out=(mm[a:a + 4096], cc[a:a + 4096], nm[a:a + 4096]),
                          prepped=True)

    def wall(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t), e0.elapsed_time(e1)

    match_all()
    _, match_ms, _ = wall(match_all)
    nmh = nm.cpu().numpy()
    print(f"matching all {P} pairs: {match_ms:.1f} ms; matches per pair min {nmh.min()} mean {nmh.mean():.0f} max "
          f"{nmh.max()}, pairs with >= 8 matches {(nmh >= 8).sum()}", flush=True)
    # the subset: every (P // subset)-th pair
    step = max(P // max(args.subset, 1), 1)
    sel = np.arange(0, P, step)[:args.subset]
    sp = np.ascontiguousarray(pairs[sel])
    spt = torch.from_numpy(sp).to(dev)
    seld = torch.from_numpy(sel).to(dev)
    smm, snm = mm[seld].contiguous(), nm[seld].contiguous()
    K = len(sel)
    print(f"subset: {K} pairs (every {step}-th of the schedule), distinct match counts {len(set(nmh[sel].tolist()))}",
          flush=True)

    def new(conf, p, m, n):
        return lambda: S.verify_matches(cache, p, (m, None, n), threshold=args.threshold, max_iterations=args.iters,
                                        confidence=conf)

    routes = {"new_fixed": new(None, spt, smm, snm), "new_stop": new(0.98, spt, smm, snm)}
    if not args.no_parent:
        routes["parent"] = lambda: parent_route(torch, pose, cache.slots, sp, smm, snm, args.iters, args.threshold, dev)
    runs = {k: [] for k in routes}
    ev = {k: [] for k in routes}
    last = {}
    for r in range(args.warmup + args.reps):
        for k, fn in routes.items():   # interleaved: one run of each route per round
            out, ms, ems = wall(fn)
            last[k] = out
            if r >= args.warmup:
                runs[k].append(ms)
                ev[k].append(ems)
            print(f"  round {r}{' (warm-up)' if r < args.warmup else ''} {k}: {ms:.1f} ms wall, {ems:.1f} ms events",
                  flush=True)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    res = {"frames": N, "pairs": P, "cap": cap, "iters": args.iters, "threshold": args.threshold, "subset": K,
           "subset_step": step, "match_all_ms": match_ms,
           "subset_ms_runs": {k: [round(t, 2) for t in v] for k, v in runs.items()},
           "subset_ms_median": med, "subset_events_ms_median": {k: float(np.median(v)) for k, v in ev.items()},
           "scaled_to_full_ms": {k: v * P / K for k, v in med.items()}}
    vf, vs = last["new_fixed"], last["new_stop"]
    res["subset_verified"] = {"new_fixed": int(vf.verified.sum()), "new_stop": int(vs.verified.sum())}
    res["subset_inliers"] = {"new_fixed": int(vf.keep.sum()), "new_stop": int(vs.keep.sum())}
    res["subset_samples_mean"] = {"new_fixed": float(vf.samples.mean()), "new_stop": float(vs.samples.mean())}
    if "parent" in last:
        res["subset_inliers"]["parent"] = int(last["parent"][0].sum())
        res["parent_phases_ms"] = {k: round(1e3 * v, 1) for k, v in last["parent"][1].items()}
        res["new_fixed_over_parent"] = med["new_fixed"] / med["parent"]
    print(json.dumps({"bench_verify_subset": res}), flush=True)
    # the whole schedule through the new call
    full = {}
    for name, conf, key in (("new_stop", 0.98, "new_stop"), ("new_fixed", None, "new_fixed")):
        predicted = med[key] * P / K / 1e3
        if predicted > args.full_budget:
            print(f"full schedule {name}: skipped, the subset predicts {predicted:.0f} s per run", flush=True)
            continue
        fn = new(conf, pt, mm, nm)
        fn()
        ts = []
        for _ in range(args.reps):
            v, ms, ems = wall(fn)
            ts.append(ems)
        full[name] = {"events_ms_runs": [round(t, 2) for t in ts], "events_ms_median": float(np.median(ts)),
                      "verified": int(v.verified.sum()), "inliers": int(v.keep.sum()),
                      "samples_mean": float(v.samples.mean())}
        print(f"full schedule {name}: {full[name]}", flush=True)
        tr, tms, tems = wall(lambda: S.build_tracks(cache, pt, (mm, None, nm), keep=v.keep_dev))
        tr, tms, tems = wall(lambda: S.build_tracks(cache, pt, (mm, None, nm), keep=v.keep_dev))
        full[name]["build_tracks_events_ms"] = tems
        full[name]["tracks"] = tr.stats
        print(f"  build_tracks with that mask: {tems:.2f} ms, {tr.stats}", flush=True)
    print(json.dumps({"bench_verify_full": full}), flush=True)


if __name__ == "__main__":
    main()
