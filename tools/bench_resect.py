"""Resection timing (diagnostic, not part of bench.py).  The job: a resident table of --slots slots
at cap --cap, about --links links per slot from seeded planted scenes (tests/pnp_ref.py scene, 30 %
outliers, a pose per slot) scattered among rows that are not links, all but two slots without a
pose, --iters samples per slot.  Timed between HIP events after one warm-up round, the two routes
alternating window by window in the same process, each on preallocated outputs:

  resect      sfm_resect_tracks_dev, one call for the whole table
  per_frame   what the parent commit offers for the same work: a torch gather of each unposed
              frame's links (node_track -> X, the mask's nonzero, which synchronises) followed by
              sfm_pnp_ransac_dev, one frame after another

The sample streams differ (the counter stream against numpy's, uploaded per (n, iters)); the work
per sample does not.  Reported: median and min-max per route, the frames each route posed (at
least --min-inliers inliers) and the wall time of one round.  Nothing is asserted on the figures.
Writes profiles/resect_bench.txt (or --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_table(np, PR, RR, slots, cap, links, frac, seed):
    rng = np.random.default_rng(seed)
    xy = rng.integers(0, 540, (slots, cap, 2)).astype(np.int32)
    node_track = np.full((slots, cap), -1, np.int32)
    count = np.zeros(slots, np.int32)
    Xs, Ks, T = [], [], 0
    for s in range(slots):
        n = int(links + rng.integers(-links // 20, links // 20 + 1))
        K = PR.K_SKEW if s % 3 == 2 else PR.K_SCENE
        R, t = RR.slot_pose(s % 12)
        X, x, _, _, _ = PR.scene(seed + s, n, frac, K=K, R=R, t=t)
        c = min(cap, n + int(rng.integers(cap // 4, cap // 2)))
        pos = np.sort(rng.choice(c, n, replace=False))
        node_track[s, pos] = T + np.arange(n)
        xy[s, pos] = x.astype(np.int32)
        count[s] = c
        Xs.append(X)
        Ks.append(K)
        T += n
    return xy, count, node_track, np.concatenate(Xs), np.array(Ks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--cap", type=int, default=2500)
    ap.add_argument("--links", type=int, default=1000)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--iters", type=int, default=248)
    ap.add_argument("--threshold", type=float, default=8.0)
    ap.add_argument("--min-inliers", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resect_bench.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from sfmfromscratch_amd import _abi, pose
    from sfmfromscratch_amd._native import context_for
    from tests import pnp_ref as PR
    from tests import resect_ref as RR
    if not torch.cuda.is_available():
        raise SystemExit("bench_resect.py measures on the device: no GPU found")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    ctx = context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), 0)
    N, cap = args.slots, args.cap
    t0 = time.perf_counter()
    xy_h, count_h, nt_h, X_h, K_h = build_table(np, PR, RR, N, cap, args.links, args.outliers, 1000)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    xy, count, nt, X, K = up(xy_h), up(count_h), up(nt_h), up(X_h), up(K_h.reshape(N, 9))
    T = int(X.shape[0])
    posed = np.zeros(N, bool)
    posed[:2] = True
    attempt = up((~posed).astype(np.uint8))
    say(f"{N} slots at cap {cap}, {T} tracks, links per slot {int((nt_h >= 0).sum(1).min())}..{int((nt_h >= 0).sum(1).max())}, "
        f"{int((~posed).sum())} slots without a pose, {args.iters} samples; built in {time.perf_counter() - t0:.1f} s")

    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)   # noqa: E731
    rt, rstat, rcost, rkeep = z((N, 12), torch.float64), z((N, 8), torch.int32), z((N, 2), torch.float64), z((N, cap), torch.uint8)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def resect():
        ctx.resect_tracks_dev(xy, count, nt, X, T, K, attempt, args.iters, args.threshold, args.min_inliers, 5,
                              pose.REFINE_MAX_ITER, rt, rstat, rcost, rkeep, None, None, stream)

    held = {}

    def per_frame():
        outs = []
        for s in np.flatnonzero(~posed):
            t = nt[s, :int(count_h[s])].long()
            ok = (t >= 0) & (t < T)
            Xg = X[t.clamp(0, T - 1)]
            ok &= torch.isfinite(Xg).all(dim=1)
            rows = ok.nonzero().reshape(-1)          # (the gather's size is a host value: this synchronises)
            o = pose._pnp_ransac_dev(Xg[rows].contiguous(), xy[s, rows].double().contiguous(), K[s].contiguous(),
                                     args.iters, args.threshold, pose.REFINE_MAX_ITER, dev, ctx)
            outs.append((s, o["n"]))
        held["n"] = outs

    routes = {"resect": resect, "per_frame": per_frame}
    runs = {k: [] for k in routes}
    wall = {k: [] for k in routes}
    for r in range(args.warmup + args.reps):
        for k, fn in routes.items():   # alternating: one window of each route per round
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                runs[k].append(e0.elapsed_time(e1) / args.inner)
                wall[k].append(1e3 * (time.perf_counter() - w0) / args.inner)
    st = rstat.cpu().numpy()
    n_frame = np.array([int(n.cpu()[0]) for _, n in held["n"]])
    res = {"slots": N, "cap": cap, "tracks": T, "unposed": int((~posed).sum()), "iters": args.iters,
           "threshold": args.threshold, "min_inliers": args.min_inliers, "reps": args.reps, "inner": args.inner,
           "events_ms_per_call": {k: {"median": round(float(np.median(v)), 3), "min": round(min(v), 3),
                                      "max": round(max(v), 3)} for k, v in runs.items()},
           "wall_ms_per_call": {k: round(float(np.median(v)), 3) for k, v in wall.items()},
           "posed": {"resect": int(st[:, 4].sum()), "per_frame": int((n_frame >= max(args.min_inliers, 1)).sum())},
           "inliers_mean": {"resect": float(st[st[:, 4] != 0, 0].mean()) if st[:, 4].any() else 0.0,
                            "per_frame": float(n_frame[n_frame > 0].mean()) if (n_frame > 0).any() else 0.0}}
    for k, v in res["events_ms_per_call"].items():
        say(f"{k}: {v['median']:.3f} ms per table (min {v['min']:.3f}, max {v['max']:.3f}; HIP events, {args.reps} "
            f"windows of {args.inner} calls; wall {res['wall_ms_per_call'][k]:.3f} ms), posed {res['posed'][k]} of "
            f"{res['unposed']}")
    say(json.dumps({"bench_resect": res}))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
