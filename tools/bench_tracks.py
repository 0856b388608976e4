"""Feature-track timing (diagnostic, not part of bench.py): device time between HIP events of one
sfm_build_tracks_dev call on the matches of N synthetic frames (synth.py, extracted and matched
on the device as bench.py's all-pairs job does), for two schedules:

  all     BASELINE configs[2]'s shape: 256 slots, all 32,640 pairs
  window  consecutive plus a window of 4: every pair with j - i <= 4

after --warmup calls (the first also sizes the workspace); every run's time is printed, the
median is the figure.  The match tensors are already resident; nothing is copied inside the
timed span.

The host path is timed on the same graph and the same machine: download the match tensors
(matches [P][cap][2], nmatch, count), assemble the edge list with numpy, and run
scipy.sparse.csgraph.connected_components.  That is what a user of the library does today; it
stops at the component labels (the consistency filter and the CSR would come on top), so the
comparison favours the host.  The labels are checked against the device's node_track."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P_OCT = {"num_interest_points": 2500, "ksize": 3, "gaussian_size": 7, "sigma": 6, "alpha": 0.05,
         "feature_width": 18, "pyramid_level": 4, "pyramid_scale_factor": 2}


def host_components(mm, nm, count, pairs, cap):
    """Download + numpy edge list + scipy connected_components -> (labels [N], seconds by phase)."""
    import numpy as np
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    m, n, c = mm.cpu().numpy(), nm.cpu().numpy(), count.cpu().numpy()
    t1 = time.perf_counter()
    P = len(pairs)
    live = np.arange(cap)[None, :] < np.clip(n[:P], 0, cap)[:, None]
    p, k = np.nonzero(live)
    s0, s1 = pairs[p, 0].astype(np.int64), pairs[p, 1].astype(np.int64)
    r0, r1 = m[p, k, 0].astype(np.int64), m[p, k, 1].astype(np.int64)
    ok = (s0 != s1) & (r0 >= 0) & (r0 < c[s0]) & (r1 >= 0) & (r1 < c[s1])
    a, b = (s0 * cap + r0)[ok], (s1 * cap + r1)[ok]
    N = len(c) * cap
    t2 = time.perf_counter()
    _, labels = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(N, N)), directed=False)
    t3 = time.perf_counter()
    return labels, len(a), {"download": t1 - t0, "edges": t2 - t1, "components": t3 - t2, "total": t3 - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--schedules", default="all,window")
    ap.add_argument("--min-len", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from sfmfromscratch_amd import sequence as S, synth
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
    out = {}
    for name in args.schedules.split(","):
        pairs = S.pair_schedule(N, "all" if name == "all" else args.window)
        P = len(pairs)
        pt = torch.from_numpy(pairs).to(dev)
        mm = torch.zeros((P, cap, 2), dtype=torch.int32, device=dev)
        cc = torch.zeros((P, cap), dtype=torch.float32, device=dev)
        nm = torch.zeros(P, dtype=torch.int32, device=dev)
        matcher.prep(cache.slots)
        for a in range(0, P, 4096):
            matcher.match(cache.slots, pt[a:a + 4096], out=(mm[a:a + 4096], cc[a:a + 4096], nm[a:a + 4096]),
                          prepped=True)
        torch.cuda.synchronize()
        del cc
        tr = None
        for _ in range(args.warmup):
            tr = S.build_tracks(cache, pt, (mm, None, nm), min_len=args.min_len)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr = S.build_tracks(cache, pt, (mm, None, nm), min_len=args.min_len)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        hs = []
        for _ in range(args.host_reps):
            labels, n_edges, h = host_components(mm, nm, cache.slots.count, pairs, cap)
            hs.append(h)
        # the host's partition is the device's: nodes of one kept track share a label, tracks differ
        nt = tr.node_track.ravel()
        kept = nt >= 0
        first = np.full(tr.n_tracks, -1, np.int64)
        first[nt[kept]] = labels[kept]
        assert (labels[kept] == first[nt[kept]]).all() and len(set(first.tolist())) == tr.n_tracks
        med_h = sorted(hs, key=lambda d: d["total"])[len(hs) // 2]
        line = {"schedule": name, "frames": N, "pairs": P, "cap": cap, "edges": n_edges, **tr.stats,
                "device_ms_median": float(np.median(ts)), "device_ms_runs": [round(t, 4) for t in ts],
                "host_ms_median": 1e3 * med_h["total"],
                "host_ms_runs": [round(1e3 * h["total"], 2) for h in hs],
                "host_ms_phases": {k: round(1e3 * v, 2) for k, v in med_h.items()}}
        out[name] = line
        print(f"tracks {name}: {P} pairs, {n_edges} edges -> {tr.n_tracks} tracks, {tr.n_obs} observations "
              f"(longest {tr.stats['max_len']}, inconsistent {tr.stats['inconsistent']}): device "
              f"{line['device_ms_median']:.3f} ms median of {args.reps} (min {min(ts):.3f}, max {max(ts):.3f}); host "
              f"{line['host_ms_median']:.1f} ms median of {args.host_reps} (download "
              f"{1e3 * med_h['download']:.1f}, edges {1e3 * med_h['edges']:.1f}, scipy "
              f"{1e3 * med_h['components']:.1f})", flush=True)
        del mm, nm
    print(json.dumps({"bench_tracks": out}), flush=True)


if __name__ == "__main__":
    main()
