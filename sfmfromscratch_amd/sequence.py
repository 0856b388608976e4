"""Stage 1 of SFMRunner (Runner.py:176-191) on the device: every frame extracted once into a
resident descriptor table, then the pair schedule matched from it.

The reference runs `corner_detect_and_matching_process(i1, i1 + 1)` for every
consecutive pair on an 8-thread pool (Runner.py:183-191, 336-355); each task builds a
FeatureRunner, so every interior frame is decoded, resized and extracted twice, and the
ThreadPool's Python work serialises on the GIL.  Here:

* `FeatureCache` decodes each frame once on the host, ingests it on the device
  (PIL BICUBIC x scale + _rgb2gray, ingest.hip) and extracts it once, in batches, into
  one slot table (xy, desc, count) that stays resident — the descriptor-table cache;
* `match_schedule` matches any pair schedule (the reference's consecutive pairs, all
  pairs, or a sliding window) from that table in large batched launches;
* `stage1` mirrors what SFMRunner.perform leaves in `all_matches` after its thread pool:
  `all_matches[i1][i2] = Matches(matches, confidences, p1, p2, K1, K2)` and the swapped
  entry `[i2][i1]` (Runner.py:354-355), with p1 / p2 from _convert_matches_to_coords
  (Runner.py:423-434, first 2,500 matches).  With `ransac=True` the RANSAC inlier
  filter the reference applies to every pair but (1, 2) (Runner.py:349-351) runs on the
  device for all pairs at once (pose.find_inliers_batch); otherwise p1 /
  p2 are the pre-RANSAC correspondences.  EXIF intrinsics (CameraPose.construct_K) are
  out of scope: K is the caller's `single_K` (or None).

Feature tables and matches are saved / loaded as .npz (the
reference's own output format is np.savez, Runner.py:357-359).

Semantics are the batch path's: a pyramid level that yields exactly one keypoint is
stored as one keypoint (the drop-in ScaleRotInvSIFT reproduces the reference's ragged
`extend` of such a level instead, ScaleRotInvSIFT.py:103).
"""
from __future__ import annotations

import numpy as np

from .pose import PNP_THRESHOLD
from .runner import convert_matches_to_coords, drop_opaque_alpha, load_image_u8


class Matches:
    """Runner.Matches (Runner.py:118-125)."""

    def __init__(self, matches, confidence, p1, p2, K1, K2):
        self.matches = matches
        self.confidence = confidence
        self.p1 = p1
        self.p2 = p2
        self.K1 = K1
        self.K2 = K2


def pair_schedule(n: int, schedule="consecutive") -> np.ndarray:
    """Frame-index pairs (i, j), i < j: "consecutive" (Runner.py:183), "all", or an int w
    for every pair with j - i <= w."""
    if schedule == "consecutive":
        schedule = 1
    if schedule == "all":
        i, j = np.triu_indices(n, k=1)
    else:
        w = int(schedule)
        if w < 1:
            raise ValueError("window must be >= 1")
        i, j = np.triu_indices(n, k=1)
        keep = (j - i) <= w
        i, j = i[keep], j[keep]
    return np.stack([i, j], axis=1).astype(np.int32)


class FeatureCache:
    """Descriptor-table cache: frames extracted once, resident on the device.

    `frames` are decoded frames — [H, W, 3] uint8 RGB (ingested on the device with the
    reference's resize + gray conversion, Runner.py:33-46) or [H, W] float32 gray images
    (used as given) — or image paths (decoded with PIL on the host)."""

    def __init__(self, frames, extractor_params: dict | None = None, scale_factor: float = 0.5,
                 batch: int = 32, device: int = 0):
        import torch
        from .pipeline import BatchExtractor, SlotTable, ingest_rgb
        self.torch = torch
        dev = torch.device("cuda", device)
        self.extractor = BatchExtractor(extractor_params, device=device)
        self.cap = self.extractor.cap
        n = len(frames)
        self.n = n
        self.slots = SlotTable(torch, max(n, 1), self.cap, dev)
        self.shapes = [None] * n
        loaded = []
        for f in frames:
            if isinstance(f, str):
                # a 2-D gray file fails in the reference's _rgb2gray (Runner.py:478), so it
                # fails here instead of being extracted at the wrong scale; opaque RGBA
                # files work there and here
                a = drop_opaque_alpha(load_image_u8(f), f)
            else:
                a = np.asarray(f)
                if a.ndim == 3:
                    a = drop_opaque_alpha(a)
                if a.ndim == 2 and a.dtype != np.float32:
                    raise ValueError("gray frames must be float32 [H, W] in [0, 1] (the extractor's input)")
            loaded.append(a)
        # group frames of one kind and size into batches (one launch sequence per batch)
        groups: dict = {}
        for i, a in enumerate(loaded):
            key = (a.dtype.str, a.shape)
            groups.setdefault(key, []).append(i)
        for (_, shape), idx in groups.items():
            for b0 in range(0, len(idx), batch):
                chunk = idx[b0:b0 + batch]
                arr = np.stack([loaded[i] for i in chunk])
                t = torch.from_numpy(arr).to(dev)
                if t.dim() == 4:  # decoded RGB -> device ingest
                    if t.dtype != torch.uint8 or t.shape[3] != 3:
                        raise ValueError("RGB frames must be [H, W, 3] uint8")
                    gray = ingest_rgb(self.extractor.ctx, t, scale_factor)
                elif t.dim() == 3:
                    gray = t
                else:
                    raise ValueError("frames must be [H, W, 3] uint8 RGB or [H, W] gray")
                sel = torch.tensor(chunk, device=dev)
                tmp = self.extractor.extract(gray.contiguous())
                self.slots.xy.index_copy_(0, sel, tmp.xy)
                self.slots.desc.index_copy_(0, sel, tmp.desc)
                self.slots.count.index_copy_(0, sel, tmp.count)
                for i in chunk:
                    self.shapes[i] = tuple(gray.shape[1:])
        torch.cuda.synchronize(dev)

    # host views of one frame's features (the reference's X, Y, descriptors)
    def keypoints(self, i: int):
        n = int(self.slots.count[i].item())
        xy = self.slots.xy[i, :n].cpu().numpy().astype(np.int64)
        return xy[:, 0], xy[:, 1]

    def descriptors(self, i: int) -> np.ndarray:
        n = int(self.slots.count[i].item())
        return self.slots.desc[i, :n].cpu().numpy()

    def save(self, path: str) -> None:
        """Features of every frame as .npz: counts, offsets, X, Y (int64), desc (float32)."""
        counts = self.slots.count.cpu().numpy().astype(np.int64)[: self.n]
        xy = self.slots.xy.cpu().numpy()
        desc = self.slots.desc.cpu().numpy()
        save_features(path, [xy[i, :counts[i], 0] for i in range(self.n)],
                      [xy[i, :counts[i], 1] for i in range(self.n)],
                      [desc[i, :counts[i]] for i in range(self.n)])


def save_features(path: str, X: list, Y: list, D: list) -> None:
    """Per-frame keypoints + descriptors as one .npz (concatenated, with offsets)."""
    counts = np.array([len(x) for x in X], np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    np.savez(path, format=np.array("sfmfeat-features-v1"), counts=counts, offsets=off,
             X=np.concatenate([np.asarray(x, np.int64) for x in X]) if len(X) else np.zeros(0, np.int64),
             Y=np.concatenate([np.asarray(y, np.int64) for y in Y]) if len(Y) else np.zeros(0, np.int64),
             desc=np.concatenate([np.asarray(d, np.float32).reshape(-1, 128) for d in D]) if len(D)
             else np.zeros((0, 128), np.float32))


def load_features(path: str):
    """-> (X list, Y list, desc list) as written by save_features."""
    with np.load(path, allow_pickle=False) as z:
        if str(z["format"]) != "sfmfeat-features-v1":
            raise ValueError(f"{path}: not an sfmfeat feature file")
        off = z["offsets"]
        X, Y, D = z["X"], z["Y"], z["desc"]
        return ([X[off[i]:off[i + 1]] for i in range(len(off) - 1)],
                [Y[off[i]:off[i + 1]] for i in range(len(off) - 1)],
                [D[off[i]:off[i + 1]] for i in range(len(off) - 1)])


def save_matches(path: str, pairs: np.ndarray, results: list) -> None:
    """Per-pair (matches (k,2) int64, confidences (k,) float32) as one .npz."""
    counts = np.array([len(c) for _, c in results], np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    m = [np.asarray(mm, np.int64).reshape(-1, 2) for mm, _ in results]
    c = [np.asarray(cc, np.float32).reshape(-1) for _, cc in results]
    np.savez(path, format=np.array("sfmfeat-matches-v1"), pairs=np.asarray(pairs, np.int32), offsets=off,
             matches=np.concatenate(m) if m else np.zeros((0, 2), np.int64),
             conf=np.concatenate(c) if c else np.zeros(0, np.float32))


def load_matches(path: str):
    """-> (pairs, [(matches, conf), ...]); empty pairs come back as the reference's
    float64 (0,) arrays (NNRatioFeatureMatcher.py:53-60)."""
    with np.load(path, allow_pickle=False) as z:
        if str(z["format"]) != "sfmfeat-matches-v1":
            raise ValueError(f"{path}: not an sfmfeat match file")
        off, m, c = z["offsets"], z["matches"], z["conf"]
        res = []
        for p in range(len(off) - 1):
            if off[p + 1] == off[p]:
                res.append((np.array([]), np.array([])))
            else:
                res.append((m[off[p]:off[p + 1]], c[off[p]:off[p + 1]]))
        return z["pairs"], res


def match_schedule(cache: FeatureCache, pairs: np.ndarray, ratio_threshold: float = 0.85, chunk: int = 4096):
    """Match every (i, j) of `pairs` from the resident table; returns per pair
    (matches (k,2) int64, confidences (k,) float32) exactly as
    NNRatioFeatureMatcher.match_features_ratio_test on the two frames' descriptors,
    including its float64 (0,) empty results.  Raises IndexError like the reference
    when a pair's second frame has fewer than 2 keypoints."""
    torch = cache.torch
    from .pipeline import BatchMatcher
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    dev = cache.slots.desc.device
    m = BatchMatcher(ratio_threshold, device=dev.index, ctx=cache.extractor.ctx)
    out = []
    for a in range(0, len(pairs), chunk):
        pt = torch.from_numpy(pairs[a:a + chunk]).to(dev)
        mm, cc, nm = m.match(cache.slots, pt)
        nm = nm.cpu().numpy()
        mm = mm.cpu().numpy()
        cc = cc.cpu().numpy()
        for p in range(len(pt)):
            k = int(nm[p])
            if k < 0:
                raise IndexError("index 1 is out of bounds (fewer than 2 target descriptors)")
            if k == 0:
                out.append((np.array([]), np.array([])))
            else:
                out.append((mm[p, :k].astype(np.int64), cc[p, :k].astype(np.float32)))
    return out


def stage1(img_path: str, max_img: int, extractor_params: dict, match_threshold: float = 0.85,
           single_K=None, scale_factor: float = 0.5, num_matches: int = 2500, device: int = 0,
           ransac: bool = False, ransac_max_it: int | None = None):
    """SFMRunner.perform's stage 1 (Runner.py:183-191): frames "{img_path}/{i}.jpg" for
    i = 1..max_img, consecutive pairs; returns all_matches[(max_img+1) x (max_img+1)] of
    Matches as the reference fills it (Runner.py:174-175, 354-355).  With ransac=True the
    pairs other than (1, 2) get the reference's inlier filter (Runner.py:349-351,
    pose.find_inliers with max_iterations = ransac_max_it, default
    calculate_num_ransac_iterations(0.98, 8, 0.4) as Runner.py:170), all pairs in one
    device pass; a pair with fewer than 8 correspondences raises ValueError, as the
    reference's tuple unpacking of find_inliers' four Nones does."""
    paths = ["{}/{}.jpg".format(img_path, i) for i in range(1, max_img + 1)]
    cache = FeatureCache(paths, extractor_params, scale_factor=scale_factor, device=device)
    pairs = pair_schedule(max_img, "consecutive")
    res = match_schedule(cache, pairs, match_threshold)
    all_matches = [[None for _ in range(max_img + 1)] for _ in range(max_img + 1)]
    coords = []
    for (a, b), (mm, cc) in zip(pairs, res):
        X1, Y1 = cache.keypoints(int(a))
        X2, Y2 = cache.keypoints(int(b))
        coords.append(convert_matches_to_coords(mm, X1, Y1, X2, Y2, num_matches))
    if ransac:
        from . import pose
        iters = ransac_max_it if ransac_max_it is not None else pose.calculate_num_ransac_iterations(0.98, 8, 0.4)
        sel = [k for k, (a, b) in enumerate(pairs) if (int(a) + 1, int(b) + 1) != (1, 2)]
        filt = pose.find_inliers_batch([coords[k] for k in sel], max_iterations=iters, device=device)
        for k, r in zip(sel, filt):
            if len(r) != 2:
                raise ValueError("too many values to unpack (expected 2)")  # Runner.py:351 on four Nones
            coords[k] = r
    for k, ((a, b), (mm, cc)) in enumerate(zip(pairs, res)):
        i1, i2 = int(a) + 1, int(b) + 1
        p1, p2 = coords[k]
        all_matches[i1][i2] = Matches(mm, cc, p1, p2, single_K, single_K)
        all_matches[i2][i1] = Matches(mm, cc, p2, p1, single_K, single_K)
    return all_matches, cache


# ---------------- feature tracks (tracks.hip) ----------------

TRACK_STATS = ("n_tracks", "n_obs", "inconsistent", "short", "skipped_edges", "max_len")


class Tracks:
    """The feature tracks of a match graph (include/sfmfeat.h sfm_build_tracks_dev): a CSR by
    track of (slot, row) observations, ascending by slot within a track, tracks in ascending
    order of their smallest node id slot * cap + row.  The device tensors stay resident
    (`offsets_dev`, `obs_slot_dev`, `obs_row_dev`, `node_track_dev`, `xy`: the slot table's
    pixels); the numpy properties copy on first use, which synchronises."""

    def __init__(self, offsets, obs_slot, obs_row, node_track, out_n, xy, min_len: int = 2, count=None):
        self._offsets, self._obs_slot, self._obs_row = offsets, obs_slot, obs_row
        self.node_track_dev, self._out_n, self.xy, self.min_len = node_track, out_n, xy, int(min_len)
        self.count_dev = count   # the slot table's count [nimg] (None: loaded tracks, every row counts)
        self._host = {}

    def _stat(self):
        if "stats" not in self._host:
            self._host["stats"] = self._out_n.cpu().numpy().astype(np.int64)
        return self._host["stats"]

    def _np(self, key, t):
        if key not in self._host:
            self._host[key] = t.cpu().numpy()
        return self._host[key]

    @property
    def stats(self) -> dict:
        """n_tracks, n_obs, inconsistent and short components, skipped edges, the longest track."""
        return dict(zip(TRACK_STATS, (int(v) for v in self._stat())))

    @property
    def n_tracks(self) -> int:
        return int(self._stat()[0])

    @property
    def n_obs(self) -> int:
        return int(self._stat()[1])

    @property
    def offsets_dev(self):
        return self._offsets[: self.n_tracks + 1]

    @property
    def obs_slot_dev(self):
        return self._obs_slot[: self.n_obs]

    @property
    def obs_row_dev(self):
        return self._obs_row[: self.n_obs]

    @property
    def offsets(self) -> np.ndarray:
        return self._np("offsets", self.offsets_dev)

    @property
    def obs_slot(self) -> np.ndarray:
        return self._np("obs_slot", self.obs_slot_dev)

    @property
    def obs_row(self) -> np.ndarray:
        return self._np("obs_row", self.obs_row_dev)

    @property
    def node_track(self) -> np.ndarray:
        return self._np("node_track", self.node_track_dev)

    @property
    def obs_xy(self) -> np.ndarray:
        """[n_obs, 2] int32: the pixel of every observation."""
        if "obs_xy" not in self._host:
            s, r = self.obs_slot_dev.long(), self.obs_row_dev.long()
            self._host["obs_xy"] = self.xy[s, r].cpu().numpy()
        return self._host["obs_xy"]

    def ba_inputs(self):
        """(camera_indices [n_obs], point_indices [n_obs], points_2d [n_obs, 2]) as
        pose.BundleAdjustment and PointRegistry.prepare_for_ba take them: the camera of an
        observation is its slot, its point is its track."""
        point_indices = np.repeat(np.arange(self.n_tracks, dtype=np.int64), np.diff(self.offsets))
        return self.obs_slot.astype(np.int64), point_indices, self.obs_xy.astype(np.float64)

    def save(self, path: str) -> None:
        """The tracks as one .npz (the style of save_matches), format tag sfmfeat-tracks-v1."""
        np.savez(path, format=np.array("sfmfeat-tracks-v1"), offsets=self.offsets, obs_slot=self.obs_slot,
                 obs_row=self.obs_row, node_track=self.node_track, obs_xy=self.obs_xy, stats=self._stat(),
                 min_len=np.array(self.min_len, np.int64))

    @classmethod
    def load(cls, path: str, device: int = 0) -> "Tracks":
        """Tracks as written by `save`, uploaded to `device`; `xy` holds the saved observations'
        pixels and zeros elsewhere."""
        import torch
        with np.load(path, allow_pickle=False) as z:
            if str(z["format"]) != "sfmfeat-tracks-v1":
                raise ValueError(f"{path}: not an sfmfeat track file")
            off, s, r, nt, oxy, st, ml = (z[k] for k in ("offsets", "obs_slot", "obs_row", "node_track", "obs_xy",
                                                          "stats", "min_len"))
        dev = torch.device("cuda", device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(dev)  # noqa: E731
        xy = torch.zeros(tuple(nt.shape) + (2,), dtype=torch.int32, device=dev)
        if len(s):
            xy[up(s).long(), up(r).long()] = up(oxy)
        return cls(up(off), up(s), up(r), up(nt), up(st), xy, int(ml))


def _padded_matches(torch, matches, keep, P, cap, dev, who="build_tracks"):
    """The host list of match_schedule (and an optional list of per-pair masks) in the padded
    device layout of sfm_match_pairs_dev: matches [P, cap, 2], nmatch [P], keep [P, cap] or None."""
    if len(matches) != P:
        raise ValueError(f"{who}: one (matches, confidences) entry per pair")
    mm = np.zeros((max(P, 1), cap, 2), np.int32)
    nm = np.zeros(max(P, 1), np.int32)
    kk = None if keep is None else np.zeros((max(P, 1), cap), np.uint8)
    for p, entry in enumerate(matches):
        m = np.asarray(entry[0] if isinstance(entry, (tuple, list)) else entry).reshape(-1, 2)
        if len(m) > cap:
            raise ValueError(f"{who}: pair {p} has {len(m)} matches, more than the table's capacity {cap}")
        mm[p, :len(m)] = m
        nm[p] = len(m)
        if kk is not None:
            k = np.asarray(keep[p]).reshape(-1)
            if len(k) != len(m):
                raise ValueError(f"{who}: keep[{p}] must have one entry per match of pair {p}")
            kk[p, :len(m)] = k != 0
    return (torch.from_numpy(mm).to(dev), torch.from_numpy(nm).to(dev),
            None if kk is None else torch.from_numpy(kk).to(dev))


def build_tracks(cache, pairs, matches, keep=None, min_len: int = 2) -> Tracks:
    """Feature tracks of the matches of a pair schedule: the connected components of the graph
    whose nodes are the table's keypoints and whose edges are the matches; a component that visits
    one frame twice is dropped whole, one with fewer than `min_len` keypoints too
    (include/sfmfeat.h sfm_build_tracks_dev has the rule in full).

    cache: the FeatureCache the matches came from (or its SlotTable).  pairs [P, 2].  matches:
    the device triple of BatchMatcher.match (matches [P, cap, 2], conf, nmatch), used in place, or
    the host list match_schedule returns, uploaded into that layout.  keep (optional): which
    matches count — [P, cap] (numpy or a device tensor, non-zero = keep), or with a host list one
    mask per pair; this is where geometric verification comes in: `verify_matches(...).keep_dev`
    is that mask, computed on the device, and a caller may pass one of its own.
    Enqueued on torch's current stream; nothing synchronises until a host property is read."""
    import torch
    from . import _abi
    from ._native import context_for
    slots = getattr(cache, "slots", cache)
    dev = slots.xy.device
    nimg, cap = int(slots.count.numel()), int(slots.xy.shape[1])
    extractor = getattr(cache, "extractor", None)
    ctx = extractor.ctx if extractor is not None else \
        context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), dev.index or 0)
    if isinstance(pairs, torch.Tensor):
        pt = pairs.to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    else:
        pt = torch.from_numpy(np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), np.int32)).to(dev)
    P = int(pt.shape[0])
    with torch.cuda.device(dev):
        if len(matches) == 3 and isinstance(matches[0], torch.Tensor):
            mm, nm = matches[0], matches[2]
            if mm.dim() != 3 or tuple(mm.shape[1:]) != (cap, 2) or int(mm.shape[0]) < P:
                raise ValueError(f"build_tracks: matches must be [P, {cap}, 2] for the table's capacity")
            kk = None
            if keep is not None:
                kk = keep if isinstance(keep, torch.Tensor) else torch.from_numpy(np.asarray(keep))
                if tuple(kk.shape) != (int(mm.shape[0]), cap) and tuple(kk.shape) != (P, cap):
                    raise ValueError(f"build_tracks: keep must be [P, {cap}]")
                kk = (kk != 0).to(device=dev, dtype=torch.uint8).contiguous()
        else:
            mm, nm, kk = _padded_matches(torch, matches, keep, P, cap, dev)
        N = nimg * cap
        offsets = torch.empty(N // 2 + 1, dtype=torch.int32, device=dev)
        obs_slot = torch.empty(N, dtype=torch.int32, device=dev)
        obs_row = torch.empty(N, dtype=torch.int32, device=dev)
        node_track = torch.empty((nimg, cap), dtype=torch.int32, device=dev)
        out_n = torch.empty(6, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ctx.build_tracks_dev(slots.count, cap, pt, mm, nm, kk, int(min_len), offsets, obs_slot, obs_row, node_track,
                             out_n, stream)
    return Tracks(offsets, obs_slot, obs_row, node_track, out_n, slots.xy, min_len, count=slots.count)


# ---------------- geometric verification (verify.hip) ----------------

class Verified:
    """What sfm_verify_matches_dev leaves for a pair schedule (include/sfmfeat.h has the rule).  The
    device tensors stay resident: `keep_dev` [P, cap] uint8 (the `keep` of build_tracks), `F_dev`
    [P, 9] float64 (each pair's winning F, NaN where no sample had an inlier), `stat_dev` [P, 4]
    int32.  The numpy properties copy on first use, which synchronises."""

    def __init__(self, keep, F, stat, pairs, matches, conf, nmatch):
        self.keep_dev, self.F_dev, self.stat_dev = keep, F, stat
        self._pairs, self._matches, self._conf, self._nmatch = pairs, matches, conf, nmatch
        self._host = {}

    def _np(self, key, t):
        if key not in self._host:
            self._host[key] = t.cpu().numpy()
        return self._host[key]

    @property
    def keep(self) -> np.ndarray:
        return self._np("keep", self.keep_dev)

    @property
    def F(self) -> np.ndarray:
        """[P, 3, 3] float64."""
        return self._np("F", self.F_dev).reshape(-1, 3, 3)

    @property
    def stat(self) -> np.ndarray:
        return self._np("stat", self.stat_dev)

    @property
    def n_inliers(self) -> np.ndarray:
        """The winner's inlier count per pair (-1: the pair was not attempted)."""
        return self.stat[:, 0]

    @property
    def best_iter(self) -> np.ndarray:
        return self.stat[:, 1]

    @property
    def samples(self) -> np.ndarray:
        """Samples evaluated per pair (fewer than max_iterations where the early stop fired)."""
        return self.stat[:, 2]

    @property
    def verified(self) -> np.ndarray:
        return self.stat[:, 3] != 0

    def inlier_matches(self) -> list:
        """The host list of match_schedule with only the kept matches of each pair: (matches (k, 2)
        int64, confidences (k,) float32), the float64 (0,) arrays where nothing is kept.  The
        confidences are the caller's — the device triple's conf tensor, or the second entries of the
        host list; only where the caller gave none (a triple with conf=None, a list of bare match
        arrays) is every confidence 1."""
        P, keep = len(self.stat), self.keep
        mm = self._np("matches", self._matches)
        cc = self._conf
        if cc is not None and not isinstance(cc, np.ndarray):
            cc = self._np("conf", cc)
        out = []
        for p in range(P):
            sel = np.flatnonzero(keep[p])
            if len(sel) == 0:
                out.append((np.array([]), np.array([])))
            else:
                c = np.ones(len(sel), np.float32) if cc is None else cc[p, sel].astype(np.float32)
                out.append((mm[p, sel].astype(np.int64), c))
        return out


def verify_matches(cache, pairs, matches, threshold: float = 1.0, max_iterations: int | None = None,
                   confidence: float | None = 0.98, min_inliers: int = 16, seed: int = 5) -> Verified:
    """Two-view geometric verification of the matches of a pair schedule on the device: an 8-point
    RANSAC per pair (epipolar distance < `threshold` pixels) whose inlier mask is the `keep` of
    build_tracks — `build_tracks(cache, pairs, matches, keep=verify_matches(...).keep_dev)`
    (include/sfmfeat.h sfm_verify_matches_dev has the rule in full).

    cache, pairs, matches: as build_tracks takes them (the device triple of BatchMatcher.match, used
    in place, or the host list of match_schedule, uploaded).  max_iterations=None is
    pose.calculate_num_ransac_iterations(0.98, 8, 0.4), the runner's own 5,967.  confidence: a pair
    stops after a round of 256 samples once its best inlier ratio reaches the ratio at which the
    samples drawn so far contain an all-inlier one with this probability
    (pose.ransac_stop_ratios); None or 0 turns the early stop off.  min_inliers: a pair whose
    winner has fewer inliers keeps nothing; 16, twice the sample size, is this library's own
    default (the reference has no such step).  Samples depend on (seed, the pair's two slots, the
    sample's number) only.  Enqueued on torch's current stream; nothing synchronises until a host
    property of the result is read."""
    import torch
    from . import _abi, pose
    from ._native import context_for
    slots = getattr(cache, "slots", cache)
    dev = slots.xy.device
    nimg, cap = int(slots.count.numel()), int(slots.xy.shape[1])
    extractor = getattr(cache, "extractor", None)
    ctx = extractor.ctx if extractor is not None else \
        context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), dev.index or 0)
    if isinstance(pairs, torch.Tensor):
        pt = pairs.to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    else:
        pt = torch.from_numpy(np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), np.int32)).to(dev)
    P = int(pt.shape[0])
    iters = pose.calculate_num_ransac_iterations(0.98, 8, 0.4) if max_iterations is None else int(max_iterations)
    stop = None
    if confidence:
        stop = pose.ransac_stop_ratios(float(confidence), min(64, (max(iters, 0) + 255) // 256))
    with torch.cuda.device(dev):
        if len(matches) == 3 and isinstance(matches[0], torch.Tensor):
            mm, cc, nm = matches
            if mm.dim() != 3 or tuple(mm.shape[1:]) != (cap, 2) or int(mm.shape[0]) < P:
                raise ValueError(f"verify_matches: matches must be [P, {cap}, 2] for the table's capacity")
        else:
            mm, nm, _ = _padded_matches(torch, matches, None, P, cap, dev, who="verify_matches")
            cc = np.zeros((max(P, 1), cap), np.float32)   # the list's confidences stay on the host
            for p, entry in enumerate(matches):
                if isinstance(entry, (tuple, list)) and len(entry) > 1:
                    c = np.asarray(entry[1], np.float32).reshape(-1)
                    k = np.asarray(entry[0]).size // 2   # (host counts: nm is on the device already)
                    if len(c) != k:
                        raise ValueError(f"verify_matches: pair {p} has {k} matches and {len(c)} confidences")
                    cc[p, :len(c)] = c
                else:
                    cc = None   # a list of bare match arrays carries no confidences
                    break
        keep = torch.empty((P, cap), dtype=torch.uint8, device=dev)
        F = torch.empty((P, 9), dtype=torch.float64, device=dev)
        stat = torch.empty((P, 4), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ctx.verify_matches_dev(slots.xy, slots.count, pt, mm, nm, iters, float(threshold), int(min_inliers), int(seed),
                               stop, keep, F, stat, stream)
    return Verified(keep, F, stat, pt, mm, cc, nm)


# ---------------- two-view geometry (twoview.hip) ----------------

class TwoView:
    """The two-view geometry record of every pair of a schedule, as sfm_homography_matches_dev and
    sfm_two_view_pose_dev leave it (include/sfmfeat.h has both rules).  The device tensors stay
    resident: `H_dev` [P, 9] float64, `hstat_dev` [P, 4] int32, `hkeep_dev` [P, cap] uint8 (the
    homography's inlier mask), `pose_dev` [P, 12] float64 (R row-major, then t), `pstat_dev` [P, 4]
    int32.  The numpy properties copy on first use, which synchronises."""

    def __init__(self, H, hstat, hkeep, pose, pstat, verified_stat, planar_ratio):
        self.H_dev, self.hstat_dev, self.hkeep_dev, self.pose_dev, self.pstat_dev = H, hstat, hkeep, pose, pstat
        self._vstat, self.planar_ratio = verified_stat, float(planar_ratio)
        self._host = {}

    def _np(self, key, t):
        if key not in self._host:
            self._host[key] = t.cpu().numpy()
        return self._host[key]

    @property
    def H(self) -> np.ndarray:
        """[P, 3, 3] float64: the homography RANSAC's winner (NaN where it had no inlier)."""
        return self._np("H", self.H_dev).reshape(-1, 3, 3)

    @property
    def n_homography(self) -> np.ndarray:
        """The homography's inlier count per pair (-1: not attempted)."""
        return self._np("hstat", self.hstat_dev)[:, 0]

    @property
    def R(self) -> np.ndarray:
        """[P, 3, 3]: the second camera's rotation relative to the first (NaN without a pose)."""
        return self._np("pose", self.pose_dev)[:, :9].reshape(-1, 3, 3)

    @property
    def t(self) -> np.ndarray:
        """[P, 3]: the unit translation that goes with R."""
        return self._np("pose", self.pose_dev)[:, 9:]

    @property
    def n_front(self) -> np.ndarray:
        """Inliers in front of both cameras under the chosen pose (-1: not attempted)."""
        return self._np("pstat", self.pstat_dev)[:, 0]

    @property
    def n_wide(self) -> np.ndarray:
        """Those of them whose parallax reaches min_parallax_deg."""
        return self._np("pstat", self.pstat_dev)[:, 2]

    @property
    def config(self) -> np.ndarray:
        """int8 per pair: 0 not verified; 1 general; 2 planar or panoramic (the homography explains
        at least planar_ratio of verify's inliers); 3 verified, but no candidate pose has a point in
        front of both cameras."""
        if "config" not in self._host:
            vs = self._np("vstat", self._vstat)
            out = np.zeros(len(vs), np.int8)
            ok = vs[:, 3] != 0
            planar = ok & (self.n_homography >= self.planar_ratio * vs[:, 0])
            out[ok] = 1
            out[ok & ~planar & (self._np("pstat", self.pstat_dev)[:, 1] < 0)] = 3
            out[planar] = 2
            self._host["config"] = out
        return self._host["config"]

    def initial_pair(self) -> int:
        """The index of the general pair with the most wide points, the lowest index on a tie; -1 if
        the schedule has no general pair."""
        general = np.flatnonzero(self.config == 1)
        if len(general) == 0:
            return -1
        return int(general[np.argmax(self.n_wide[general])])   # argmax: the first of the largest

    def seed(self, pairs, index=None):
        """(a, b, R [3, 3], t [3]) of pair `index` of the schedule `pairs` [P, 2] (None: initial_pair()),
        the seed_pair of `reconstruct`.  ValueError when the schedule has no general pair, the index is
        outside the schedule or that pair has no pose."""
        pairs = np.asarray(pairs.cpu() if hasattr(pairs, "cpu") else pairs).reshape(-1, 2)
        i = self.initial_pair() if index is None else int(index)
        if len(pairs) != len(self.R):
            raise ValueError(f"TwoView.seed: pairs has {len(pairs)} rows, the record {len(self.R)}: not its schedule")
        if i < 0 or i >= len(pairs):
            raise ValueError("TwoView.seed: the schedule has no such pair" if index is not None
                             else "TwoView.seed: the schedule has no general pair to start from")
        R, t = self.R[i], self.t[i]
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            raise ValueError(f"TwoView.seed: pair {i} has no relative pose")
        return int(pairs[i, 0]), int(pairs[i, 1]), R.copy(), t.copy()


def two_view_geometry(cache, pairs, matches, verified, K, h_threshold: float = 2.0, h_iterations: int | None = None,
                      confidence: float | None = 0.98, planar_ratio: float = 0.8, min_parallax_deg: float = 2.0,
                      seed: int = 5) -> TwoView:
    """The two-view geometry record of every verified pair of a schedule, on the device between
    verify_matches and build_tracks / triangulate_tracks: a homography RANSAC (symmetric transfer
    error < `h_threshold` pixels) whose inlier count, set against verify's, marks planar and
    rotation-only pairs; the relative pose (R, t) out of verify's F and the intrinsics, chosen by a
    cheirality count; and the number of inliers whose parallax reaches `min_parallax_deg`
    (include/sfmfeat.h sfm_homography_matches_dev and sfm_two_view_pose_dev have the rules).
    `TwoView.initial_pair()` names the pair to start a reconstruction from.

    cache, pairs, matches: as verify_matches took them.  verified: its result.  K: [3, 3], or
    [nimg, 3, 3] with one matrix per slot; a host array is uploaded, a device tensor used in place.
    h_iterations=None is pose.calculate_num_ransac_iterations(0.98, 4, 0.4) = 150.  confidence: the
    early stop of verify_matches, for four-point samples (None or 0: off).  planar_ratio=0.8 is
    COLMAP's max_H_inlier_ratio; the other defaults are this library's own: h_threshold is 2.0 px
    because keypoints are integer pixels in both images (at 1.0 px planar and rotation-only scenes
    land on either side of 0.8).  Only pairs that verify_matches verified are
    attempted.  Enqueued on torch's current stream; nothing synchronises until a host property of
    the result is read."""
    import math
    import torch
    from . import _abi, pose
    from ._native import context_for
    slots = getattr(cache, "slots", cache)
    dev = slots.xy.device
    nimg, cap = int(slots.count.numel()), int(slots.xy.shape[1])
    extractor = getattr(cache, "extractor", None)
    ctx = extractor.ctx if extractor is not None else \
        context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), dev.index or 0)
    if isinstance(pairs, torch.Tensor):
        pt = pairs.to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    else:
        pt = torch.from_numpy(np.ascontiguousarray(np.asarray(pairs).reshape(-1, 2), np.int32)).to(dev)
    P = int(pt.shape[0])
    if tuple(verified.stat_dev.shape) != (P, 4) or tuple(verified.keep_dev.shape) != (P, cap):
        raise ValueError(f"two_view_geometry: verified must be verify_matches' result for these {P} pairs")
    iters = pose.calculate_num_ransac_iterations(0.98, 4, 0.4) if h_iterations is None else int(h_iterations)
    stop = None
    if confidence:
        stop = pose.ransac_stop_ratios(float(confidence), min(64, (max(iters, 0) + 255) // 256), 4)
    if not 0.0 <= float(min_parallax_deg) <= 90.0:
        raise ValueError("two_view_geometry: min_parallax_deg must lie in [0, 90]")
    cos2_min = math.cos(math.radians(float(min_parallax_deg))) ** 2
    with torch.cuda.device(dev):
        if isinstance(K, torch.Tensor):
            Kt = K.to(device=dev, dtype=torch.float64)
        else:
            Kt = torch.from_numpy(np.ascontiguousarray(np.asarray(K, np.float64))).to(dev)
        if tuple(Kt.shape) == (3, 3):
            Kt = Kt.reshape(1, 9).expand(nimg, 9)
        elif tuple(Kt.shape) != (nimg, 3, 3):
            raise ValueError(f"two_view_geometry: K must be [3, 3] or [{nimg}, 3, 3]")
        Kt = Kt.reshape(nimg, 9).contiguous()
        if len(matches) == 3 and isinstance(matches[0], torch.Tensor):
            mm, nm = matches[0], matches[2]
            if mm.dim() != 3 or tuple(mm.shape[1:]) != (cap, 2) or int(mm.shape[0]) < P:
                raise ValueError(f"two_view_geometry: matches must be [P, {cap}, 2] for the table's capacity")
        else:
            mm, nm, _ = _padded_matches(torch, matches, None, P, cap, dev, who="two_view_geometry")
        attempt = verified.stat_dev[:, 3].contiguous()
        H = torch.empty((P, 9), dtype=torch.float64, device=dev)
        hkeep = torch.empty((P, cap), dtype=torch.uint8, device=dev)
        hstat = torch.empty((P, 4), dtype=torch.int32, device=dev)
        rt = torch.empty((P, 12), dtype=torch.float64, device=dev)
        pstat = torch.empty((P, 4), dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ctx.homography_matches_dev(slots.xy, slots.count, pt, mm, nm, attempt, iters, float(h_threshold), int(seed),
                                   stop, H, hkeep, hstat, stream)
        ctx.two_view_pose_dev(slots.xy, slots.count, pt, mm, nm, verified.keep_dev, verified.F_dev, Kt, attempt,
                              cos2_min, rt, pstat, stream)
    return TwoView(H, hstat, hkeep, rt, pstat, verified.stat_dev, planar_ratio)


# ---------------- resection from tracks and the reconstruction loop (resect.hip) ----------------

RESECT_STATS = ("n_inliers", "best_iter", "samples", "n_links", "posed", "status", "iters", "lm_iters")


class Resected:
    """What sfm_resect_tracks_dev leaves for every slot of a table (include/sfmfeat.h has the rule).
    The device tensors stay resident: `pose_dev` [nimg, 12] float64 (R row-major, then t; NaN
    without a pose), `rstat_dev` [nimg, 8] int32, `cost_dev` [nimg, 2] float64, `keep_dev`
    [nimg, cap] uint8 (1 at the rows that are links and inliers of a posed slot), `K_dev` [nimg, 9].
    The numpy properties copy on first use, which synchronises."""

    def __init__(self, pose, rstat, cost, keep, K):
        self.pose_dev, self.rstat_dev, self.cost_dev, self.keep_dev, self.K_dev = pose, rstat, cost, keep, K
        self._host = {}

    def _np(self, key, t):
        if key not in self._host:
            self._host[key] = t.cpu().numpy()
        return self._host[key]

    @property
    def stat(self) -> np.ndarray:
        """[nimg, 8] int32: best count, winning sample, samples, n_links, posed, LM status, accepted
        steps, LM iterations."""
        return self._np("rstat", self.rstat_dev)

    @property
    def R(self) -> np.ndarray:
        return self._np("pose", self.pose_dev)[:, :9].reshape(-1, 3, 3)

    @property
    def t(self) -> np.ndarray:
        return self._np("pose", self.pose_dev)[:, 9:]

    @property
    def P(self) -> np.ndarray:
        """[nimg, 3, 4]: K [R | t] (NaN without a pose)."""
        K = self._np("K", self.K_dev).reshape(-1, 3, 3)
        return K @ np.concatenate([self.R, self.t[:, :, None]], axis=2)

    @property
    def n_links(self) -> np.ndarray:
        return self.stat[:, 3]

    @property
    def n_inliers(self) -> np.ndarray:
        """The winner's inlier count per slot (-1: the slot was not attempted)."""
        return self.stat[:, 0]

    @property
    def posed(self) -> np.ndarray:
        return self.stat[:, 4] != 0

    @property
    def status(self) -> np.ndarray:
        """The refinement's status per slot (pose.REFINE_STATUS; -1 without a pose)."""
        return self.stat[:, 5]

    @property
    def cost(self) -> np.ndarray:
        """[nimg, 2]: the sum of squared residuals over the inliers before and after the refinement."""
        return self._np("cost", self.cost_dev)

    def next_views(self) -> np.ndarray:
        """The posed slots by descending n_inliers, the lowest slot first on a tie."""
        s = np.flatnonzero(self.posed)
        return s[np.argsort(-self.n_inliers[s].astype(np.int64), kind="stable")]


def _slot_K(torch, K, nimg, dev, who):
    """K [3, 3] or [nimg, 3, 3] -> [nimg, 9] float64 on the device; a host K is checked as
    pose._pnp_inputs checks it (a device K is checked by the kernel, slot by slot)."""
    if isinstance(K, torch.Tensor) and K.is_cuda:
        Kt = K.to(device=dev, dtype=torch.float64)
    else:
        Kh = np.asarray(K.numpy() if isinstance(K, torch.Tensor) else K, np.float64)
        if Kh.shape != (3, 3) and Kh.shape != (nimg, 3, 3):
            raise ValueError(f"{who}: K must be [3, 3] or [{nimg}, 3, 3]")
        Kf = Kh.reshape(-1, 9)
        if not np.isfinite(Kf).all():
            raise ValueError(f"{who}: K must be finite")
        if (Kf[:, [3, 6, 7]] != 0).any() or (Kf[:, [0, 4, 8]] == 0).any():
            raise ValueError(f"{who}: K must be upper triangular with a non-zero diagonal")
        Kt = torch.from_numpy(np.ascontiguousarray(Kh)).to(dev)
    if tuple(Kt.shape) == (3, 3):
        Kt = Kt.reshape(1, 9).expand(nimg, 9)
    elif tuple(Kt.shape) not in ((nimg, 3, 3), (nimg, 9)):   # ([nimg, 9]: this function's own result)
        raise ValueError(f"{who}: K must be [3, 3] or [{nimg}, 3, 3]")
    return Kt.reshape(nimg, 9).contiguous()


def _tracks_ctx(tracks):
    import torch
    from . import _abi
    from ._native import context_for
    dev = tracks.xy.device
    return context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), dev.index or 0), dev, \
        torch.cuda.current_stream(dev).cuda_stream


def resect_frames(tracks, X, K, posed=None, iterations=None, threshold: float = PNP_THRESHOLD, min_inliers: int = 12,
                  seed: int = 5) -> Resected:
    """The pose of every frame without one from the 2D-3D links its tracks give it, all frames in
    one call on the device (include/sfmfeat.h sfm_resect_tracks_dev has the rule in full): row r of
    slot s is linked to X[tracks.node_track[s][r]]; a 6-point RANSAC per slot over those links
    (reprojection error < `threshold` pixels), the winner refined on its inliers.

    tracks: build_tracks' result.  X [n_tracks, 3]: triangulate_tracks' points (numpy, uploaded, or a
    device tensor, used in place; NaN = no point).  K: [3, 3], or [nimg, 3, 3] with one matrix per
    slot; a host K must be finite and upper triangular with a non-zero diagonal (ValueError), a
    device K is used in place and a slot whose K is not is left unattempted.  posed (optional)
    [nimg]: the slots to skip.  iterations=None is pose.calculate_num_ransac_iterations(0.98, 6, 0.5)
    = 248.  threshold defaults to pose.PNP_THRESHOLD, 8 px.  min_inliers=12, twice the sample size,
    is how verify_matches chose its 16.  Samples depend on (seed, the slot, the sample's number) only.
    Enqueued on torch's current stream; nothing synchronises until a host property of the result is
    read."""
    import torch
    from . import pose
    ctx, dev, stream = _tracks_ctx(tracks)
    nimg, cap = int(tracks.xy.shape[0]), int(tracks.xy.shape[1])
    iters = pose.calculate_num_ransac_iterations(0.98, 6, 0.5) if iterations is None else int(iterations)
    thr = float(threshold)
    with torch.cuda.device(dev):
        Kt = _slot_K(torch, K, nimg, dev, "resect_frames")
        Xt = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(X, np.float64)))
        if Xt.dim() != 2 or Xt.shape[1] != 3:
            raise ValueError("resect_frames: X must be [n_tracks, 3]")
        Xt = Xt.to(device=dev, dtype=torch.float64).contiguous()
        T = int(Xt.shape[0])
        count = getattr(tracks, "count_dev", None)
        if count is None:
            count = torch.full((nimg,), cap, dtype=torch.int32, device=dev)
        attempt = None
        if posed is not None:
            pm = posed if isinstance(posed, torch.Tensor) else torch.from_numpy(np.asarray(posed))
            if pm.numel() != nimg:
                raise ValueError("resect_frames: posed must have one entry per slot")
            attempt = (pm.reshape(-1).to(dev) == 0).to(torch.uint8).contiguous()
        rt = torch.empty((nimg, 12), dtype=torch.float64, device=dev)
        rstat = torch.empty((nimg, 8), dtype=torch.int32, device=dev)
        rcost = torch.empty((nimg, 2), dtype=torch.float64, device=dev)
        rkeep = torch.empty((nimg, cap), dtype=torch.uint8, device=dev)
        ctx.resect_tracks_dev(tracks.xy, count, tracks.node_track_dev, Xt if T else None, T, Kt, attempt, iters, thr,
                              int(min_inliers), int(seed), pose.REFINE_MAX_ITER, rt, rstat, rcost, rkeep, None, None,
                              stream)
    return Resected(rt, rstat, rcost, rkeep, Kt)


class Reconstruction:
    """What `reconstruct` leaves: `P_dev` [nimg, 12] and `X_dev` [n_tracks, 3] float64 on the device;
    on the host `P` [nimg, 3, 4], `R` [nimg, 3, 3], `t` [nimg, 3] (NaN for a slot without a pose),
    `posed` [nimg] bool, `X` [n_tracks, 3] (NaN: fewer than two posed views), `views` [n_tracks] and
    `rounds`, the slots that joined in each round (the seed pair first)."""

    def __init__(self, tracks, K, R, t, posed, P_dev, X_dev, views_dev, rounds):
        self.tracks, self.K, self.R, self.t, self.posed = tracks, K, R, t, posed
        self.P_dev, self.X_dev, self._views_dev, self.rounds = P_dev, X_dev, views_dev, rounds
        self._host = {}

    @property
    def P(self) -> np.ndarray:
        return self.K @ np.concatenate([self.R, self.t[:, :, None]], axis=2)

    @property
    def X(self) -> np.ndarray:
        if "X" not in self._host:
            self._host["X"] = self.X_dev.cpu().numpy()
        return self._host["X"]

    @property
    def views(self) -> np.ndarray:
        if "views" not in self._host:
            self._host["views"] = self._views_dev.cpu().numpy()
        return self._host["views"]

    def ba_inputs(self):
        """(camera_indices, point_indices, points_2d, camera_params [nimg, 6], points_3d) for
        pose.BundleAdjustment(nimg, len(points_3d), ..., K_list): the observations of posed slots on
        tracks with a point, the points re-indexed to those tracks in order, a camera's index its
        slot.  camera_params holds (Rodrigues vector, t) and zeros for a slot without a pose, which
        no observation refers to."""
        from . import pose
        cam, pt, xy = self.tracks.ba_inputs()
        good = np.isfinite(self.X).all(axis=1)
        sel = good[pt] & self.posed[cam]
        remap = np.cumsum(good) - 1
        params = np.zeros((len(self.posed), 6))
        for s in np.flatnonzero(self.posed):
            params[s, :3] = pose.rodrigues(self.R[s])[0].reshape(3)
            params[s, 3:] = self.t[s]
        return cam[sel], remap[pt[sel]], xy[sel], params, self.X[good]


def reconstruct(tracks, K, seed_pair, per_round=None, max_rounds=None, **resect_kwargs) -> Reconstruction:
    """From the initial pair to a pose for every frame the tracks can give one, on the device.
    seed_pair: (a, b, R, t) as `TwoView.seed` returns it.  P[a] = K_a [I | 0] and P[b] = K_b [R | t];
    all tracks are triangulated from the posed slots (pose.triangulate_tracks); then, round after
    round, `resect_frames` runs over the slots without a pose, those it poses are accepted in
    `next_views()` order (per_round=None: all of them, an int: that many), their P is set and all
    tracks are triangulated again.  The loop ends with the round that accepts nothing (or after
    max_rounds rounds).  K and **resect_kwargs as resect_frames takes them.

    One small host read per round (the resection's rstat [nimg, 8], to decide which slots join) is
    the only read-back, and the indices of the slots that join (a few int64) are the only upload;
    the points, the tracks, the poses and the mask of posed slots stay on the device.
    Out of scope: bundle adjustment inside the loop, filtering tracks by
    reprojection error, re-resection of posed frames."""
    import torch
    from . import pose
    a, b, R01, t01 = seed_pair
    ctx, dev, stream = _tracks_ctx(tracks)
    nimg = int(tracks.xy.shape[0])
    a, b = int(a), int(b)
    if not (0 <= a < nimg and 0 <= b < nimg) or a == b:
        raise ValueError("reconstruct: the seed pair's slots must be two different slots of the table")
    with torch.cuda.device(dev):
        Kt = _slot_K(torch, K, nimg, dev, "reconstruct")
        K3 = Kt.reshape(nimg, 3, 3)
        rt = torch.full((nimg, 12), float("nan"), dtype=torch.float64, device=dev)
        P = torch.zeros((nimg, 12), dtype=torch.float64, device=dev)
        valid = torch.zeros(nimg, dtype=torch.uint8, device=dev)
        posed = np.zeros(nimg, bool)

        def set_pose(slots, source):   # rt, P and valid of `slots` from source(idx) [len(slots), 12], on the device
            idx = torch.from_numpy(np.asarray(slots, np.int64)).to(dev)   # (the round's one upload)
            src = source(idx)
            rt[idx] = src
            Rt34 = torch.cat([src[:, :9].reshape(-1, 3, 3), src[:, 9:].reshape(-1, 3, 1)], dim=2)
            P[idx] = torch.bmm(K3[idx], Rt34).reshape(-1, 12)
            valid[idx] = 1
            posed[slots] = True

        first = np.concatenate([np.eye(3).reshape(9), np.zeros(3), np.asarray(R01, np.float64).reshape(9),
                                np.asarray(t01, np.float64).reshape(3)]).reshape(2, 12)
        first = torch.from_numpy(first).to(dev)
        set_pose([a, b], lambda idx: first)
        rounds = [[a, b]]
        X, views = pose.triangulate_tracks(tracks, P, valid)
        while max_rounds is None or len(rounds) - 1 < int(max_rounds):
            res = resect_frames(tracks, X, Kt, posed=valid, **resect_kwargs)   # (valid: the posed mask, resident)
            order = res.next_views()          # (the round's one host read: rstat)
            if per_round is not None:
                order = order[:max(int(per_round), 0)]
            joined = [int(s) for s in order]
            rounds.append(joined)
            if not joined:
                break
            set_pose(joined, lambda idx: res.pose_dev[idx])
            X, views = pose.triangulate_tracks(tracks, P, valid)
        Kh = K3.cpu().numpy()
        rth = rt.cpu().numpy()
        R, t = rth[:, :9].reshape(nimg, 3, 3), rth[:, 9:]
    return Reconstruction(tracks, Kh, R, t, posed, P, X, views, rounds)
