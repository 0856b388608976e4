"""The block-driven certified NMS (nms.hip k_nms_blocks) restated in numpy, and the planes its
tests run on.

The kernel reads, per 4 x 4 block of R, one entry of a map M that is an upper bound of the
block's maximum, and looks at the block's pixels only where M >= T (T the float whose order key
is the plane's threshold tnms).  skip_candidates restates that on top of
tests/select_ref.certified_candidates, the reference's predicate written from the reference's
lines: the candidates the block kernel can find are the reference candidates inside the blocks
it does not skip.  The claim the tests hold it to: with any upper bound for M, none is lost.

Cases are built once and shared, unchanged, by tests/test_nms_blocks_cpu.py and
tests/test_gpu_nms_blocks.py."""
from __future__ import annotations

import numpy as np

from tests.select_ref import certified_candidates, fkey, planes

KEY_MIN, KEY_MAX = 0x007FFFFF, 0xFF800000   # the order keys of -inf and +inf


def threshold_float(tnms: int) -> np.float32:
    """T of k_nms_band / k_nms_blocks: fkey's inverse inside the keys' range, -inf below it
    (every value passes), NaN above it (none does)."""
    tnms = int(tnms)
    if tnms <= KEY_MIN:
        return np.float32(-np.inf)
    if tnms > KEY_MAX:
        return np.float32(np.nan)
    b = (tnms & 0x7FFFFFFF) if tnms & 0x80000000 else (~tnms & 0xFFFFFFFF)
    return np.array([b], np.uint32).view(np.float32)[0]


def block_max(R: np.ndarray) -> np.ndarray:
    """ceil(H / 4) x (W / 4): each 4 x 4 block's maximum over its in-image pixels, a NaN dropped
    (np.fmax), -inf for a block of NaN only."""
    H, W = R.shape
    assert W % 4 == 0
    P = np.full(((H + 3) // 4 * 4, W), -np.inf, np.float32)
    P[:H] = R
    ninf = np.float32(-np.inf)
    return np.fmax.reduce(np.fmax.reduce(P.reshape(P.shape[0] // 4, 4, W // 4, 4), axis=3, initial=ninf), axis=1,
                          initial=ninf)


def inflated(M: np.ndarray) -> np.ndarray:
    """Another upper bound: +inf on every third block, the next float up elsewhere (what
    sfm_debug_nms_blocks does with inflate = 1)."""
    out = np.nextafter(M, np.float32(np.inf)).astype(np.float32)
    out.ravel()[::3] = np.inf
    return out


def keys_of(R: np.ndarray, mask: np.ndarray) -> np.ndarray:
    """The candidate list as the kernels write it, sorted: ~fkey(R) << 32 | raster index."""
    idx = np.flatnonzero(mask.ravel()).astype(np.uint64)
    k = fkey(R).ravel()[idx.astype(np.int64)]
    return np.sort(((~k).astype(np.uint64) << np.uint64(32)) | idx)


def reference_keys(R: np.ndarray, tnms: int) -> np.ndarray:
    return keys_of(R, certified_candidates(R, tnms, 3))


def skip_candidates(R: np.ndarray, tnms: int, M: np.ndarray) -> np.ndarray:
    """The reference candidates inside the blocks with M >= T."""
    H, W = R.shape
    with np.errstate(invalid="ignore"):
        hit = M >= threshold_float(tnms)
    full = np.repeat(np.repeat(hit, 4, axis=0), 4, axis=1)[:H]
    return keys_of(R, certified_candidates(R, tnms, 3) & full)


def quantile_key(R: np.ndarray, q: float) -> int:
    k = fkey(R[np.isfinite(R)] if np.isnan(R).any() else R)
    return int(np.quantile(k.astype(np.float64), q))


def position_planes() -> np.ndarray:
    """16 planes of 12 x 16, one per position (i, e) of the block at rows 4-7, columns 4-7: a
    6 x 6 plateau of 5.0 over rows and columns 3-8 — the block and one pixel beyond each of its
    four borders and four corners — on a background of distinct lower values, and a single 6.0
    at the block's pixel (i, e).  The candidates at or above 5.0: the peak, and the plateau's
    pixels that do not touch it; they lie in nine blocks."""
    rng = np.random.default_rng(16)
    out = []
    for p in range(16):
        R = rng.permutation(12 * 16).reshape(12, 16).astype(np.float32) / 100.0
        R[3:9, 3:9] = 5.0
        R[4 + p // 4, 4 + p % 4] = 6.0
        out.append(R)
    return np.stack(out)


def edge_plane(H: int, W: int, seed: int) -> np.ndarray:
    """Maxima on the image's corners and on each of its edges, over a lower random background."""
    R = np.random.default_rng(seed).random((H, W), dtype=np.float32)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2 + 1), (H // 2, 0),
                 (H // 2 + 1, W - 1)):
        R[y, x] = 2.0 + y + x
    return R


def zero_nan_plane(H: int, W: int, seed: int) -> np.ndarray:
    """Negative values with a patch of zeros of both signs (a plateau of equal values whose bits
    differ: candidates at the threshold key of 0) and one NaN.  The NaN's eight neighbours lie
    below every other value, so no threshold used here lets them be candidates: the reference's
    maxpool spreads a NaN over its neighbours' windows, the kernels' fmaxf drops it, and the two
    agree only on pixels that are no candidates either way."""
    rng = np.random.default_rng(seed)
    R = -(1 + rng.random((H, W), dtype=np.float32))
    zy, zx = H // 2, W // 2
    R[zy - 1:zy + 2, zx - 2:zx + 3] = 0.0
    R[zy, zx - 1] = -0.0
    R[zy + 1, zx + 2] = -0.0
    R[1:4, 1:4] = -9.0
    R[2, 2] = np.nan
    return R


SHAPES = [(8, 8), (12, 16), (70, 132), (66, 260)]


def cases():
    """[(name, R [B, H, W], tnms [B], fallback [B])].  Every shape: the three kinds of
    select_ref.planes at a low, a middle and a high threshold; the edge plane; the -0.0 / NaN
    plane at the key of zero; thresholds at the -inf end and above every value; a fallback plane
    in the middle of a batch of three.  66 and 70 rows: H % 4 == 2, the last block row is cut."""
    out = []
    for H, W in SHAPES:
        R = planes(3, H, W, seed=1000 * H + W)
        for q in (0.05, 0.6, 0.97):
            out.append((f"{H}x{W}_q{q}", R, np.array([quantile_key(R[b], q) for b in range(3)], np.uint32),
                        np.zeros(3, np.uint32)))
        out.append((f"{H}x{W}_all_pass", R, np.array([0, KEY_MIN, KEY_MIN + 1], np.uint32), np.zeros(3, np.uint32)))
        top = np.array([int(fkey(R[b]).max()) + 1 for b in range(2)] + [0xFFFFFFFF], np.uint32)
        out.append((f"{H}x{W}_none_pass", R, top, np.zeros(3, np.uint32)))
        out.append((f"{H}x{W}_fallback", R, np.array([quantile_key(R[b], 0.6) for b in range(3)], np.uint32),
                    np.array([0, 1, 0], np.uint32)))
        E = np.stack([edge_plane(H, W, seed=H + W), zero_nan_plane(H, W, seed=H * W)])
        out.append((f"{H}x{W}_edges_zero_nan", E,
                    np.array([quantile_key(E[0], 0.5), int(fkey(np.zeros(1, np.float32))[0])], np.uint32),
                    np.zeros(2, np.uint32)))
    P = position_planes()
    out.append(("positions", P, np.full(16, int(fkey(np.array([5.0], np.float32))[0]), np.uint32), np.zeros(16, np.uint32)))
    return out


_CASES = None


def shared_cases():
    global _CASES
    if _CASES is None:
        _CASES = cases()
    return _CASES
