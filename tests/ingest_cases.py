"""TEST INFRASTRUCTURE ONLY — the shapes at which tests/test_gpu_ingest.py runs every ingest
kernel pair, and a restatement of the rule by which launch_ingest_rgb (ingest.hip) picks the
pair, so that tests/test_ingest_cpu.py can assert which pair each shape must take.

The rule, restated from DESIGN.md §12: an axis whose sizes are equal has a table one tap wide
(the identity, tap 2^22); otherwise the table is Pillow's precompute_coeffs.  KS is 5, 7 or 9,
the smallest of them that holds max(ks_h, ks_v); above 9 there is none.  A column's tap set is
its first `count` taps padded with zeros to KS; equal sets are stored once.  The row pair
k_rows_h<KS> / k_rows_v<KS> runs when KS exists, W and W2 are multiples of 4 and at most 4096,
and there are at most 64 distinct sets; every other call takes k_resample_h /
k_resample_v_gray."""
from __future__ import annotations

import numpy as np

from oracle import ingest as I

ROWS_MAX_W = 4096
ROWS_MAX_SETS = 64


def table(n_in: int, n_out: int):
    """(bounds [out, 2], int taps [out, ksize]) of one axis, the identity included."""
    if n_in == n_out:
        b = np.stack([np.arange(n_out), np.ones(n_out, np.int64)], axis=1)
        return b, np.full((n_out, 1), 1 << I.PRECISION_BITS, np.int64)
    return I.precompute_coeffs(n_in, n_out)


def rows_ks(ks_h: int, ks_v: int) -> int:
    ks = max(ks_h, ks_v)
    return 5 if ks <= 5 else 7 if ks <= 7 else 9 if ks <= 9 else 0


def tap_sets(bounds, taps, ks: int) -> int:
    sets = set()
    for (_, cnt), t in zip(bounds, taps):
        k = [0] * ks
        k[:int(cnt)] = [int(v) for v in t[:int(cnt)]]
        sets.add(tuple(k))
    return len(sets)


def dispatch(H: int, H2: int, W: int, W2: int):
    """(ks_h, ks_v, "rows" | "pixel", KS (0 on the per-pixel pair), tap sets or None when no KS)."""
    bh, th = table(W, W2)
    _, tv = table(H, H2)
    ks_h, ks_v = th.shape[1], tv.shape[1]
    ks = rows_ks(ks_h, ks_v)
    nsets = tap_sets(bh, th, ks) if ks else None
    rows = bool(ks) and W % 4 == 0 and W2 % 4 == 0 and W <= ROWS_MAX_W and W2 <= ROWS_MAX_W and nsets <= ROWS_MAX_SETS
    return ks_h, ks_v, "rows" if rows else "pixel", ks if rows else 0, nsets


# name -> (B, H, H2, W, W2, (ks_h, ks_v, pair, KS, tap sets)): what each shape must reach
CASES = {
    "rows5_upscale":        (1, 32, 48, 64, 96, (5, 5, "rows", 5, 7)),
    "rows7":                (1, 48, 36, 64, 48, (7, 7, "rows", 7, 7)),
    "rows7_47_sets":        (1, 32, 24, 256, 172, (7, 7, "rows", 7, 47)),
    "pixel_71_sets":        (1, 32, 24, 400, 268, (7, 7, "pixel", 0, 71)),
    "rows9":                (1, 36, 18, 64, 32, (9, 9, "rows", 9, 5)),
    "rows9_h9_v5":          (1, 36, 48, 64, 32, (9, 5, "rows", 9, 5)),
    "rows7_h5_v7":          (1, 64, 48, 64, 96, (5, 7, "rows", 7, 7)),
    "rows7_identity_h":     (1, 48, 36, 64, 64, (1, 7, "rows", 7, 1)),
    "rows7_identity_v":     (1, 48, 48, 64, 48, (7, 1, "rows", 7, 7)),
    "rows5_identity_both":  (1, 16, 16, 64, 64, (1, 1, "rows", 5, 1)),
    "pixel_ks11":           (1, 32, 14, 64, 28, (11, 11, "pixel", 0, None)),
    "rows9_width_cap":      (1, 6, 3, 4096, 2048, (9, 9, "rows", 9, 5)),
    "pixel_above_cap":      (1, 6, 3, 4100, 2052, (9, 9, "pixel", 0, 517)),   # 4100 / 2052 is not 2
    "pixel_above_cap_only": (1, 6, 3, 4104, 2052, (9, 9, "pixel", 0, 5)),     # the width alone decides
    "rows7_batch7":         (7, 240, 180, 64, 48, (7, 7, "rows", 7, 7)),
    "rows7_batch13":        (13, 240, 180, 64, 48, (7, 7, "rows", 7, 7)),
}
ROWS_GRID = 1536  # k_rows_h's workgroups: B * H above it makes workgroups walk several rows

# one crafted 0 / 255 frame per kernel pair (clip8 at both ends in both passes)
SATURATION = ["rows5_upscale", "rows7", "rows9", "pixel_ks11"]


def random_frames(name: str) -> np.ndarray:
    B, H, _, W, _, _ = CASES[name]
    seed = sum(name.encode()) + H * W
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def step_frame(H: int, W: int) -> np.ndarray:
    """0 / 255 blocks of 8 x 8 pixels, the three channels out of phase: step edges up and down
    along both axes, on which the bicubic taps' negative lobes overshoot at both ends."""
    y, x = np.mgrid[0:H, 0:W]
    ch = [((y // 8 + x // 8 + c) % 2) * 255 for c in range(3)]
    ch[2] = ((y // 8) % 2 ^ 1) * ((x // 8) % 2) * 255   # isolated bright blocks on black
    return np.stack(ch, axis=-1).astype(np.uint8)


def reference(frames: np.ndarray, H2: int, W2: int) -> np.ndarray:
    return np.stack([I.rgb_to_gray(I.pil_bicubic_resize(f, H2, W2)) for f in frames])
