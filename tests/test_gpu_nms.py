"""Certified-mode NMS kernels against a numpy restatement of the predicate.

NaiveSIFT.py:77-95: a pixel is a candidate when R equals the max of R over the ksize x
ksize window clipped to the image; the certified path keeps those whose
order key fkey(R) reaches the plane's threshold tnms.  The streaming kernel (k_nms_stream,
the default for 3x3 and W % 4 == 0) and the tiled kernel (k_nms_tile) must both produce
exactly the numpy candidate key set, on ragged shapes (strips cut by the bottom edge,
column groups wrapping across wavefronts), plateaus and negative values.
"""
from __future__ import annotations

import numpy as np
import pytest

from sfmfromscratch_amd import _native
from tests.select_ref import planes, ring_planes

pytestmark = pytest.mark.gpu


def fkey(a: np.ndarray) -> np.ndarray:
    b = a.astype(np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def numpy_candidates(R: np.ndarray, tnms: int, ksize: int) -> np.ndarray:
    H, W = R.shape
    h = ksize // 2
    P = np.full((H + 2 * h, W + 2 * h), -np.inf, np.float32)
    P[h:h + H, h:h + W] = R
    m = np.full((H, W), -np.inf, np.float32)
    for dy in range(ksize):
        for dx in range(ksize):
            m = np.maximum(m, P[dy:dy + H, dx:dx + W])
    k = fkey(R)
    ok = (k >= np.uint32(tnms)) & (R == m)
    idx = np.flatnonzero(ok.ravel()).astype(np.uint64)
    keys = ((~k.ravel()[idx]).astype(np.uint64) << np.uint64(32)) | idx
    return np.sort(keys)


@pytest.mark.parametrize("B,H,W", [(3, 37, 100), (2, 64, 256), (3, 270, 480), (2, 9, 4), (1, 540, 960),
                                   (2, 33, 102)])
@pytest.mark.parametrize("quantile", [0.0, 0.5, 0.97])
def test_certified_nms_stream_and_tile_vs_numpy(B, H, W, quantile):
    R = planes(B, H, W, seed=H * 1000 + W)
    tnms = np.array([np.quantile(fkey(R[b]).astype(np.float64), quantile) for b in range(B)]).astype(np.uint32)
    want = [numpy_candidates(R[b], int(tnms[b]), 3) for b in range(B)]
    for tile in (False, True):
        got = _native.debug_nms(R, tnms, ksize=3, tile=tile)
        for b in range(B):
            assert got[b].size == want[b].size, (tile, b, got[b].size, want[b].size)
            assert np.array_equal(got[b], want[b]), (tile, b)


@pytest.mark.parametrize("ksize", [1, 5, 7, 9, 11, 13, 21, 31])
def test_certified_nms_other_window_sizes_vs_numpy(ksize):
    """k_nms_tile<0>, <2>, <3>, <4> (ksize 9) and k_nms_generic (11 and above, up to the largest
    the context accepts); on 33 x 102 (W % 4 != 0) ksize 13 and above exceed a third of the
    plane's height, so every window is clipped by an edge.  Two random planes and, for windows
    wider than one pixel, the ring planes."""
    for H, W in ((45, 120), (33, 102)):
        R = planes(2, H, W, seed=ksize)
        tnms = np.array([np.quantile(fkey(R[b]).astype(np.float64), 0.8) for b in range(2)]).astype(np.uint32)
        if ksize > 1:
            ring = ring_planes(H, W, ksize // 2)
            R = np.concatenate([R, ring])
            tnms = np.concatenate([tnms, np.full(len(ring), fkey(np.zeros(1, np.float32))[0], np.uint32)])
        got = _native.debug_nms(R, tnms, ksize=ksize)
        kept_a = 0
        for b in range(len(R)):
            want = numpy_candidates(R[b], int(tnms[b]), ksize)
            assert np.array_equal(got[b], want), (H, W, b)
            if b >= 2:
                v = R[b].ravel()[(want & np.uint64(0xFFFFFFFF)).astype(np.int64)]
                kept_a += int(((v >= 1) & (v < 100)).sum())
        # the design holds: the eight A pixels with B just outside the window stay, the eight
        # with B on its border do not
        assert ksize == 1 or kept_a == 8
