"""TEST INFRASTRUCTURE ONLY — numpy restatement of the two resize rules of DESIGN.md §4
(cv2.resize(img, (dw, dh)), INTER_LINEAR, on float32), written from the rules and not from
pyramid.hip or oracle/sfm_oracle.c, so that the level-image tests have a reference the device
code was not written beside.

Rule 1, a source exactly twice the destination in both axes (OpenCV switches INTER_LINEAR to
its fast INTER_AREA there): dst = ((a00 + a01) + (a10 + a11)) * 0.25 in float32.

Rule 2, otherwise: half-pixel bilinear.  Per axis, with scale = 1 / (dn / sn) in double,
    f = float32((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s
    s < 0       -> s = 0, f = 0
    s + 1 >= sn -> s = sn - 1, f = 0, and the horizontal pass reads the one tap S[s]
horizontal h = S[s] * (1 - f) + S[s + 1] * f, vertical v = h0 * (1 - g) + h1 * g with the second
row clamped to the last one; every product and sum rounded to float32 (numpy's element-wise
ufuncs do not contract).  Checked against oracle.resize by tests/test_resample_ref_cpu.py.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def pyramid_dims(H: int, W: int, L: int, s: float):
    """Level sizes of ScaleRotInvSIFT._build_image_pyramid: (int(h / s), int(w / s)) level by level."""
    dims = [(int(H), int(W))]
    for _ in range(1, L):
        h, w = dims[-1]
        dims.append((int(h / float(s)), int(w / float(s))))
    return dims


def area2(src: np.ndarray) -> np.ndarray:
    src = np.asarray(src, F32)
    t0 = src[0::2, 0::2] + src[0::2, 1::2]
    t1 = src[1::2, 0::2] + src[1::2, 1::2]
    return (t0 + t1) * F32(0.25)


def linear_taps(dn: int, sn: int):
    """(s, s1, a0, a1, single) of every destination index along one axis."""
    scale = 1.0 / (float(dn) / float(sn))
    f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(F32)
    low = s < 0
    s[low], f[low] = 0, 0
    single = s + 1 >= sn
    s[single], f[single] = sn - 1, 0
    assert f.dtype == F32
    return s, np.minimum(s + 1, sn - 1), F32(1) - f, f, single


def linear(src: np.ndarray, dh: int, dw: int) -> np.ndarray:
    src = np.asarray(src, F32)
    sh, sw = src.shape
    sx, sx1, ax0, ax1, onex = linear_taps(dw, sw)
    sy, sy1, ay0, ay1, _ = linear_taps(dh, sh)

    def across(rows):
        return np.where(onex, rows[:, sx], rows[:, sx] * ax0 + rows[:, sx1] * ax1)

    out = across(src[sy]) * ay0[:, None] + across(src[sy1]) * ay1[:, None]
    assert out.dtype == F32
    return out


def resize(src: np.ndarray, dh: int, dw: int) -> np.ndarray:
    sh, sw = src.shape
    if sh == 2 * dh and sw == 2 * dw:
        return area2(src)
    return linear(src, dh, dw)


def pyramid(img: np.ndarray, L: int, s: float):
    """The level images of an H x W float32 frame, level 0 included."""
    out = [np.asarray(img, F32)]
    for h, w in pyramid_dims(img.shape[0], img.shape[1], L, s)[1:]:
        out.append(resize(out[-1], h, w))
    return out


# The level-image cases of tests/test_gpu_pyramid_levels.py: name -> (H, W, L, factor, the sizes
# of levels 1 .. L - 1).  The sizes are asserted on the CPU against both pyramid_dims.
PYRAMID_CASES = {
    "down2_twice": (200, 328, 3, 2, [(100, 164), (50, 82)]),
    "down2_odd_dw_then_linear": (200, 330, 3, 2, [(100, 165), (50, 82)]),
    "linear_odd_h": (75, 100, 3, 2, [(37, 50), (18, 25)]),
    "factor_1.1": (97, 131, 3, 1.1, [(88, 119), (80, 108)]),
    "factor_1.3": (97, 131, 3, 1.3, [(74, 100), (56, 76)]),
    "factor_1.5": (96, 132, 3, 1.5, [(64, 88), (42, 58)]),
    "factor_3": (200, 328, 3, 3, [(66, 109), (22, 36)]),
    "factor_1_same_size": (45, 53, 3, 1, [(45, 53), (45, 53)]),
    "fused_then_level4": (208, 336, 5, 2, [(104, 168), (52, 84), (26, 42), (13, 21)]),
    "fused_L4": (200, 328, 4, 2, [(100, 164), (50, 82), (25, 41)]),
}
