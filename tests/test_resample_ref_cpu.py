"""CPU: the numpy restatement of the resize rules (tests/resample_ref.py) against the C oracle's
orc_resize, bit for bit: on every level of the GPU level-image cases, on sources one and two
pixels wide or high (the `s + 1 >= sn` clamp at every index), and on upscales (the `s < 0`
clamp).  Two restatements written apart that agree here are the two references of
tests/test_gpu_pyramid_levels.py."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import resample_ref as R


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frame(h, w, seed):
    """u8 / 255 values, as the extractor's frames, with the extremes at the corners and edges."""
    u8 = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    u8[0, 0], u8[-1, -1], u8[0, -1], u8[-1, 0] = 255, 255, 0, 0
    return u8.astype(np.float32) / np.float32(255)


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("name", sorted(R.PYRAMID_CASES))
def test_pyramid_case_dims_and_levels_vs_oracle(name, kind):
    H, W, L, s, want_dims = R.PYRAMID_CASES[name]
    dims = R.pyramid_dims(H, W, L, s)
    assert dims == O.pyramid_dims(H, W, L, s) and dims[1:] == want_dims
    assert min(min(d) for d in dims) >= 13 and min(d[1] for d in dims) >= 21
    # u8 / 255 frames, and float32 frames with full mantissas (every product and sum rounds)
    cur = frame(H, W, H + W) if kind == "u8" else np.random.default_rng(H * W).random((H, W), dtype=np.float32)
    for lvl, img in enumerate(R.pyramid(cur, L, s)):
        if lvl:
            cur = O.resize(cur, *dims[lvl])
        assert img.dtype == np.float32 and img.shape == dims[lvl]
        assert np.array_equal(bits(img), bits(cur)), (name, lvl)


def test_pyramid_cases_take_the_rules_they_are_named_for():
    """Which rule each level of each case takes (exact 2x in both axes, or bilinear), so that a
    change of a case's size cannot move it to the other kernel unnoticed."""
    def rules(name):
        H, W, L, s, _ = R.PYRAMID_CASES[name]
        d = R.pyramid_dims(H, W, L, s)
        return ["area" if d[i - 1] == (2 * d[i][0], 2 * d[i][1]) else "linear" for i in range(1, L)]
    assert rules("down2_twice") == ["area", "area"]
    assert rules("down2_odd_dw_then_linear") == ["area", "linear"]     # 165 != 2 * 82
    assert rules("linear_odd_h") == ["linear", "linear"]               # 75 != 2 * 37, 37 != 2 * 18
    for name in ("factor_1.1", "factor_1.3", "factor_1.5", "factor_3"):
        assert rules(name) == ["linear", "linear"]
    # a factor of 1 is the one pyramid whose last row and column reach the `s + 1 >= sn` clamp
    # (f = d exactly, so s = sn - 1 at d = dn - 1; every factor above 1 ends at s <= sn - 2)
    assert rules("factor_1_same_size") == ["linear", "linear"]
    assert R.linear_taps(53, 53)[4].tolist() == [False] * 52 + [True]
    for name, (H, W, L, s, _) in R.PYRAMID_CASES.items():
        d = R.pyramid_dims(H, W, L, s)
        for i in range(1, L):
            for dn, sn in zip(d[i], d[i - 1]):
                assert R.linear_taps(dn, sn)[4].any() == (s == 1), (name, i)
    assert rules("fused_then_level4") == ["area"] * 4
    assert rules("fused_L4") == ["area"] * 3
    # the odd-dw guard of the 2x kernel's second output, and a frame whose pixel count is no
    # multiple of 4 (the scalar tail of the u8 conversion)
    assert R.PYRAMID_CASES["down2_odd_dw_then_linear"][4][0][1] % 2 == 1
    assert (3 * 97 * 131) % 4 != 0


@pytest.mark.parametrize("sh,sw,dh,dw", [
    (1, 1, 1, 1), (1, 1, 3, 5), (1, 9, 1, 4), (9, 1, 4, 1), (1, 9, 2, 13), (2, 2, 1, 1), (2, 9, 1, 4),
    (2, 9, 5, 4), (9, 2, 4, 1), (9, 2, 4, 7), (2, 2, 3, 3), (2, 3, 7, 2),
    (13, 21, 26, 42), (13, 21, 27, 43), (13, 21, 14, 22), (37, 50, 75, 100), (25, 41, 100, 164),
    (13, 21, 13, 21), (50, 82, 25, 41), (50, 83, 25, 41), (51, 82, 25, 41), (6, 8, 2, 4), (97, 131, 11, 7)])
def test_thin_sources_upscales_and_mixed_factors_vs_oracle(sh, sw, dh, dw):
    src = frame(sh, sw, 1000 * sh + sw)
    assert np.array_equal(bits(R.resize(src, dh, dw)), bits(O.resize(src, dh, dw)))


def test_linear_taps_clamps():
    """The two clamps by hand: upscaling by 2 starts at f = -0.25 -> (s, f) = (0, 0), and ends at
    s = sn - 1 with one tap; a factor of 3 skips a source pixel between its two taps."""
    s, s1, a0, a1, one = R.linear_taps(8, 4)
    assert s.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and s1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]
    assert a1.tolist() == [0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0] and one.tolist() == [False] * 7 + [True]
    assert np.array_equal(a0, np.float32(1) - a1)
    s, s1, _, a1, one = R.linear_taps(3, 9)
    assert s.tolist() == [1, 4, 7] and s1.tolist() == [2, 5, 8] and a1.tolist() == [0, 0, 0] and not one.any()
    s, s1, _, a1, one = R.linear_taps(36, 109)
    assert np.all(np.diff(s) >= 3) and s[-1] + 1 < 109 and not one.any()
