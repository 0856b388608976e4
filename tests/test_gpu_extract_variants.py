"""GPU: the extractor's compiled kernel variants that the stock parameter sets never select.

The launchers choose a kernel from gaussian_size, ksize and feature_width: k_describe_q<WS, ROT>
for every even window width 2..22 (describe_q.hip), k_describe above that (describe.hip),
k_harris<KS> for twelve window sizes (harris.hip), k_nms_tile<0..4> / k_nms_generic and the
exact path's clipped-window loop (nms.hip, select.hip).  Every variant listed in DESIGN.md
('Variants and the tests that run them') and not reached by the other test files runs here,
against the C oracle bit for bit and, where tests/golden/variants.npz holds the reference's
output, against the reference by the project's desc_close.  The conditions on the fixture that
these tests rely on are asserted on the CPU by tests/test_oracle_golden.py."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from sfmfromscratch_amd import NaiveSIFT, ScaleRotInvSIFT, _abi, _native, synth
from tests.golden_util import P_MAIN, desc_close, frame, load
from tests.test_gpu_select import mixed_batch, run

pytestmark = pytest.mark.gpu

DESC_WIDTHS = [2, 6, 7, 10, 11, 12, 13, 20, 21, 22, 23, 24, 64]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_extract(img, pp, mode=_abi.SFM_MODE_SCALEROT):
    """-> X, Y, D (n, 128), C, level counts, through the C-ABI's host-pointer call."""
    return _native.context_for(_abi.params_from_dict(pp, mode)).extract(img)


@pytest.mark.parametrize("fw", DESC_WIDTHS)
def test_descriptors_every_width_vs_golden_and_oracle(fw):
    """Both modes at one width: with tests/test_gpu_parity.py's widths (3, 4, 9, 14, 16, 18) every
    k_describe_q<WS, ROT> for WS 2..22 has run (WS 10 is the one 128-slot sort network; 6, 10,
    12 have partly filled cell rows; 20, 22 windows wider than the 16 x 16 the cells see), and
    k_describe at its first width (24, with 23 the last of the quad kernel) and at SFM_MAX_FW."""
    z = load("variants.npz")
    assert list(z["desc_widths"]) == DESC_WIDTHS
    H, W, seed, idx = z["desc_frame"]
    img = frame(H, W, seed, idx, z["desc_sha"])
    pp = dict(P_MAIN, num_interest_points=int(z["desc_k"]), feature_width=fw)
    for rotate in (0, 1):
        obj = ScaleRotInvSIFT(img, dict(pp, pyramid_level=1)) if rotate else NaiveSIFT(img, pp)
        x, y = obj.detect_keypoints()
        d = obj.extract_descriptors()
        assert np.array_equal(x, z[f"d{fw}_x"]) and np.array_equal(y, z[f"d{fw}_y"]), (fw, rotate)
        assert desc_close(z[f"d{fw}_r{rotate}_d"], d), (fw, rotate)
        od = O.descriptors(img, x, y, fw, bool(rotate))
        assert np.array_equal(bits(d), bits(od)), (fw, rotate)


@pytest.mark.parametrize("fw", [0, 1])
def test_zero_width_window_naive_gives_zero_descriptors(fw):
    """feature_width 0 and 1: the window is empty (ws = 0), launch_describe_quad declines and
    k_describe runs with n = 0, P = 1 and a 2 x 2 patch.  Its loops over the window do nothing;
    every cell slot is outside the window, so the 128 bins are 0, the norm is 0 and the
    descriptor is 128 zeros, as the reference's and the oracle's.  (desc_layout keeps every
    region inside the launch's LDS at n = 0: the cell stage reads s_ori[0] / s_mag[0] for slots
    it then discards, and those addresses fall in the regions that follow.)"""
    z = load("variants.npz")
    H, W, seed, idx = z["desc_frame"]
    img = frame(H, W, seed, idx, z["desc_sha"])
    obj = NaiveSIFT(img, dict(P_MAIN, num_interest_points=60, feature_width=fw))
    x, y = obj.detect_keypoints()
    d = obj.extract_descriptors()
    ox, oy, _ = O.detect(img, 60, fw, P_MAIN)
    assert len(x) == 60 and np.array_equal(x, ox) and np.array_equal(y, oy)
    od = O.descriptors(img, x, y, fw, False)
    assert d.shape == (60, 128) and d.dtype == np.float32
    assert not bits(d).any() and np.array_equal(bits(d), bits(od))


@pytest.mark.parametrize("fw,scale,L,widths", [(22, 1.1, 4, [22, 20, 18, 16]), (13, 1.1, 4, [13, 11, 10, 9]),
                                               (6, 2, 3, [6, 3, 3])])
def test_pyramid_levels_take_different_widths_vs_oracle(fw, scale, L, widths):
    """One extraction whose levels select different k_describe_q variants (the per-level width
    is max(int(fw / scale**l), 3), ScaleRotInvSIFT.py:95-96)."""
    assert [max(int(fw / scale ** l), 3) for l in range(L)] == widths
    img = synth.make_frame(120, 160, 57, L)
    pp = dict(P_MAIN, num_interest_points=60 * L, feature_width=fw, pyramid_level=L, pyramid_scale_factor=scale)
    X, Y, D, C, lc = gpu_extract(img, pp)
    OX, OY, OD, olc, OC = O.extract(img, pp, with_conf=True)
    assert np.array_equal(lc, olc) and all(n > 0 for n in lc)
    assert np.array_equal(X, OX) and np.array_equal(Y, OY)
    assert np.array_equal(bits(C), bits(OC))
    assert np.array_equal(bits(D), bits(OD))


@pytest.mark.parametrize("fw", [6, 10, 18, 22, 24])
def test_tiny_orientations_exact_double_key_path(fw):
    """variants.npz's float32 frame with orientations 0 < |ori| < 2^-25 (Iy / Ix ~ 2^-29; no
    u8 / 255 frame has one).  At widths 6, 10, 18, 22 k_describe_q takes grp_tiny for the
    keypoints whose window holds such a pixel and the rank path for the others, and one
    wavefront's four keypoints disagree (asserted on the fixture by test_oracle_golden.py);
    width 24 is k_describe over the same frame."""
    z = load("variants.npz")
    img = z["tiny_img"]
    pp = dict(P_MAIN, num_interest_points=int(z["tiny_k"]), feature_width=fw, pyramid_level=1)
    X, Y, D, C, _ = gpu_extract(img, pp)
    OX, OY, OD, _, OC = O.extract(img, pp, with_conf=True)
    assert len(X) >= 16
    assert np.array_equal(X, OX) and np.array_equal(Y, OY) and np.array_equal(bits(C), bits(OC))
    assert np.array_equal(bits(D), bits(OD))
    if fw in z["tiny_widths"]:
        assert np.array_equal(X, z[f"y{fw}_x"]) and np.array_equal(Y, z[f"y{fw}_y"])
        assert desc_close(z[f"y{fw}_d"], D)


def merged_angle_frame(H=64, W=96, seed=7):
    """Even rows n / 255 (n in 1..255), odd rows multiples of 2^-62: on an even row with Ix > 0
    the orientation is about Iy / Ix ~ 2^-60, far below half an ulp of any dominant
    orientation's double (2^-57 at pi / 36), so the float64 relative angles of a cell's tiny
    orientations are all equal and np.histogram's stable sort leaves them in raster order,
    while their float32 values differ.  The magnitudes are inexact floats, so the order in
    which they are summed shows in the bins."""
    rng = np.random.default_rng(seed)
    img = np.empty((H, W), np.float64)
    img[0::2] = rng.integers(1, 256, img[0::2].shape) / 255
    img[1::2] = rng.integers(0, 8, img[1::2].shape) * 2.0 ** -62
    return img.astype(np.float32)


@pytest.mark.parametrize("fw", [6, 10, 18, 22])
def test_merged_relative_angles_take_the_exact_order(fw):
    """Where the tiny-orientation fixture only reaches grp_tiny (its orientations, ~2^-29,
    stay distinct after the dominant orientation is subtracted, so the rank order and the exact
    order agree), this frame's do not: a k_describe_q that ordered such a cell by float32 value
    instead of (float64 relative angle, raster slot) sums the weights in another order.
    At width 6 the 36-pixel windows often have a diagonal dominant orientation (+-pi/4,
    +-3pi/4), for which the relative angle of a tiny orientation falls exactly on a cell edge:
    the case that showed edge_key's short walk (describe_q.hip) putting orientations in
    (-2^-54, -2^-143) one bin low.
    Against the oracle only: its histogram is the stable-sort restatement of np.histogram."""
    img = merged_angle_frame()
    pp = dict(P_MAIN, num_interest_points=96, feature_width=fw, pyramid_level=1)
    X, Y, D, C, _ = gpu_extract(img, pp)
    OX, OY, OD, _, OC = O.extract(img, pp, with_conf=True)
    assert len(X) >= 16
    assert np.array_equal(X, OX) and np.array_equal(Y, OY) and np.array_equal(bits(C), bits(OC))
    assert np.array_equal(bits(D), bits(OD))


def asymmetric_taps(gs):
    """A seeded random positive gs x gs kernel, normalised, in float32, two taps exactly 0, and
    not symmetric under transpose, row flip or column flip."""
    rng = np.random.default_rng(1000 + gs)
    t = rng.uniform(0.1, 1.0, (gs, gs))
    t = (t / t.sum()).astype(np.float32)
    t.flat[1] = 0.0
    t.flat[gs * gs - 1] = 0.0
    assert not np.array_equal(t, t.T) and not np.array_equal(t, t[::-1]) and not np.array_equal(t, t[:, ::-1])
    return t


@pytest.mark.parametrize("gs", [2, 3, 4, 7, 8, 15])
@pytest.mark.parametrize("H,W", [(70, 200), (97, 131)])
def test_harris_asymmetric_taps_R_bitexact_vs_oracle(H, W, gs):
    """Every other test's window is a symmetric Gaussian, which a kernel that transposed or
    mirrored its taps (or its tap pairs, harris_taps_build) would still pass."""
    taps = asymmetric_taps(gs)
    p = _abi.params_from_dict(dict(P_MAIN, gaussian_size=gs), _abi.SFM_MODE_SCALEROT)
    for i, v in enumerate(taps.ravel()):
        p.gauss_kernel[i] = float(v)
    p.gauss_kernel_set = 1
    img = synth.make_frame(H, W, 29, gs)
    R, _, _ = _native.debug_harris(img, p)
    assert np.array_equal(bits(R), bits(O.harris_response_taps(img, taps, p.alpha)))


@pytest.mark.parametrize("ksize", [9, 11, 31])
@pytest.mark.parametrize("H,W", [(70, 200), (97, 131)])
def test_exact_nms_candidate_count_large_windows_vs_oracle(H, W, ksize):
    """launch_nms in its exact mode (mode 1) through launch_tile<4> (ksize 9) and
    k_nms_generic (ksize 11, 31): the candidate count of one plane against the oracle's."""
    pp = dict(P_MAIN, ksize=ksize)
    img = synth.make_frame(H, W, 19, ksize)
    _, med, ncand = _native.debug_harris(img, _abi.params_from_dict(pp, _abi.SFM_MODE_SCALEROT))
    _, _, _, dbg = O.detect(img, 10 ** 7, 0, pp, debug=True)
    assert np.float32(med) == dbg["median"]
    assert ncand == dbg["n_candidates"] and ncand > 0


@pytest.mark.parametrize("ksize", [0, 2, 4, 9, 11, 31])
def test_extract_other_nms_windows_certified_and_exact_vs_oracle(ksize):
    """Whole extractions at the NMS windows no other test selects: launch_tile<0>, <1> (even
    ksize 2 = ksize // 2 of 1), <2> (4), <4> (9) and k_nms_generic (11, 31) in the certified mode,
    and select.hip's clipped-window loop on the planes that fall back and under
    SFMFEAT_SELECT=exact.  One level of 120 x 160 has 19,200 pixels, which the size rule lets
    certify for k <= 150 (extract_layout.h: h * w >= 128 k); a plane certifies only if it also has
    k candidates (select.hip k_select), and a 31 x 31 window leaves a 120 x 160 plane about ten,
    so k is half the smallest candidate count of the two textured planes (at most 120).  With
    that k the textured and the noise plane certify and the flat ones fall back, so the
    `0 < fb < tot` check of test_certified_select_equals_exact_and_oracle holds at every ksize."""
    imgs = mixed_batch(120, 160)
    base = dict(P_MAIN, ksize=ksize, pyramid_level=1, feature_width=8)
    ncand = [O.detect(imgs[b], 10 ** 7, 0, base, debug=True)[3]["n_candidates"] for b in (0, 3)]
    k = min(120, min(ncand) // 2)
    assert k >= 2, ncand
    pp = dict(base, num_interest_points=k)
    xy, desc, cnt, (fb, tot) = run(imgs, pp, exact=False)
    xe, de, ce, (fbe, tote) = run(imgs, pp, exact=True)
    assert fbe == tote == tot == len(imgs)
    assert 0 < fb < tot, (fb, tot)  # both select paths in one batch
    assert np.array_equal(cnt, ce)
    for b in range(len(imgs)):
        n = cnt[b]
        assert np.array_equal(xy[b, :n], xe[b, :n])
        assert np.array_equal(bits(desc[b, :n]), bits(de[b, :n]))
        X, Y, D, _, C = O.extract(imgs[b], pp, with_conf=True)
        assert n == len(X)
        assert np.array_equal(xy[b, :n, 0], X) and np.array_equal(xy[b, :n, 1], Y)
        assert np.array_equal(bits(desc[b, :n]), bits(D))
        # the batch call returns no confidences: the host-pointer call of the same plane does
        hx, hy, hd, hc, _ = gpu_extract(imgs[b], pp)
        assert np.array_equal(hx, X) and np.array_equal(hy, Y) and np.array_equal(bits(hc), bits(C))
        assert np.array_equal(bits(hd), bits(D))
