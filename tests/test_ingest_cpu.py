"""CPU: the ingest restatement (oracle/ingest.py) against the golden vectors made by the
reference's own _load_image / _PIL_resize / _rgb2gray (Runner.py:33-46, 467-563) and
against PIL itself (the reference's resize is PIL's BICUBIC, Pillow pinned 11.0.0)."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import ingest as I
from sfmfromscratch_amd import synth
from tests import ingest_cases as C
from tests.golden_util import load


def golden_cases():
    z = load("ingest.npz")
    for i in range(int(z["ncases"])):
        H, W, seed, idx = (int(v) for v in z[f"c{i}_meta"])
        yield i, z, H, W, seed, idx, float(z[f"c{i}_scale"])


@pytest.mark.parametrize("i", range(5))
def test_ingest_restatement_vs_reference_golden(i):
    z = load("ingest.npz")
    H, W, seed, idx = (int(v) for v in z[f"c{i}_meta"])
    rgb = synth.make_frame_rgb_u8(H, W, seed, idx)
    assert synth.frame_sha256(rgb) == str(z[f"c{i}_sha_in"])
    g = I.ingest(rgb, float(z[f"c{i}_scale"]))
    assert g.dtype == np.float32 and tuple(g.shape) == tuple(z[f"c{i}_shape"])
    if f"c{i}_gray" in z:
        assert np.array_equal(g.view(np.uint32), z[f"c{i}_gray"].view(np.uint32))
    assert synth.frame_sha256(g) == str(z[f"c{i}_sha_out"])


@pytest.mark.parametrize("H,W,s", [(37, 53, 0.5), (120, 91, 0.5), (64, 64, 0.25), (45, 77, 0.6), (30, 41, 1.7)])
def test_bicubic_restatement_vs_pil(H, W, s):
    Image = pytest.importorskip("PIL.Image")
    rgb = np.random.default_rng(H * W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    H2, W2 = I.resize_dims(H, W, s)
    ref = np.asarray(Image.fromarray(rgb).resize((W2, H2)))
    assert np.array_equal(I.pil_bicubic_resize(rgb, H2, W2), ref)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_gpu_case_reaches_the_kernel_pair_it_is_named_for(name):
    """Tap counts, distinct tap sets and hence the kernel pair of every shape that
    tests/test_gpu_ingest.py runs, by the restated dispatch rule (tests/ingest_cases.py): a later
    change of a shape or of a threshold cannot move a case to the other pair unnoticed."""
    B, H, H2, W, W2, want = C.CASES[name]
    assert C.dispatch(H, H2, W, W2) == want
    if name.startswith("rows7_batch"):   # workgroups walk 2 and 3 rows, which cross frames
        assert -(-B * H // C.ROWS_GRID) == {7: 2, 13: 3}[B] and C.ROWS_GRID % H != 0


def test_gpu_cases_cover_every_pair_and_both_fallbacks():
    got = {v[5][2:4] for v in C.CASES.values()}
    assert got == {("rows", 5), ("rows", 7), ("rows", 9), ("pixel", 0)}
    assert C.CASES["rows9_width_cap"][3] == C.ROWS_MAX_W < C.CASES["pixel_above_cap_only"][3]
    assert C.CASES["rows7_47_sets"][5][4] <= C.ROWS_MAX_SETS < C.CASES["pixel_71_sets"][5][4]
    assert C.rows_ks(1, 1) == 5 and C.rows_ks(5, 7) == 7 and C.rows_ks(9, 5) == 9 and C.rows_ks(11, 3) == 0


def test_identity_table_reproduces_the_input():
    """An axis of equal sizes is PIL's skipped pass: one tap of 2^22 gives (2^21 + u * 2^22) >> 22
    = u for every u8 value, below clip8's upper cut, so the identity pass is exact."""
    u = np.arange(256, dtype=np.int64)
    ss = (1 << (I.PRECISION_BITS - 1)) + u * (1 << I.PRECISION_BITS)
    assert ss.max() < (1 << I.PRECISION_BITS << 8) and ss.min() > 0
    assert np.array_equal(I._clip8(ss), u.astype(np.uint8))
    rgb = C.random_frames("rows5_identity_both")[0]
    assert np.array_equal(I.pil_bicubic_resize(rgb, 16, 64), rgb)


def _sums(src, bounds, taps, axis):
    """The pre-clip int sums of one pass (oracle.ingest._pass before _clip8)."""
    src = np.moveaxis(src, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], np.int64)
    for o, (xmin, cnt) in enumerate(bounds):
        out[o] = (1 << (I.PRECISION_BITS - 1)) + sum(src[xmin + x] * taps[o, x] for x in range(cnt))
    return np.moveaxis(out, 0, axis)


@pytest.mark.parametrize("name", C.SATURATION)
def test_step_frame_clips_at_both_ends_in_both_passes(name):
    """The crafted 0 / 255 frame of each kernel pair: sums at or above 2^30 and at or below 0 in
    the horizontal pass and, on its clipped output, in the vertical pass; all within int32, and
    every product within the 24-bit multiply of the device code."""
    _, H, H2, W, W2, _ = C.CASES[name]
    rgb = C.step_frame(H, W)
    assert set(np.unique(rgb)) == {0, 255}
    top = 1 << I.PRECISION_BITS << 8
    bx, kx = I.precompute_coeffs(W, W2)
    sh = _sums(rgb, bx, kx, 1)
    mid = I._clip8(sh)
    by, ky = I.precompute_coeffs(H, H2)
    sv = _sums(mid, by, ky, 0)
    for ss in (sh, sv):
        assert (ss >= top).sum() > 0 and (ss <= 0).sum() > 0
        assert ss.max() < 2 ** 31 and ss.min() >= -2 ** 31
    assert max(np.abs(kx).max(), np.abs(ky).max()) < 2 ** 23
    assert np.array_equal(I._clip8(sv), I.pil_bicubic_resize(rgb, H2, W2))
    assert {0, 255} <= set(np.unique(I._clip8(sv)))


def test_vertical_step_on_the_64_to_48_table():
    """A single 0 -> 255 step across 64 rows, resized to 48: one output row overshoots and one
    undershoots, in each of the 48 columns."""
    col = np.repeat(np.where(np.arange(64) < 32, 0, 255).astype(np.uint8)[:, None], 48, axis=1)
    by, ky = I.precompute_coeffs(64, 48)
    ss = _sums(col, by, ky, 0)
    assert ss.size == 2304 and (ss >= (1 << 30)).sum() == 48 and (ss <= 0).sum() == 48


def test_u8_float_roundtrip_is_exact():
    """_PIL_resize multiplies _load_image's u8/255 float32 by 255 and truncates to u8
    (Runner.py:541-545): exact for every value, so ingest may start from the u8 frame."""
    u = np.arange(256, dtype=np.uint8)
    f = u.astype(np.float64).astype(np.float32) / 255
    f *= 255
    assert np.array_equal(np.uint8(f), u)


def test_opaque_rgba_drops_alpha_translucent_rejected():
    """PIL resizes RGBA premultiplied: an opaque RGBA frame resizes to the same RGB as its
    RGB channels (so runner.drop_opaque_alpha is exact), a translucent one does not and is
    rejected (ValueError, the documented divergence)."""
    from PIL import Image

    from sfmfromscratch_amd.runner import drop_opaque_alpha
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (37, 53, 4), dtype=np.uint8)
    a[..., 3] = 255
    via_rgba = np.asarray(Image.fromarray(a).resize((26, 18)))[..., :3]
    rgb = drop_opaque_alpha(a)
    assert rgb.shape == (37, 53, 3) and rgb.flags.c_contiguous
    assert np.array_equal(via_rgba, np.asarray(Image.fromarray(rgb).resize((26, 18))))
    a[0, 0, 3] = 254
    with pytest.raises(ValueError):
        drop_opaque_alpha(a)
    with pytest.raises(ValueError):
        drop_opaque_alpha(a[..., 0])
