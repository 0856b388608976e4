"""GPU: device ingest (sfm_ingest_rgb*, ingest.hip) against the golden vectors made by the
reference's own _load_image / _PIL_resize / _rgb2gray (Runner.py:33-46), against PIL and
the oracle restatement on other sizes, and FeatureRunner end to end against the oracle.
Every kernel pair of launch_ingest_rgb at the smallest shapes that reach it
(tests/ingest_cases.py, DESIGN.md §12's table), clip8's two cuts in each pair, and one context
called with changing shapes on the default and on a side stream.
Bar: bit-identical float32 gray frames."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import ingest as I
from oracle import oracle as O
from sfmfromscratch_amd import _abi, _native, synth
from tests import ingest_cases as C
from tests.golden_util import P_OCT, assert_matches_equal, load

pytestmark = pytest.mark.gpu


def ctx():
    return _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))


@pytest.mark.parametrize("i", range(5))
def test_ingest_vs_reference_golden(i):
    z = load("ingest.npz")
    H, W, seed, idx = (int(v) for v in z[f"c{i}_meta"])
    rgb = synth.make_frame_rgb_u8(H, W, seed, idx)
    g = ctx().ingest_rgb(rgb, float(z[f"c{i}_scale"]))
    assert tuple(g.shape) == tuple(z[f"c{i}_shape"])
    if f"c{i}_gray" in z:
        assert np.array_equal(g.view(np.uint32), z[f"c{i}_gray"].view(np.uint32))
    assert synth.frame_sha256(g) == str(z[f"c{i}_sha_out"])


@pytest.mark.parametrize("H,W,s", [(37, 53, 0.5), (120, 91, 0.5), (64, 64, 0.25), (45, 77, 0.6), (30, 41, 1.7),
                                   (1080, 1920, 0.5)])
def test_ingest_vs_pil_and_oracle(H, W, s):
    Image = pytest.importorskip("PIL.Image")
    rgb = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    H2, W2 = I.resize_dims(H, W, s)
    ref = I.rgb_to_gray(np.asarray(Image.fromarray(rgb).resize((W2, H2))))
    g = ctx().ingest_rgb(rgb, s)
    assert np.array_equal(g.view(np.uint32), ref.view(np.uint32))
    if H * W < 100000:
        assert np.array_equal(g.view(np.uint32), I.ingest(rgb, s).view(np.uint32))


def test_ingest_batch_dev_equals_host():
    torch = pytest.importorskip("torch")
    from sfmfromscratch_amd.pipeline import ingest_rgb
    frames = np.stack([synth.make_frame_rgb_u8(270, 481, 5, i) for i in range(3)])
    g = ingest_rgb(ctx(), torch.from_numpy(frames).cuda(), 0.5)
    torch.cuda.synchronize()
    got = g.cpu().numpy()
    for b in range(3):
        assert np.array_equal(got[b].view(np.uint32), I.ingest(frames[b], 0.5).view(np.uint32))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def fresh_ctx():
    """A context of the test's own (ctx() hands every test of a thread the same cached one)."""
    return _native.Context(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))


def ingest_dev(c, frames, H2, W2, stream=0, torch=None):
    """Context.ingest_rgb_dev on [B, H, W, 3] u8 frames with explicit target sizes (the C ABI takes
    them freely) -> the device tensor [B, H2, W2]; not synchronised."""
    torch = torch or pytest.importorskip("torch")
    d = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    B, H, W, _ = d.shape
    out = torch.full((B, H2, W2), -1.0, dtype=torch.float32, device="cuda")
    c.ingest_rgb_dev(d.data_ptr(), B, H, W, H2, W2, out.data_ptr(), stream)
    return out


def assert_equals_references(got, frames, H2, W2, tag):
    """Bit equality with the restatement (oracle/ingest.py) and, where PIL imports, with
    Image.resize + gray."""
    want = C.reference(frames, H2, W2)
    assert got.shape == want.shape
    for b in range(len(frames)):
        assert np.array_equal(bits(got[b]), bits(want[b])), (tag, b)
    try:
        from PIL import Image
    except ImportError:
        return
    for b in (0, len(frames) - 1):
        pil = I.rgb_to_gray(np.asarray(Image.fromarray(frames[b]).resize((W2, H2))))
        assert np.array_equal(bits(got[b]), bits(pil)), (tag, b, "PIL")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_every_kernel_pair_vs_restatement_and_pil(name):
    """Each ingest kernel pair at the smallest shapes that reach it (tests/ingest_cases.py; the
    pair of every shape is asserted on the CPU by tests/test_ingest_cpu.py): k_rows_h / k_rows_v
    at KS 5, 7 and 9, horizontal and vertical tap counts that differ, the identity pass in either
    axis and in both, the fallbacks to the per-pixel pair on the tap-set count, on the tap count
    and on the width, and batches whose B * H rows exceed k_rows_h's grid (workgroups walk 2 and
    3 rows and prefetch across frame boundaries)."""
    torch = pytest.importorskip("torch")
    B, H, H2, W, W2, _ = C.CASES[name]
    frames = C.random_frames(name)
    c = fresh_ctx()             # alive until the device is synchronised
    got = ingest_dev(c, frames, H2, W2)
    torch.cuda.synchronize()
    assert_equals_references(got.cpu().numpy(), frames, H2, W2, name)


@pytest.mark.parametrize("name", C.SATURATION)
def test_step_edges_clip_at_both_ends(name):
    """The 0 / 255 block frame on which both passes over- and underflow (asserted on the CPU by
    test_step_frame_clips_at_both_ends_in_both_passes): clip8's two cuts in each kernel pair.
    Two frames, the second inverted, so the row pair also walks a frame boundary."""
    torch = pytest.importorskip("torch")
    _, H, H2, W, W2, _ = C.CASES[name]
    f = C.step_frame(H, W)
    frames = np.stack([f, 255 - f])
    c = fresh_ctx()             # alive until the device is synchronised
    got = ingest_dev(c, frames, H2, W2)
    torch.cuda.synchronize()
    assert_equals_references(got.cpu().numpy(), frames, H2, W2, name)


# One context, changing shapes (names of C.CASES, or (H, H2, W, W2)): (a) only the vertical table
# changes; (b) row pair KS 9 -> per-pixel -> row pair KS 5 -> the first again; (c) 47 tap sets
# after 7 and back (the set table grows and shrinks under the same KS).
SEQUENCES = {
    "a_vertical_table_only": ["rows7", (36, 18, 64, 48), "rows7"],
    "b_rows9_pixel_rows5_rows9": ["rows9", "pixel_ks11", "rows5_upscale", "rows9"],
    "c_set_count_7_47_7": [(32, 24, 64, 48), "rows7_47_sets", (32, 24, 64, 48)],
}


def sequence_shapes(seq):
    return [C.CASES[s][1:5] if isinstance(s, str) else s for s in seq]


@pytest.mark.parametrize("stream_kind", ["default", "side"])
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
def test_one_context_changing_shapes(seq, stream_kind):
    """ingest_impl caches the tap tables per (W, W2) and (H, H2) and uploads them again when the
    shape changes.  Every call of a sequence on one context equals the restatement, on the
    default stream and on a non-default torch stream with no synchronisation between the calls
    (the upload is ordered on the call's stream, behind the previous call's kernels)."""
    torch = pytest.importorskip("torch")
    c = fresh_ctx()
    shapes = sequence_shapes(SEQUENCES[seq])
    frames = [np.random.default_rng(11 * i + H * W).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
              for i, (H, _, W, _) in enumerate(shapes)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()
    side = torch.cuda.Stream() if stream_kind == "side" else None
    outs = []
    with torch.cuda.stream(side):
        st = side.cuda_stream if side is not None else 0
        for d, (H, H2, W, W2) in zip(dev, shapes):
            outs.append(ingest_dev(c, d, H2, W2, st, torch))
    torch.cuda.synchronize()
    for i, (o, f, (H, H2, W, W2)) in enumerate(zip(outs, frames, shapes)):
        assert_equals_references(o.cpu().numpy(), f, H2, W2, (seq, i))


def test_second_shape_on_a_side_stream_while_the_first_call_runs():
    """8 frames of 1080 x 1920 -> 540 x 960, then at once 240 x 320 -> 120 x 160 on the same
    context and non-default stream, nothing synchronised in between: the second call's tables
    must not reach the device while the first call's kernels still read the context's tables
    (before the fix of ingest_impl a blocking copy on the null stream, which torch's non-blocking
    side streams do not join, could overwrite them).

    The case can give a wrong image and cannot fault, and has to keep that property: the second
    shape is smaller than the first in both axes with the same tap count (9, the row pair in both
    calls), so a kernel of the first call that read the second call's column map, tap sets or
    vertical table would read source columns below 320 < 1920 and temp rows below 240 < 1080,
    inside the first call's buffers, and would write only its own outputs."""
    torch = pytest.importorskip("torch")
    big, small = (1080, 540, 1920, 960), (240, 120, 320, 160)
    assert small[0] < big[0] and small[1] < big[1] and small[2] < big[2] and small[3] < big[3]
    db, ds = C.dispatch(*big), C.dispatch(*small)
    assert db[:4] == ds[:4] == (9, 9, "rows", 9) and ds[4] <= db[4]
    rng = np.random.default_rng(1080)
    two = rng.integers(0, 256, (2, 1080, 1920, 3), dtype=np.uint8)
    fb = two[[0, 1, 0, 1, 1, 0, 1, 0]]          # 8 frames, two distinct: one reference each
    fs = rng.integers(0, 256, (1, 240, 320, 3), dtype=np.uint8)
    c = fresh_ctx()
    d_b, d_s = torch.from_numpy(fb).cuda(), torch.from_numpy(fs).cuda()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        o_b = ingest_dev(c, d_b, 540, 960, side.cuda_stream, torch)
        o_s = ingest_dev(c, d_s, 120, 160, side.cuda_stream, torch)
    torch.cuda.synchronize()
    want = C.reference(two, 540, 960)
    got = o_b.cpu().numpy()
    for b, src in enumerate([0, 1, 0, 1, 1, 0, 1, 0]):
        assert np.array_equal(bits(got[b]), bits(want[src])), b
    assert_equals_references(o_s.cpu().numpy(), fs, 120, 160, "second")


def test_feature_runner_end_to_end(tmp_path):
    """runner.FeatureRunner (Runner.py:22-73 mirror) on two PNG-encoded synthetic RGB
    frames == oracle ingest + extract + match."""
    Image = pytest.importorskip("PIL.Image")
    from sfmfromscratch_amd import ScaleRotInvSIFT
    from sfmfromscratch_amd.runner import FeatureRunner, convert_matches_to_coords
    paths = []
    frames = [synth.make_frame_rgb_u8(540, 960, 7, i) for i in range(2)]
    for i, f in enumerate(frames):
        p = str(tmp_path / f"{i + 1}.png")
        Image.fromarray(f).save(p)
        paths.append(p)
    pp = dict(P_OCT, num_interest_points=800)
    r = FeatureRunner(paths[0], paths[1], feature_extractor_class=ScaleRotInvSIFT, extractor_params=pp,
                      match_threshold=0.85)
    g = [I.ingest(f, 0.5) for f in frames]
    assert np.array_equal(r._image1_bw, g[0]) and np.array_equal(r._image2_bw, g[1])
    X1, Y1, D1, _ = O.extract(g[0], pp)
    X2, Y2, D2, _ = O.extract(g[1], pp)
    assert np.array_equal(r.X1, X1) and np.array_equal(r.Y2, Y2)
    om, oc = O.match(D1, D2, 0.85)
    assert_matches_equal(om, oc, r.matches, r.confidences)
    p1, p2 = convert_matches_to_coords(r.matches, r.X1, r.Y1, r.X2, r.Y2)
    assert p1.shape == (len(r.matches), 2) and np.array_equal(p1[:, 0], r.X1[r.matches[:, 0]])
