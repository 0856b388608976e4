"""GPU: the Harris window's pipelined tap and gradient loads (harris.hip WinBlocks) leave R
bit-identical to the oracle's harris_response.

The window is a sequence of blocks (gradient row x output row pair); each block's tap pairs are
loaded into SGPRs while the block before runs, and each row's gradients are read from LDS a
block ahead.  What can go wrong is a block running with another block's taps or gradients, so
the cases cover every window size whose block sequence differs (3, 5, 7, 9: first- and
last-row half-packed taps included) and every other size the launcher dispatches (1, 2, 4, 6,
8, 11, 13, 15), border tiles in both directions, the non-vector path
(W % 4 != 0), workgroups that walk more than one tile (the first block's taps are loaded
before the previous phase's barrier) and the 64 x 32 form of the small levels."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from sfmfromscratch_amd import _abi, _native, synth
from tests.golden_util import P_MAIN, P_OCT

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("gs", [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13, 15])
@pytest.mark.parametrize("H,W", [(64, 64), (70, 200), (97, 131)])
def test_one_plane_R_bitexact_vs_oracle(H, W, gs):
    """Every window size launch_harris_levels dispatches: the even ones have the anchor gs // 2
    off the window's centre, 11-15 are the sizes that reach one wave per SIMD."""
    pp = dict(P_MAIN, gaussian_size=gs, ksize=3)
    img = synth.make_frame(H, W, 23, 2)
    R, med, ncand = _native.debug_harris(img, _abi.params_from_dict(pp, _abi.SFM_MODE_SCALEROT))
    Ro = O.harris_response(img, pp)
    assert np.array_equal(bits(R), bits(Ro))
    assert np.float32(med) == O.median(Ro)
    _, _, _, dbg = O.detect(img, 10 ** 7, 0, pp, debug=True)
    assert ncand == dbg["n_candidates"]


def batch_32_planes_vs_oracle(W, L, pp, check_images):
    torch = pytest.importorskip("torch")
    from sfmfromscratch_amd.pipeline import BatchExtractor
    B, H = 32, 200
    u8 = synth.make_batch_u8(B, H, W, seed=91)
    ex = BatchExtractor(pp)
    s = ex.extract(torch.from_numpy(u8).cuda())
    torch.cuda.synchronize()
    planes = (0, 13, 31)
    want = {b: synth.u8_to_gray(u8[b]) for b in planes}
    for lvl, (h, w) in enumerate(O.pyramid_dims(H, W, L, 2)):
        R = torch.empty((B, h, w), dtype=torch.float32, device="cuda")
        im = torch.empty((B, h, w), dtype=torch.float32, device="cuda")
        ex.ctx.copy_level(lvl, 0, R.data_ptr(), 0)
        ex.ctx.copy_level(lvl, 1, im.data_ptr(), 0)
        torch.cuda.synchronize()
        for b in planes:
            img = im[b].cpu().numpy()
            if check_images:  # the level image itself: the oracle's resize, level by level
                if lvl > 0:
                    want[b] = O.resize(want[b], h, w)
                assert np.array_equal(bits(img), bits(want[b])), (lvl, b)
            Ro = O.harris_response(img, pp)
            assert np.array_equal(bits(R[b].cpu().numpy()), bits(Ro)), (lvl, b)
    counts, xy = s.count.cpu().numpy(), s.xy.cpu().numpy()
    for b in planes:
        X, Y, _, _ = O.extract(synth.u8_to_gray(u8[b]), pp)
        n = counts[b]
        assert n == len(X) and n > 0
        assert np.array_equal(xy[b, :n, 0], X) and np.array_equal(xy[b, :n, 1], Y)


@pytest.mark.parametrize("W", [328, 330])
def test_batch_32_planes_levels_R_and_keypoints_vs_oracle(W):
    """32 planes of 200 x W, three octaves: level 0 has 24 tiles for 14 workgroups per plane
    (two tiles per workgroup, form 0), levels 1 and 2 take the 64 x 32 form.  R of planes 0, 13
    and 31 at every level against the oracle on the same level images, and their keypoints
    against the oracle's extraction."""
    batch_32_planes_vs_oracle(W, 3, dict(P_OCT, pyramid_level=3, num_interest_points=300), check_images=False)


@pytest.mark.parametrize("gs", [4, 7, 15])
def test_batch_32_planes_fused_pyramid_levels_images_R_and_keypoints_vs_oracle(gs):
    """The fused pyramid at other window sizes: four octaves of 200 x 328 (both multiples of 8),
    so the level-0 Harris launch also writes levels 1-3 (extract_layout.h pyr_fused needs
    L >= 4; the three-octave test above resizes with separate launches).  It is taken at every
    gaussian_size, an even one and the largest included.  Level 0 has 6 x 4 = 24 tiles of
    64 x 64; harris.hip's harris_plan gives a batch of 32 planes 448 / 32 = 14 workgroups per
    plane, so T = ceil(24 / 14) = 2 tiles per workgroup at every window size (form 0 is the only
    form of a fused launch).  Level images of planes 0, 13, 31 against the oracle's resize, R on
    them and the keypoints against the oracle."""
    B, H, W = 32, 200, 328
    assert H % 8 == 0 and W % 8 == 0
    tiles = -(-W // 64) * -(-H // 64)
    per_plane = (448 * 2 // 2) // B           # slots2 * WPC / 2 over the batch, WPC = 2 in form 0
    assert tiles == 24 and per_plane == 14 and -(-tiles // per_plane) >= 2
    pp = dict(P_OCT, pyramid_level=4, num_interest_points=300, gaussian_size=gs)
    batch_32_planes_vs_oracle(W, 4, pp, check_images=True)
