"""GPU: the Harris window's pipelined tap and gradient loads (harris.hip WinBlocks) leave R
bit-identical to the oracle's harris_response.

The window is a sequence of blocks (gradient row x output row pair); each block's tap pairs are
loaded into SGPRs while the block before runs, and each row's gradients are read from LDS a
block ahead.  What can go wrong is a block running with another block's taps or gradients, so
the cases cover every window size whose block sequence differs (3, 5, 7, 9: first- and
last-row half-packed taps included), border tiles in both directions, the non-vector path
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


@pytest.mark.parametrize("gs", [3, 5, 7, 9])
@pytest.mark.parametrize("H,W", [(64, 64), (70, 200), (97, 131)])
def test_one_plane_R_bitexact_vs_oracle(H, W, gs):
    pp = dict(P_MAIN, gaussian_size=gs, ksize=3)
    img = synth.make_frame(H, W, 23, 2)
    R, _, _ = _native.debug_harris(img, _abi.params_from_dict(pp, _abi.SFM_MODE_SCALEROT))
    assert np.array_equal(bits(R), bits(O.harris_response(img, pp)))


@pytest.mark.parametrize("W", [328, 330])
def test_batch_32_planes_levels_R_and_keypoints_vs_oracle(W):
    """32 planes of 200 x W, three octaves: level 0 has 24 tiles for 14 workgroups per plane
    (two tiles per workgroup, form 0), levels 1 and 2 take the 64 x 32 form.  R of planes 0, 13
    and 31 at every level against the oracle on the same level images, and their keypoints
    against the oracle's extraction."""
    torch = pytest.importorskip("torch")
    from sfmfromscratch_amd.pipeline import BatchExtractor
    B, H, L = 32, 200, 3
    pp = dict(P_OCT, pyramid_level=L, num_interest_points=300)
    u8 = synth.make_batch_u8(B, H, W, seed=91)
    ex = BatchExtractor(pp)
    s = ex.extract(torch.from_numpy(u8).cuda())
    torch.cuda.synchronize()
    planes = (0, 13, 31)
    for lvl, (h, w) in enumerate(O.pyramid_dims(H, W, L, 2)):
        R = torch.empty((B, h, w), dtype=torch.float32, device="cuda")
        im = torch.empty((B, h, w), dtype=torch.float32, device="cuda")
        ex.ctx.copy_level(lvl, 0, R.data_ptr(), 0)
        ex.ctx.copy_level(lvl, 1, im.data_ptr(), 0)
        torch.cuda.synchronize()
        for b in planes:
            Ro = O.harris_response(im[b].cpu().numpy(), pp)
            assert np.array_equal(bits(R[b].cpu().numpy()), bits(Ro)), (lvl, b)
    counts, xy = s.count.cpu().numpy(), s.xy.cpu().numpy()
    for b in planes:
        X, Y, _, _ = O.extract(synth.u8_to_gray(u8[b]), pp)
        n = counts[b]
        assert n == len(X) and n > 0
        assert np.array_equal(xy[b, :n, 0], X) and np.array_equal(xy[b, :n, 1], Y)
