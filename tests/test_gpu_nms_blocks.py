"""GPU: the block-driven certified 3x3 NMS (nms.hip k_nms_blocks) against the band kernel and the
numpy restatement, and the block-maximum map the Harris kernel writes for it.

Kernel level (sfm_debug_nms_blocks, debug_nms.hip): on the planes of tests/nms_blocks_ref.py —
8 x 8, 12 x 16, 70 x 132 (a partial Harris tile in both axes) and 66 x 260, two of them with
H % 4 == 2; a maximum at each of a block's 16 positions inside a plateau that crosses the
block's borders and corners; maxima on the image's edges and corners; thresholds at the -inf end
and above every value; -0.0 and a NaN; a fallback plane in a batch of three — the band kernel,
the block kernel on the blocks' true maxima and the block kernel on raised upper bounds must
each give exactly the restatement's sorted (key, index) list (tests/select_ref.py's predicate).

End to end: extraction with the block kernel forced wherever the shape allows it against the
band kernel everywhere, on 128 x 192 and 70 x 132 frames with two levels: keypoints, descriptors
and counts bit for bit.  The switch is sfm_debug_set_nms_blocks — the shipped library does not
read the diagnostic SFMFEAT_NMS_BLOCKS, and the call takes effect at the next extraction, so
both runs share this process.  The map as k_harris wrote it is read back beside R: at least the
block maximum of R at every in-image block, equal to it on the tiles that lie inside the image."""
from __future__ import annotations

import numpy as np
import pytest

from sfmfromscratch_amd import _native, synth
from tests import nms_blocks_ref as nb
from tests.golden_util import P_OCT

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in nb.shared_cases()]
_REF = {}


def reference(name):
    """The restatement's lists of a case, computed once and shared by the three kernel runs."""
    if name not in _REF:
        _, R, tnms, fb = next(c for c in nb.shared_cases() if c[0] == name)
        _REF[name] = [np.zeros(0, np.uint64) if fb[b] else nb.reference_keys(R[b], int(tnms[b])) for b in range(len(R))]
    return _REF[name]


@pytest.mark.parametrize("form", ["band", "blocks", "blocks_inflated"])
@pytest.mark.parametrize("name", NAMES)
def test_kernels_equal_the_restatement(name, form):
    _, R, tnms, fb = next(c for c in nb.shared_cases() if c[0] == name)
    got = _native.debug_nms_blocks(R, tnms, fb, blocks=form != "band", inflate=form == "blocks_inflated")
    want = reference(name)
    for b in range(len(R)):
        assert got[b].size == want[b].size, (name, form, b, got[b].size, want[b].size)
        assert np.array_equal(got[b], want[b]), (name, form, b)
    if name.endswith("_fallback"):
        assert got[1].size == 0 and want[0].size > 0 and want[2].size > 0


def extract(frames, params, mode):
    import torch

    from sfmfromscratch_amd.pipeline import BatchExtractor
    _native.set_nms_blocks(mode)
    try:
        ex = BatchExtractor(params)
        slots = ex.extract(torch.from_numpy(frames).cuda())
        torch.cuda.synchronize()
        B, H, W = frames.shape
        out = {"count": slots.count.cpu().numpy(), "xy": slots.xy.cpu().numpy(),
               "desc": slots.desc.cpu().numpy().view(np.uint32)}
        Rm = torch.zeros((B, H, W), dtype=torch.float32, device="cuda")
        ex.ctx.copy_level(0, 0, Rm.data_ptr(), 0)
        torch.cuda.synchronize()
        out["R"] = Rm.cpu().numpy()
        if mode == 1:
            M = torch.full((B, _native.bmax_stride(H, W)), float("nan"), dtype=torch.float32, device="cuda")
            ex.ctx.copy_level(0, 2, M.data_ptr(), 0)
            torch.cuda.synchronize()
            out["M"] = M.cpu().numpy()[:, :(H + 3) // 4 * (W // 4)].reshape(B, (H + 3) // 4, W // 4)
        else:
            with pytest.raises(Exception):   # the band kernel's levels write no map
                ex.ctx.copy_level(0, 2, Rm.data_ptr(), 0)
        out["fallback"] = ex.ctx.select_stats()[0]
        return out
    finally:
        _native.set_nms_blocks(-2)


@pytest.mark.parametrize("H,W", [(128, 192), (70, 132)])
def test_extraction_with_blocks_equals_band_and_the_map_bounds_r(H, W):
    B = 3
    frames = np.stack([synth.make_frame_u8(H, W, 77, i) for i in range(B)])
    # 40 keypoints per level: both levels of 128 x 192 and level 0 of 70 x 132 hold at least
    # 128 x 40 pixels, so they certify by size and run the certified NMS
    params = dict(P_OCT, pyramid_level=2, num_interest_points=80)
    band = extract(frames, params, 0)
    blk = extract(frames, params, 1)
    assert np.array_equal(blk["count"], band["count"]) and blk["count"].min() > 0
    for b, k in enumerate(band["count"]):
        assert np.array_equal(blk["xy"][b, :k], band["xy"][b, :k]), b
        assert np.array_equal(blk["desc"][b, :k], band["desc"][b, :k]), b
    assert np.array_equal(blk["R"].view(np.uint32), band["R"].view(np.uint32))
    # level 0's planes took the certified path (else the NMS kernels under test did not decide them)
    assert band["fallback"] < 2 * B and blk["fallback"] == band["fallback"]
    for b in range(B):
        want = nb.block_max(blk["R"][b])
        M = blk["M"][b]
        assert not np.isnan(M).any() and (M >= want).all(), b
        ih, iw = H // 64 * 16, W // 64 * 16   # blocks of the 64 x 64 tiles that lie inside the image
        assert ih > 0 and iw > 0
        assert np.array_equal(M[:ih, :iw], want[:ih, :iw]), b
