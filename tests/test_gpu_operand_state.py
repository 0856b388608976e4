"""The matcher operand buffers of a context have one owner record (csrc/ctx.h MatchOperandsWs,
api_match.hip operands_claim): whatever rewrites them for another table, or reallocates them,
leaves nothing of the earlier table valid.  The sequences here are permitted by the C-ABI but
never issued by BatchPipeline; before the single record they matched against another table's
operands (or uninitialised memory) without an error."""
from __future__ import annotations

import pytest

from sfmfromscratch_amd import synth
from tests.golden_util import P_OCT

pytestmark = pytest.mark.gpu

B, H, W = 3, 270, 480
PARAMS = dict(P_OCT, num_interest_points=800)


def frames(torch, n, seed):
    return torch.from_numpy(synth.make_batch_u8(n, H, W, seed=seed)).cuda()


def fused_lane(torch):
    """An extractor whose context writes the matcher operands itself, a matcher on that context,
    and a second, plain extractor for the other tables."""
    from sfmfromscratch_amd.pipeline import BatchExtractor, BatchMatcher
    ex = BatchExtractor(PARAMS)
    ex.ctx.set_fused_prep(True)
    return ex, BatchMatcher(0.85, ctx=ex.ctx), BatchExtractor(PARAMS)


def reference(slots, pairs):
    from sfmfromscratch_amd.pipeline import BatchMatcher
    return BatchMatcher(0.85).match(slots, pairs)  # a fresh matcher on its own context


def assert_same(torch, got, ref):
    torch.cuda.synchronize()
    for g, r in zip(got, ref):
        assert torch.equal(g, r)


def test_fused_slots_do_not_outlive_their_table():
    """extract(T) -> match(T) -> match(U) -> match(T) -> match(V, reallocating) -> match(T): every
    match equals a fresh matcher's.  (The third and fifth steps reused the extraction's slots
    after match(U) / the reallocation had overwritten them.)"""
    torch = pytest.importorskip("torch")
    from sfmfromscratch_amd.pipeline import all_pairs
    ex, m, other = fused_lane(torch)
    pairs = torch.from_numpy(all_pairs(B)).cuda()
    pairs_v = torch.from_numpy(all_pairs(16)[:8]).cuda()
    T = ex.extract(frames(torch, B, 201))
    U = other.extract(frames(torch, B, 202))
    V = other.extract(frames(torch, 16, 203))  # more slots than B + 8: the operand buffers grow
    ref_t, ref_u, ref_v = reference(T, pairs), reference(U, pairs), reference(V, pairs_v)
    assert_same(torch, m.match(T, pairs), ref_t)
    assert_same(torch, m.match(U, pairs), ref_u)
    assert_same(torch, m.match(T, pairs), ref_t)
    assert_same(torch, m.match(V, pairs_v), ref_v)
    assert_same(torch, m.match(T, pairs), ref_t)


def test_fused_extraction_invalidates_a_prep():
    """prep(T) -> fused extraction into another table -> prepped match(T) is refused (SFM_ESTATE:
    the extraction rewrote the operand slots); after a new prep(T) it equals a fresh matcher's."""
    torch = pytest.importorskip("torch")
    from sfmfromscratch_amd.pipeline import all_pairs
    ex, m, _ = fused_lane(torch)
    pairs = torch.from_numpy(all_pairs(B)).cuda()
    T = ex.extract(frames(torch, B, 201))
    ref_t = reference(T, pairs)
    m.prep(T)
    Wt = ex.new_slots(B)
    ex.extract(frames(torch, B, 204), out=Wt)
    with pytest.raises(RuntimeError):
        m.match(T, pairs, prepped=True)
    m.prep(T)
    assert_same(torch, m.match(T, pairs, prepped=True), ref_t)
