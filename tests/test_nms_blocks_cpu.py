"""CPU: the block-driven certified NMS's skip rule and the host's choice of kernel.

tests/nms_blocks_ref.py restates the kernel's rule — a 4 x 4 block is looked at only where its
entry of the map M reaches the threshold — on top of the reference's predicate
(tests/select_ref.certified_candidates).  With M the blocks' true maxima, and with M raised to
other upper bounds, the rule must keep every reference candidate of every plane the GPU test
runs (tests/test_gpu_nms_blocks.py shares the cases).  The choice of kernel per level is a size
rule (extract_layout.h nms_blocks_level, read through sfm_debug_nms_blocks_rule): the levels it
picks at the two documented workloads are pinned here."""
from __future__ import annotations

import numpy as np
import pytest

from sfmfromscratch_amd import _native
from tests import nms_blocks_ref as nb

NAMES = [c[0] for c in nb.shared_cases()]


@pytest.mark.parametrize("name", NAMES)
def test_skip_rule_keeps_every_reference_candidate(name):
    _, R, tnms, _ = next(c for c in nb.shared_cases() if c[0] == name)
    skipped_some = False
    for b in range(len(R)):
        want = nb.reference_keys(R[b], int(tnms[b]))
        M = nb.block_max(R[b])
        assert M.shape == ((R[b].shape[0] + 3) // 4, R[b].shape[1] // 4)
        for m in (M, nb.inflated(M)):
            assert np.array_equal(nb.skip_candidates(R[b], int(tnms[b]), m), want), (name, b)
        with np.errstate(invalid="ignore"):
            skipped_some = skipped_some or bool((~(M >= nb.threshold_float(int(tnms[b])))).any())
    # the rule is exercised: at the high thresholds (and on the crafted planes) blocks are skipped
    if name.endswith(("_q0.97", "_none_pass", "_edges_zero_nan")) or name == "positions":
        assert skipped_some, name


def test_a_lower_bound_would_drop_candidates():
    """Non-vacuity: with the map lowered below the blocks' maxima the restated rule does lose
    candidates, so the equality above is a statement about upper bounds."""
    _, R, tnms, _ = next(c for c in nb.shared_cases() if c[0] == "70x132_q0.6")
    want = nb.reference_keys(R[1], int(tnms[1]))
    low = np.full_like(nb.block_max(R[1]), -np.inf)
    assert want.size > 0 and nb.skip_candidates(R[1], int(tnms[1]), low).size == 0


def test_position_planes_cover_the_sixteen_positions_and_nine_blocks():
    _, P, tnms, _ = next(c for c in nb.shared_cases() if c[0] == "positions")
    peaks = set()
    for b in range(16):
        idx = (nb.reference_keys(P[b], int(tnms[b])) & np.uint64(0xFFFFFFFF)).astype(np.int64)
        y, x = idx // 16, idx % 16
        peaks.add((int(y[0]), int(x[0])))               # the largest value sorts first
        assert P[b, y[0], x[0]] == 6.0
        blocks = {(int(a) // 4, int(c) // 4) for a, c in zip(y, x)}
        assert len(blocks) >= 8, (b, blocks)            # the plateau's candidates cross every border and corner
    assert peaks == {(4 + i, 4 + e) for i in range(4) for e in range(4)}


def test_size_rule_picks_the_documented_levels():
    """1080p (k = 2500 over 4 levels: 625 per level, vmin 80,000) and 4K (k = 8000 over 5 levels:
    1,600 per level, vmin 204,800): the two largest levels of each take the block kernel."""
    try:
        lib_rule = _native.nms_blocks_rule
        _native.load_library()
    except _native.NativeLibraryMissing:
        pytest.skip("libsfmfeat.so not built")
    hd = [(1080 >> l, 1920 >> l) for l in range(3)]
    uhd = [(2160 >> l, 3840 >> l) for l in range(4)]
    assert [lib_rule(h, w, 625) for h, w in hd] == [True, True, False]
    assert [lib_rule(h, w, 1600) for h, w in uhd] == [True, True, False, False]
    # shapes the kernel does not take, whatever the size
    assert not lib_rule(1080, 1922, 625) and not lib_rule(1080, 1920, 625, ksize=5)
