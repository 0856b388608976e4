"""CPU: the schedule of the Harris window's loads in the built library's ISA (tools/isa_phases.py).

The window's tap pairs are scalar loads into SGPRs.  A scalar load returns out of order, so
the wait that retires it is `s_waitcnt lgkmcnt(0)`, which drains every scalar load and LDS read
issued before it; a load issued right before such a wait exposes its whole latency ten times
per tile.  harris.hip (WinBlocks) therefore issues every block's taps a block of fmas ahead,
directly behind the wait that retires the block before's.  A compiler or source change that
moves the loads back to their use fails here, on the CPU.

Figures of the kernel this file was written against (profiles/r07_harris_tap_loads.txt): 45 tap
loads in the window, 84-110 VALU instructions before the next lgkmcnt wait (the parent commit:
48 loads, 0-15).  SGPR spill moves in the tile loop: 2, the parent commit's count and the bar
below.  The staggered sets alone brought 9 (seven kernel-wide invariants reloaded once per tile);
reading the histogram pointer and the scan parameters after the tile loop and building harris.o
with -mllvm -greedy-reverse-local-assignment (csrc/Makefile) brought them back to 2."""
from __future__ import annotations

import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sfmfromscratch_amd", "lib", "libsfmfeat.so")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "k_harrisILi7ELb1ELi0ELi0E"
# half a row of the window is 84 VALU instructions; the bar is below it so that a reordered
# prologue cannot fail it
MIN_COVER = 64
# v_readlane_b32 / v_writelane_b32 in the tile loop of the kernel before the loads were staggered
LANE_MOVES_BEFORE = 2


@pytest.fixture(scope="module")
def harris_isa():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_phases as ip
    tools = [os.path.join(LLVM, t) for t in ("llvm-objdump", "clang-offload-bundler")]
    if not os.path.exists(LIB) or not all(os.path.exists(t) for t in tools):
        pytest.skip("library or ROCm LLVM tools not available")
    _, ins = ip.kernel_body(ip.disassemble(LIB), KERNEL)
    return ip, ins


def test_every_window_tap_load_has_a_block_of_valu_before_the_next_wait(harris_isa):
    ip, ins = harris_isa
    cover = ip.scalar_load_cover(ins)
    print("\n".join(f"{off:6d} {valu:4d}  {text}" for off, text, valu in cover))
    assert len(cover) >= 14, cover  # the scan found the window's loads
    short = [(off, text, valu) for off, text, valu in cover if valu < MIN_COVER]
    assert not short, f"{len(short)} of {len(cover)} tap loads wait within {MIN_COVER} VALU instructions: {short[:3]}"


def test_tile_loop_has_no_more_sgpr_spill_moves_than_before(harris_isa):
    ip, ins = harris_isa
    n = ip.lane_moves(ins)
    print("lane moves in the tile loop:", n)
    assert n <= LANE_MOVES_BEFORE, f"{n} v_readlane/v_writelane in the tile loop (before: {LANE_MOVES_BEFORE})"
