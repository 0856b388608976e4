"""csrc/extract_layout.h is the one place the device layout of an extraction is computed (the
reservation, the launch sequence and sfm_debug_copy_level read it).  A tiny C++ main built with
plain g++ prints the layout for a list of cases; checked here: the levels against the library's
sfm_pyramid_dims, every region inside its buffer, regions that are live together disjoint, and
every buffer size against the formulas the reservation used before the header existed (written
out below, not derived from the header)."""
from __future__ import annotations

import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, W, mode, params, serial)
CASES = [
    (32, 1080, 1920, "scalerot", dict(pyramid_level=4, pyramid_scale_factor=2, num_interest_points=2500), False),
    (4, 360, 640, "scalerot", dict(pyramid_level=4, pyramid_scale_factor=1.1, num_interest_points=2000), False),
    (4, 360, 640, "scalerot", dict(pyramid_level=4, pyramid_scale_factor=1.1, num_interest_points=2000), True),
    (2, 512, 1024, "scalerot", dict(pyramid_level=7, num_interest_points=1400), False),
    (2, 2160, 3840, "scalerot", dict(pyramid_level=5, num_interest_points=8000), False),
    (3, 37, 53, "scalerot", dict(pyramid_level=3, pyramid_scale_factor=1.3), False),
    (1, 16, 16, "naive", dict(), False),
]
BUFS = ["img0", "lvl", "R", "hist", "med", "medlist", "counts", "cand", "scratch", "kpx", "kpy", "kpc", "lc"]
PER_LEVEL = ["h", "w", "fw", "exact", "plane", "lvl", "hist", "state", "kp", "counter", "sel"]
MED_BINS, COUNTER_STRIDE, MEDIAN_STATE_BYTES = 2048, 32, 44  # kernels.h

MAIN = r"""
#include <stdio.h>
#include "extract_layout.h"
int main() {
  struct { int B, H, W, mode, k, fw, L; double s; int kcap, serial; } cases[] = {%s};
  for (auto& q : cases) {
    sfm_params p = {};
    p.mode = q.mode; p.num_interest_points = q.k; p.feature_width = q.fw; p.pyramid_level = q.L;
    p.pyramid_scale_factor = q.s;
    sfm::ExtractLayout y;
    if (sfm::extract_layout(&p, q.kcap, q.B, q.H, q.W, q.serial != 0, sfm::LayoutSwitches(), &y) != SFM_OK) return 1;
    printf("%%d %%d %%d %%d %%lld", y.L, y.L_aux, (int)y.pyr_fused, (int)y.select_merged, (long long)y.counter_block);
    for (int l = 0; l < y.L; ++l)
      printf(" %%d %%d %%d %%d %%lld %%lld %%lld %%lld %%lld %%lld %%lld", y.lv[l].h, y.lv[l].w, y.lv[l].fw, (int)y.exact[l],
             (long long)y.plane[l], (long long)y.lvl[l], (long long)y.hist[l], (long long)y.state[l],
             (long long)y.kp[l], (long long)y.counter[l], (long long)y.sel[l]);
    for (int i = 0; i < sfm::kExtractBufs; ++i) printf(" %%zu", y.bytes[i]);
    printf("\n");
  }
  return 0;
}
"""


def case_params(mode, pp):
    p = _abi.params_from_dict(pp, _abi.SFM_MODE_NAIVE if mode == "naive" else _abi.SFM_MODE_SCALEROT)
    L = 1 if mode == "naive" else p.pyramid_level
    kcap = p.num_interest_points if mode == "naive" else int(p.num_interest_points / L)
    return p, L, kcap


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("layout")
    rows = []
    for B, H, W, mode, pp, serial in CASES:
        p, L, kcap = case_params(mode, pp)
        rows.append("{%d, %d, %d, %d, %d, %d, %d, %r, %d, %d}" % (B, H, W, p.mode, p.num_interest_points,
                                                                  p.feature_width, p.pyramid_level,
                                                                  float(p.pyramid_scale_factor), kcap, int(serial)))
    src = tmp / "layout.cpp"
    src.write_text(MAIN % ", ".join(rows))
    exe = tmp / "layout"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "sfmfromscratch_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    out = []
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        v = [int(t) for t in line.split()]
        L = v[0]
        y = dict(L=L, L_aux=v[1], pyr_fused=bool(v[2]), select_merged=bool(v[3]), counter_block=v[4])
        lv = np.array(v[5:5 + L * len(PER_LEVEL)]).reshape(L, len(PER_LEVEL))
        y.update({"l_" + n: lv[:, i].tolist() for i, n in enumerate(PER_LEVEL)})
        y["bytes"] = dict(zip(BUFS, v[5 + L * len(PER_LEVEL):]))
        assert len(y["bytes"]) == len(BUFS)
        out.append(y)
    assert len(out) == len(CASES)
    return out


def regions(case, y):
    """{buffer: [(level, first byte, end byte)]} of everything a level addresses."""
    B, H, W, mode, pp, serial = case
    _, L, kcap = case_params(mode, pp)
    r = {b: [] for b in BUFS}
    for l in range(L):
        n = B * y["l_h"][l] * y["l_w"][l]
        r["R"].append((l, 4 * y["l_plane"][l], 4 * (y["l_plane"][l] + n)))
        r["cand"].append((l, 8 * y["l_plane"][l], 8 * (y["l_plane"][l] + n)))
        if l > 0:
            r["lvl"].append((l, 4 * y["l_lvl"][l], 4 * (y["l_lvl"][l] + n)))
        r["hist"].append((l, 4 * y["l_hist"][l], 4 * (y["l_hist"][l] + B * MED_BINS)))
        r["med"].append((l, MEDIAN_STATE_BYTES * y["l_state"][l], MEDIAN_STATE_BYTES * (y["l_state"][l] + B)))
        r["lc"].append((l, 4 * y["l_state"][l], 4 * (y["l_state"][l] + B)))
        for b in ("kpx", "kpy", "kpc"):
            r[b].append((l, 4 * y["l_kp"][l], 4 * (y["l_kp"][l] + B * max(kcap, 1))))
        for blk in range(4):
            o = blk * y["counter_block"] + y["l_counter"][l]
            r["counts"].append(((blk, l), 8 * o, 8 * (o + B * COUNTER_STRIDE)))
        r["medlist"].append((l, 4 * y["l_sel"][l], 4 * (y["l_sel"][l] + n)))
        r["scratch"].append((l, 8 * y["l_sel"][l], 8 * (y["l_sel"][l] + n)))
    r["img0"].append((0, 0, 4 * B * H * W))
    return r


def disjoint(a, b):
    return a[2] <= b[1] or b[2] <= a[1]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_levels_equal_the_librarys_pyramid_dims(layouts, i):
    B, H, W, mode, pp, serial = CASES[i]
    p, L, _ = case_params(mode, pp)
    d = np.zeros(2 * L, np.int32)
    lib = _native.load_library()
    assert lib.sfm_pyramid_dims(ctypes.byref(p), H, W, d.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    y = layouts[i]
    assert y["L"] == L
    assert [v for hw in zip(y["l_h"], y["l_w"]) for v in hw] == d.tolist()


@pytest.mark.parametrize("i", range(len(CASES)))
def test_regions_inside_their_buffers_and_disjoint(layouts, i):
    case, y = CASES[i], layouts[i]
    L, L_aux = y["L"], y["L_aux"]
    assert L_aux == (0 if case[5] else min(L, 2))
    r = regions(case, y)
    for b, regs in r.items():
        for _, lo, hi in regs:
            assert 0 <= lo <= hi <= y["bytes"][b], (b, lo, hi, y["bytes"][b])
    # the per-level regions of one buffer (the selection regions are taken in turn unless merged)
    for b in set(BUFS) - {"medlist", "scratch"}:
        for p, q in itertools.combinations(r[b], 2):
            assert disjoint(p, q), (b, p, q)
    for b in ("medlist", "scratch"):
        aux, caller = r[b][:L_aux], r[b][L_aux:]
        for p, q in itertools.product(aux, caller):  # the two streams select concurrently
            assert disjoint(p, q), (b, p, q)
        if y["select_merged"]:  # one launch selects every caller-stream level
            for p, q in itertools.combinations(caller, 2):
                assert disjoint(p, q), (b, p, q)
    assert y["select_merged"] == (1 < L - L_aux <= 4)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_sizes_and_predicates_are_the_earlier_formulas(layouts, i):
    """The byte sizes as reserve_impl computed them (and the level predicates as extract_impl
    did) before extract_layout.h."""
    B, H, W, mode, pp, serial = CASES[i]
    _, L, kcap = case_params(mode, pp)
    y = layouts[i]
    hw = list(zip(y["l_h"], y["l_w"]))
    A0 = H * W
    Arest = sum(h * w for h, w in hw[1:])
    sel_slots = B * (2 * A0 + Arest)
    nk = L * B * max(kcap, 1)
    want = {"img0": B * A0 * 4, "lvl": B * Arest * 4, "R": B * (A0 + Arest) * 4, "hist": L * B * MED_BINS * 4,
            "med": L * B * MEDIAN_STATE_BYTES, "medlist": sel_slots * 4, "counts": 4 * L * B * 8 * COUNTER_STRIDE,
            "cand": B * (A0 + Arest) * 8, "scratch": sel_slots * 8, "kpx": nk * 4, "kpy": nk * 4, "kpc": nk * 4,
            "lc": L * B * 4}
    # ensure() rounds an empty request up to 16 bytes; the layout reports the request
    assert y["bytes"] == want
    assert y["l_exact"] == [int(h * w < 128 * kcap) for h, w in hw]
    fused = (L >= 4 and H % 8 == 0 and W % 8 == 0
             and all(hw[l][0] << l == H and hw[l][1] << l == W for l in (1, 2, 3)))
    assert y["pyr_fused"] == fused
    assert fused == (i in (0, 3, 4))
