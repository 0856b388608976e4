"""CPU: the restatement of the feature-track rules (tests/tracks_ref.py) against scipy's
connected_components on every case, the conditions the GPU tests rely on, the restated N-view
triangulation against the same SVD in extended-precision rows, and the binding of the two C-ABI
calls against the header's prototypes.

Figure measured here (printed before its assertion), bound 100 x the figure:
  TRI_LD  |X_rest - X_ld| / |X_ld| over the planted scene's tracks, X_ld from the rows assembled
          in np.longdouble and rounded to float64 before the same np.linalg.svd: measured
          5.125e-15, bound 5.125e-13.  This is the restatement's own distance from the exact
          rows, the floor under any comparison against it."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from tests import tracks_ref as TR
from sfmfromscratch_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_TRI_LD = 5.125e-15
TRI_LD = 100 * MEASURED_TRI_LD


@pytest.mark.parametrize("name", TR.CASE_NAMES)
def test_restatement_components_equal_scipys(name):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    c = TR.case(name)
    cap, nimg = c["cap"], len(c["count"])
    N = nimg * cap
    edges, skipped = TR.graph_edges(c["count"], cap, c["pairs"], c["matches"], c["nmatch"], c["keep"])
    label = TR.component_labels(c["count"], cap, edges)
    g = coo_matrix((np.ones(len(edges), np.int8), (edges[:, 0], edges[:, 1])), shape=(N, N))
    _, sl = connected_components(g, directed=False)
    smallest = np.full(sl.max() + 1, N, np.int64)
    np.minimum.at(smallest, sl, np.arange(N))
    valid = label >= 0
    assert np.array_equal(label[valid], smallest[sl][valid])
    # rows at or beyond count carry no edge
    assert (np.bincount(edges.ravel(), minlength=N)[~valid] == 0).all()
    e = TR.expected(name)
    assert e["out_n"][4] == skipped
    # the outputs agree with each other: CSR, node_track, counters
    T, n_obs = int(e["out_n"][0]), int(e["out_n"][1])
    assert len(e["offsets"]) == T + 1 and e["offsets"][-1] == n_obs == len(e["obs_slot"])
    for t in range(T):
        s = e["obs_slot"][e["offsets"][t]:e["offsets"][t + 1]]
        r = e["obs_row"][e["offsets"][t]:e["offsets"][t + 1]]
        assert (np.diff(s) > 0).all() and (e["node_track"][s, r] == t).all()
    assert (e["node_track"] >= 0).sum() == n_obs


def test_case_conditions_the_gpu_tests_rely_on():
    e = TR.expected("random", 3)
    st = dict(zip(TR.STATS, e["out_n"].tolist()))
    print("random case, min_len 3:", st)
    assert st["n_tracks"] >= 1 and st["inconsistent"] >= 1 and st["short"] >= 1 and st["skipped_edges"] >= 1
    c = TR.case("random")
    assert len(c["count"]) == 12 and c["cap"] == 257 and len(c["pairs"]) == 66
    # an inconsistent component small enough to take the (root, slot) table, not the counting shortcut
    lab = e["label"]
    sizes = np.bincount(lab[e["node_track"].ravel() == -2])
    assert ((sizes > 0) & (sizes <= 12)).any()

    h2, h3 = TR.expected("hand", 2), TR.expected("hand", 3)
    assert h2["out_n"].tolist() == [2, 6, 1, 0, 2, 4] and h3["out_n"].tolist() == [1, 4, 1, 1, 2, 4]
    assert h2["obs_slot"].tolist() == [0, 1, 2, 3, 0, 1] and h2["obs_row"].tolist() == [0, 0, 0, 0, 3, 3]
    nt = h2["node_track"]
    assert nt[0, 1] == nt[1, 1] == nt[2, 1] == nt[2, 2] == -2      # reaches rows 1 and 2 of slot 2
    assert nt[2, 3] == -1 and nt[1, 7] == -1 and nt[0, 5] == -1    # cut off by keep; beyond count; its partner
    assert h3["node_track"][0, 3] == -3

    lp = TR.expected("long_path")
    assert lp["out_n"].tolist() == [1, 300, 0, 0, 0, 300]
    g = TR.expected("giant")
    assert g["out_n"].tolist() == [1, 64, 1, 0, 0, 64] and (g["node_track"][:, 1:] == -2).all()
    assert TR.expected("no_pairs")["out_n"].tolist() == [0, 0, 0, 0, 0, 0]
    z = TR.expected("zero_counts")["out_n"]
    assert z[0] == 0 and z[4] >= 1
    for name in TR.CASE_NAMES:
        if name.startswith("size_"):
            a, b = TR.expected(name, 2)["out_n"], TR.expected(name, 3)["out_n"]
            assert a[0] >= b[0] and a[0] + a[3] == b[0] + b[3]
    # a permutation of the input is the same graph
    p = TR.permuted(TR.case("random"), 1)
    q = TR.build_tracks(p["count"], p["cap"], p["pairs"], p["matches"], p["nmatch"], p["keep"], 3)
    assert all(np.array_equal(q[k], e[k]) for k in ("offsets", "obs_slot", "obs_row", "node_track", "out_n"))


def test_restated_triangulation_against_extended_precision_rows():
    s = TR.planted_scene()
    e = TR.build_tracks(s["count"], s["cap"], s["pairs"], s["matches"], s["nmatch"], None, 2)
    lens = np.diff(e["offsets"])
    assert {2, 3, 6} <= set(lens.tolist()) and e["out_n"][2] >= 1   # wrong matches made inconsistent components
    X, views = TR.triangulate_tracks(e["offsets"], e["obs_slot"], e["obs_row"], s["xy"], s["P"])
    assert np.array_equal(views, lens) and np.isfinite(X).all()
    worst = 0.0
    for t in range(len(lens)):
        A, _ = TR.track_rows(e["offsets"], e["obs_slot"], e["obs_row"], s["xy"], s["P"], None, t, np.longdouble)
        h = np.linalg.svd(A.astype(np.float64))[2][-1]
        worst = max(worst, float(np.linalg.norm(X[t] - h[:3] / h[3]) / np.linalg.norm(h[:3] / h[3])))
    print(f"MEASURED triangulate_tracks restatement vs extended-precision rows: {worst:.3e}")
    assert worst <= TRI_LD
    # the clean tracks land on the planted points (integer pixels: a few millimetres at 8 m)
    clean = [t for t in range(len(lens)) if lens[t] == 6]
    d = np.linalg.norm(X[clean][:, None, :] - s["Xw"][None], axis=2).min(axis=1)
    assert np.median(d) < 0.02


C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double,
           "float": ctypes.c_float}


def header_prototype(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sfmfeat.h")).read(), flags=re.S)
    m = re.search(r"(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sfmfeat.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        if "*" in a:
            args.append(ctypes.c_void_p)
        else:
            args.append(C_TYPES[a.replace("const ", "").split()[0]])
    return C_TYPES[m.group(1)], args


@pytest.mark.parametrize("name", ["sfm_build_tracks_dev", "sfm_triangulate_tracks_dev"])
def test_abi_declares_the_track_calls_with_the_headers_signatures(name):
    res, args = header_prototype(name)
    assert name in _abi.TRACK_SIGNATURES
    assert _abi.TRACK_SIGNATURES[name] == (res, args)
    from sfmfromscratch_amd import _native
    assert _native.SIGNATURES[name] == (res, args)
    lib = _native.load_library()
    assert hasattr(lib, name)
    # argument errors come back before any device call
    fn = getattr(lib, name)
    assert fn(*[None if a is ctypes.c_void_p else 0 for a in args]) == _abi.SFM_EINVAL
