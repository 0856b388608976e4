"""GPU: the structure stage (refine.hip; pose.non_linear_triangulation, refine_points_batch,
reprojection_error, link_points, initial_structure) against the reference's own outputs and
this repository's restatement (tests/golden/structure.npz, tests/structure_ref.py).  The
conditions the comparisons rely on are asserted on the CPU in tests/test_structure_cpu.py.

Tolerances.  Each is 100 x the largest value measured on the MI355X over the fixture, with
its cap; every figure is printed before its assertion.
  X_GPU_TOL    ||X_gpu - X_rest|| / ||X_rest||, all cases: measured 3.725e-9 (k1k2base; the
               others 5.9e-10 to 2.8e-9), so the cap, 1e-8, is the bound.  Accepting a step on
               "cost strictly smaller" locates a minimiser to about sqrt(eps) of its scale, which
               is what two implementations of this rule differ by.
  COST_GPU_TOL |cost_gpu - cost_rest| / cost_rest, all cases: measured 3.212e-11 (wild10), bound
               3.212e-9 (cap 1e-8)
  ERR_TOL      reprojection errors against the restatement's, |e_gpu - e_rest| / (e_rest + ||p||)
               with p the observed pixel: measured 5.659e-16 (wild10), bound 5.659e-14 (cap 1e-10).  An error e is the
               norm of p - pi(P X), a difference of numbers of about ||p||, so float64 resolves it
               to ulp(||p||) ~ 1e-13 absolute whatever its size.  The first version of this test
               divided by e alone and measured 2.5e-10 on wild10 (a point whose error is 4.7e-4
               pixels, one ulp of its 685-pixel coordinate), above the cap; under that measure
               the restatement itself is 8.1e-11 (wild10) and 5.4e-11 (c200) from the same
               formula in extended precision, so the measure, not the kernel, was at fault.
  MEAN_TOL     |mean_gpu - mean_rest| / mean_rest: measured 3.332e-14 (c1), bound 3.332e-12
X_REF_TOL and COST_DELTA (against the reference) are defined and justified in
tests/structure_ref.py / tests/test_structure_cpu.py."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from sfmfromscratch_amd import _abi, _native, pose
from tests import structure_ref as SR
from tests.golden_util import load

pytestmark = pytest.mark.gpu

MEASURED_X = 3.725e-9
MEASURED_COST = 3.212e-11
MEASURED_ERR = 5.659e-16
MEASURED_MEAN = 3.332e-14
X_GPU_TOL = min(1e-8, 100 * MEASURED_X)
COST_GPU_TOL = min(1e-8, 100 * MEASURED_COST)
ERR_TOL = min(1e-10, 100 * MEASURED_ERR)
MEAN_TOL = min(1e-10, 100 * MEASURED_MEAN)

REFINE_NAMES = list(SR.refine_cases().keys())
LINK_NAMES = list(SR.link_cases().keys())


def rcase(z, name):
    g = lambda k: z[f"{name}_{k}"]
    return g("X0"), g("p1"), g("p2"), g("P1"), g("P2")


def rel_err(X, ref):
    return np.linalg.norm(X - ref, axis=1) / np.linalg.norm(ref, axis=1)


_cache = {}


def refined(name):
    """One device refinement per case, shared by the tests (never modified)."""
    if name not in _cache:
        info = {}
        X = pose.non_linear_triangulation(*rcase(load("structure.npz"), name), info=info)
        _cache[name] = (X, info)
    return _cache[name]


@pytest.mark.parametrize("name", REFINE_NAMES)
def test_refine_vs_restatement(name):
    z = load("structure.npz")
    X, info = refined(name)
    g = lambda k: z[f"{name}_rest_{k}"]
    assert X.shape == g("X").shape and X.dtype == np.float64
    ex = rel_err(X, g("X")).max()
    ec = (np.abs(info["cost"] - g("cost")) / g("cost")).max()
    firm = g("all_firm")
    print(f"MEASURED refine {name}: X vs restatement {ex:.3e}, cost {ec:.3e}; {int(firm.sum())} of {len(firm)} "
          f"points without a marginal comparison; accepted steps gpu max {info['iters'].max()} "
          f"restatement max {g('iters').max()}; status counts {np.bincount(info['status'], minlength=4).tolist()}")
    assert ex <= X_GPU_TOL
    assert ec <= COST_GPU_TOL
    # where no comparison of the restatement's run was marginal the device takes the same path
    assert np.array_equal(info["iters"][firm], g("iters")[firm])
    assert np.array_equal(info["status"][firm], g("status")[firm])
    # and every point takes at least the accepted steps that came before the first marginal one
    assert (info["iters"] >= g("firm")).all()


@pytest.mark.parametrize("name", REFINE_NAMES)
def test_refine_vs_reference(name):
    z = load("structure.npz")
    X0, p1, p2, P1, P2 = rcase(z, name)
    X, info = refined(name)
    cost_ref = SR.point_costs(z[f"{name}_Xref"], p1, p2, P1, P2)
    excess = ((info["cost"] - cost_ref) / cost_ref).max()
    print(f"MEASURED refine {name}: largest relative cost excess over the reference {excess:.3e}")
    assert (info["cost"] <= cost_ref * (1 + SR.COST_DELTA)).all()
    # the cost the kernel reports is the cost of the points it returns
    assert np.allclose(SR.point_costs(X, p1, p2, P1, P2), info["cost"], rtol=1e-9, atol=0)
    if name in SR.CLEAN:
        e = rel_err(X, z[f"{name}_Xref"]).max()
        moved = rel_err(X0, X).max()
        print(f"MEASURED refine {name}: X vs reference {e:.3e} (the refinement moves the points by {moved:.3e})")
        assert e <= SR.X_REF_TOL


def test_batch_is_bit_equal_to_single_calls_and_device_tensors():
    torch = pytest.importorskip("torch")
    z = load("structure.npz")
    cases = [rcase(z, n) for n in SR.BATCH]
    info = {}
    out = pose.refine_points_batch(cases, info=info)
    for k, name in enumerate(SR.BATCH):
        X, inf = refined(name)
        assert isinstance(out[k], np.ndarray) and np.array_equal(out[k], X), name
        for key in ("cost", "iters", "status"):
            assert np.array_equal(info[key][k], inf[key]), (name, key)
    # device tensors in, device tensors out, the same bits
    dcases = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in c) for c in cases]
    dout = pose.refine_points_batch(dcases)
    for k, name in enumerate(SR.BATCH):
        assert dout[k].is_cuda and np.array_equal(dout[k].cpu().numpy(), refined(name)[0]), name
    Xd = pose.non_linear_triangulation(*dcases[1])
    assert Xd.is_cuda and Xd.dtype == torch.float64 and np.array_equal(Xd.cpu().numpy(), refined(SR.BATCH[1])[0])
    # CPU tensors behave as numpy
    Xc = pose.non_linear_triangulation(*(torch.from_numpy(np.ascontiguousarray(a)) for a in cases[0]))
    assert isinstance(Xc, np.ndarray) and np.array_equal(Xc, refined(SR.BATCH[0])[0])
    # an empty case inside a batch, and alone
    e = (np.empty((0, 3)), np.empty((0, 2)), np.empty((0, 2)), cases[0][3], cases[0][4])
    out = pose.refine_points_batch([e, cases[0]])
    assert out[0].shape == (0, 3) and np.array_equal(out[1], refined(SR.BATCH[0])[0])
    assert pose.non_linear_triangulation(*e).shape == (0, 3)


def test_refine_degenerate_inputs_are_defined():
    """Non-finite start: returned unchanged with status 2; max_iter = 1: status 3 or an
    earlier stop; seg values outside [0, S) are clamped."""
    torch = pytest.importorskip("torch")
    z = load("structure.npz")
    X0, p1, p2, P1, P2 = rcase(z, "c12")
    X0 = X0.copy()
    X0[3] = np.nan
    X0[5, 2] = np.inf
    info = {}
    X = pose.non_linear_triangulation(X0, p1, p2, P1, P2, info=info)
    assert info["status"][3] == 2 and info["status"][5] == 2 and info["iters"][3] == 0
    assert np.isnan(X[3]).all() and np.array_equal(X[5], X0[5])
    ok = np.ones(12, bool)
    ok[[3, 5]] = False
    assert np.array_equal(X[ok], refined("c12")[0][ok])
    # the raw call: max_iter = 1 and out-of-range seg values
    ctx = _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))
    dev = torch.device("cuda", 0)
    n = 12
    X0, p1, p2, P1, P2 = rcase(z, "c12")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)
    dX0, da, db = t(X0), t(p1), t(p2)
    Pm = t(np.concatenate([P1.ravel(), P2.ravel()] * 2))
    seg = torch.tensor([-5, 7, 0, 1] * 3, dtype=torch.int32, device=dev)
    X = torch.empty((n, 3), dtype=torch.float64, device=dev)
    cost = torch.empty(n, dtype=torch.float64, device=dev)
    it = torch.empty(n, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _native.check(ctx.lib.sfm_refine_points_dev(ctx.handle, dX0.data_ptr(), da.data_ptr(), db.data_ptr(), n,
                                                Pm.data_ptr(), 2, seg.data_ptr(), 50, X.data_ptr(), cost.data_ptr(),
                                                it.data_ptr(), st or None), ctx.handle)
    assert np.array_equal(X.cpu().numpy(), refined("c12")[0])  # both pairs are the same cameras
    _native.check(ctx.lib.sfm_refine_points_dev(ctx.handle, dX0.data_ptr(), da.data_ptr(), db.data_ptr(), n,
                                                Pm.data_ptr(), 1, None, 1, X.data_ptr(), cost.data_ptr(),
                                                it.data_ptr(), st or None), ctx.handle)
    itn = it.cpu().numpy()
    assert ((itn & 0xFFFFFF) <= 1).all() and ((itn >> 24) == 3).all()


@pytest.mark.parametrize("name", REFINE_NAMES)
def test_reprojection_error(name, capsys):
    z = load("structure.npz")
    X0, p1, p2, P1, P2 = rcase(z, name)
    Xref = z[f"{name}_Xref"]
    mean, err = pose.reprojection_error(Xref, p1, p2, P1, P2)
    mean2, err2 = pose.reprojection_error(Xref, p1, p2, P1, P2)
    rmean, rerr = SR.reprojection_error(Xref, p1, p2, P1, P2)
    pn = np.column_stack([np.linalg.norm(p1, axis=1), np.linalg.norm(p2, axis=1)])
    ee = (np.abs(err - rerr) / (rerr + pn)).max()
    em = abs(mean - rmean) / rmean
    with capsys.disabled():
        print(f"MEASURED reprojection {name}: errors {ee:.3e} (over e + |p|; over e alone "
              f"{(np.abs(err - rerr) / rerr).max():.3e}) mean {em:.3e}, against the restatement")
    assert err.shape == (len(p1), 2) and err.dtype == np.float64
    assert ee <= ERR_TOL and em <= MEAN_TOL
    assert np.float64(mean).tobytes() == np.float64(mean2).tobytes() and np.array_equal(err, err2)
    capsys.readouterr()
    pose.print_reprojection_error(Xref, p1, p2, P1, P2)
    assert capsys.readouterr().out.strip() == str(z[f"{name}_line"])


def test_reprojection_error_of_no_points_is_nan():
    z = load("structure.npz")
    _, _, _, P1, P2 = rcase(z, "c12")
    mean, err = pose.reprojection_error(np.empty((0, 3)), np.empty((0, 2)), np.empty((0, 2)), P1, P2)
    assert np.isnan(mean) and err.shape == (0, 2)


@pytest.mark.parametrize("name", LINK_NAMES)
def test_link_equals_fixture(name):
    z = load("structure.npz")
    g = lambda k: z[f"link_{name}_{k}"]
    info = {}
    rp, rn = pose.link_points(g("tgt"), g("p3d"), g("qry"), g("nxt"), dist_threshold=float(g("thr")), info=info)
    assert np.array_equal(info["target_index"], g("ti")) and np.array_equal(info["query_index"], g("qi"))
    assert rp.shape == g("prev").shape and rp.dtype == g("prev").dtype and np.array_equal(rp, g("prev"))
    assert rn.shape == g("next").shape and rn.dtype == g("next").dtype and np.array_equal(rn, g("next"))
    if len(g("ti")) == 0:
        assert rp.shape == (0,) and rp.dtype == np.float64 and rn.shape == (0,) and rn.dtype == np.float64


def test_link_default_threshold_and_no_queries():
    z = load("structure.npz")
    g = lambda k: z[f"link_edge5_{k}"]
    info = {}
    pose.link_points(g("tgt"), g("p3d"), g("qry"), g("nxt"), info=info)  # dist_threshold = 5.0
    assert np.array_equal(info["query_index"], g("qi")) and 0 not in info["query_index"]
    rp, rn = pose.link_points(g("tgt"), g("p3d"), np.empty((0, 2), np.int32), np.empty((0, 2), np.int32))
    assert rp.shape == (0,) and rn.shape == (0,)


def test_c_abi_argument_errors_leave_a_message():
    torch = pytest.importorskip("torch")
    ctx = _native.context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE))
    L, h = ctx.lib, ctx.handle
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    E = _abi.SFM_EINVAL
    msg = lambda: (L.sfm_last_error(h) or b"").decode()

    def refine(X0=p, x1=p, x2=p, N=2, P=p, S=1, seg=None, mi=50, X=p, cost=p, it=p):
        return L.sfm_refine_points_dev(h, X0, x1, x2, N, P, S, seg, mi, X, cost, it, None)

    for kw in ({"X0": None}, {"x1": None}, {"x2": None}, {"N": -1}, {"P": None}, {"S": 0}, {"S": -2}, {"mi": 0},
               {"mi": -1}, {"X": None}, {"cost": None}, {"it": None}):
        assert refine(**kw) == E and "sfm_refine_points_dev" in msg(), kw
    assert L.sfm_refine_points_dev(None, p, p, p, 2, p, 1, None, 50, p, p, p, None) == E
    assert refine(N=0, X0=None, x1=None, x2=None, X=None, cost=None, it=None) == _abi.SFM_OK

    def reproj(X=p, x1=p, x2=p, N=2, P1=p, P2=p, err=p, mean=p):
        return L.sfm_reprojection_error_dev(h, X, x1, x2, N, P1, P2, err, mean, None)

    for kw in ({"X": None}, {"x1": None}, {"x2": None}, {"N": -1}, {"P1": None}, {"P2": None}, {"err": None},
               {"mean": None}):
        assert reproj(**kw) == E and "sfm_reprojection_error_dev" in msg(), kw

    def link(tgt=p, m=2, qry=p, nq=2, ot=p, oq=p, on=p):
        return L.sfm_link_points_dev(h, tgt, m, qry, nq, ctypes.c_double(5.0), ot, oq, on, None)

    for kw in ({"tgt": None}, {"m": -1}, {"qry": None}, {"nq": -1}, {"ot": None}, {"oq": None}, {"on": None}):
        assert link(**kw) == E and "sfm_link_points_dev" in msg(), kw
    assert link(m=0) == E and "np.argmin of an empty sequence" in msg()
    torch.cuda.synchronize()


def test_initial_structure_is_the_chain_of_its_parts():
    z = load("pose.npz")
    g = lambda k: z[f"g0_{k}"]
    p1, p2, K1, K2, iters = g("p1"), g("p2"), g("K1"), g("K2"), int(g("iters"))
    R2, t2, in1, in2, p3d, mean = pose.initial_structure(p1, p2, K1, K2, iters, threshold=float(g("thr")))
    r = pose.ransac_camera_motion(p1, p2, K1, K2, np.eye(3), np.zeros(3), threshold=float(g("thr")),
                                  max_iterations=iters)
    assert np.array_equal(R2, r[0]) and np.array_equal(t2, r[1])
    assert np.array_equal(in1, r[2]) and np.array_equal(in2, r[3]) and in1.dtype == r[2].dtype
    P1 = pose.calculate_projection_matrix(np.eye(3), np.zeros(3), K1)
    P2 = pose.calculate_projection_matrix(R2, t2, K2)
    X = pose.non_linear_triangulation(pose.triangulate(in1, in2, P1, P2), in1, in2, P1, P2)
    assert p3d.dtype == np.float64 and np.array_equal(p3d, X)
    m, _ = pose.reprojection_error(X, in1, in2, P1, P2)
    print(f"MEASURED initial_structure g0: {len(in1)} inliers, mean reprojection error {mean:.6f}")
    assert np.float64(mean).tobytes() == np.float64(m).tobytes()
    # no pose: ransac_camera_motion's own conventions
    assert pose.initial_structure(p1[:7], p2[:7], K1, K2, iters) == (None, None, None, None)
    q = pose.initial_structure(p1, p2, K1, K2, 0)
    assert q[0] is None and q[1] is None and q[2].shape == (0,) and q[3].shape == (0,)
