"""The match consumer on the HIP path: CameraPose.find_inliers (SFM.py:126-160), the
8-point RANSAC SFMRunner applies to every stage-1 pair but (1, 2) (Runner.py:349-351)
— SURVEY.md §8f row 2.  Same signature, sampling stream, selection rule and return
values as the reference (ransac.hip has the numerics):

* samples: numpy's legacy RandomState after np.random.seed(5), one
  np.random.choice(n, 8, replace=False) per iteration (replayed natively, bit-exact);
* per sample the normalised 8-point fundamental matrix with rank 2 enforced, and the
  count of correspondences whose epipolar distance is below `threshold` (float64);
* the first sample with the most inliers wins; its inliers are returned in input order
  as p1[mask], p2[mask]; no inliers at all gives the reference's empty float64 arrays;
  fewer than 8 correspondences gives its (None, None, None, None).

Below: the consumer of the pair the filter leaves alone, CameraPose.ransac_camera_motion
(SFM.py:38-124), and the linear triangulation it is built from (pose.hip).
At the end: what SFMRunner.perform does with the triangulated points — refinement
(CameraPose.non_linear_triangulation), the reprojection error and the 2D -> 3D association
of the next pair (refine.hip).
"""
from __future__ import annotations

import numpy as np

from . import _abi
from ._native import check, context_for, load_library


def calculate_num_ransac_iterations(prob_success: float, sample_size: int, ind_prob_correct: float) -> int:
    """CameraPose.calculate_num_ransac_iterations (SFM.py:184-187)."""
    num_samples = np.log(1 - prob_success) / np.log(1 - (ind_prob_correct ** sample_size))
    return int(num_samples)


def sample_indices(n: int, iters: int, seed: int = 5) -> np.ndarray:
    """[iters, 8] int32: np.random.seed(seed); [np.random.choice(n, 8, replace=False) ...]
    (numpy's legacy MT19937 + Fisher-Yates, replayed natively; host only)."""
    import ctypes
    out = np.empty((max(iters, 0), 8), np.int32)
    rc = load_library().sfm_ransac_sample_indices(int(n), int(iters), ctypes.c_uint32(seed),
                                                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    check(rc)
    return out


def find_inliers(p1, p2, threshold=1.0, max_iterations=1000, device: int = 0):
    """Drop-in for CameraPose.find_inliers (SFM.py:126-160).

    Deliberate divergence: the reference also accepts non-integer coordinates; the device
    path stores points as int32 (what Runner._convert_matches_to_coords, Runner.py:423-434,
    produces from the int64 keypoints), so non-integer input raises ValueError instead of
    being silently truncated."""
    p1 = np.asarray(p1)
    p2 = np.asarray(p2)
    if len(p1) < 8:
        return None, None, None, None  # the reference's 4-tuple (SFM.py:130-131)
    if not (np.array_equal(p1, np.round(p1)) and np.array_equal(p2, np.round(p2))):
        raise ValueError("find_inliers takes integer pixel coordinates (Runner.py:423-434)")
    ctx = context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), device)
    res = ctx.ransac_find_inliers(p1, p2, float(threshold), int(max_iterations))
    in1, in2, _ = res
    if len(in1) == 0:
        return np.array([]), np.array([])
    return in1.astype(p1.dtype, copy=False), in2.astype(p2.dtype, copy=False)


def find_inliers_batch(pairs, threshold=1.0, max_iterations=1000, device: int = 0):
    """find_inliers over many correspondence sets in one device pass (one launch set for
    all pairs; sample streams shared by sets of equal size).  Integer coordinates only, as
    `find_inliers` (a documented divergence).  pairs: [(p1, p2), ...];
    returns the per-pair results of find_inliers."""
    import ctypes

    import torch
    res = [None] * len(pairs)
    todo = []
    for k, (a, b) in enumerate(pairs):
        a, b = np.asarray(a), np.asarray(b)
        if len(a) < 8:
            res[k] = (None, None, None, None)
            continue
        if not (np.array_equal(a, np.round(a)) and np.array_equal(b, np.round(b))):
            raise ValueError(f"pair {k}: find_inliers takes integer pixel coordinates (Runner.py:423-434)")
        if a.shape != b.shape or a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"pair {k}: p1 and p2 must both be [n, 2]")
        todo.append((k, a, b))
    if not todo:
        return res
    nmax = max(len(a) for _, a, _ in todo)
    P = len(todo)
    pts = np.zeros((P, nmax, 4), np.int32)
    npts = np.array([len(a) for _, a, _ in todo], np.int32)
    for p, (_, a, b) in enumerate(todo):
        pts[p, :len(a), :2] = a
        pts[p, :len(a), 2:] = b
    ctx = context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), device)
    dev = torch.device("cuda", device)
    d_pts = torch.from_numpy(pts).to(dev)
    d_n = torch.from_numpy(npts).to(dev)
    o_pts = torch.zeros_like(d_pts)
    o_n = torch.zeros(P, dtype=torch.int32, device=dev)
    o_it = torch.zeros(P, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    check(ctx.lib.sfm_ransac_find_inliers_dev(ctx.handle, d_pts.data_ptr(), d_n.data_ptr(),
                                              npts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), P, nmax,
                                              int(max_iterations), ctypes.c_double(threshold), o_pts.data_ptr(),
                                              o_n.data_ptr(), o_it.data_ptr(), stream or None), ctx.handle)
    on = o_n.cpu().numpy()
    op = o_pts.cpu().numpy()
    for p, (k, a, b) in enumerate(todo):
        n = int(on[p])
        if n <= 0:
            res[k] = (np.array([]), np.array([]))
        else:
            res[k] = (op[p, :n, :2].astype(a.dtype), op[p, :n, 2:].astype(b.dtype))
    return res


# ---------------- the initial pair: pose RANSAC and triangulation (pose.hip) ----------------

def calculate_projection_matrix(R, t, K):
    """CameraPose.calculate_projection_matrix (SFM.py:307-309)."""
    return np.asarray(K) @ np.hstack([np.asarray(R), np.asarray(t).reshape(-1, 1)])


def _check_pose_points(p1, p2, what):
    if p1.shape != p2.shape or p1.ndim != 2 or p1.shape[1] != 2:
        raise ValueError(f"{what}: pts1 and pts2 must both be [n, 2]")
    if not (np.array_equal(p1, np.round(p1)) and np.array_equal(p2, np.round(p2))):
        raise ValueError(f"{what}: ransac_camera_motion takes integer pixel coordinates (Runner.py:423-434)")


def ransac_camera_motion(pts1, pts2, K1, K2, R_base, T_base, threshold=1.0, max_iterations=1000, device: int = 0):
    """Drop-in for CameraPose(pts1, pts2, K1, K2).ransac_camera_motion(R_base, T_base, ...)
    (SFM.py:38-103), the initial pair's own RANSAC (Runner.py:202-208): the samples and
    inlier test of `find_inliers`, and among the samples one of whose four (R, t)
    candidates puts every triangulated correspondence in front of both cameras
    (_check_valid_pose, SFM.py:105-124) the first with the most inliers.  Returns
    (R, t, inliers1, inliers2); (None, None, None, None) below 8 correspondences;
    (None, None, array([]), array([])) when no sample won.

    Integer pixel coordinates only, the divergence documented at `find_inliers`."""
    p1 = np.asarray(pts1)
    p2 = np.asarray(pts2)
    if len(p1) < 8:
        return None, None, None, None  # SFM.py:42-43
    _check_pose_points(p1, p2, "ransac_camera_motion")
    ctx = context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), device)
    R, t, in1, in2, _ = ctx.ransac_camera_motion(p1, p2, K1, K2, R_base, T_base, float(threshold),
                                                 int(max_iterations))
    if len(in1) == 0:
        return None, None, np.array([]), np.array([])
    return R, t, in1.astype(p1.dtype, copy=False), in2.astype(p2.dtype, copy=False)


def ransac_camera_motion_batch(cases, threshold=1.0, max_iterations=1000, device: int = 0, info=None):
    """ransac_camera_motion over many correspondence sets in one device pass.
    cases: [(pts1, pts2, K1, K2, R_base, T_base), ...]; returns the per-case results of
    `ransac_camera_motion`.  info (optional dict) receives "out_iter" (the winning sample per
    case, -1 for none) and "candidates" (per case the [iters] valid-candidate index of every
    sample, -1 for none or for a sample without inliers; None below 8 points)."""
    import ctypes

    import torch
    res = [None] * len(cases)
    todo = []
    for k, (a, b, K1, K2, Rb, Tb) in enumerate(cases):
        a, b = np.asarray(a), np.asarray(b)
        if len(a) < 8:
            res[k] = (None, None, None, None)
            continue
        _check_pose_points(a, b, f"case {k}")
        Km = np.concatenate([np.asarray(K1, np.float64).reshape(-1), np.asarray(K2, np.float64).reshape(-1)])
        bm = np.concatenate([np.asarray(Rb, np.float64).reshape(-1), np.asarray(Tb, np.float64).reshape(-1)])
        if Km.size != 18 or bm.size != 12:
            raise ValueError(f"case {k}: K1, K2, R_base are 3 x 3 and T_base has 3 entries")
        todo.append((k, a, b, Km, bm))
    iters = int(max_iterations)
    if info is not None:
        info["out_iter"] = [-1] * len(cases)
        info["candidates"] = [None] * len(cases)
    if not todo:
        return res
    nmax = max(len(t[1]) for t in todo)
    P = len(todo)
    pts = np.zeros((P, nmax, 4), np.int32)
    npts = np.array([len(t[1]) for t in todo], np.int32)
    Kh = np.ascontiguousarray(np.stack([t[3] for t in todo]))
    bh = np.ascontiguousarray(np.stack([t[4] for t in todo]))
    for p, (_, a, b, _, _) in enumerate(todo):
        pts[p, :len(a), :2] = a
        pts[p, :len(a), 2:] = b
    ctx = context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), device)
    dev = torch.device("cuda", device)
    d_pts = torch.from_numpy(pts).to(dev)
    d_n = torch.from_numpy(npts).to(dev)
    o_pts = torch.zeros_like(d_pts)
    o_n = torch.zeros(P, dtype=torch.int32, device=dev)
    o_it = torch.zeros(P, dtype=torch.int32, device=dev)
    oR = np.zeros((P, 3, 3), np.float64)
    ot = np.zeros((P, 3), np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    stream = torch.cuda.current_stream(dev).cuda_stream
    check(ctx.lib.sfm_ransac_camera_motion_dev(
        ctx.handle, d_pts.data_ptr(), d_n.data_ptr(), npts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), P, nmax,
        iters, ctypes.c_double(threshold), Kh.ctypes.data_as(dp), bh.ctypes.data_as(dp), o_pts.data_ptr(),
        o_n.data_ptr(), o_it.data_ptr(), oR.ctypes.data_as(dp), ot.ctypes.data_as(dp), stream or None), ctx.handle)
    on = o_n.cpu().numpy()
    oit = o_it.cpu().numpy()
    op = o_pts.cpu().numpy()
    cand = ctx.pose_candidates(P, iters) if info is not None else None
    for p, (k, a, b, _, _) in enumerate(todo):
        n = int(on[p])
        if n <= 0:
            res[k] = (None, None, np.array([]), np.array([]))
        else:
            res[k] = (oR[p].copy(), ot[p].copy(), op[p, :n, :2].astype(a.dtype), op[p, :n, 2:].astype(b.dtype))
        if info is not None:
            info["out_iter"][k] = int(oit[p])
            info["candidates"][k] = cand[p].copy()
    return res


def _triangulate(x1, x2, P1, P2, normalize, device):
    import torch
    host = not (isinstance(x1, torch.Tensor) and x1.is_cuda)
    dev = torch.device("cuda", device) if host else x1.device

    def put(a, shape):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float64))
        if t.numel() != int(np.prod(shape)):
            raise ValueError("triangulate: x1, x2 are [n, 2] (or [n, 3] homogeneous) and P1, P2 are 3 x 4")
        return t.to(device=dev, dtype=torch.float64).contiguous().reshape(shape)

    n = int(x1.shape[0])
    a, b = put(x1[:, :2], (n, 2)), put(x2[:, :2], (n, 2))
    A, B = put(P1, (12,)), put(P2, (12,))
    X = torch.empty((n, 3), dtype=torch.float64, device=dev)
    ctx = context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), dev.index or 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    check(ctx.lib.sfm_triangulate_dev(ctx.handle, a.data_ptr(), b.data_ptr(), n, A.data_ptr(), B.data_ptr(),
                                      1 if normalize else 0, X.data_ptr(), stream or None), ctx.handle)
    return X.cpu().numpy() if host else X


def triangulate(p1, p2, P1, P2, device: int = 0):
    """[CameraPose.triangulate_point(a, b, P1, P2) for a, b in zip(p1, p2)] (SFM.py:239-253, the
    loops of Runner.py:208 and :278) in one launch: p1, p2 [n, 2] (a third homogeneous column
    is ignored), P1, P2 3 x 4 -> [n, 3] float64.  numpy or CPU tensors in, numpy out; device
    tensors in, a device tensor out."""
    return _triangulate(p1, p2, P1, P2, False, device)


def triangulate_points(x1, x2, P1, P2, device: int = 0):
    """CameraPose.triangulate_points (SFM.py:292-305): both point sets Hartley-normalised on
    the device, the transforms applied to P1, P2, then `triangulate`."""
    return _triangulate(x1, x2, P1, P2, True, device)


# ---------------- the structure stage: refine, score, link (refine.hip) ----------------

REFINE_MAX_ITER = 50           # iterations of the per-point Levenberg-Marquardt
REFINE_STATUS_SHIFT = 24       # sfm_refine_points_dev packs status << 24 | accepted steps
REFINE_STATUS = {0: "converged", 1: "lambda", 2: "non-finite", 3: "max_iter"}
LINK_COORD_MAX = 1 << 30       # the int64 squared distance cannot overflow below this


def _is_dev(a):
    import torch
    return isinstance(a, torch.Tensor) and a.is_cuda


def _shape_of(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape


def _check_structure_shapes(p3d, p1, p2, P1, P2, what):
    """[n, 3], [n, 2], [n, 2] and two 3 x 4 matrices (host-side, before any device call) -> n."""
    s3, s1, s2 = _shape_of(p3d), _shape_of(p1), _shape_of(p2)
    if len(s3) != 2 or s3[1] != 3:
        raise ValueError(f"{what}: p3d must be [n, 3]")
    n = s3[0]
    if s1 != (n, 2) or s2 != (n, 2):
        raise ValueError(f"{what}: p1 and p2 must both be [n, 2] with p3d's n")
    if int(np.prod(_shape_of(P1))) != 12 or int(np.prod(_shape_of(P2))) != 12:
        raise ValueError(f"{what}: P1 and P2 are 3 x 4")
    return n


def _f64_dev(a, shape, dev):
    import torch
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float64))
    return t.to(device=dev, dtype=torch.float64).contiguous().reshape(shape)


def _structure_ctx(dev):
    import torch
    ctx = context_for(_abi.params_from_dict({}, _abi.SFM_MODE_NAIVE), dev.index or 0)
    return ctx, torch.cuda.current_stream(dev).cuda_stream


def _refine_dev(X0, a, b, Pm, S, seg, dev, max_iter=REFINE_MAX_ITER):
    """One launch over device tensors: X0 [n, 3], a, b [n, 2], Pm [S, 2, 12], seg [n] int32 or None
    -> X, cost, packed iters (device tensors)."""
    import torch
    n = int(X0.shape[0])
    X = torch.empty((n, 3), dtype=torch.float64, device=dev)
    cost = torch.empty(n, dtype=torch.float64, device=dev)
    it = torch.empty(n, dtype=torch.int32, device=dev)
    ctx, stream = _structure_ctx(dev)
    check(ctx.lib.sfm_refine_points_dev(ctx.handle, X0.data_ptr(), a.data_ptr(), b.data_ptr(), n, Pm.data_ptr(),
                                        int(S), seg.data_ptr() if seg is not None else None, int(max_iter),
                                        X.data_ptr(), cost.data_ptr(), it.data_ptr(), stream or None), ctx.handle)
    return X, cost, it


def _refine_info(cost, it):
    it = it.cpu().numpy()
    return {"cost": cost.cpu().numpy(), "iters": it & ((1 << REFINE_STATUS_SHIFT) - 1),
            "status": it >> REFINE_STATUS_SHIFT}


def non_linear_triangulation(p3d, p1, p2, P1, P2, device: int = 0, info=None):
    """Drop-in for CameraPose.non_linear_triangulation (SFM.py:255-289; Runner.py:209, :279):
    the points that minimise the reprojection error of SFM.py:262-273, [n, 3] float64.

    The reference solves one Levenberg-Marquardt problem over all 3n coordinates; its cost is
    a sum of per-point terms, so the device refines every point on its own (one thread each,
    analytic Jacobian; the rule is in include/sfmfeat.h).  numpy or CPU tensors in, numpy out;
    device tensors in, a device tensor out.  Float pixel coordinates are accepted, as in the
    reference.  info (optional dict) receives "cost" (final sum of squared residuals per
    point), "iters" (accepted steps) and "status" (REFINE_STATUS) as numpy arrays.

    Deliberate divergence: n == 0 returns an empty (0, 3) array; the reference's
    least_squares raises on an empty problem."""
    import torch
    n = _check_structure_shapes(p3d, p1, p2, P1, P2, "non_linear_triangulation")
    host = not _is_dev(p3d)
    if n == 0:
        if info is not None:
            info.update(cost=np.empty(0), iters=np.empty(0, np.int32), status=np.empty(0, np.int32))
        return np.empty((0, 3)) if host else torch.empty((0, 3), dtype=torch.float64, device=p3d.device)
    dev = torch.device("cuda", device) if host else p3d.device
    Pm = torch.cat([_f64_dev(P1, (12,), dev), _f64_dev(P2, (12,), dev)])
    X, cost, it = _refine_dev(_f64_dev(p3d, (n, 3), dev), _f64_dev(p1, (n, 2), dev), _f64_dev(p2, (n, 2), dev), Pm,
                              1, None, dev)
    if info is not None:
        info.update(_refine_info(cost, it))
    return X.cpu().numpy() if host else X


def refine_points_batch(cases, device: int = 0, info=None):
    """non_linear_triangulation over many point sets in one launch: cases is
    [(p3d, p1, p2, P1, P2), ...], each point carries its case's camera pair.  Returns the
    per-case arrays, bit-equal to the single calls (a device tensor for a case whose p3d is
    one).  info (optional dict) receives per-case lists "cost", "iters", "status"."""
    import torch
    ns = [_check_structure_shapes(*c, f"case {k}") for k, c in enumerate(cases)]
    if info is not None:
        info.update(cost=[np.empty(0)] * len(cases), iters=[np.empty(0, np.int32)] * len(cases),
                    status=[np.empty(0, np.int32)] * len(cases))
    devs = [c[0].device for c in cases if _is_dev(c[0])]
    dev = devs[0] if devs else torch.device("cuda", device)
    out = [None] * len(cases)
    live = [k for k, n in enumerate(ns) if n > 0]
    for k, n in enumerate(ns):
        if n == 0:
            out[k] = (torch.empty((0, 3), dtype=torch.float64, device=dev) if _is_dev(cases[k][0])
                      else np.empty((0, 3)))
    if not live:
        return out
    X0 = torch.cat([_f64_dev(cases[k][0], (ns[k], 3), dev) for k in live])
    a = torch.cat([_f64_dev(cases[k][1], (ns[k], 2), dev) for k in live])
    b = torch.cat([_f64_dev(cases[k][2], (ns[k], 2), dev) for k in live])
    Pm = torch.cat([_f64_dev(cases[k][j], (12,), dev) for k in live for j in (3, 4)])
    seg = torch.from_numpy(np.repeat(np.arange(len(live), dtype=np.int32), [ns[k] for k in live])).to(dev)
    X, cost, it = _refine_dev(X0, a, b, Pm, len(live), seg, dev)
    inf = _refine_info(cost, it) if info is not None else None
    o = 0
    for k in live:
        Xk = X[o:o + ns[k]]
        out[k] = Xk.clone() if _is_dev(cases[k][0]) else Xk.cpu().numpy()
        if inf is not None:
            for key in ("cost", "iters", "status"):
                info[key][k] = inf[key][o:o + ns[k]].copy()
        o += ns[k]
    return out


def _reprojection_dev(X, a, b, A, B, dev):
    """Device tensors in -> (mean [1], err [n, 2]) device tensors."""
    import torch
    n = int(X.shape[0])
    err = torch.empty((n, 2), dtype=torch.float64, device=dev)
    mean = torch.empty(1, dtype=torch.float64, device=dev)
    ctx, stream = _structure_ctx(dev)
    check(ctx.lib.sfm_reprojection_error_dev(ctx.handle, X.data_ptr() if n else None, a.data_ptr() if n else None,
                                             b.data_ptr() if n else None, n, A.data_ptr(), B.data_ptr(),
                                             err.data_ptr() if n else None, mean.data_ptr(), stream or None),
          ctx.handle)
    return mean, err


def reprojection_error(p3d, p1, p2, P1, P2, device: int = 0):
    """The figures of Util.print_reprojection_error (Util.py:65-82): (mean, errors) with
    errors [n, 2] the norms of Util.py:76-77 per point and mean (a float) the mean over points
    of their average (Util.py:81; NaN for n == 0, as numpy's).  The mean is summed in a fixed
    order on the device: the same bits every run.  errors is numpy for host input, a device
    tensor for device input."""
    import torch
    n = _check_structure_shapes(p3d, p1, p2, P1, P2, "reprojection_error")
    host = not _is_dev(p3d)
    dev = torch.device("cuda", device) if host else p3d.device
    mean, err = _reprojection_dev(_f64_dev(p3d, (n, 3), dev), _f64_dev(p1, (n, 2), dev), _f64_dev(p2, (n, 2), dev),
                                  _f64_dev(P1, (12,), dev), _f64_dev(P2, (12,), dev), dev)
    return float(mean.cpu()[0]), (err.cpu().numpy() if host else err)


def print_reprojection_error(p3d, p1, p2, P1, P2, device: int = 0):
    """Drop-in for Util.print_reprojection_error (Runner.py:211, :282): prints the reference's line."""
    mean, _ = reprojection_error(p3d, p1, p2, P1, P2, device)
    print(f"Mean Reprojection Error: {mean:.4f}")


def _link_coords(a, what):
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"link_points: {what} must be [n, 2]")
    if a.size and not np.array_equal(a, np.round(a)):
        raise ValueError(f"link_points: {what} must hold integer pixel coordinates (Runner.py:423-434)")
    if a.size and (a.min() < -LINK_COORD_MAX or a.max() > LINK_COORD_MAX):
        raise ValueError(f"link_points: {what} must fit int32 and lie within +-2^30")
    return a


def link_points(points_2d_prev, p3d, prev_frame_2d, next_frame_2d, dist_threshold=5.0, info=None, device: int = 0):
    """The 2D -> 3D association loop of Runner.py:241-250: for each row of prev_frame_2d the
    first nearest of points_2d_prev; where it is closer than dist_threshold, that point's 3D
    coordinate and the row's next_frame_2d pixel are kept.  Returns (result_prev, result_next)
    as Runner.py:249-250 builds them: p3d[idx] (float64 [k, 3]) and next_frame_2d[q] (its
    dtype), both np.array([]) when nothing links.  info (optional dict) receives
    "target_index" and "query_index".

    Integer pixel coordinates only (ValueError otherwise, the divergence documented at
    `find_inliers`), within +-2^30.  An empty points_2d_prev raises ValueError, as the
    reference's np.argmin does."""
    import torch
    tgt = _link_coords(points_2d_prev, "points_2d_prev")
    qry = _link_coords(prev_frame_2d, "prev_frame_2d")
    p3d = np.asarray(p3d)
    nxt = np.asarray(next_frame_2d)
    if len(tgt) == 0:
        raise ValueError("attempt to get argmin of an empty sequence (Runner.py:243)")
    if p3d.shape != (len(tgt), 3):
        raise ValueError("link_points: p3d must be [m, 3] with one row per row of points_2d_prev")
    if len(nxt) != len(qry):
        raise ValueError("link_points: prev_frame_2d and next_frame_2d must have the same number of rows")
    m, nq = len(tgt), len(qry)
    ti = np.empty(0, np.int32)
    qi = np.empty(0, np.int32)
    if nq:
        dev = torch.device("cuda", device)
        d_t = torch.from_numpy(np.ascontiguousarray(tgt, np.int32)).to(dev)
        d_q = torch.from_numpy(np.ascontiguousarray(qry, np.int32)).to(dev)
        o_t = torch.empty(nq, dtype=torch.int32, device=dev)
        o_q = torch.empty(nq, dtype=torch.int32, device=dev)
        o_n = torch.zeros(1, dtype=torch.int32, device=dev)
        ctx, stream = _structure_ctx(dev)
        check(ctx.lib.sfm_link_points_dev(ctx.handle, d_t.data_ptr(), m, d_q.data_ptr(), nq,
                                          float(dist_threshold), o_t.data_ptr(), o_q.data_ptr(), o_n.data_ptr(),
                                          stream or None), ctx.handle)
        k = int(o_n.cpu()[0])
        ti, qi = o_t[:k].cpu().numpy(), o_q[:k].cpu().numpy()
    if info is not None:
        info.update(target_index=ti, query_index=qi)
    if len(ti) == 0:
        return np.array([]), np.array([])
    return p3d[ti].astype(np.float64, copy=False), nxt[qi]


def initial_structure(p1, p2, K1, K2, max_iterations, threshold=1.0, device: int = 0):
    """Runner.py:198-211 in one call: ransac_camera_motion with R1 = I, t1 = 0, the two
    projection matrices, `triangulate` of the inliers, `non_linear_triangulation` and
    `reprojection_error`; the points stay on the device between the last three.  Returns
    (R2, t2, inliers1, inliers2, p3d, mean_error), or ransac_camera_motion's own result
    ((None, None, None, None) / (None, None, array([]), array([]))) when no pose is found."""
    import torch
    R1, t1 = np.eye(3), np.zeros(3)
    r = ransac_camera_motion(p1, p2, K1, K2, R1, t1, threshold=threshold, max_iterations=max_iterations,
                             device=device)
    if r[0] is None:
        return r
    R2, t2, in1, in2 = r
    P1 = calculate_projection_matrix(R1, t1, K1)
    P2 = calculate_projection_matrix(R2, t2, K2)
    dev = torch.device("cuda", device)
    n = len(in1)
    a, b = _f64_dev(in1, (n, 2), dev), _f64_dev(in2, (n, 2), dev)
    A, B = _f64_dev(P1, (12,), dev), _f64_dev(P2, (12,), dev)
    X = non_linear_triangulation(_triangulate(a, b, A, B, False, device), a, b, A, B)
    mean, _ = _reprojection_dev(X, a, b, A, B, dev)
    return R2, t2, in1, in2, X.cpu().numpy(), float(mean.cpu()[0])
