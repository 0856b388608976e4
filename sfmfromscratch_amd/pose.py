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
of the next pair (refine.hip) — and then with every batch of them: the
global point registry (SFMRunner.add_points), prepare_for_ba and total_reprojection_error
(PointRegistry; registry.hip), with a host stand-in for cv2.Rodrigues.
Between the two: the pose of every frame after the second from its 2D-3D links (PnPRansac, PnP,
next_structure; pnp.hip) — the library's own rule, OpenCV parity not pinned.
Last: bundle adjustment over the registry (BundleAdjustment; ba.hip) — the
library's own Schur-complement Levenberg-Marquardt; scipy's stopping iterate is not pinned, the
minimum is.
"""
from __future__ import annotations

import numpy as np

from . import _abi
from ._native import check, context_for, load_library


def calculate_num_ransac_iterations(prob_success: float, sample_size: int, ind_prob_correct: float) -> int:
    """CameraPose.calculate_num_ransac_iterations (SFM.py:184-187)."""
    num_samples = np.log(1 - prob_success) / np.log(1 - (ind_prob_correct ** sample_size))
    return int(num_samples)


def ransac_stop_ratios(confidence: float, rounds: int, sample_size: int = 8) -> np.ndarray:
    """The early-stop table of sequence.verify_matches (sfm_verify_matches_dev's stop_ratio): entry
    r - 1, r = 1..rounds, is (1 - (1 - confidence)^(1 / (256 r)))^(1 / 8), the inlier ratio w at which
    256 r eight-point samples contain an all-inlier one with probability `confidence`
    (1 - (1 - w^8)^(256 r) = confidence).  sample_size=4 gives the table of
    sequence.two_view_geometry's homography RANSAC (w^4 in place of w^8).  Pure numpy, float64;
    strictly decreasing in r."""
    if not 0.0 < confidence < 1.0:
        raise ValueError("confidence must lie in (0, 1)")
    if int(sample_size) < 1:
        raise ValueError("sample_size must be >= 1")
    r = np.arange(1, int(rounds) + 1, dtype=np.float64)
    return (-np.expm1(np.log1p(-np.float64(confidence)) / (256.0 * r))) ** (1.0 / int(sample_size))


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


# ---------------- the pose of the next frame: PnP (pnp.hip) ----------------

PNP_THRESHOLD = 8.0            # cv2.solvePnPRansac's reprojectionError of PoseEstimator.py:59
PNP_MIN_POINTS = 6             # the minimal solver is a 6-point DLT


def sample_indices_k(n: int, iters: int, size: int, seed: int = 5) -> np.ndarray:
    """[iters, size] int32: np.random.seed(seed); [np.random.choice(n, size, replace=False) ...]
    (`sample_indices` with the sample size as an argument; host only)."""
    import ctypes
    out = np.empty((max(iters, 0), size), np.int32)
    check(load_library().sfm_ransac_sample_indices_k(int(n), int(iters), ctypes.c_uint32(seed), int(size),
                                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return out


def _pnp_inputs(points3d, points2d, K, dist_coeffs, device, what):
    """-> (X [n, 3], x [n, 2], K [9]) float64 device tensors, host flag, device; None for X when
    there are no points at all."""
    import torch
    if dist_coeffs is not None:
        raise NotImplementedError(f"{what}: lens distortion is not supported (dist_coeffs must be None)")
    if K is None:
        raise ValueError(f"{what}: K is required")
    host = not _is_dev(points3d)
    dev = torch.device("cuda", device) if host else points3d.device
    s3, s2 = _shape_of(points3d), _shape_of(points2d)
    n = s3[0] if len(s3) else 0
    if int(np.prod(s3)) == 0 or int(np.prod(s2)) == 0:  # np.array([]) of a frame without links
        return None, None, None, host, dev
    if len(s3) != 2 or s3[1] != 3 or s2 != (n, 2):
        raise ValueError(f"{what}: points3d must be [n, 3] and points2d [n, 2]")
    Kh = (K.cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K)).astype(np.float64).reshape(-1)
    if Kh.size != 9:
        raise ValueError(f"{what}: K is 3 x 3")
    if not np.isfinite(Kh).all():
        raise ValueError(f"{what}: points3d, points2d and K must be finite")
    if Kh[3] != 0 or Kh[6] != 0 or Kh[7] != 0 or Kh[0] == 0 or Kh[4] == 0 or Kh[8] == 0:
        raise ValueError(f"{what}: K must be upper triangular with a non-zero diagonal")
    fin = (lambda a: bool(torch.isfinite(a).all())) if not host else (lambda a: bool(np.isfinite(np.asarray(a)).all()))
    if not (fin(points3d) and fin(points2d)):
        raise ValueError(f"{what}: points3d, points2d and K must be finite")
    if n < PNP_MIN_POINTS:  # no pose, and no device call
        return None, None, None, host, dev
    return _f64_dev(points3d, (n, 3), dev), _f64_dev(points2d, (n, 2), dev), _f64_dev(Kh, (9,), dev), host, dev


def _pnp_ransac_dev(X, x, K, iters, threshold, max_refine_iter, dev, ctx=None):
    """One sfm_pnp_ransac_dev call over device tensors (on the thread's context unless one is
    given) -> dict of device tensors."""
    import torch
    n = int(X.shape[0])
    i32 = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device=dev)
    f64 = lambda k: torch.empty(k, dtype=torch.float64, device=dev)
    o = dict(R=f64(9), t=f64(3), inliers=i32(n), n=i32(1), iteration=i32(1), status=i32(4), cost=f64(2),
             counts=i32(iters))
    own, stream = _structure_ctx(dev)
    ctx = ctx or own
    check(ctx.lib.sfm_pnp_ransac_dev(ctx.handle, X.data_ptr(), x.data_ptr(), K.data_ptr(), n, int(iters),
                                     float(threshold), int(max_refine_iter), o["R"].data_ptr(), o["t"].data_ptr(),
                                     o["inliers"].data_ptr(), o["n"].data_ptr(), o["iteration"].data_ptr(),
                                     o["status"].data_ptr(), o["cost"].data_ptr(), o["counts"].data_ptr(),
                                     stream or None), ctx.handle)
    return o


def _pnp_info(info, status, cost, iteration=None, counts=None):
    if info is None:
        return
    st = status.cpu().numpy()
    c = cost.cpu().numpy()
    info.update(status=int(st[1]), iters=int(st[2]), lm_iters=int(st[3]), cost0=float(c[0]), cost=float(c[1]))
    if iteration is not None:
        info.update(iteration=int(iteration.cpu()[0]), counts=counts.cpu().numpy())


class PnPRansac:
    """Stands in for PoseEstimator.PnPRansac (PoseEstimator.py:32-69; Runner.py:257-262) with the
    library's own rule (include/sfmfeat.h sfm_pnp_ransac_dev): 6-point DLT
    hypotheses from the np.random.seed(5) sample stream, inliers under 8 pixels of reprojection
    error, the first sample with the most inliers, Levenberg-Marquardt refinement on its inliers.
    Parity with cv2.solvePnPRansac is not pinned.

    Attributes as the reference's: R [3, 3] float64 or None, t [3, 1] (cv2's tvec shape),
    inliers int32 [k, 1] ascending (cv2's shape) or None.  Fewer than 6 points, or no sample with
    an inlier, leaves all three None (Runner.py:263 then raises).  numpy or CPU tensors in, numpy
    out; device tensors in, device tensors out.  Float32 input (Runner.py:258-259) converts
    exactly.  dist_coeffs other than None raises NotImplementedError; non-finite input raises
    ValueError.  info (optional dict) receives "iteration" (the winning sample, -1 for none),
    "counts" [ransac_max_it], "cost0" / "cost" (sum of squared residuals over the inliers before
    and after the refinement), "status" (REFINE_STATUS; -1 without a pose), "iters" (accepted
    steps) and "lm_iters" (iterations run)."""

    def __init__(self, points3d, points2d, K=None, ransac_max_it=100, dist_coeffs=None, threshold=PNP_THRESHOLD,
                 device: int = 0, info=None, **kwargs):
        self.R = self.t = self.inliers = None
        iters = int(ransac_max_it)
        if iters < 0:
            raise ValueError("PnPRansac: ransac_max_it is negative")
        X, x, Kd, host, dev = _pnp_inputs(points3d, points2d, K, dist_coeffs, device, "PnPRansac")
        if info is not None:
            info.update(iteration=-1, counts=np.zeros(iters, np.int32), cost0=float("nan"), cost=float("nan"),
                        status=-1, iters=0, lm_iters=0)
        if X is None or int(X.shape[0]) < PNP_MIN_POINTS:
            return
        o = _pnp_ransac_dev(X, x, Kd, iters, threshold, REFINE_MAX_ITER, dev)
        _pnp_info(info, o["status"], o["cost"], o["iteration"], o["counts"][:iters])
        k = int(o["n"].cpu()[0])
        if k <= 0:
            return
        R, t, inl = o["R"].reshape(3, 3), o["t"].reshape(3, 1), o["inliers"][:k].reshape(k, 1)
        self.R, self.t, self.inliers = (R.cpu().numpy(), t.cpu().numpy(), inl.cpu().numpy()) if host else (R, t, inl)


class PnP:
    """Stands in for PoseEstimator.PnP (PoseEstimator.py:71-105): the DLT over all n >= 6 points,
    then the refinement of `PnPRansac` over all of them (sfm_pnp_dev).  R, t as PnPRansac's;
    inliers stays None.  info receives "cost0", "cost", "status", "iters", "lm_iters"."""

    def __init__(self, points3d, points2d, K=None, dist_coeffs=None, device: int = 0, info=None, **kwargs):
        import torch
        self.R = self.t = self.inliers = None
        X, x, Kd, host, dev = _pnp_inputs(points3d, points2d, K, dist_coeffs, device, "PnP")
        if info is not None:
            info.update(cost0=float("nan"), cost=float("nan"), status=-1, iters=0, lm_iters=0)
        if X is None or int(X.shape[0]) < PNP_MIN_POINTS:
            return
        R = torch.empty(9, dtype=torch.float64, device=dev)
        t = torch.empty(3, dtype=torch.float64, device=dev)
        status = torch.empty(4, dtype=torch.int32, device=dev)
        cost = torch.empty(2, dtype=torch.float64, device=dev)
        ctx, stream = _structure_ctx(dev)
        check(ctx.lib.sfm_pnp_dev(ctx.handle, X.data_ptr(), x.data_ptr(), Kd.data_ptr(), int(X.shape[0]),
                                  REFINE_MAX_ITER, R.data_ptr(), t.data_ptr(), status.data_ptr(), cost.data_ptr(),
                                  stream or None), ctx.handle)
        _pnp_info(info, status, cost)
        if int(status.cpu()[0]) != 1:
            return
        R, t = R.reshape(3, 3), t.reshape(3, 1)
        self.R, self.t = (R.cpu().numpy(), t.cpu().numpy()) if host else (R, t)


def next_structure(points_2d_prev, p3d, P_prev, p1, p2, K, ransac_max_it=100, dist_threshold=5.0, device: int = 0,
                   info=None):
    """Runner.py:241-282 in one call, as `initial_structure` is for :198-211: `link_points` of the
    previous pair's second-image pixels (points_2d_prev, with their 3-D points p3d) to this
    pair's matches (p1 in the previous frame, p2 in the next), `PnPRansac` on the links cast to
    float32 (Runner.py:258-259), P_next = `calculate_projection_matrix`, then `triangulate`,
    `non_linear_triangulation` and `reprojection_error` of (p1, p2) under (P_prev, P_next); the
    new points stay on the device between the last three.  Returns (R3, t3, inliers,
    result_prev, result_next, P_next, p3d_new, mean_error); R3 is None (and P_next, p3d_new,
    mean_error with it) when no pose is found, where Runner.py:263 raises.  info (optional dict)
    receives PnPRansac's entries."""
    import torch
    result_prev, result_next = link_points(points_2d_prev, p3d, p1, p2, dist_threshold=dist_threshold, device=device)
    pe = PnPRansac(np.asarray(result_prev, dtype=np.float32), np.asarray(result_next, dtype=np.float32), K=K,
                   ransac_max_it=ransac_max_it, device=device, info=info)
    if pe.R is None:
        return None, None, None, result_prev, result_next, None, None, None
    P_next = calculate_projection_matrix(pe.R, pe.t, K)
    dev = torch.device("cuda", device)
    n = len(p1)
    a, b = _f64_dev(np.asarray(p1), (n, 2), dev), _f64_dev(np.asarray(p2), (n, 2), dev)
    A, B = _f64_dev(P_prev, (12,), dev), _f64_dev(P_next, (12,), dev)
    X = non_linear_triangulation(_triangulate(a, b, A, B, False, device), a, b, A, B)
    mean, _ = _reprojection_dev(X, a, b, A, B, dev)
    return pe.R, pe.t, pe.inliers, result_prev, result_next, P_next, X.cpu().numpy(), float(mean.cpu()[0])


# ---------------- the point registry and the BA-input score (registry.hip) ----------------

REGISTRY_THRESHOLD = 1e-6      # is_new_point / find_existing_point's default (Runner.py:373, :380)
REGISTRY_CHUNK = 256           # registry entries one workgroup stages at a time (kernels.h kRegChunk)
REGISTRY_MIN_CAPACITY = 1024


def rodrigues(a):
    """Host numpy drop-in for the cv2.Rodrigues calls of Runner.py:213, :285 and
    PoseEstimator.py:68: a 3-vector gives (R [3, 3], None) with theta = |r|, R = I for
    theta < DBL_EPSILON, else cos(theta) I + (1 - cos(theta)) k k^T + sin(theta) [k]x, k = r / theta;
    a 3 x 3 rotation gives (r [3, 1], None): the axis from the antisymmetric part, the angle
    from atan2(sin, cos); beyond theta = pi / 2, where the antisymmetric part fades, the axis
    comes from the symmetric part (R_ii = c + (1 - c) k_i^2, the signs from the off-diagonal
    sums and what is left of the antisymmetric part), so theta = pi is an ordinary case.  Parity with OpenCV is not pinned
    (DESIGN.md §13C); no Jacobian is returned."""
    a = np.asarray(a, np.float64)
    if a.size == 3:
        r = a.reshape(3)
        th = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
        if th < np.finfo(np.float64).eps:
            return np.eye(3), None
        k = r / th
        c, s = np.cos(th), np.sin(th)
        Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
        return c * np.eye(3) + (1.0 - c) * np.outer(k, k) + s * Kx, None
    if a.shape != (3, 3):
        raise ValueError("rodrigues: a 3-vector or a 3 x 3 matrix")
    v = np.array([a[2, 1] - a[1, 2], a[0, 2] - a[2, 0], a[1, 0] - a[0, 1]]) / 2.0
    s = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    c = (a[0, 0] + a[1, 1] + a[2, 2] - 1.0) / 2.0
    th = np.arctan2(s, c)
    if c >= 0:  # theta <= pi / 2: the antisymmetric part is sin(theta) k
        return (v.copy() if s == 0 else v * (th / s)).reshape(3, 1), None
    k2 = np.maximum((np.diag(a) - c) / (1.0 - c), 0.0)
    i = int(np.argmax(k2))
    k = np.zeros(3)
    k[i] = -np.sqrt(k2[i]) if v[i] < 0 else np.sqrt(k2[i])
    for j in range(3):
        if j != i:
            k[j] = (a[i, j] + a[j, i]) / 2.0 / ((1.0 - c) * k[i])
    k = k / np.sqrt((k[0] * k[0] + k[1] * k[1]) + k[2] * k[2])
    return (k * th).reshape(3, 1), None


def _i32_dev(a, n, dev, what):
    import torch
    if isinstance(a, torch.Tensor):
        t = a
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a).reshape(-1), np.int64))
    if t.numel() < n:
        raise ValueError(f"{what} has fewer than {n} entries")
    return t.reshape(-1)[:n].to(device=dev, dtype=torch.int32).contiguous()


class PointRegistry:
    """The global 3-D point list of SFMRunner (global_points_3D, global_points_2D,
    frame_indices, point_indices; Runner.py:361-401) kept on the device.

    add_points is SFMRunner.add_points: the points are processed in order; one that lies at
    least `threshold` (float64 norm) from every registered point — those appended earlier in the
    same call included — is appended, any other takes the first index of the smallest distance.
    Indices and registry equal the reference's bit for bit.  Nothing synchronises until a
    property is read: the table grows geometrically from the number of points passed in so
    far, an upper bound of the registered count that needs no device read."""

    def __init__(self, device: int = 0, threshold: float = REGISTRY_THRESHOLD):
        import torch
        if not threshold > 0:
            raise ValueError("PointRegistry: threshold must be positive")
        self.threshold = float(threshold)
        self._dev = torch.device("cuda", device)
        self._table = torch.empty((REGISTRY_MIN_CAPACITY, 3), dtype=torch.float64, device=self._dev)
        self._count = torch.zeros(1, dtype=torch.int32, device=self._dev)
        self._bound = 0           # points passed in so far >= the registered count
        self._idx, self._new, self._frames, self._p2 = [], [], [], []

    def _reserve(self, n):
        import torch
        need = self._bound + n
        cap = int(self._table.shape[0])
        if need <= cap:
            return
        grown = torch.empty((max(2 * cap, need), 3), dtype=torch.float64, device=self._dev)
        grown[:self._bound].copy_(self._table[:self._bound])
        self._table = grown

    def add_points(self, points_3d, points_2d, frame_idx, info=None):
        """SFMRunner.add_points(points_3d, points_2d, frame_idx).  numpy arrays or device
        tensors; points_3d [n, 3], points_2d [n, 2] (an empty array of any shape is no points,
        as the reference's np.array([]) of a frame without links).  ValueError on a shape
        mismatch and on non-finite numpy points_3d (for device tensors finite coordinates
        are the caller's contract).  info (optional dict) receives the call's "point_indices"
        and "is_new" as device tensors."""
        import torch
        s3, s2 = _shape_of(points_3d), _shape_of(points_2d)
        if int(np.prod(s3)) == 0 and int(np.prod(s2)) == 0:
            if info is not None:
                e = torch.empty(0, dtype=torch.int32, device=self._dev)
                info.update(point_indices=e, is_new=e.clone())
            return
        if len(s3) != 2 or s3[1] != 3:
            raise ValueError("add_points: points_3d must be [n, 3]")
        n = s3[0]
        if s2 != (n, 2):
            raise ValueError("add_points: points_2d must be [n, 2] with points_3d's n")
        if not _is_dev(points_3d) and not np.isfinite(np.asarray(points_3d, np.float64)).all():
            raise ValueError("add_points: points_3d must be finite")
        with torch.cuda.device(self._dev):
            pts = _f64_dev(points_3d, (n, 3), self._dev)
            self._reserve(n)
            idx = torch.empty(n, dtype=torch.int32, device=self._dev)
            new = torch.empty(n, dtype=torch.int32, device=self._dev)
            ctx, stream = _structure_ctx(self._dev)
            check(ctx.lib.sfm_registry_add_dev(ctx.handle, self._table.data_ptr(), self._count.data_ptr(),
                                               int(self._table.shape[0]), pts.data_ptr(), n, self.threshold,
                                               idx.data_ptr(), new.data_ptr(), stream or None), ctx.handle)
            self._bound += n
            self._idx.append(idx)
            self._new.append(new)
            self._frames.append(torch.full((n,), int(frame_idx), dtype=torch.int64, device=self._dev))
            self._p2.append(points_2d if _is_dev(points_2d)
                            else torch.from_numpy(np.ascontiguousarray(points_2d)).to(self._dev))
        if info is not None:
            info.update(point_indices=idx, is_new=new)

    def __len__(self):
        return int(self._count.cpu()[0])

    @staticmethod
    def _cat(chunks, empty):
        return np.concatenate([c.cpu().numpy() for c in chunks]) if chunks else empty

    @property
    def point_indices(self):
        return self._cat(self._idx, np.empty(0, np.int32)).astype(np.int64)

    @property
    def frame_indices(self):
        return self._cat(self._frames, np.empty(0, np.int64))

    @property
    def points_3d(self):
        return self._table[:len(self)].cpu().numpy()

    @property
    def points_2d(self):
        return self._cat(self._p2, np.empty((0, 2)))

    @property
    def points_3d_device(self):
        """The registered points as a device tensor view (valid until the next add_points)."""
        return self._table[:len(self)]

    def prepare_for_ba(self, global_poses, global_K):
        """SFMRunner.prepare_for_ba (Runner.py:387-401) with the poses [(Rodrigues vector, t), ...]
        and intrinsics perform collects: (num_cameras, num_points, camera_indices, point_indices,
        points_2D, camera_params, points_3D, K_list)."""
        frames = self.frame_indices
        camera_params = np.array([np.hstack((np.asarray(p[0]).flatten(), np.asarray(p[1]).flatten()))
                                  for p in global_poses])
        p3 = self.points_3d
        return (len(set(frames.tolist())), len(p3), frames, self.point_indices, self.points_2d, camera_params,
                p3, np.array(global_K))

    def total_reprojection_error(self, num_points, camera_indices, point_indices, points_2D, camera_params,
                                 points_3D, K_list, info=None):
        """SFMRunner.total_reprojection_error (Runner.py:311-334): the mean over the first
        num_points observations (the reference's bound, although prepare_for_ba's num_points
        counts 3-D points) of |pi(K (R X + t)) - observation|, on the device, summed in a fixed
        order.  Arrays are numpy or device tensors; numpy indices outside their tables raise
        IndexError (device indices are the caller's contract).  info (optional dict) receives
        "errors" [num_points] (numpy)."""
        import torch
        M = int(num_points)
        if M < 0:
            raise ValueError("total_reprojection_error: num_points is negative")
        dev = self._dev
        with torch.cuda.device(dev):
            cams = _f64_dev(camera_params, (-1, 6), dev)
            K = _f64_dev(K_list, (-1, 3, 3), dev)
            X = _f64_dev(points_3D, (-1, 3), dev)
            obs = _f64_dev(points_2D, (-1, 2), dev)
            n_cam, n_pts = int(cams.shape[0]), int(X.shape[0])
            if int(K.shape[0]) < n_cam:
                raise ValueError("total_reprojection_error: K_list has fewer entries than camera_params")
            if int(obs.shape[0]) < M:
                raise ValueError("total_reprojection_error: fewer than num_points observations")
            for a, hi, what in ((camera_indices, n_cam, "camera"), (point_indices, n_pts, "point")):
                if not _is_dev(a) and M:
                    h = np.asarray(a).reshape(-1)[:M]
                    if h.size and (h.min() < 0 or h.max() >= hi):
                        raise IndexError(f"total_reprojection_error: a {what} index is outside its table")
            ci = _i32_dev(camera_indices, M, dev, "camera_indices")
            pi = _i32_dev(point_indices, M, dev, "point_indices")
            err = torch.empty(max(M, 1), dtype=torch.float64, device=dev)
            mean = torch.empty(1, dtype=torch.float64, device=dev)
            ctx, stream = _structure_ctx(dev)
            check(ctx.lib.sfm_total_reprojection_error_dev(
                ctx.handle, ci.data_ptr(), pi.data_ptr(), obs.data_ptr(), M, cams.data_ptr(), n_cam, K.data_ptr(),
                X.data_ptr(), n_pts, err.data_ptr(), mean.data_ptr(), stream or None), ctx.handle)
            if info is not None:
                info["errors"] = err[:M].cpu().numpy()
            return float(mean.cpu()[0])

    def set_points_3d(self, X):
        """Runner.py:304 (global_points_3D = the adjusted points): writes X [len(self), 3] (numpy
        or a device tensor) over the registered coordinates; the count, the indices and the
        observations stay.  `save` then writes the adjusted model.  ValueError on any other
        shape.  (Later add_points calls compare against the adjusted coordinates.)"""
        n = len(self)
        if _shape_of(X) != (n, 3):
            raise ValueError(f"set_points_3d: X must be [{n}, 3], the registered count")
        if n:
            self._table[:n].copy_(_f64_dev(X, (n, 3), self._dev))

    def save(self, path):
        """SFMRunner.save_data's file (Runner.py:357-359): p3d, frame_idx, pt_idx."""
        np.savez(path, p3d=self.points_3d, frame_idx=self.frame_indices, pt_idx=self.point_indices)

    @classmethod
    def load(cls, path, device: int = 0, threshold: float = REGISTRY_THRESHOLD):
        """A registry holding a saved model's points and indices (the file has no 2-D observations:
        points_2d starts empty)."""
        import torch
        z = np.load(path)
        p3 = np.ascontiguousarray(z["p3d"], np.float64).reshape(-1, 3)
        r = cls(device, threshold)
        m = len(p3)
        r._reserve(m)
        r._bound = m
        if m:
            r._table[:m].copy_(torch.from_numpy(p3))
        r._count.fill_(m)
        pt = np.ascontiguousarray(z["pt_idx"], np.int64).reshape(-1)
        fr = np.ascontiguousarray(z["frame_idx"], np.int64).reshape(-1)
        if len(pt):
            r._idx.append(torch.from_numpy(pt.astype(np.int32)).to(r._dev))
            r._frames.append(torch.from_numpy(fr).to(r._dev))
        return r


# ---------------- bundle adjustment (ba.hip) ----------------

BA_MAX_CAMERAS = _abi.SFM_BA_MAX_CAMERAS
BA_MAX_POINTS = _abi.SFM_BA_MAX_POINTS
BA_MAX_OBSERVATIONS = _abi.SFM_BA_MAX_OBSERVATIONS


class BundleAdjustment:
    """Stands in for SFM.BundleAdjustment (SFM.py:405-464; Runner.py:294-303) with the library's
    own rule (include/sfmfeat.h sfm_bundle_adjust_dev): Levenberg-Marquardt with
    the Schur complement over every camera's (R, t) and every point, Marquardt damping, strict
    acceptance, stopping at the first accepted step whose relative decrease is <= ftol (the
    reference's 1e-2 by default).  Which iterate scipy's TRF path stops at is not pinned; the
    minimum is.  All observations count, as compute_residuals zips them all.

    The constructor takes the reference's arguments (the tuple of PointRegistry.prepare_for_ba);
    arrays are numpy or device tensors.  fixed_cameras (optional): a boolean mask [num_cameras] or
    a list of camera indices that do not move.  numpy indices outside their tables raise
    IndexError (device indices are the caller's contract).  info (optional dict) receives
    "cost0", "cost" (the sum of squared residuals before and after), "status" (REFINE_STATUS),
    "iters" (accepted steps), "lm_iters" (iterations run) and "rejected_factorisations"."""

    def __init__(self, num_cameras, num_points, camera_indices, point_indices, points_2d, camera_params, points_3d,
                 K_list, device: int = 0, fixed_cameras=None, ftol=1e-2, max_iter=50, info=None):
        self.num_cameras, self.num_points = int(num_cameras), int(num_points)
        self.camera_indices, self.point_indices, self.points_2d = camera_indices, point_indices, points_2d
        self.camera_params, self.points_3d, self.K_list = camera_params, points_3d, K_list
        self.device, self.fixed_cameras, self.ftol, self.max_iter, self.info = device, fixed_cameras, ftol, max_iter, info

    def sparse_bundle_adjustment(self, as_device: bool = False):
        """-> (optimized_camera_params [num_cameras, 6], optimized_points_3d [num_points, 3]):
        float64 numpy, or device tensors with as_device=True (nothing synchronises then unless
        info is given)."""
        import torch
        n_cam, n_pts = self.num_cameras, self.num_points
        ftol, max_iter = float(self.ftol), int(self.max_iter)
        if not 1 <= n_cam <= BA_MAX_CAMERAS:
            raise ValueError(f"BundleAdjustment: num_cameras must be in [1, {BA_MAX_CAMERAS}]")
        if not 0 <= n_pts <= BA_MAX_POINTS:
            raise ValueError("BundleAdjustment: num_points must be in [0, 2^24]")
        if not ftol >= 0:
            raise ValueError("BundleAdjustment: ftol must be >= 0")
        if not 1 <= max_iter < (1 << REFINE_STATUS_SHIFT):
            raise ValueError("BundleAdjustment: max_iter must be in [1, 2^24)")
        probe = next((a for a in (self.points_3d, self.camera_params, self.points_2d) if _is_dev(a)), None)
        dev = probe.device if probe is not None else torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            cams = _f64_dev(self.camera_params, (-1, 6), dev)
            K = _f64_dev(self.K_list, (-1, 3, 3), dev)
            X = _f64_dev(self.points_3d, (-1, 3), dev)
            obs = _f64_dev(self.points_2d, (-1, 2), dev)
            M = int(obs.shape[0])
            if M > BA_MAX_OBSERVATIONS:
                raise ValueError("BundleAdjustment: at most 2^26 observations")
            if int(cams.shape[0]) != n_cam or int(X.shape[0]) != n_pts:
                raise ValueError("BundleAdjustment: camera_params must be [num_cameras, 6] and points_3d [num_points, 3]")
            if int(K.shape[0]) < n_cam:
                raise ValueError("BundleAdjustment: K_list has fewer entries than camera_params")
            for a, hi, what in ((self.camera_indices, n_cam, "camera"), (self.point_indices, n_pts, "point")):
                if int(np.prod(_shape_of(a))) != M:
                    raise ValueError(f"BundleAdjustment: {what}_indices must have one entry per observation")
                if not _is_dev(a) and M:
                    h = np.asarray(a).reshape(-1)
                    if h.min() < 0 or h.max() >= hi:
                        raise IndexError(f"BundleAdjustment: a {what} index is outside its table")
            ci = _i32_dev(self.camera_indices, M, dev, "camera_indices")
            pi = _i32_dev(self.point_indices, M, dev, "point_indices")
            fixed = None
            if self.fixed_cameras is not None:
                f = self.fixed_cameras.cpu().numpy() if isinstance(self.fixed_cameras, torch.Tensor) \
                    else np.asarray(self.fixed_cameras)
                mask = np.zeros(n_cam, np.uint8)
                if f.dtype == np.bool_:
                    if f.shape != (n_cam,):
                        raise ValueError("BundleAdjustment: a fixed_cameras mask must be [num_cameras]")
                    mask[f] = 1
                elif f.size:
                    f = f.astype(np.int64).reshape(-1)
                    if f.min() < 0 or f.max() >= n_cam:
                        raise IndexError("BundleAdjustment: a fixed camera index is outside its table")
                    mask[f] = 1
                fixed = torch.from_numpy(mask).to(dev)
            out_c = torch.empty((n_cam, 6), dtype=torch.float64, device=dev)
            out_X = torch.empty((n_pts, 3), dtype=torch.float64, device=dev)
            cost = torch.empty(2, dtype=torch.float64, device=dev)
            status = torch.empty(4, dtype=torch.int32, device=dev)
            ctx, stream = _structure_ctx(dev)
            check(ctx.lib.sfm_bundle_adjust_dev(
                ctx.handle, ci.data_ptr(), pi.data_ptr(), obs.data_ptr(), M, cams.data_ptr(), n_cam, K.data_ptr(),
                X.data_ptr() if n_pts else None, n_pts, fixed.data_ptr() if fixed is not None else None, ftol,
                max_iter, out_c.data_ptr(), out_X.data_ptr() if n_pts else None, cost.data_ptr(), status.data_ptr(),
                stream or None), ctx.handle)
            if self.info is not None:
                st, c = status.cpu().numpy(), cost.cpu().numpy()
                self.info.update(cost0=float(c[0]), cost=float(c[1]), status=int(st[0]), iters=int(st[1]),
                                 lm_iters=int(st[2]), rejected_factorisations=int(st[3]))
            if as_device:
                return out_c, out_X
            return out_c.cpu().numpy(), out_X.cpu().numpy()


# ---------------- N-view triangulation of feature tracks (tracks.hip) ----------------

def triangulate_tracks(tracks, P, cam_valid=None, device: int = 0):
    """Every track's 3-D point from all its views (include/sfmfeat.h sfm_triangulate_tracks_dev):
    triangulate_point (SFM.py:241-246) with the two rows of every valid view stacked in ascending
    slot order.  tracks: sequence.Tracks; P [n_cam, 3, 4] (or [n_cam, 12]), the projection matrix
    of each slot; cam_valid (optional) [n_cam], zero / False where a slot has no pose.
    -> (X [n_tracks, 3] float64, NaN with fewer than 2 valid views; views [n_tracks] int32).
    numpy in, numpy out; a device tensor P gives device tensors.  The work runs on the tracks'
    device (`device` is kept for symmetry with the other calls and must agree with it)."""
    import torch
    dev = tracks.xy.device
    if (dev.index or 0) != int(device) and not _is_dev(P):
        raise ValueError(f"triangulate_tracks: the tracks live on {dev}, not on cuda:{device}")
    host = not _is_dev(P)
    if int(np.prod(_shape_of(P))) % 12 or int(np.prod(_shape_of(P))) == 0:
        raise ValueError("triangulate_tracks: P must be [n_cam, 3, 4]")
    with torch.cuda.device(dev):
        Pm = _f64_dev(P, (-1, 12), dev)
        n_cam = int(Pm.shape[0])
        cv = None
        if cam_valid is not None:
            cv = cam_valid if isinstance(cam_valid, torch.Tensor) else torch.from_numpy(np.asarray(cam_valid))
            if cv.numel() != n_cam:
                raise ValueError("triangulate_tracks: cam_valid must have one entry per camera")
            cv = (cv.reshape(-1) != 0).to(device=dev, dtype=torch.uint8).contiguous()
        T, M = tracks.n_tracks, tracks.n_obs
        X = torch.empty((T, 3), dtype=torch.float64, device=dev)
        views = torch.empty(T, dtype=torch.int32, device=dev)
        ctx, stream = _structure_ctx(dev)
        ctx.triangulate_tracks_dev(tracks.offsets_dev, tracks.obs_slot_dev, tracks.obs_row_dev, T, M, tracks.xy, Pm, cv,
                                   X, views, stream)
    if host:
        return X.cpu().numpy(), views.cpu().numpy()
    return X, views
