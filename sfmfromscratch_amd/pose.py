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
