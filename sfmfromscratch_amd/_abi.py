"""ctypes mirror of include/sfmfeat.h (constants and the POD parameter struct).

Pure Python: importing this module loads no native code.  `params_from_dict` maps the
reference's `extractor_params` dict (read with `.get(key, default)` at
FeatureExtractor.py:11, NaiveSIFT.py:35-39, ScaleRotInvSIFT.py:12-13) onto `SfmParams`.
"""
from __future__ import annotations

import ctypes

import numpy as np

SFM_OK = 0
SFM_EINVAL = 1
SFM_ESTATE = 2
SFM_EDEVICE = 3
SFM_ERANGE = 4
SFM_EINDEX = 5

SFM_MODE_SCALEROT = 0
SFM_MODE_NAIVE = 1

SFM_DESC_DIM = 128
SFM_MAX_GAUSS = 15
SFM_MAX_KSIZE = 31
SFM_MAX_FW = 64
SFM_MAX_LEVELS = 12
SFM_BA_MAX_CAMERAS = 256          # sfm_bundle_adjust_dev: n_cam
SFM_BA_MAX_POINTS = 1 << 24       # n_pts
SFM_BA_MAX_OBSERVATIONS = 1 << 26  # M
SFM_TRACKS_MAX_NODES = 1 << 30     # sfm_build_tracks_dev: nimg * cap

_vp = ctypes.c_void_p
# include/sfmfeat.h's feature-track calls as (restype, argtypes); device pointers are void*
# (_native binds them; tests/test_tracks_cpu.py holds them against the header's prototypes)
TRACK_SIGNATURES = {
    # ctx, count, nimg, cap, pairs, P, matches, nmatch, keep, min_len, track_offsets, obs_slot,
    # obs_row, node_track, out_n, stream
    "sfm_build_tracks_dev": (ctypes.c_int32, [_vp, _vp, ctypes.c_int32, ctypes.c_int64, _vp, ctypes.c_int32, _vp,
                                              _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    # ctx, track_offsets, obs_slot, obs_row, n_tracks, n_obs, xy, nimg, cap, P, cam_valid, n_cam,
    # X, out_views, stream
    "sfm_triangulate_tracks_dev": (ctypes.c_int32, [_vp, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp,
                                                    ctypes.c_int32, ctypes.c_int64, _vp, _vp, ctypes.c_int32, _vp,
                                                    _vp, _vp]),
}


# include/sfmfeat.h's read-backs of the matcher's intermediate state (host pointers as void*;
# tests/test_abi_cpu.py holds them against the header's prototypes)
MATCH_DEBUG_SIGNATURES = {
    # ctx, slot, rows, hi, lo, norm2, rnorm, pmax
    "sfm_debug_match_operands": (ctypes.c_int32, [_vp, ctypes.c_int32, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp]),
    # ctx, pair, rows, cand_n, cand_thr, cand
    "sfm_debug_match_windows": (ctypes.c_int32, [_vp, ctypes.c_int32, ctypes.c_int64, _vp, _vp, _vp]),
    # ctx, pair, rows, skip
    "sfm_debug_match_skips": (ctypes.c_int32, [_vp, ctypes.c_int32, ctypes.c_int64, _vp]),
}
# include/sfmfeat.h's probe of the geometry kernels' shared float64 helpers (host pointers as void*;
# tests/test_abi_cpu.py holds it against the header's prototype): device, op, in, n, out
GEOM_DEBUG_SIGNATURES = {
    "sfm_debug_geom": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int64, _vp]),
}
(SFM_GEOM_RODRIGUES, SFM_GEOM_RODRIGUES_INV, SFM_GEOM_EIG3, SFM_GEOM_NULL4, SFM_GEOM_COMPOSE, SFM_GEOM_ROTATE,
 SFM_GEOM_WAVE_SUM, SFM_GEOM_BLOCK_SUM) = range(8)
GEOM_ROW_IN = (3, 9, 6, 16, 18, 12, 64, 512)    # doubles per row, by op
GEOM_ROW_OUT = (9, 3, 12, 4, 9, 3, 64, 512)
SFM_GEOM_MAX_ROWS = 1 << 20
# include/sfmfeat.h's probe of the keypoint selection on host R planes (tests/test_abi_cpu.py holds
# it against the header's prototype): device, nlevels, B, R[], H[], W[], half_window[], k, ksize,
# vmin, force_exact, x, y, conf, count, state, ncand, consts
SELECT_DEBUG_SIGNATURES = {
    "sfm_debug_select": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, _vp,
                                          ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# include/sfmfeat.h's read-back of the PnP samples (host pointers as void*; tests/test_abi_cpu.py
# holds it against the header's prototype): ctx, hyp, counts, start_Rt, entries
PNP_DEBUG_SIGNATURES = {
    "sfm_debug_pnp_fits": (ctypes.c_int32, [_vp, _vp, _vp, _vp, ctypes.c_int64]),
}
SFM_SELECT_MAX_LEVELS = 4
SFM_SELECT_MAX_K = 8192
# the u32 words of a plane's selection state, in the library's order (median: float32 bits)
SELECT_STATE_FIELDS = ("bucket0", "bucket1", "rank0", "rank1", "odd", "median", "tnms", "tcert", "fallback",
                       "tsub0", "tsub1")
SFM_SELECT_STATE_WORDS = len(SELECT_STATE_FIELDS)
# the sizes the selection's branches turn on, in the order sfm_debug_select reports them
SELECT_CONST_FIELDS = ("sel_cap", "topk_direct", "tie_lds_cap", "reg_keys", "med_cap")
SFM_SELECT_CONSTS = len(SELECT_CONST_FIELDS)
MATCH_CAND_CAP = 256   # list words per query row (two half-lists of 128)
MATCH_PREP_ROWS = 16   # rows per block of the operands' (norm2, rnorm) maxima


class SfmParams(ctypes.Structure):
    _fields_ = [
        ("mode", ctypes.c_int32),
        ("num_interest_points", ctypes.c_int32),
        ("ksize", ctypes.c_int32),
        ("gaussian_size", ctypes.c_int32),
        ("feature_width", ctypes.c_int32),
        ("pyramid_level", ctypes.c_int32),
        ("sigma", ctypes.c_double),
        ("alpha", ctypes.c_double),
        ("pyramid_scale_factor", ctypes.c_double),
        ("gauss_kernel_set", ctypes.c_int32),
        ("reserved0", ctypes.c_int32),
        ("gauss_kernel", ctypes.c_float * (SFM_MAX_GAUSS * SFM_MAX_GAUSS)),
    ]


def generate_gaussian_kernel(ksize: int, sigma: float) -> np.ndarray:
    """Same expression as NaiveSIFT._generate_gaussian_kernel (NaiveSIFT.py:175-199),
    evaluated by numpy so the float32 taps handed to the device are the reference's."""
    mean = ksize // 2
    axis = np.linspace(-mean, mean, ksize)
    x_square = axis[:, np.newaxis] ** 2
    y_square = axis[np.newaxis, :] ** 2
    kernel = (1 / (2 * np.pi * sigma ** 2)) * np.exp(-(x_square + y_square) / (2 * sigma ** 2))
    kernel = kernel / np.sum(kernel)
    return kernel


def params_from_dict(extractor_params: dict | None, mode: int) -> SfmParams:
    ep = {} if extractor_params is None else extractor_params
    p = SfmParams()
    p.mode = mode
    p.num_interest_points = int(ep.get("num_interest_points", 2500))
    p.ksize = int(ep.get("ksize", 7))
    p.gaussian_size = int(ep.get("gaussian_size", 7))
    p.sigma = float(ep.get("sigma", 5))
    p.alpha = float(ep.get("alpha", 0.05))
    p.feature_width = int(ep.get("feature_width", 16))
    p.pyramid_level = int(ep.get("pyramid_level", 4)) if mode == SFM_MODE_SCALEROT else 1
    p.pyramid_scale_factor = float(ep.get("pyramid_scale_factor", 2))
    gs = p.gaussian_size
    if 1 <= gs <= SFM_MAX_GAUSS:
        k = generate_gaussian_kernel(gs, ep.get("sigma", 5)).astype(np.float32).ravel()
        for i, v in enumerate(k):
            p.gauss_kernel[i] = float(v)
        p.gauss_kernel_set = 1
    return p


def keypoint_capacity(p: SfmParams) -> int:
    if p.mode == SFM_MODE_NAIVE:
        return max(int(p.num_interest_points), 0)
    L = int(p.pyramid_level)
    return max(L * int(p.num_interest_points / L), 0)
