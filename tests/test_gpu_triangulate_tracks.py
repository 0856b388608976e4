"""GPU: N-view triangulation of feature tracks (pose.triangulate_tracks, tracks.hip) on the planted
scene of tests/tracks_ref.py: 6 cameras on an arc, 200 points, integer pixels, tracks built on
the device from ground-truth matches with 5 % wrong ones.

Tolerance (the convention of test_gpu_registry.py / test_gpu_structure.py): 100 x the largest value
measured on the MI355X, capped at 1e-10; the figure is printed before its assertion.
  X_TOL  max |X_gpu - X_rest| / |X_rest| against the restatement's SVD over every track and every
         cam_valid case: measured 1.568e-14 (cam_valid 1, 0, 1, 1, 0, 1; all cameras valid
         1.534e-14, by track length 2: 1.534e-14, 3: 1.140e-14, 6: 1.113e-14), bound 1.568e-12.
         The same bound holds the two-view tracks against pose.triangulate on the same rows
         (measured 2.351e-15 over 53 tracks).
The restatement's own distance from extended-precision rows is in tests/test_tracks_cpu.py."""
from __future__ import annotations

import functools
import types

import numpy as np
import pytest

from tests import tracks_ref as TR

pytestmark = pytest.mark.gpu

MEASURED_X = 1.568e-14
X_TOL = min(1e-10, 100 * MEASURED_X)


@functools.lru_cache(maxsize=None)
def scene():
    """The planted scene, its tracks from the device and from the restatement (built once)."""
    import torch
    from sfmfromscratch_amd import sequence as S
    s = TR.planted_scene()
    dev = torch.device("cuda", 0)
    table = types.SimpleNamespace(count=torch.from_numpy(s["count"]).to(dev), xy=torch.from_numpy(s["xy"]).to(dev))
    tr = S.build_tracks(table, s["pairs"], (torch.from_numpy(s["matches"]).to(dev), None,
                                            torch.from_numpy(s["nmatch"]).to(dev)))
    e = TR.build_tracks(s["count"], s["cap"], s["pairs"], s["matches"], s["nmatch"], None, 2)
    for k in ("offsets", "obs_slot", "obs_row"):
        assert np.array_equal(getattr(tr, k), e[k])
    return s, tr, e


def rel(X, R):
    return float((np.linalg.norm(X - R, axis=1) / np.linalg.norm(R, axis=1)).max())


def test_points_equal_the_restatements_svd():
    from sfmfromscratch_amd import pose
    s, tr, e = scene()
    lens = np.diff(e["offsets"])
    assert {2, 3, 6} <= set(lens.tolist())            # track lengths 2, 3 and 6
    X, views = pose.triangulate_tracks(tr, s["P"])
    Xr, vr = TR.triangulate_tracks(e["offsets"], e["obs_slot"], e["obs_row"], s["xy"], s["P"])
    assert X.shape == (tr.n_tracks, 3) and X.dtype == np.float64 and views.dtype == np.int32
    assert np.array_equal(views, vr) and np.array_equal(views, lens)
    worst = {int(L): rel(X[lens == L], Xr[lens == L]) for L in sorted(set(lens.tolist()))}
    print(f"MEASURED triangulate_tracks vs restatement: {max(worst.values()):.3e} (by track length {worst})")
    assert max(worst.values()) <= X_TOL
    # the same bits every run
    X2, _ = pose.triangulate_tracks(tr, s["P"])
    assert X.tobytes() == X2.tobytes()
    # a device tensor P gives device tensors
    import torch
    Xd, vd = pose.triangulate_tracks(tr, torch.from_numpy(s["P"]).to(tr.xy.device))
    assert Xd.is_cuda and Xd.cpu().numpy().tobytes() == X.tobytes() and np.array_equal(vd.cpu().numpy(), views)


def test_two_view_tracks_equal_the_two_view_triangulation():
    from sfmfromscratch_amd import pose
    s, tr, e = scene()
    X, _ = pose.triangulate_tracks(tr, s["P"])
    off, lens = e["offsets"], np.diff(e["offsets"])
    worst, n = 0.0, 0
    for a in range(5):
        for b in range(a + 1, 6):
            ts = [t for t in np.nonzero(lens == 2)[0] if e["obs_slot"][off[t]] == a and e["obs_slot"][off[t] + 1] == b]
            if not ts:
                continue
            p1 = np.array([s["xy"][a, e["obs_row"][off[t]]] for t in ts], np.float64)
            p2 = np.array([s["xy"][b, e["obs_row"][off[t] + 1]] for t in ts], np.float64)
            X2 = pose.triangulate(p1, p2, s["P"][a], s["P"][b])
            worst = max(worst, rel(X[ts], X2))
            n += len(ts)
    print(f"MEASURED triangulate_tracks vs pose.triangulate on {n} two-view tracks: {worst:.3e}")
    assert n >= 20 and worst <= X_TOL


@pytest.mark.parametrize("valid", [(1, 1, 0, 0, 0, 0), (0, 0, 0, 1, 0, 0), (0, 0, 0, 0, 0, 0), (1, 0, 1, 1, 0, 1)])
def test_cam_valid(valid):
    """Masks that leave 2 views, 1 view and 0 views: below 2 the point is NaN; views is exact."""
    from sfmfromscratch_amd import pose
    s, tr, e = scene()
    cv = np.array(valid, np.uint8)
    X, views = pose.triangulate_tracks(tr, s["P"], cam_valid=cv)
    Xr, vr = TR.triangulate_tracks(e["offsets"], e["obs_slot"], e["obs_row"], s["xy"], s["P"], cv)
    assert np.array_equal(views, vr)
    if sum(valid) == 2:
        assert {0, 1, 2} <= set(views.tolist())
    if sum(valid) <= 1:
        assert views.max() == sum(valid)
    ok = views >= 2
    assert np.isnan(X[~ok]).all() and np.isfinite(X[ok]).all()
    if ok.any():
        d = rel(X[ok], Xr[ok])
        print(f"MEASURED triangulate_tracks cam_valid {valid}: {d:.3e}")
        assert d <= X_TOL
    Xb, vb = pose.triangulate_tracks(tr, s["P"], cam_valid=cv.astype(bool))
    assert Xb.tobytes() == X.tobytes() and np.array_equal(vb, views)


def test_tracks_feed_bundle_adjustment():
    """ba_inputs() and the triangulated points go straight into pose.BundleAdjustment."""
    from sfmfromscratch_amd import pose
    s, tr, _ = scene()
    X, _ = pose.triangulate_tracks(tr, s["P"])
    cam, pt, p2 = tr.ba_inputs()
    params = np.array([np.hstack((pose.rodrigues(s["R"][c])[0].ravel(), s["t"][c])) for c in range(6)])
    info = {}
    ba = pose.BundleAdjustment(6, tr.n_tracks, cam, pt, p2, params, X, np.array([s["K"]] * 6), fixed_cameras=[0],
                               info=info)
    cams, pts = ba.sparse_bundle_adjustment()
    print(f"bundle adjustment over {tr.n_tracks} tracks, {tr.n_obs} observations: cost {info['cost0']:.6e} -> "
          f"{info['cost']:.6e}, status {info['status']}")
    assert np.isfinite(info["cost0"]) and info["cost"] <= info["cost0"]
    assert cams.shape == (6, 6) and pts.shape == (tr.n_tracks, 3) and np.isfinite(pts).all()


def test_tracks_with_unposed_frames_feed_bundle_adjustment():
    """INTEGRATION.md's recipe when some frames have no pose yet: the NaN tracks go, with them the
    observations in unposed frames, and the remaining indices are renumbered."""
    from sfmfromscratch_amd import pose
    s, tr, _ = scene()
    have_pose = np.array([1, 1, 1, 1, 0, 0], bool)
    X, views = pose.triangulate_tracks(tr, s["P"], cam_valid=have_pose)
    cam, pt, p2 = tr.ba_inputs()
    good = np.isfinite(X).all(axis=1)
    assert good.any() and (~good).any() and np.array_equal(good, views >= 2)
    sel = good[pt] & have_pose[cam]
    remap = np.cumsum(good) - 1
    params = np.array([np.hstack((pose.rodrigues(s["R"][c])[0].ravel(), s["t"][c])) for c in range(6)])
    info = {}
    ba = pose.BundleAdjustment(6, int(good.sum()), cam[sel], remap[pt[sel]], p2[sel], params, X[good],
                               np.array([s["K"]] * 6), fixed_cameras=[0], info=info)
    cams, pts = ba.sparse_bundle_adjustment()
    assert np.isfinite(info["cost0"]) and info["cost"] <= info["cost0"]
    assert np.array_equal(np.bincount(remap[pt[sel]], minlength=int(good.sum())), views[good])
    assert cams[4:].tobytes() == params[4:].tobytes() and np.isfinite(pts).all()   # unposed cameras: untouched


def test_argument_errors():
    from sfmfromscratch_amd import pose
    s, tr, _ = scene()
    with pytest.raises(ValueError):
        pose.triangulate_tracks(tr, s["P"][:, :, :3])
    with pytest.raises(ValueError):
        pose.triangulate_tracks(tr, s["P"], cam_valid=np.ones(5, np.uint8))
