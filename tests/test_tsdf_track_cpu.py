"""CPU: the restatement of frame-to-model tracking (tests/tsdf_track_ref.py) against itself -- its Jacobian
against central differences, the conditions the GPU fixture must meet, the chained sequence inside the caps, a lost frame -- and
reconstruct.py's option handling for pose_source "track"."""
import functools

import numpy as np
import pytest

from foundpose_amd import reconstruct
from tests import tsdf_ref
from tests import tsdf_track_ref as tr

CAP_DEG, CAP_MM = 3.0, 2.5


def test_jacobian_matches_central_differences():
    """The interpolant is multilinear inside a cell: away from cell faces the only error of a central difference is its step."""
    vol, tau = tr.hand_volume(), 4.0
    rng = np.random.default_rng(0)
    R = tr.rot_exp(rng.normal(size=3) * 0.4)
    t = np.array([3.0, -2.0, 300.0])
    Xm = rng.uniform(-9.0, 9.0, size=(400, 3))
    Xc = Xm @ R.T + t
    p = tr.point_terms(vol, R, t, Xc, tau, 1)
    frac = p["g"] - np.floor(p["g"])
    keep = p["measurable"] & np.all((frac > 1e-3) & (frac < 1.0 - 1e-3), axis=1) & (np.abs(p["J"]).max(1) > 0)
    assert keep.sum() > 100
    eps, worst = 1e-6, 0.0
    for a in range(6):
        d = np.zeros(6)
        d[a] = eps
        rp, okp = tr.residual(vol, *tr.update(R, t, d), Xc, tau, 1)
        rm, okm = tr.residual(vol, *tr.update(R, t, -d), Xc, tau, 1)
        assert okp[keep].all() and okm[keep].all()
        num = (rp - rm)[keep] / (2 * eps)
        worst = max(worst, float(np.abs(num - p["J"][keep, a]).max() / np.abs(p["J"][keep]).max()))
    print("largest |numeric - analytic| relative to the largest entry:", worst)
    assert worst <= 1e-6


def test_fixture_meets_the_conditions_of_the_gpu_comparison():
    fx, vol = tr.track_fixture(), tr.fixture_volume()
    tau = fx["fx"]["tau"]
    X = fx["X"].astype(np.float64)
    p = tr.point_terms(vol, fx["R"], fx["t"], X, tau, tr.TRACK_MIN_COUNT)
    inside = np.all(np.isfinite(p["g"]), axis=1)
    assert np.abs(p["g"][inside] - np.rint(p["g"][inside])).min() > 1e-7          # no grid coordinate at an integer
    assert np.abs(np.abs(p["r"][p["measurable"]]) - tr.TRACK_MAX_DIST).min() > 1e-7   # no |r| at max_dist
    n = np.array(vol["dims"], np.float64)
    g = p["g"]
    in_vol = np.all((g >= 0) & (g < n - 1), axis=1)
    k = fx["kinds"]
    assert not in_vol[k["outside"]]
    assert in_vol[k["unseen"]] and not p["measurable"][k["unseen"]]
    assert p["measurable"][k["free"]] and abs(p["r"][k["free"]]) >= tr.TRACK_MAX_DIST
    E, _, _, inl = tr.system(vol, fx["R"], fx["t"], X, tau, tr.TRACK_MIN_COUNT, tr.TRACK_MAX_DIST)
    out = tr.track(vol, fx["R"], fx["t"], X, tau, tr.TRACK_MIN_COUNT, tr.TRACK_MAX_DIST, 20)
    e0 = tr.pose_error(np.concatenate([fx["R"].reshape(9), fx["t"]]), fx["fx"]["poses"][0])
    e1 = tr.pose_error(np.concatenate([out["R"].reshape(9), out["t"]]), fx["fx"]["poses"][0])
    print(f"{len(X)} points, {inl.sum()} inliers; cost {out['cost_in']:.4f} -> {out['cost_out']:.4f} in {out['iters_used']} iterations; "
          f"{e0[0]:.3f} deg / {e0[1]:.3f} mm -> {e1[0]:.3f} deg / {e1[1]:.3f} mm")
    assert 6 <= inl.sum() < len(X) and out["status"] == 0 and out["cost_out"] < out["cost_in"] == E
    for n_pts in (6, 31, 32, 33, 65, 1000):
        P = tr.sized_points(n_pts)
        assert len(P) == n_pts and tr.system(vol, fx["R"], fx["t"], P.astype(np.float64), tau, tr.TRACK_MIN_COUNT, tr.TRACK_MAX_DIST)[3].sum() >= 6


def test_lift_points_rule():
    depth = np.zeros((5, 7), np.float32)
    mask = np.zeros((5, 7), np.uint8)
    depth[1:4, 2:6], mask[1:5, 1:5] = 500.0, 1
    depth[2, 3] = 0.0
    cam = (100.0, 110.0, 3.2, 2.1)
    P = tr.lift_points(depth, mask, cam, 100)
    assert len(P) == 8 and P.dtype == np.float32                            # rows 1..3 x columns 2..4, less the hole
    assert np.allclose(P[0], [(2 - 3.2) / 100.0 * 500.0, (1 - 2.1) / 110.0 * 500.0, 500.0], rtol=1e-6)
    assert np.array_equal(tr.lift_points(depth, mask, cam, 3), P[::3])       # every ceil(8 / 3)-th
    assert np.array_equal(tr.lift_points(depth, mask, cam, 8), P)


def test_motion_models():
    T1 = tr.to_T(tr.rot_exp([0.0, 0.0, 0.1]), [1.0, 2.0, 400.0])
    D = tr.to_T(tr.rot_exp([0.02, -0.01, 0.03]), [0.5, 0.0, -1.0])
    T2 = D @ T1
    assert np.array_equal(tr.predict([(0, T1)], 1, "velocity"), T1)
    assert np.array_equal(tr.predict([(0, T1), (1, T2)], 2, "hold"), T2)
    assert np.allclose(tr.predict([(0, T1), (1, T2)], 2, "velocity"), D @ T2, atol=1e-12)
    assert np.array_equal(tr.predict([(0, T1), (1, T2)], 3, "velocity"), T2)   # frame 2 was lost: hold
    for hist, idx, motion in (([(0, T1), (1, T2)], 2, "velocity"), ([(0, T1), (1, T2)], 3, "velocity"), ([(0, T1)], 1, "hold")):
        assert np.allclose(reconstruct.predict_pose(hist, idx, motion), tr.predict(hist, idx, motion), atol=1e-14)


@functools.lru_cache(maxsize=None)
def _chain(motion):
    frames, truth = tr.ring_frames_cpu()
    given = [truth[0]] + [None] * (len(frames) - 1)
    return tr.fuse_tracked(frames, given, tr.RING_BOUNDS[0], tr.RING_H, tr.RING_DIMS, tr.RING_TRUNC_VOXELS, track_motion=motion)


@pytest.mark.parametrize("motion", ["hold", "velocity"])
def test_chained_sequence_stays_inside_the_caps(motion):
    _, truth = tr.ring_frames_cpu()
    vol, poses, records = _chain(motion)
    assert [r["role"] for r in records] == ["anchor"] + ["tracked"] * (tr.RING_FRAMES - 1)
    errs = np.array([tr.pose_error(p, g) for p, g in zip(poses, truth)])
    print(f"{motion}: worst rotation error {errs[:, 0].max():.3f} deg, worst |dt| {errs[:, 1].max():.3f} mm, "
          f"lowest inlier share {min(r['share'] for r in records[1:]):.3f}")
    assert errs[:, 0].max() <= CAP_DEG and errs[:, 1].max() <= CAP_MM


def test_restatement_chain_mesh_renders_back_onto_the_frames():
    """The mesh of the restatement's chain, rendered at the TRACKED poses of four frames round the ring, agrees with the input frames
    within one voxel (median |d depth| over co-covered pixels): the cap tests/test_gpu_reconstruct_track.py holds the kernel's chain to."""
    from tests import render_ref
    frames, _ = tr.ring_frames_cpu()
    vol, poses, _ = _chain("velocity")
    v, _, f = tr.mesh_from_volume(vol, 2, reconstruct.largest_component)
    cam = np.array([tr.RING_CAM[0], tr.RING_CAM[1], tr.RING_CAM[2] + 0.5, tr.RING_CAM[3] + 0.5])
    pick = (0, 8, 16, 23)
    rd, rm = [], []
    for k in pick:
        d, tri, _ = render_ref.rasterize(v, f, tsdf_ref.render_cam(cam, poses[k][:9].reshape(3, 3), poses[k][9:]), tsdf_ref.SEQ_W, tsdf_ref.SEQ_H)
        rd.append(np.where(tri >= 0, d, 0)), rm.append(tri >= 0)
    med, p95, iou = tsdf_ref.render_agreement(np.stack(rd), np.stack(rm), np.stack([frames[k].depth for k in pick]), np.stack([frames[k].mask for k in pick]))
    print(f"{len(v)} vertices, {len(f)} faces; median |d depth| {med:.3f} mm, 95th percentile {p95:.3f} mm, silhouette IoU {iou:.4f}")
    assert med <= CAP_MM


# The share of inliers that tells a lost frame in these two tests.  A frame tracked correctly lays all its points on the surface fused from
# the frames before it, less what the 5 degree step newly reveals (about 5 / 180 of the visible half) and the pixels on the silhouette,
# whose depth mixes in nothing here but whose cells end at the seen surface: nine points in ten and more.  The default, 0.5, asks only
# that most points fit, and on this smooth blob a view from 60 degrees further on still finds a pose that fits two thirds of them
# (limits); 0.8 sits between.
LOST_SHARE = 0.8


def _with_wrong_depth(frames, positions):
    """The frames at `positions` keep their mask and take the depth image of the 12th frame's view 60 degrees further on."""
    wrong = tr.ring_frames_cpu(1, tr.RING_STEP_DEG, 11 * tr.RING_STEP_DEG + 60.0)[0][0]
    return [tr.RefFrame(wrong.depth, f.mask, f.rgb, f.cam) if k in positions else f for k, f in enumerate(frames)]


def test_a_lost_frame_is_left_out_and_the_next_starts_from_the_last_kept_pose():
    frames, truth = tr.ring_frames_cpu()
    frames = _with_wrong_depth(frames[:14], (11,))
    given = [truth[0]] + [None] * 13
    vol, poses, records = tr.fuse_tracked(frames, given, tr.RING_BOUNDS[0], tr.RING_H, tr.RING_DIMS, tr.RING_TRUNC_VOXELS,
                                             track_min_inlier_share=LOST_SHARE)
    print("the wrong frame:", {k: v for k, v in records[11].items() if k != "start"})
    assert [r["role"] for r in records] == ["anchor"] + ["tracked"] * 10 + ["lost", "tracked", "tracked"]
    assert poses[11] is None and np.array_equal(records[12]["start"], poses[10])
    again = tsdf_ref.new_volume(tr.RING_BOUNDS[0], tr.RING_H, tr.RING_DIMS)
    for f, p in zip(frames, poses):
        if p is not None:
            tsdf_ref.integrate(again, f.depth[None], f.mask[None], f.rgb[None], np.array([f.cam]), p[None], tr.RING_TRUNC_VOXELS * tr.RING_H)
    assert np.array_equal(again["sdf_cnt"], vol["sdf_cnt"]) and np.array_equal(again["sdf_sum"], vol["sdf_sum"])   # the lost frame was not fused
    assert max(tr.pose_error(poses[k], truth[k])[1] for k in (12, 13)) <= CAP_MM


def test_four_lost_frames_in_a_row_raise():
    frames, truth = tr.ring_frames_cpu()
    frames = _with_wrong_depth(frames[:15], (11, 12, 13, 14))
    with pytest.raises(RuntimeError, match="frame 14"):
        tr.fuse_tracked(frames, [truth[0]] + [None] * 14, tr.RING_BOUNDS[0], tr.RING_H, tr.RING_DIMS, tr.RING_TRUNC_VOXELS, track_min_inlier_share=LOST_SHARE)


# ---------------------------------------------------------------------------------------------------------- reconstruct.py's options
def test_track_options_are_checked():
    o = reconstruct.load_opts({"pose_source": "track", "bounds": tr.RING_BOUNDS, "track_anchor_every": 8})
    assert o.pose_source == "track" and o.track_anchor_every == 8 and o.track_iters == 20 and o.track_max_dist_voxels == 3.0
    assert o.track_min_count == 1 and o.track_max_points == 16384 and o.track_motion == "velocity" and o.track_min_inlier_share == 0.5 and o.track_max_lost == 3
    for bad in ({"pose_source": "guess"}, {"track_motion": "acceleration"}, {"track_anchor_every": -1}, {"track_anchor_every": 1.5}, {"track_iters": 1001},
                {"track_iters": True}, {"track_max_dist_voxels": 0.0}, {"track_max_dist_voxels": float("nan")}, {"track_max_dist_voxels": 4.5},
                {"track_max_dist_voxels": 3.0, "trunc_voxels": 2.0}, {"track_min_count": 0}, {"track_max_points": 0}, {"track_min_inlier_share": 1.5},
                {"track_min_inlier_share": -0.1}, {"track_max_lost": -1}, {"track_motion": None}):
        with pytest.raises(ValueError):
            reconstruct.load_opts(bad)


def test_given_mode_is_what_it_was(monkeypatch):
    from foundpose_amd import ops
    o = reconstruct.load_opts()
    assert o.pose_source == "given"
    assert o._asdict() == dict(reconstruct.ReconstructOpts()._asdict())
    assert tuple(o)[:7] == (2.0, 4.0, 2, None, "mask_visib", True, 32) and o._fields[:7] == (
        "voxel_mm", "trunc_voxels", "min_count", "bounds", "mask_dir", "keep_largest", "frame_batch")
    # fuse's call sequence: one new volume, then one tsdf_integrate per batch of frame_batch frames with the given poses; never tsdf_track
    frames, truth = tr.ring_frames_cpu()
    fr = [reconstruct.Frame(f.depth, f.mask, f.rgb, f.cam, p) for f, p in zip(frames[:5], truth)]
    calls = []
    monkeypatch.setattr(ops, "tsdf_new_volume", lambda origin, h, dims, device: calls.append(("new", origin, h, dims)) or {"dims": dims})
    monkeypatch.setattr(ops, "tsdf_integrate", lambda vol, d, m, c, cams, poses, tau: calls.append(("integrate", tuple(d.shape), poses.copy(), tau)))
    monkeypatch.setattr(ops, "tsdf_track", lambda *a, **k: pytest.fail("pose_source 'given' tracked a frame"))
    reconstruct.fuse(fr, {"bounds": tr.RING_BOUNDS, "voxel_mm": 2.5, "frame_batch": 2, "pose_source": "given"}, device="cpu")
    assert [c[0] for c in calls] == ["new", "integrate", "integrate", "integrate"]
    assert calls[0][1:] == (tr.RING_BOUNDS[0], 2.5, tr.RING_DIMS)
    assert [c[1][0] for c in calls[1:]] == [2, 2, 1] and all(c[3] == 10.0 for c in calls[1:])
    assert np.array_equal(np.concatenate([c[2] for c in calls[1:]]), np.stack(truth[:5]))


def test_track_mode_needs_bounds_and_a_first_pose():
    frames, truth = tr.ring_frames_cpu()
    fr = [reconstruct.Frame(f.depth, f.mask, f.rgb, f.cam, p) for f, p in zip(frames[:3], truth)]
    with pytest.raises(ValueError, match="bounds.*span.*leave room"):
        reconstruct.fuse_tracked(fr, [truth[0], None, None], {"pose_source": "track", "voxel_mm": 2.5}, device="cpu")
    with pytest.raises(ValueError, match="no pose"):
        reconstruct.fuse_tracked(fr, [None, truth[1], None], {"pose_source": "track", "voxel_mm": 2.5, "bounds": tr.RING_BOUNDS}, device="cpu")
    with pytest.raises(ValueError, match="no pose"):
        reconstruct.fuse_tracked(fr, [truth[0], None, None], {"pose_source": "track", "bounds": tr.RING_BOUNDS}, device="cpu", sequence=[0, 0, 1])
