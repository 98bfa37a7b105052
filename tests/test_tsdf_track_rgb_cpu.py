"""CPU: the restatement of tracking on shape and colour (tests/tsdf_track_rgb_ref.py) against itself -- its joint
Jacobian against central differences, the conditions the GPU fixture must meet, both halves of the claim on the ambiguous ring -- and
reconstruct.py's handling of track_color_weight / track_color_max."""
import numpy as np
import pytest

from foundpose_amd import reconstruct
from tests import tsdf_track_ref as tr
from tests import tsdf_track_rgb_ref as rr

MC, MD, W, CMAX = tr.TRACK_MIN_COUNT, tr.TRACK_MAX_DIST, rr.RGB_WEIGHT, rr.RGB_MAX


def test_joint_jacobian_matches_central_differences():
    """Shape and colour are multilinear inside a cell: away from cell faces the only error of a central difference is its step.  The
    bounds are set wide so that every point keeps its four residuals on both sides of the step."""
    vol, tau, md, cmax, w = rr.hand_volume_rgb(), 4.0, 1e3, 10.0, 7.0
    rng = np.random.default_rng(0)
    R = tr.rot_exp(rng.normal(size=3) * 0.4)
    t = np.array([3.0, -2.0, 300.0])
    Xm = rng.uniform(-9.0, 9.0, size=(400, 3))
    Xc = Xm @ R.T + t
    col = rng.uniform(0.0, 1.0, size=(400, 3)).astype(np.float32)
    p = rr.point_terms(vol, R, t, Xc, col, tau, 1, md, w, cmax)
    frac = p["g"] - np.floor(p["g"])
    keep = p["color_measurable"] & np.all((frac > 1e-3) & (frac < 1.0 - 1e-3), axis=1) & (np.abs(p["Jc"]).max((1, 2)) > 0)
    assert keep.sum() > 100 and p["channel"][keep].all()
    J = np.concatenate([p["J"][:, None, :], p["Jc"]], 1)[keep]              # [P, 4 residuals, 6]
    eps, worst = 1e-6, 0.0
    for a in range(6):
        d = np.zeros(6)
        d[a] = eps
        rp, ep, ip, cp = rr.residuals(vol, *tr.update(R, t, d), Xc, col, tau, 1, md, w, cmax)
        rm, em, im, cm = rr.residuals(vol, *tr.update(R, t, -d), Xc, col, tau, 1, md, w, cmax)
        assert ip[keep].all() and im[keep].all() and cp[keep].all() and cm[keep].all()
        num = np.concatenate([(rp - rm)[:, None], ep - em], 1)[keep] / (2 * eps)
        worst = max(worst, float(np.abs(num - J[:, :, a]).max() / np.abs(J).max()))
    print("largest |numeric - analytic| relative to the largest entry:", worst, "; largest colour entry / largest entry:", np.abs(J[:, 1:]).max() / np.abs(J).max())
    assert worst <= 1e-6


def test_fixture_meets_the_conditions_of_the_gpu_comparison():
    fx, vol = rr.track_fixture_rgb(), rr.fixture_volume()
    tau = fx["fx"]["tau"]
    X = fx["X"].astype(np.float64)
    p = rr.point_terms(vol, fx["R"], fx["t"], X, fx["colors"], tau, MC, MD, W, CMAX)
    inside = np.all(np.isfinite(p["g"]), axis=1)
    assert np.abs(p["g"][inside] - np.rint(p["g"][inside])).min() > 1e-7          # section 30's: no grid coordinate at an integer
    assert np.abs(np.abs(p["r"][p["measurable"]]) - MD).min() > 1e-7               # ... no |r| at max_dist
    cm = p["color_measurable"]
    assert np.abs(np.abs(p["e"][cm]) - CMAX).min() > 1e-7                          # no |e| at color_max
    # a geometric inlier whose cell has a corner with rgb_cnt < min_count while every sdf_cnt passes
    assert (p["inlier"] & ~cm).sum() >= 1 and p["measurable"][p["inlier"] & ~cm].all()
    # a channel outlier next to two channel inliers of the same point
    k = fx["kinds"]
    assert p["channel"][k["channel_out"]].tolist() == [True, False, True]
    # geometric outliers: never colour-measurable
    assert not p["inlier"][k["free"]] and not p["inlier"][k["outside"]] and not p["inlier"][k["unseen"]] and not cm[~p["inlier"]].any()
    E, _, _, inl = rr.system(vol, fx["R"], fx["t"], X, fx["colors"], tau, MC, MD, W, CMAX)
    Eg = tr.system(vol, fx["R"], fx["t"], X, tau, MC, MD)[0]
    out = rr.track(vol, fx["R"], fx["t"], X, fx["colors"], tau, MC, MD, W, CMAX, 20)
    print(f"{len(X)} points, {inl.sum()} geometric inliers, {cm.sum()} colour-measurable, channel inliers {p['channel'].sum(0).tolist()}; joint cost "
          f"{out['cost_in']:.4f} (geometric {Eg:.4f}) -> {out['cost_out']:.4f} in {out['iters_used']} iterations")
    assert 6 <= inl.sum() < len(X) and out["status"] == 0 and out["cost_out"] < out["cost_in"] == E and E > Eg
    for n_pts in (6, 31, 32, 33, 65, 1000):
        P, c = rr.sized_points_rgb(n_pts)
        q = rr.point_terms(vol, fx["R"], fx["t"], P.astype(np.float64), c, tau, MC, MD, W, CMAX)
        assert len(P) == len(c) == n_pts and q["inlier"].sum() >= 6 and q["channel"].sum() > 0
    Xu, cu = rr.uncoloured_points()
    q = rr.point_terms(vol, fx["R"], fx["t"], Xu.astype(np.float64), cu, tau, MC, MD, W, CMAX)
    assert len(Xu) == 40 and q["inlier"].all() and not q["color_measurable"].any()


def test_lift_points_rgb_rule():
    """The colours are those of lift_points' pixels, uint8 / 255 in fp32, on both sides; lift_points' own bits stay what they were."""
    frames, truth = rr.ambiguous_ring()
    f = frames[3]
    fr = reconstruct.Frame(f.depth, f.mask, f.rgb, f.cam, truth[3])
    for cap in (16384, 100):
        P, c = rr.lift_points_rgb(f.depth, f.mask, f.rgb, f.cam, cap)
        assert np.array_equal(P, tr.lift_points(f.depth, f.mask, f.cam, cap)) and c.dtype == np.float32 and c.shape == P.shape
        gp, gc = reconstruct.lift_points_rgb(fr, cap, device="cpu")
        assert np.array_equal(gp.numpy(), P) and np.array_equal(gc.numpy(), c) and gc.dtype == gp.dtype
        assert np.array_equal(reconstruct.lift_points(fr, cap, device="cpu").numpy(), P)
    v, u = np.nonzero(f.mask)
    assert np.array_equal(rr.lift_points_rgb(f.depth, f.mask, f.rgb, f.cam, 16384)[1][0], f.rgb[v[0], u[0]].astype(np.float32) / np.float32(255))


def _errors(weight):
    _, truth = rr.ambiguous_ring()
    _, poses, records = rr.ambiguous_chain(weight)
    assert [r["role"] for r in records] == ["anchor"] + ["tracked"] * (tr.RING_FRAMES - 1)          # no frame is lost
    errs = np.array([tr.pose_error(p, g) for p, g in zip(poses, truth)])
    print(f"weight {weight}: worst {errs[:, 0].max():.2f} deg / {errs[:, 1].max():.2f} mm, last frame {errs[-1, 0]:.2f} deg, lowest inlier share "
          f"{min(r['share'] for r in records[1:]):.3f}, iterations {sorted(set(r['iters'] for r in records[1:]))}")
    return errs, records


def test_ambiguous_ring_geometry_alone_slides_and_says_nothing():
    """The fixture is one that shape cannot track: of the 115 degrees turned the last frame must be MORE THAN 90 off, with every frame
    kept and every inlier share >= 0.95.  (The planning record measured 114.5 degrees, lowest share 0.992.)"""
    errs, records = _errors(0.0)
    assert min(r["share"] for r in records[1:]) >= 0.95
    assert errs[-1, 0] > 90.0
    assert all("color_weight" not in r for r in records)


def test_ambiguous_ring_with_colour_stays_within_one_step_and_one_voxel():
    """Weight 30 mm per unit, color_max 0.25, "velocity": every frame within 5 degrees (one ring step) and 2.5 mm (one voxel).  (The
    planning record measured 2.83 degrees / 0.88 mm, lowest share 0.984, all 20 iterations used.)"""
    errs, records = _errors(30.0)
    assert errs[:, 0].max() <= 5.0 and errs[:, 1].max() <= 2.5
    assert all(r["color_weight"] == 30.0 for r in records[1:])


# ---------------------------------------------------------------------------------------------------------- reconstruct.py's options
def test_colour_options_are_checked():
    o = reconstruct.load_opts()
    assert o.track_color_weight == 0.0 and o.track_color_max == 0.25 and o._fields[-2:] == ("track_color_weight", "track_color_max")
    o = reconstruct.load_opts({"track_color_weight": 30, "track_color_max": 0.1})
    assert o.track_color_weight == 30 and o.track_color_max == 0.1
    for bad in ({"track_color_weight": -1.0}, {"track_color_weight": float("nan")}, {"track_color_weight": float("inf")}, {"track_color_weight": True},
                {"track_color_weight": "30"}, {"track_color_max": 0.0}, {"track_color_max": -0.25}, {"track_color_max": float("nan")},
                {"track_color_max": float("inf")}, {"track_color_max": False}, {"track_color_max": None}):
        with pytest.raises(ValueError):
            reconstruct.load_opts(bad)


def _fake_ops(monkeypatch, calls):
    import torch

    from foundpose_amd import ops

    def track(vol, pts, rb, re, R, t, md, mc, tau, iters, **kw):
        calls.append(dict(kw, iters=iters, points=pts))
        one = lambda v, dt: torch.full((1,), v, dtype=dt)   # noqa: E731
        return {"R": R.reshape(1, 3, 3).double(), "t": t.reshape(1, 3).double(), "cost_in": one(2.0, torch.float64), "cost_out": one(1.0, torch.float64),
                "num_points": one(int(pts.shape[0]), torch.int32), "iters_used": one(iters, torch.int32), "status": one(0, torch.int32)}
    monkeypatch.setattr(ops, "tsdf_new_volume", lambda origin, h, dims, device: {"dims": dims})
    monkeypatch.setattr(ops, "tsdf_integrate", lambda *a: None)
    monkeypatch.setattr(ops, "tsdf_track", track)


def _three_frames():
    frames, truth = rr.ambiguous_ring()
    return [reconstruct.Frame(f.depth, f.mask, f.rgb, f.cam, p) for f, p in zip(frames[:3], truth)], [truth[0], None, None]


def test_weight_zero_leaves_the_call_sequence_as_it_was(monkeypatch):
    calls = []
    _fake_ops(monkeypatch, calls)
    fr, given = _three_frames()
    opts = {"pose_source": "track", "voxel_mm": 2.5, "bounds": tr.RING_BOUNDS}
    for o in (opts, dict(opts, track_color_weight=0.0, track_color_max=0.1)):
        calls.clear()
        _, poses, records = reconstruct.fuse_tracked(fr, given, o, device="cpu")
        assert [c["iters"] for c in calls] == [20, 0, 20, 0]                     # per tracked frame: the track, the score at the result
        assert all(set(c) == {"iters", "points"} for c in calls)                 # no colors, color_weight or color_max keyword arrives
        assert all("color_weight" not in r for r in records)
        assert np.array_equal(calls[0]["points"].numpy(), tr.lift_points(fr[1].depth, fr[1].mask, fr[1].cam, 16384))


def test_a_weight_passes_the_colours_to_the_track_call_only(monkeypatch):
    calls = []
    _fake_ops(monkeypatch, calls)
    fr, given = _three_frames()
    _, poses, records = reconstruct.fuse_tracked(fr, given, {"pose_source": "track", "voxel_mm": 2.5, "bounds": tr.RING_BOUNDS, "track_color_weight": 30.0,
                                                             "track_color_max": 0.2}, device="cpu")
    assert [c["iters"] for c in calls] == [20, 0, 20, 0]
    for k, (trk, score) in enumerate(zip(calls[0::2], calls[1::2]), start=1):
        P, c = rr.lift_points_rgb(fr[k].depth, fr[k].mask, fr[k].rgb, fr[k].cam, 16384)
        assert set(trk) == {"iters", "points", "colors", "color_weight", "color_max"} and trk["color_weight"] == 30.0 and trk["color_max"] == 0.2
        assert np.array_equal(trk["colors"].numpy(), c) and np.array_equal(trk["points"].numpy(), P)
        assert set(score) == {"iters", "points"}                                 # share, rms and the lost-frame rule keep their meaning
        assert records[k]["color_weight"] == 30.0 and records[k]["cost_in"] == 2.0 and records[k]["cost_out"] == 1.0
    assert "color_weight" not in records[0]
