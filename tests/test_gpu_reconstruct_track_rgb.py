"""GPU: reconstruct.fuse_tracked on shape and colour (track_color_weight) over the ambiguous ring of
tests/tsdf_track_rgb_ref.py -- an ellipsoid of revolution rendered analytically, 24 cameras 5 degrees apart, only frame 0's pose known:
tracked on shape alone the chain slides by the whole turn without a lost frame, tracked on shape and colour it stays within one ring
step and one voxel.  Then once through the command line, on the ring written as a BOP scene directory."""
import json

import numpy as np
import pytest

from foundpose_amd import reconstruct
from foundpose_amd.gt_info import _read_json
from tests import tsdf_track_ref as tr
from tests import tsdf_track_rgb_ref as rr

pytestmark = pytest.mark.gpu
BASE = {"pose_source": "track", "voxel_mm": tr.RING_H, "trunc_voxels": tr.RING_TRUNC_VOXELS, "bounds": tr.RING_BOUNDS}


@pytest.fixture(scope="module")
def ring():
    frames, truth = rr.ambiguous_ring()
    return [reconstruct.Frame(f.depth, f.mask, f.rgb, f.cam, np.full(12, np.nan)) for f in frames], truth


def _chain(ring, weight):
    frames, truth = ring
    _, poses, records = reconstruct.fuse_tracked(frames, [truth[0]] + [None] * (len(frames) - 1), dict(BASE, track_color_weight=weight, track_color_max=rr.RGB_MAX))
    assert [r["role"] for r in records] == ["anchor"] + ["tracked"] * (tr.RING_FRAMES - 1)          # no frame is lost
    errs = np.array([tr.pose_error(p, g) for p, g in zip(poses, truth)])
    # the chain against the restatement's: printed, not barred -- after a 1e-9 pose difference one nearest-pixel tap of the integration
    # may legitimately flip, and the chains part by more than rounding from there (section 30)
    drift = np.array([tr.pose_error(p, q) for p, q in zip(poses, rr.ambiguous_chain(weight)[1])])
    print(f"weight {weight}: worst {errs[:, 0].max():.3f} deg / {errs[:, 1].max():.3f} mm, last frame {errs[-1, 0]:.3f} deg, lowest inlier share "
          f"{min(r['share'] for r in records[1:]):.3f}, iterations {sorted(set(r['iters'] for r in records[1:]))}; against the restatement's chain at most "
          f"{drift[:, 0].max():.3e} deg, {drift[:, 1].max():.3e} mm apart")
    return errs, records


def test_geometry_alone_slides_by_the_whole_turn_and_loses_no_frame(ring):
    errs, records = _chain(ring, 0.0)
    assert min(r["share"] for r in records[1:]) >= 0.95
    assert errs[-1, 0] > 90.0
    assert all("color_weight" not in r for r in records)


def test_with_colour_every_frame_stays_within_one_step_and_one_voxel(ring):
    errs, records = _chain(ring, 30.0)
    assert errs[:, 0].max() <= 5.0 and errs[:, 1].max() <= 2.5
    for r in records[1:]:
        assert r["color_weight"] == 30.0 and r["status"] in (0, 1) and r["cost_out"] <= r["cost_in"] and r["points"] > 1000
        assert 0.0 <= r["rms"] <= tr.RING_H * 3.0 and r["inliers_out"] == round(r["share"] * r["points"])   # the score is the geometric one


def test_command_line_run_records_the_weight(tmp_path):
    truth = tr.ring_poses()
    raw = [rr.render_ellipsoid(p) for p in truth]
    scene = str(tmp_path / "ring" / "000001")
    tr.write_ring_scene(scene, np.stack([r[2] for r in raw]) / 255.0, np.stack([r[0] for r in raw]), np.stack([r[1] for r in raw]), truth)
    (tmp_path / "opts.json").write_text(json.dumps(dict(BASE, track_color_weight=30.0)))
    args = ["--sequence", scene, "--obj-id", "1", "--output", str(tmp_path / "models"), "--opts", str(tmp_path / "opts.json"), "--report",
            str(tmp_path / "report.json"), "--tracked-poses", str(tmp_path / "poses")]
    assert reconstruct.main(args) == 0
    rep = json.load(open(tmp_path / "report.json"))
    assert rep["opts"]["track_color_weight"] == 30.0 and rep["opts"]["track_color_max"] == 0.25
    assert rep["tracking"]["totals"] == {"anchor": 1, "tracked": 23, "lost": 0, "color_weight": 30.0} and rep["frames_used"] == 24
    assert all(r["color_weight"] == 30.0 for r in rep["tracking"]["frames"][1:])
    got = _read_json(str(tmp_path / "poses" / "000000_scene_gt.json"))
    assert len(got) == 24 and sorted(int(k) for k in got) == list(range(24))
    errs = np.array([[r["rot_err_deg"], r["t_err_mm"]] for r in rep["tracking"]["frames"][1:]])
    print(f"command line, weight 30: worst {errs[:, 0].max():.3f} deg / {errs[:, 1].max():.3f} mm; {rep['tracking']['seconds']:.3f} s tracking")
    assert errs[:, 0].max() <= 5.0 and errs[:, 1].max() <= 2.5
