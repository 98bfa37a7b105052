"""coarse_select_type "depth_verify" through both drivers on the planted split of tests/test_gpu_depth_refine.py's driver test: infer and
infer_batched write the same estimated-poses.json, every instance is found, the option composes with pnp_type "kabsch_depth" and with a
depth-refining final pose, a frame without depth is refused by name, and the default is the path it was.  The split's correspondences are
exact: this shows that the stage is wired, not that it chooses better.  That it chooses better is shown at the pnp_util level on the
blob fixture of tests/pose_verify_ref.py: select_best_coarse takes the turned pose of the higher quality, select_best_verified the planted one."""

import numpy as np
import pytest
import torch

from tests import pose_verify_ref as pv
from tests.test_gpu_depth_refine import _drive, driver_split  # noqa: F401  (the module-scoped fixture and the driver runner)

pytestmark = pytest.mark.gpu


def _same_in_both_drivers(tmp_path, driver_split, tag, vopts):
    ex, split, _, depths = driver_split
    per_object, full = _drive(tmp_path, tag, ex, split, vopts, depths)
    assert [len(per_object[lid]) for lid in (1, 2)] == [4, 2]          # every instance of the split is found
    for batch in (1, 4):
        batched, _ = _drive(tmp_path, f"{tag}_b{batch}", ex, split, vopts, depths, batch=batch)
        assert batched == per_object, batch
    assert all(e["time"]["pose_coarse"] > 0 for es in full.values() for e in es)
    return per_object, full


def test_both_drivers_write_the_same_poses(tmp_path, driver_split):
    ex, split, opts, depths = driver_split
    vopts = opts._replace(coarse_select_type="depth_verify")
    _same_in_both_drivers(tmp_path, driver_split, "v", vopts)
    with pytest.raises(ValueError, match="scene 1 image 3: coarse_select_type 'depth_verify'"):
        _drive(tmp_path, "nodepth", ex, split, vopts, None)
    with pytest.raises(ValueError, match="scene 1 image 3: coarse_select_type 'depth_verify'"):
        _drive(tmp_path, "nodepth_b", ex, split, vopts, None, batch=4)


def test_composes_with_kabsch_depth_and_a_depth_refining_final_pose(tmp_path, driver_split):
    opts = driver_split[2]
    _same_in_both_drivers(tmp_path, driver_split, "vk", opts._replace(coarse_select_type="depth_verify", pnp_type="kabsch_depth"))
    _, full = _same_in_both_drivers(tmp_path, driver_split, "vd", opts._replace(coarse_select_type="depth_verify", final_pose_type="depth",
                                                                               depth_refine_iters=10, depth_verify_thresh=6.0,
                                                                               depth_verify_max_points=500))
    assert all(e["time"]["pose_refine"] > 0 for es in full.values() for e in es)


def test_the_default_is_the_inlier_count(tmp_path, driver_split):
    ex, split, opts, depths = driver_split
    assert opts.coarse_select_type == "inliers"
    default, _ = _drive(tmp_path, "d", ex, split, opts, None)   # (no depth needed)
    explicit, _ = _drive(tmp_path, "e", ex, split, opts._replace(coarse_select_type="inliers"), None)
    assert explicit == default and [len(default[lid]) for lid in (1, 2)] == [4, 2]
    batched, _ = _drive(tmp_path, "e_b4", ex, split, opts._replace(coarse_select_type="inliers"), None, batch=4)
    assert batched == default


@pytest.fixture(scope="module")
def blob():
    fix = pv.gpu_fixture()
    ref = pv.run_ref_on(fix)
    assert ref["min_margin"] > 1e-6
    return fix, ref, pv.make_bank(fix)


def test_verification_picks_the_planted_pose_where_the_inlier_count_picks_the_turned_one(blob):
    """One detection, two hypotheses: the pose turned 180 degrees about the view axis with the higher coarse quality, the planted pose with
    a lower one."""
    from foundpose_amd import pnp_util
    fix, ref, bank = blob
    dev = "cuda"
    sel = np.array([[2, 0]])
    poses = {"success": torch.from_numpy(fix["success"][sel]).to(dev), "R": torch.from_numpy(fix["R"][sel]).to(dev), "t": torch.from_numpy(fix["t"][sel]).to(dev),
             "quality": torch.tensor([[80.0, 35.0]], dtype=torch.float64, device=dev)}
    verify = pnp_util.verify_poses_depth(poses, bank, [fix["det_obj"][0]], [fix["solve"][0]], [fix["frames"][0]], torch.from_numpy(fix["depth"]).to(dev),
                                         [fix["image_index"][0]], [fix["tau"][0]], max_points=fix["max_points"], grid=fix["grid"])
    res = {k: v.reshape(2, *v.shape[2:]).cpu().numpy() for k, v in verify.items()}
    assert np.array_equal(res["counts"], ref["counts"][[2, 0]])
    coarse = pnp_util.select_best_coarse(poses)
    best = pnp_util.select_best_verified(poses, verify)
    assert coarse["corresp_id"].tolist() == [0] and coarse["quality"].tolist() == [80.0]
    assert best["found"].tolist() == [True] and best["corresp_id"].tolist() == [1] and best["quality"].tolist() == [35.0]
    assert best["verify_score"].cpu().numpy()[0] == ref["score"][0] > ref["score"][2]
    assert torch.equal(best["R"][0], poses["R"][0, 1]) and torch.equal(best["t"][0], poses["t"][0, 1])
