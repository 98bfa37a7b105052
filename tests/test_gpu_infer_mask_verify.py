"""coarse_select_type "mask_verify" through both drivers on the planted split of tests/test_gpu_depth_refine.py's driver test, WITHOUT
depth: infer and infer_batched write the same estimated-poses.json, every instance is found, the option composes with pnp_type
"kabsch_depth" (which does read depth) and with final_pose_type "featuremetric".  The split's correspondences are exact: this shows that
the stage is wired, not that it chooses better.  That it chooses better is shown at the pnp_util level on the blob fixture of
tests/mask_verify_ref.py: select_best_coarse takes the sideways-shifted pose of the higher quality, select_best_verified the planted one."""

import numpy as np
import pytest
import torch

from tests import mask_verify_ref as mv
from tests import pose_verify_ref as pv
from tests.test_gpu_depth_refine import _drive, driver_split  # noqa: F401  (the module-scoped fixture and the driver runner)

pytestmark = pytest.mark.gpu


def _same_in_both_drivers(tmp_path, driver_split, tag, vopts, depths):
    ex, split, _, _ = driver_split
    per_object, full = _drive(tmp_path, tag, ex, split, vopts, depths)
    assert [len(per_object[lid]) for lid in (1, 2)] == [4, 2]          # every instance of the split is found
    for batch in (1, 4):
        batched, _ = _drive(tmp_path, f"{tag}_b{batch}", ex, split, vopts, depths, batch=batch)
        assert batched == per_object, batch
    assert all(e["time"]["pose_coarse"] > 0 for es in full.values() for e in es)
    return per_object, full


def test_both_drivers_write_the_same_poses_without_depth(tmp_path, driver_split, monkeypatch):
    from foundpose_amd import pnp_util
    opts = driver_split[2]
    calls = []
    real = pnp_util.verify_poses_mask

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append((tuple(a[5].shape), k, out["status"].cpu().numpy()))
        return out
    monkeypatch.setattr(pnp_util, "verify_poses_mask", spy)
    _same_in_both_drivers(tmp_path, driver_split, "m", opts._replace(coarse_select_type="mask_verify", mask_verify_grid=32, mask_verify_max_points=500), None)
    assert calls and all(k == {"max_points": 500, "grid": 32} for _, k, _ in calls)    # the options reach the verifier
    assert all(len(shape) == 3 and (status == 0).any(axis=1).all() for shape, _, status in calls)   # each detection's own mask; something scored


def test_composes_with_kabsch_depth_and_featuremetric(tmp_path, driver_split):
    opts, depths = driver_split[2], driver_split[3]
    _same_in_both_drivers(tmp_path, driver_split, "mk", opts._replace(coarse_select_type="mask_verify", pnp_type="kabsch_depth"), depths)
    _, full = _same_in_both_drivers(tmp_path, driver_split, "mf", opts._replace(coarse_select_type="mask_verify", final_pose_type="featuremetric",
                                                                               refine_iters=5), None)
    assert all(e["time"]["pose_refine"] > 0 for es in full.values() for e in es)


def test_verification_picks_the_planted_pose_where_the_inlier_count_picks_the_shifted_one():
    """One detection, two hypotheses: the pose shifted sideways by rho / 2 with the higher coarse quality, the planted pose with a lower one."""
    from foundpose_amd import pnp_util
    fix = mv.gpu_fixture()
    ref = mv.run_ref_on(fix)
    assert ref["min_margin"] > 1e-6
    bank = pv.make_bank(fix)
    dev = "cuda"
    sel = np.array([[1, 0]])
    poses = {"success": torch.from_numpy(fix["success"][sel]).to(dev), "R": torch.from_numpy(fix["R"][sel]).to(dev), "t": torch.from_numpy(fix["t"][sel]).to(dev),
             "quality": torch.tensor([[80.0, 35.0]], dtype=torch.float64, device=dev)}
    verify = pnp_util.verify_poses_mask(poses, bank, [fix["det_obj"][0]], [fix["solve"][0]], [fix["frames"][0]], torch.from_numpy(fix["masks"][:1]).to(dev),
                                        max_points=fix["max_points"], grid=fix["grid"])
    res = {k: v.reshape(2, *v.shape[2:]).cpu().numpy() for k, v in verify.items()}
    assert np.array_equal(res["counts"], ref["counts"][[1, 0]])
    coarse = pnp_util.select_best_coarse(poses)
    best = pnp_util.select_best_verified(poses, verify)
    assert coarse["corresp_id"].tolist() == [0] and coarse["quality"].tolist() == [80.0]
    assert best["found"].tolist() == [True] and best["corresp_id"].tolist() == [1] and best["quality"].tolist() == [35.0]
    assert best["verify_score"].cpu().numpy()[0] == ref["score"][0] > ref["score"][1]
    assert torch.equal(best["R"][0], poses["R"][0, 1]) and torch.equal(best["t"][0], poses["t"][0, 1])
