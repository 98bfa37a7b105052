"""pnp_type "kabsch_depth" through both drivers on the planted split of tests/test_gpu_depth_refine.py's driver test (the split of
tests/test_gpu_infer_batched.py with splatted depth): infer and infer_batched write the same estimated-poses.json, every instance is
found, and MSSD against the planted poses is printed beside "opencv"'s.  The split's correspondences are exact, so the pair of numbers
shows that the stage is wired, not that it is more accurate."""

import numpy as np
import pytest

from tests.test_gpu_depth_refine import _drive, driver_split  # noqa: F401  (the module-scoped fixture and the driver runner)

pytestmark = pytest.mark.gpu


def _mssd(split, est):
    by_frame = {3: 0, 4: 1, 5: 2}
    errs = []
    for lid in (1, 2):
        V = split.repres[lid].vertices.cpu().numpy().astype(np.float64)
        for e in est[lid]:
            gt = split.annos[(by_frame[int(e["img_id"])], lid)][int(e["inst_id"])].pose
            a = V @ np.array(e["R"]).T + np.array(e["t"]).reshape(1, 3)
            b = V @ gt.R.T + gt.t.reshape(1, 3)
            errs.append(float(np.linalg.norm(a - b, axis=1).max()))
    return errs


def test_both_drivers_write_the_same_poses(tmp_path, driver_split):
    ex, split, opts, depths = driver_split
    kopts = opts._replace(pnp_type="kabsch_depth")
    per_object, full = _drive(tmp_path, "k", ex, split, kopts, depths)
    assert [len(per_object[lid]) for lid in (1, 2)] == [4, 2]          # every instance of the split is found
    for batch in (1, 4):
        batched, _ = _drive(tmp_path, f"k_b{batch}", ex, split, kopts, depths, batch=batch)
        assert batched == per_object, batch
    assert all(e["time"]["pose_coarse"] > 0 for es in full.values() for e in es)
    opencv, _ = _drive(tmp_path, "o", ex, split, opts, depths)
    ek, eo = _mssd(split, per_object), _mssd(split, opencv)
    print(f"MSSD against the planted poses over {len(ek)} detections: kabsch_depth mean {np.mean(ek):.4f} mm {np.round(ek, 3).tolist()}, "
          f"opencv mean {np.mean(eo):.4f} mm {np.round(eo, 3).tolist()}")
    with pytest.raises(ValueError, match="scene 1 image 3: pnp_type 'kabsch_depth'"):
        _drive(tmp_path, "nodepth", ex, split, kopts, None)
    with pytest.raises(ValueError, match="scene 1 image 3: pnp_type 'kabsch_depth'"):
        _drive(tmp_path, "nodepth_b", ex, split, kopts, None, batch=4)


def test_composes_with_a_depth_refining_final_pose(tmp_path, driver_split):
    ex, split, opts, depths = driver_split
    kopts = opts._replace(pnp_type="kabsch_depth", final_pose_type="depth", depth_refine_iters=10, depth_pnp_inlier_thresh=8.0)
    per_object, full = _drive(tmp_path, "kd", ex, split, kopts, depths)
    assert [len(per_object[lid]) for lid in (1, 2)] == [4, 2]
    for batch in (1, 4):
        batched, _ = _drive(tmp_path, f"kd_b{batch}", ex, split, kopts, depths, batch=batch)
        assert batched == per_object, batch
    assert all(e["time"]["pose_refine"] > 0 for es in full.values() for e in es)
