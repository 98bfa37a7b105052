"""final_pose_type "mask" and "featuremetric_mask"  through both drivers on the planted split of
tests/test_gpu_infer_mask_verify.py, WITHOUT depth: infer and infer_batched write the same estimated-poses.json at batch sizes 1 and 4,
with the masks made on the host and on the device, and the time goes to pose_refine.  The split's poses are exact and its masks are
boxes: this shows that the stage is wired, not that it refines better (tests/test_gpu_mask_refine.py shows that on the blob)."""

import pytest

from foundpose_amd import infer, refine_util
from tests.test_gpu_depth_refine import _drive, driver_split  # noqa: F401  (the module-scoped fixture and the driver runner)
from tests.test_gpu_infer_batched import TARGETS, _csv, _entries

pytestmark = pytest.mark.gpu


def _drive_device_masks(tmp, tag, ex, split, opts, batch):
    d = str(tmp / tag)
    infer.infer_batched(opts, iter([split.frame(f, None) for f in range(3)]), split.dets, split.repres, d, batch_detections=batch, extractor=ex,
                        num_target_insts={lid: TARGETS[lid] for lid in (1, 2)}, device_masks=True)
    return {lid: _entries(d, lid) for lid in (1, 2)}, d


@pytest.mark.parametrize("pose_type", infer.MASK_POSE_TYPES)
def test_both_drivers_write_the_same_poses_without_depth(tmp_path, driver_split, monkeypatch, pose_type):
    ex, split, opts, _ = driver_split
    calls = []
    real = refine_util.refine_mask

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append((tuple(a[0].shape), a[11], a[12], k, out["status"].cpu().numpy(), out["cost_in"].cpu().numpy(), out["cost_out"].cpu().numpy()))
        return out
    monkeypatch.setattr(refine_util, "refine_mask", spy)
    mopts = opts._replace(final_pose_type=pose_type, mask_refine_iters=7, mask_refine_huber_px=5.0, mask_refine_max_points=300, mask_refine_max_contour=64,
                          refine_iters=5)
    per_object, full = _drive(tmp_path, "po", ex, split, mopts, None)
    assert [len(per_object[lid]) for lid in (1, 2)] == [4, 2]          # every instance of the split is found
    assert all(e["time"]["pose_refine"] > 0 for es in full.values() for e in es)
    assert calls and all(len(shape) == 3 and delta == 5.0 and iters == 7 and k["max_contour"] == 64 and k["max_points"] <= 300
                         for shape, delta, iters, k, *_ in calls)      # each detection's own frame-sized mask; the options reach the refiner
    assert all((cout <= cin).all() for *_, cin, cout in calls) and any((st != 2).any() for _, _, _, _, st, _, _ in calls)
    for batch in (1, 4):
        batched, full_b = _drive(tmp_path, f"b{batch}", ex, split, mopts, None, batch=batch)
        assert batched == per_object, batch
        assert all(e["time"]["pose_refine"] > 0 for es in full_b.values() for e in es)
        on_device, d = _drive_device_masks(tmp_path, f"dm{batch}", ex, split, mopts, batch)
        assert on_device == per_object, batch
        assert _csv(d) == _csv(str(tmp_path / f"b{batch}"))


def test_the_default_pose_type_never_reaches_the_mask_stage(tmp_path, driver_split, monkeypatch):
    ex, split, opts, _ = driver_split
    assert opts.final_pose_type == "best_coarse"

    def never(*a, **k):
        raise AssertionError("the mask stage ran")
    monkeypatch.setattr(refine_util, "refine_best_coarse_mask", never)
    monkeypatch.setattr(refine_util, "mask_contours", never)
    coarse, full = _drive(tmp_path, "coarse", ex, split, opts, None)
    batched, _ = _drive(tmp_path, "coarse_b4", ex, split, opts, None, batch=4)
    assert coarse == batched and [len(coarse[lid]) for lid in (1, 2)] == [4, 2]
    assert all("pose_refine" not in e["time"] for es in full.values() for e in es)
    # the file the default writes holds the coarse pose: a mask pose type writes another R / t for at least one instance or the same (exact poses), never other keys
    keys = {k for es in coarse.values() for e in es for k in e}
    mopts = opts._replace(final_pose_type="mask", mask_refine_iters=3)
    monkeypatch.undo()
    refined, _ = _drive(tmp_path, "mask", ex, split, mopts, None)
    assert {k for es in refined.values() for e in es for k in e} == keys
