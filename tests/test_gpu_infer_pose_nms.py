"""frame_select_type "pose_nms" through both drivers on the planted split of tests/test_gpu_infer_mask_verify.py (the module-scoped split of
tests/test_gpu_depth_refine.py), with one detection listed twice and num_preds_factor = 2, so that one instance gets two poses.  With
"none" the csv holds both and is the csv of a run without the new options; with "pose_nms" exactly the lower-ranked of the two is missing
and pose-nms.json names its suppressor -- in infer and in infer_batched at batch sizes 1 and 4.  The split's correspondences are exact and
its "models" are the bank's vertices: this shows that the stage is WIRED, not that its threshold is right.  What the kernels compute is
checked in tests/test_gpu_pose_nms.py."""

import json
import os
import types

import pytest

from foundpose_amd import eval_bop19
from tests.test_gpu_depth_refine import _drive, driver_split  # noqa: F401  (the module-scoped fixture and the driver runner)
from tests.test_gpu_infer_batched import _csv

pytestmark = pytest.mark.gpu

DUP = (1, 4, 2)   # (scene, image, object): frame 1's only instance of object 2
CSV = "coarse_synth-estimated-poses.csv"


def _doubled(split):
    """The split with the detection of DUP listed twice (nothing of the shared split is modified)."""
    dets = {k: list(v) for k, v in split.dets.items()}
    assert len(dets[DUP]) == 1
    dets[DUP] = dets[DUP] + [dict(dets[DUP][0])]
    return types.SimpleNamespace(frame=split.frame, dets=dets, repres=split.repres)


def _run(tmp_path, tag, ex, split, opts, batch=0):
    _drive(tmp_path, tag, ex, split, opts, None, batch=batch)
    d = str(tmp_path / tag)
    nms = os.path.join(d, "pose-nms.json")
    return _csv(d), eval_bop19.load_results_csv(os.path.join(d, CSV)), json.load(open(nms)) if os.path.exists(nms) else None


def test_the_lower_ranked_duplicate_is_removed_in_both_drivers(tmp_path, driver_split):
    ex, split, opts, _ = driver_split
    split = _doubled(split)
    opts = opts._replace(num_preds_factor=2)
    plain, plain_rows, none_json = _run(tmp_path, "plain", ex, split, opts)
    # "none" is the default: a run that names it (and sets the stage's other options) writes what a run without the options writes
    named, _, named_json = _run(tmp_path, "none", ex, split, opts._replace(frame_select_type="none", pose_nms_thresh=0.9, pose_nms_grid=8, pose_nms_max_points=50,
                                                                           pose_nms_cross_object=True))
    assert named == plain and none_json is None and named_json is None
    assert not os.path.exists(str(tmp_path / "none" / "pose-nms.json"))
    twins = [i for i, r in enumerate(plain_rows) if (r["scene_id"], r["im_id"], r["obj_id"]) == DUP]
    assert len(plain_rows) == 7 and len(twins) == 2                      # 4 + 2 instances and the duplicate
    first, second = sorted(twins, key=lambda i: plain_rows[i]["score"], reverse=True)   # stable: equal scores keep the input order
    want = [line for i, line in enumerate(plain[1:]) if i != second]
    nopts = opts._replace(frame_select_type="pose_nms")
    for tag, batch in (("nms", 0), ("nms_b1", 1), ("nms_b4", 4)):
        lines, rows, decisions = _run(tmp_path, tag, ex, split, nopts, batch=batch)
        assert lines[0] == plain[0] and lines[1:] == want, tag          # the kept rows, unchanged but for their time, in their order
        assert [d["row"] for d in decisions] == list(range(7)) and [d["keep"] for d in decisions] == [i != second for i in range(7)], tag
        gone = decisions[second]
        print(tag, "the duplicate's decision:", gone)
        assert gone["suppressed_by"] == first and gone["overlap"] >= nopts.pose_nms_thresh, tag
        assert (gone["scene_id"], gone["im_id"], gone["obj_id"]) == DUP
        assert all(d["suppressed_by"] == -1 and d["overlap"] is None for i, d in enumerate(decisions) if i != second), tag
        # the per-object files are what they were: both poses are in estimated-poses.json
        est = json.load(open(str(tmp_path / tag / "2" / "estimated-poses.json")))
        assert len(est) == 3, tag
        # the stage's time went to the rows: every image's rows still carry one time, larger than without the stage's share
        assert eval_bop19.average_time_per_image(rows) > 0, tag
