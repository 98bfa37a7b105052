"""GPU: foundpose_amd.eval_coco end to end on a split written into tmp_path, against tests/coco_ref.py."""

import json
import os

import numpy as np
import pytest

from tests import coco_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = tmp_path_factory.mktemp("coco")
    split_dir, targets, records = cr.write_split(root)
    refs = {(it, bt): cr.evaluate(records, split_dir, targets, it, bt) for it, bt in (("segm", "amodal"), ("bbox", "amodal"), ("bbox", "modal"))}
    return str(root), split_dir, targets, records, refs


def compare(out, ref):
    assert [int(k) for k in out["per_object"]] == ref["obj_ids"]
    for o, lid in enumerate(ref["obj_ids"]):
        po = out["per_object"][str(lid)]
        print(lid, np.abs(np.array(po["ap"]) - ref["ap"][o]).max(), po["totals"][0], ref["totals"][o][0].tolist())
        assert po["num_valid_instances"] == int(ref["n_valid"][o])
        assert np.array_equal(np.array(po["totals"]), ref["totals"][o])            # (tp, fp, ignored) per threshold
        assert np.abs(np.array(po["ap"]) - ref["ap"][o]).max() <= 1e-12
        assert np.array_equal(np.array(po["ap"]), ref["ap"][o])                     # the reference keeps the addition order: the same bits
    assert out["coco_average_precision"] == pytest.approx(ref["AP"], abs=1e-12)
    assert out["coco_average_precision_50"] == pytest.approx(ref["AP50"], abs=1e-12)
    assert out["coco_average_precision_75"] == pytest.approx(ref["AP75"], abs=1e-12)
    assert out["coco_average_recall"] == pytest.approx(ref["AR"], abs=1e-12)
    assert out["num_detections_of_other_images"] == ref["num_other"] and out["num_detections_beyond_max_dets"] == ref["num_cut"]


@pytest.mark.parametrize("iou_type,bbox_type", [("segm", "amodal"), ("bbox", "amodal"), ("bbox", "modal")])
def test_evaluate_coco_matches_the_restatement(split, iou_type, bbox_type):
    from foundpose_amd import eval_coco
    _, split_dir, targets, records, refs = split
    out = eval_coco.evaluate_coco(records, split_dir, targets, iou_type, bbox_type)
    compare(out, refs[(iou_type, bbox_type)])
    assert out["per_object"]["4"]["average_precision"] == -1.0 and out["per_object"]["4"]["num_detections"] == 1
    assert out["num_target_images"] == 3 and out["num_gt_instances"] == 11 and out["num_ignored_gt_instances"] == 2
    assert 0.0 < out["coco_average_precision"] < 1.0
    assert out["device_seconds"]["overlap"] > 0 and out["device_seconds"]["match"] > 0


def test_other_options_match_the_restatement_too(split):
    from foundpose_amd import eval_coco
    _, split_dir, targets, records, _ = split
    for kw in (dict(min_visib=0.0), dict(min_visib=0.75, max_dets=2), dict(max_dets=1)):
        compare(eval_coco.evaluate_coco(records, split_dir, targets, "segm", **kw), cr.evaluate(records, split_dir, targets, "segm", **kw))


def test_ground_truth_fed_back_scores_exactly_one(split):
    from foundpose_amd import eval_coco
    _, split_dir, targets, _, _ = split
    gt = cr.gt_records(split_dir, targets)
    out = eval_coco.evaluate_coco(gt, split_dir, targets, "segm")
    assert out["coco_average_precision"] == 1.0 and out["coco_average_recall"] == 1.0 and out["ap_per_threshold"] == [1.0] * 10
    assert eval_coco.evaluate_coco(gt, split_dir, targets, "bbox", "modal")["coco_average_precision"] == 1.0
    halved = [dict(r, score=r["score"] / 2) for r in gt]
    assert eval_coco.evaluate_coco(halved, split_dir, targets, "segm")["coco_average_precision"] == 1.0


def test_halved_scores_and_block_sizes_change_nothing(split):
    from foundpose_amd import eval_coco
    _, split_dir, targets, records, _ = split
    a = eval_coco.evaluate_coco(records, split_dir, targets, "segm", image_block=1, details=True)
    b = eval_coco.evaluate_coco(records, split_dir, targets, "segm", image_block=64, details=True)
    h = eval_coco.evaluate_coco([dict(r, score=r["score"] / 2) for r in records], split_dir, targets, "segm", details=True)
    assert len(a["tables"]["blocks"]) == 3 and len(b["tables"]["blocks"]) == 1
    for other in (b, h):
        for k in ("flag", "matched_gt", "ap", "q", "totals"):
            assert np.array_equal(a["tables"][k], other["tables"][k]), k
        assert a["coco_average_precision"] == other["coco_average_precision"] and a["per_object"] == other["per_object"]
    ov_a = np.concatenate([t["overlap"] for t in a["tables"]["blocks"]])
    assert np.array_equal(ov_a.view(np.int64), b["tables"]["blocks"][0]["overlap"].view(np.int64))


def test_command_line_writes_the_same_numbers(split):
    from foundpose_amd import eval_coco
    root, split_dir, targets, records, _ = split
    det_path, out_path = os.path.join(root, "detections.json"), os.path.join(root, "out", "scores.json")
    json.dump(records, open(det_path, "w"))
    eval_coco.main(["--detections", det_path, "--dataset-dir", split_dir, "--iou-type", "bbox", "--bbox-type", "modal", "--output", out_path])
    want = eval_coco.evaluate_coco(records, split_dir, targets, "bbox", "modal")      # (the default targets file is the split's own)
    got = json.load(open(out_path))
    for k in want:
        if k not in ("device_seconds", "host_seconds"):
            assert got[k] == want[k], k
    from foundpose_amd.infer_pose_util import load_detections_in_bop_format
    as_dict = eval_coco.evaluate_coco(load_detections_in_bop_format(det_path), split_dir, None, "bbox", "modal")
    assert as_dict["per_object"] == want["per_object"]
