"""CPU: the COCO scorer's host side.  The numpy restatement (tests/coco_ref.py) against hand-worked cases, the
closed form of the matching rule against the sequential loop it came from, the wiring of the four entry points, option validation, and the
table builder on a split written into tmp_path."""

import os
import re

import numpy as np
import pytest

from tests import coco_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fp_mask_pack", "fp_group_mask_iou", "fp_group_box_iou", "fp_coco_match")


# ---------------------------------------------------------------------------------------------------------- the restatement itself
def test_hand_worked_average_precision():
    """Two instances, detections TP 0.9 / FP 0.8 / TP 0.7: the envelope is 1 up to recall 0.5 and 2/3 up to recall 1."""
    ap, totals = cr.accumulate([1, 0, 1], 2)
    assert totals == (2, 1, 0)
    assert ap == pytest.approx((51 + 50 * 2 / 3) / 101, abs=1e-15)
    assert cr.accumulate([1, 1], 2) == (1.0, (2, 0, 0))                   # perfect detections: exactly 1
    assert cr.accumulate([], 2) == (0.0, (0, 0, 0))                       # no detections
    assert cr.accumulate([0, 0], 3)[0] == 0.0
    assert cr.accumulate([1, 2, 2, 1], 2) == (1.0, (2, 0, 2))             # detections matched to ignored instances are dropped
    assert cr.accumulate([1, 0], 0) == (-1.0, (1, 1, 0))                  # an object without a non-ignored instance has no AP


def test_object_without_instances_is_left_out_of_the_mean():
    T = len(cr.IOU_THS)
    ap = np.stack([np.full(T, 0.5), np.full(T, -1.0), np.full(T, 1.0)])
    totals = np.zeros((3, T, 3), np.int64)
    totals[0, :, 0], totals[2, :, 0] = 1, 4
    s = cr.summarize(ap, totals, [2, 0, 4])
    assert s["ap"] == 0.75 and s["ap50"] == 0.75 and s["ap75"] == 0.75 and s["ar"] == 0.75
    from foundpose_amd import eval_coco
    mine = eval_coco.summarize(ap, totals, [2, 0, 4], cr.IOU_THS)
    assert (mine["ap"], mine["ap50"], mine["ap75"], mine["ar"]) == (0.75, 0.75, 0.75, 0.75)
    assert eval_coco.summarize(ap[1:2], totals[1:2], [0], cr.IOU_THS)["ap"] == 0.0


def test_overlaps_by_hand():
    a = np.zeros((4, 70), bool)
    b = np.zeros((4, 70), bool)
    a[1, 60:70], b[1, 65:70] = True, True
    assert cr.mask_iou(a, b) == (5, 10, 0.5, 0)
    assert cr.mask_iou(a, a)[2:] == (1.0, 0) and cr.mask_iou(a & ~a, b & ~b) == (0, 0, 0.0, 2)
    w = cr.pack_bits(a)
    assert w.shape == (4, 2) and int(w[1, 0]) == 0xF << 60 and int(w[1, 1]) == 0x3F and int(w.sum()) == int(w[1].sum())
    assert cr.box_iou([0, 0, 2, 2], [1, 1, 2, 2]) == (1.0 / 7.0, 0)
    assert cr.box_iou([0, 0, 2, 2], [2, 0, 2, 2]) == (0.0, 0)             # touching boxes
    assert cr.box_iou([0, 0, 0, 2], [0, 0, 0, 2]) == (0.0, 2)             # no area at all
    assert cr.box_iou([0, 0, float("nan"), 2], [0, 0, 1, 2])[1] == 2


def test_matching_rule_by_hand():
    t = [0.5]
    f, m = cr.match([[0.5, np.nextafter(0.5, 0)]], [False, False], t)     # exactly at the threshold matches, the next double below does not
    assert (f[0, 0], m[0, 0]) == (1, 0)
    f, m = cr.match([[np.nextafter(0.5, 0)]], [False], t)
    assert (f[0, 0], m[0, 0]) == (0, -1)
    f, m = cr.match([[0.7, 0.7]], [False, False], t)                      # equal overlaps go to the higher index
    assert m[0, 0] == 1
    f, m = cr.match([[0.6, 0.9]], [False, True], t)                       # a regular instance is preferred to an ignored one
    assert (f[0, 0], m[0, 0]) == (1, 0)
    f, m = cr.match([[0.2, 0.9], [0.2, 0.9]], [False, True], t)           # the ignored one is used up
    assert f[:, 0].tolist() == [2, 0] and m[:, 0].tolist() == [1, -1]
    f, m = cr.match([[1.0]], [False], [1.0])                              # threshold 1 matches an overlap of exactly 1
    assert f[0, 0] == 1
    assert cr.match(np.zeros((2, 0)), [], t)[0].tolist() == [[0], [0]]


def test_closed_form_equals_the_sequential_loop():
    """A few thousand small tables with overlaps from a handful of rationals, so that ties and exact threshold hits are common."""
    rng = np.random.default_rng(24)
    values = np.array([0.0, 0.25, 0.5, np.nextafter(0.5, 0), 0.55, 0.6, 2.0 / 3.0, 0.75, 0.95, 1.0])
    for _ in range(3000):
        E, G = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        ov = values[rng.integers(0, len(values), (E, G))]
        ign = sorted(bool(v) for v in rng.integers(0, 2, G))               # the non-ignored first
        a, b = cr.match(ov, ign), cr.match_closed(ov, ign)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (ov, ign)


# ---------------------------------------------------------------------------------------------------------- wiring
def test_entry_points_are_declared_bound_and_built():
    from foundpose_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    assert "coco_eval.hip" in build.SOURCES
    assert re.search(r"#define FP_ABI_VERSION 20\b", header) and _lib.ABI_VERSION == 20
    for name in NEW:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl, f"{name} is not declared"
        assert len(decl.group(1).split(",")) == len(_lib._PROTOS[name]), f"{name}: the prototype and the header disagree on the argument count"
    assert header.count("without a change of FP_ABI_VERSION") + header.count("without a change of\n * FP_ABI_VERSION") >= 4
    src = open(os.path.join(ROOT, "foundpose_amd", "csrc", "api.cpp")).read()
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", src)


def test_options_are_validated_before_anything_else(tmp_path):
    from foundpose_amd import eval_coco
    for bad in (dict(iou_type="keypoints"), dict(bbox_type="tight"), dict(min_visib=-0.1), dict(min_visib=float("nan")), dict(max_dets=0),
                dict(max_dets=257), dict(image_block=0)):
        with pytest.raises(ValueError):
            eval_coco.evaluate_coco([], str(tmp_path), [], **bad)
    for bad in ([], np.linspace(0.05, 0.9, 17), [0.0, 0.5], [0.5, 1.5], [float("nan")]):
        with pytest.raises(ValueError):
            eval_coco.check_thresholds(bad)
    assert eval_coco.check_thresholds([1.0]).tolist() == [1.0]
    assert np.array_equal(eval_coco.IOU_THS, cr.IOU_THS)


def test_cpu_tensors_are_refused():
    import torch
    from foundpose_amd import eval_coco, ops
    i32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mask_pack(torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.group_mask_iou(torch.zeros(1, 4, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.int64), i32, i32, i32, 0)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.group_box_iou(torch.zeros(1, 4, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64), i32, i32, i32, 0)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.coco_match(i32, i32, i32, torch.zeros(0, dtype=torch.float64), i32, torch.tensor([0.5], dtype=torch.float64), 0)
    with pytest.raises(ValueError, match="no CPU path"):
        eval_coco.match_groups(torch.zeros(1, dtype=torch.float64), [0, 1], [0, 1], [0, 1], [0])


def test_a_canvas_that_is_not_the_image_is_refused(tmp_path):
    from foundpose_amd import eval_coco
    split, targets, records = cr.write_split(tmp_path)
    bad = [dict(r) for r in records]
    bad[0]["segmentation"] = cr.rle_encode(np.zeros((52, 70), bool))
    with pytest.raises(ValueError, match="canvas"):
        eval_coco.evaluate_coco(bad, split, targets)


# ---------------------------------------------------------------------------------------------------------- the table builder
def _tables(tmp_path, **kw):
    import json
    from foundpose_amd import eval_coco
    split, targets, records = cr.write_split(tmp_path)
    images = eval_coco.target_images(targets)
    gts = {s: json.load(open(os.path.join(split, f"{s:06d}", "scene_gt.json"))) for s in (1, 2)}
    infos = {s: json.load(open(os.path.join(split, f"{s:06d}", "scene_gt_info.json"))) for s in (1, 2)}
    recs = eval_coco.detection_records(records)
    return recs, images, eval_coco.build_tables(recs, images, infos, gts, **kw)


def test_table_builder_on_a_written_split(tmp_path):
    recs, images, tb = _tables(tmp_path, unseen={(2, 0, 2)})
    assert images == [(1, 0), (1, 1), (2, 0)]                              # the duplicate target row counts once
    assert tb["groups"] == sorted(tb["groups"]) and all(g[:2] in images for g in tb["groups"])
    assert (1, 0, 4) in tb["groups"] and tb["num_other"] == 3              # an object without GT keeps its group; the frame (2, 5) is dropped
    E, G = np.diff(tb["est_off"]), np.diff(tb["gt_off"])
    assert np.array_equal(np.diff(tb["pair_off"]), E * G) and int(E.sum()) == len(tb["est_rows"]) == len(recs) - 3
    for gi, key in enumerate(tb["groups"]):
        rows = tb["est_rows"][tb["est_off"][gi]:tb["est_off"][gi + 1]]
        assert all((recs[int(i)]["scene_id"], recs[int(i)]["image_id"], recs[int(i)]["category_id"]) == key for i in rows)
        scores = [recs[int(i)]["score"] for i in rows]
        assert scores == sorted(scores, reverse=True)
        ign = tb["gt_ignore"][tb["gt_off"][gi]:tb["gt_off"][gi + 1]].tolist()
        assert ign == sorted(ign)                                          # the ignored instances last
        assert all(k[:2] == key[:2] for k in tb["gt_ids"][tb["gt_off"][gi]:tb["gt_off"][gi + 1]])
    g = tb["groups"].index((1, 0, 3))
    assert tb["gt_ignore"][tb["gt_off"][g]:tb["gt_off"][g + 1]].tolist() == [1]      # visib_fract 0.05
    assert tb["n_valid"] == {1: 4, 2: 3, 3: 2} and tb["n_ignored"] == {3: 1, 2: 1}
    g = tb["groups"].index((1, 1, 2))                                     # two instances, both counted, scene_gt order kept
    assert [k[2] for k in tb["gt_ids"][tb["gt_off"][g]:tb["gt_off"][g + 1]]] == [1, 2]
    assert tb["gt_boxes"].shape == (len(tb["gt_ids"]), 4) and tb["num_cut"] == 0


def test_table_builder_cuts_to_max_dets_and_moves_ignored_instances_last(tmp_path):
    recs, images, full = _tables(tmp_path)
    _, _, tb = _tables(tmp_path, max_dets=2, min_visib=0.75, bbox_type="modal")
    E = np.diff(tb["est_off"])
    assert int(E.max()) == 2 and tb["num_cut"] == len(full["est_rows"]) - len(tb["est_rows"]) > 0
    g = tb["groups"].index((1, 0, 1))                                     # kept: the two best of the group, in rank order
    rows, all_rows = tb["est_rows"][tb["est_off"][g]:tb["est_off"][g + 1]], full["est_rows"][full["est_off"][g]:full["est_off"][g + 1]]
    assert rows.tolist() == all_rows[:2].tolist()
    g = tb["groups"].index((1, 1, 2))                                     # visib_fract 1.0 and 0.3: the second is ignored now
    assert tb["gt_ignore"][tb["gt_off"][g]:tb["gt_off"][g + 1]].tolist() == [0, 1]
    g = tb["groups"].index((1, 1, 1))                                     # visib_fract 0.7 < 0.75
    assert tb["gt_ignore"][tb["gt_off"][g]:tb["gt_off"][g + 1]].tolist() == [1]
    _, _, zero = _tables(tmp_path, min_visib=0.0)
    assert zero["n_ignored"] == {2: 1}                                    # only the -1 box is left ignored
    with pytest.raises(ValueError, match="NaN"):
        from foundpose_amd import eval_coco
        eval_coco.build_tables([dict(recs[0], score=float("nan"))], images, {}, {})


def test_global_rank_order_is_stable_in_table_order(tmp_path):
    from foundpose_amd import eval_coco
    recs, images, tb = _tables(tmp_path)
    obj_ids, obj_off, order = eval_coco.rank_objects(recs, tb["est_rows"], {1, 2, 3})
    assert obj_ids == [1, 2, 3, 4] and obj_off[-1] == len(tb["est_rows"])
    for o, lid in enumerate(obj_ids):
        pos = order[obj_off[o]:obj_off[o + 1]]
        assert all(recs[int(tb["est_rows"][p])]["category_id"] == lid for p in pos)
        keys = [(-recs[int(tb["est_rows"][p])]["score"], int(p)) for p in pos]
        assert keys == sorted(keys)
