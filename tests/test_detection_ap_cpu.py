"""CPU: the numpy restatement of the BOP 6D detection score (tests/detection_ap_ref.py) against cases derived by hand, the host tables of
eval_bop24, and the driver options of the detection task.  The device is compared with the restatement in tests/test_gpu_detection_ap.py."""

import numpy as np
import pytest

from tests import detection_ap_ref as ref

NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------------------------------------------- average precision
def test_tp_fp_tp_with_two_valid_instances():
    """p = (1, 1/2, 2/3) so the envelope is (1, 2/3, 2/3); r = (.5, .5, 1).  Thresholds <= 0.5 read 1, the ones above read 2/3; which
    side linspace's rounded 0.5 falls on is taken from its actual fp64 value."""
    ap, q, totals = ref.average_precision([1, 0, 1], 2)
    two_thirds = np.float64(2) / np.float64(3)
    low = ref.REC_THR <= np.float64(1) / np.float64(2)
    assert 50 <= int(low.sum()) <= 51 and totals == (2, 1, 0)
    assert np.array_equal(q, np.where(low, 1.0, two_thirds))
    s = q[0]
    for v in q[1:]:
        s = s + v
    assert ap == s / 101.0 and abs(ap - (low.sum() + (101 - low.sum()) * 2 / 3) / 101) < 1e-12


def test_all_true_all_false_ignored_and_no_valid_instance():
    assert ref.average_precision([1, 1, 1, 1], 4)[0] == 1.0
    ap, q, totals = ref.average_precision([0, 0, 0], 4)
    assert ap == 0.0 and not q.any() and totals == (0, 3, 0)
    # an ignored estimate changes neither count, wherever it stands
    want = ref.average_precision([1, 0, 1], 2)
    for flags in ([2, 1, 0, 1], [1, 2, 0, 1], [1, 0, 1, 2], [2, 1, 2, 0, 2, 1, 2]):
        got = ref.average_precision(flags, 2)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2][:2] == want[2][:2] and got[2][2] == flags.count(2)
    ap, q, totals = ref.average_precision([1, 0, 2], 0)
    assert ap == -1.0 and not q.any() and totals == (1, 1, 1)
    # no estimate at all, but instances to find: 0, not -1
    assert ref.average_precision([], 3)[0] == 0.0
    # only ignored estimates: nothing is kept, so no threshold is reached
    assert ref.average_precision([2, 2], 3)[0] == 0.0
    # a false positive FIRST: recall threshold 0 reads the envelope of the first kept entry, the maximum over all (1/2 here)
    ap, q, _ = ref.average_precision([0, 1], 1)
    assert np.array_equal(q, np.full(101, 0.5)) and ap == 0.5
    # half the instances found: the thresholds above 1/2 are never reached
    ap, q, _ = ref.average_precision([1], 2)
    assert np.array_equal(q, np.where(ref.REC_THR <= 0.5, 1.0, 0.0))


# ---------------------------------------------------------------------------------------------------- matching
def test_matching_rule():
    valid = [True, True, True]
    # the lowest error below the threshold; ties to the lower GT index; a used GT is gone
    f, m = ref.match_group([[3.0, 1.0, 1.0], [0.5, 0.1, 2.0], [9.0, 9.0, 9.0]], 5.0, valid)
    assert m.tolist() == [1, 0, -1] and f.tolist() == [1, 1, 0]
    # strictly below: an error equal to the threshold does not match
    f, m = ref.match_group([[5.0, 7.0]], 5.0, valid[:2])
    assert m.tolist() == [-1] and f.tolist() == [0]
    f, m = ref.match_group([[np.nextafter(5.0, 0.0), 7.0]], 5.0, valid[:2])
    assert m.tolist() == [0]
    # a NaN never matches, +inf neither
    f, m = ref.match_group([[NAN, 4.0], [NAN, INF]], 5.0, valid[:2])
    assert m.tolist() == [1, -1] and f.tolist() == [1, 0]
    # an invalid GT that is the best match is taken: the estimate is ignored and the GT is used up for the next estimate
    f, m = ref.match_group([[1.0, 2.0], [1.5, 9.0]], 5.0, [False, True])
    assert m.tolist() == [0, -1] and f.tolist() == [2, 0]
    # no GT at all
    f, m = ref.match_group(np.zeros((2, 0)), 5.0, [])
    assert m.tolist() == [-1, -1] and f.tolist() == [0, 0]


def test_match_batch_lays_columns_out_by_type_then_threshold():
    err = np.array([[1.0, 30.0], [4.0, 10.0]])            # one group, E = 1, G = 2: (mssd, mspd) per GT
    ths = np.array([[[2.0, 5.0], [20.0, 40.0]]])          # T = 2
    flag, matched = ref.match_batch([0, 1], [0, 2], [0, 2], err, [1, 0], [0], ths)
    assert matched.tolist() == [[0, 0, 1, 1]] and flag.tolist() == [[1, 1, 2, 2]]


# ---------------------------------------------------------------------------------------------------- eval_bop24's host side
def test_tables_rank_groups_and_objects():
    from foundpose_amd import eval_bop24
    rows = [dict(scene_id=1, im_id=0, obj_id=2, score=0.5), dict(scene_id=1, im_id=0, obj_id=2, score=0.9),
            dict(scene_id=1, im_id=1, obj_id=2, score=0.9), dict(scene_id=1, im_id=7, obj_id=2, score=1.0),    # image 7 is no target
            dict(scene_id=1, im_id=0, obj_id=1, score=0.1), dict(scene_id=1, im_id=1, obj_id=2, score=0.9)]
    eye = dict(cam_R_m2c=np.eye(3).ravel().tolist(), cam_t_m2c=[0, 0, 500.0])
    gts = {1: {"0": [dict(eye, obj_id=2), dict(eye, obj_id=2), dict(eye, obj_id=3)], "1": [dict(eye, obj_id=2)], "7": [dict(eye, obj_id=2)]}}
    infos = {1: {"0": [{"visib_fract": 0.5}, {"visib_fract": 0.05}, {"visib_fract": 1.0}], "1": [{"visib_fract": 0.1}], "7": [{"visib_fract": 1.0}]}}
    tb = eval_bop24.build_tables(rows, [(1, 0), (1, 1)], gts, infos, {1: 100.0, 2: 200.0, 3: 50.0}, {(1, 0): 640, (1, 1): 320})
    assert tb["obj_ids"] == [1, 2, 3] and tb["n_valid"].tolist() == [0, 2, 1]       # 0.1 is valid (>=), 0.05 is not; image 7 does not count
    assert tb["groups"] == [(1, 0, 1), (1, 0, 2), (1, 1, 2)]
    assert tb["est_rows"].tolist() == [4, 1, 0, 2, 5]                               # rank order inside a group, equal scores in csv order
    assert tb["est_off"].tolist() == [0, 1, 3, 5] and tb["gt_off"].tolist() == [0, 0, 2, 3] and tb["pair_off"].tolist() == [0, 0, 4, 6]
    assert tb["gt_valid"].tolist() == [1, 0, 1] and tb["group_tab"].tolist() == [0, 1, 2]
    assert np.array_equal(tb["ths"][1], np.stack([eval_bop24.MSSD_THS * 200.0, eval_bop24.MSPD_THS * 1.0]))
    assert np.array_equal(tb["ths"][2][1], eval_bop24.MSPD_THS * 0.5)
    # global rank order per object: score descending, equal scores in csv order (rows 1, 2, 5 share 0.9 -> positions 1, 3, 4)
    assert tb["obj_off"].tolist() == [0, 1, 5, 5] and tb["order"].tolist() == [0, 1, 3, 4, 2]
    assert eval_bop24.target_images([dict(scene_id=1, im_id=3, obj_id=5, inst_count=2), dict(scene_id=1, im_id=3, obj_id=6, inst_count=1),
                                     dict(scene_id=1, im_id=2)]) == [(1, 2), (1, 3)]
    s = eval_bop24.summarize(np.array([[-1.0, -1.0], [0.5, 1.0], [1.0, 0.0]]), [0, 2, 1], 1)
    assert s["ap_mssd"] == 0.75 and s["ap_mspd"] == 0.5 and s["ap"] == 0.625


# ---------------------------------------------------------------------------------------------------- the drivers' options
BASE = dict(version="v", repre_version="r", object_dataset="lmo")


def test_an_unknown_task_is_refused():
    """(On the code before the detection task this fails with TypeError: InferOpts has no such field.)"""
    from foundpose_amd import infer
    with pytest.raises(ValueError, match="task"):
        infer._check_driver_opts(infer.InferOpts(**BASE, task="segmentation"))


def test_detection_options_are_checked_before_any_device_work():
    from foundpose_amd import infer
    for bad in (dict(detection_min_score=True), dict(detection_min_score="0.5"), dict(detection_min_score=NAN), dict(detection_max_per_object=0),
                dict(detection_max_per_object=True), dict(detection_max_per_object=2.0), dict(task="detection", num_preds_factor=2),
                dict(task="detection", use_detections=False)):
        with pytest.raises(ValueError):
            infer._check_driver_opts(infer.InferOpts(**BASE, **bad))
        with pytest.raises(ValueError):
            infer.infer_object(infer.InferOpts(**BASE, **bad), 1, None, [], {})
    o = infer.load_opts({"infer_opts": dict(BASE, task="detection", detection_min_score=0.25, detection_max_per_object=3)})
    infer._check_driver_opts(o)
    assert infer.InferOpts(**BASE).task == "localization" and infer.InferOpts(**BASE).detection_max_per_object == 16
    preds = [dict(score=0.3, n=0), dict(score=0.9, n=1), dict(score=0.2, n=2), dict(score=0.9, n=3), dict(score=0.25, n=4), dict(score=0.5, n=5)]
    assert [p["n"] for p in infer.detection_predictions(o, preds)] == [1, 3, 5]          # best first, equal scores in file order, 3 at most
    assert [p["n"] for p in infer.detection_predictions(o._replace(detection_max_per_object=16), preds)] == [1, 3, 5, 0, 4]   # 0.25 stays (>=)
    assert infer.detection_predictions(o, None) == [] and infer.detection_predictions(o._replace(detection_min_score=0.95), preds[:1]) == []
    # the targets name images only: a set of images, or a localization table whose counts and objects are not read
    want = {1: {(1, 3): 0, (1, 4): 0}, 2: {(1, 3): 0, (1, 4): 0}}
    assert infer.detection_targets([(1, 3), (1, 4)], [1, 2]) == want
    assert infer.detection_targets({1: {(1, 3): 2}, 7: {(1, 4): 1, (1, 3): 1}}, [1, 2]) == want
    assert infer.detection_targets(None, [1]) is None
