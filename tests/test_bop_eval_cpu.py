"""CPU: the BOP19 protocol of foundpose_amd.eval_bop19 on hand-built error tables (top-n, valid GT, greedy matching,
thresholds, recalls), the results csv and its time rule, and the numpy VSD restatement (tests/vsd_ref.py) on analytic depth
planes whose counts are worked out by hand."""
import numpy as np
import pytest

from foundpose_amd import eval_bop19 as eb
from tests import vsd_ref

TAUS = eb.VSD_TAUS


def _m(errs, ths, valid):
    e = np.asarray(errs, np.float64)
    return eb.match_count(np.broadcast_to(e, (len(ths),) + e.shape), np.asarray(ths, np.float64), np.asarray(valid, bool))


# ------------------------------------------------------------------------------------------------ matching and recall
def test_estimate_takes_the_lowest_error_gt():
    # one estimate, three GT: it takes GT 2 (lowest error), not GT 0 (first below the threshold)
    errs = [[0.4, 0.9, 0.1]]
    assert _m(errs, [0.5], [False, True, True]).tolist() == [1]
    assert _m(errs, [0.5], [True, True, False]).tolist() == [0]    # GT 2 is invalid: the estimate is used up, nothing counts
    # the second estimate takes what is left
    errs = [[0.1, 0.2], [0.1, 0.3]]
    assert _m(errs, [0.25, 0.5, 0.15], [True, True]).tolist() == [1, 2, 1]   # 0.3 is not below 0.25


def test_match_to_an_invalid_gt_counts_nowhere():
    errs = [[0.05, 0.3], [0.2, 0.3]]     # est 0 matches invalid GT 0; est 1 then cannot take GT 0 and takes GT 1
    assert _m(errs, [0.4], [False, True]).tolist() == [1]
    assert _m(errs, [0.25], [False, True]).tolist() == [0]
    assert _m(errs, [0.4], [False, False]).tolist() == [0]


def test_error_equal_to_the_threshold_is_not_correct():
    th = np.array([0.05, 0.1, 0.15000000000000002])
    assert _m([[0.1]], th, [True]).tolist() == [0, 0, 1]
    assert _m([[th[2]]], th, [True]).tolist() == [0, 0, 0]
    assert _m([[np.nan]], th, [True]).tolist() == [0, 0, 0]


def test_ties_in_error_go_to_the_lower_gt_id():
    errs = [[0.2, 0.2, 0.2], [0.2, 0.2, 0.2]]
    assert _m(errs, [0.3], [True, False, True]).tolist() == [1]    # est 0 -> GT 0, est 1 -> GT 1 (invalid)
    assert _m(errs, [0.3], [False, True, True]).tolist() == [1]


def test_top_n_is_a_stable_descending_sort_and_ignores_non_targets():
    rows = [{"scene_id": 1, "im_id": 2, "obj_id": 5, "score": s} for s in (0.5, 0.9, 0.5, 0.7, 0.5)]
    rows.append({"scene_id": 1, "im_id": 3, "obj_id": 5, "score": 1.0})    # not a target
    rows.append({"scene_id": 1, "im_id": 2, "obj_id": 6, "score": 1.0})    # not a target object
    kept = eb.top_n(rows, {(1, 2, 5): 3})
    assert kept == {(1, 2, 5): [1, 3, 0]}                   # 0.9, 0.7, then the first of the tied 0.5s
    assert eb.top_n(rows, {(1, 2, 5): 4}) == {(1, 2, 5): [1, 3, 0, 2]}
    assert eb.top_n(rows, {(1, 2, 5): 10})[(1, 2, 5)] == [1, 3, 0, 2, 4]


def test_valid_gt_are_the_most_visible():
    assert eb.valid_gt_mask([0.2, 0.9, 0.5, 0.9], 2).tolist() == [False, True, False, True]
    assert eb.valid_gt_mask([0.3, 0.3, 0.3], 2).tolist() == [True, True, False]   # ties to the lower id
    assert eb.valid_gt_mask([0.1], 3).tolist() == [True]


def test_thresholds():
    th = eb.correct_thresholds(120.0, 640)
    assert np.array_equal(th["vsd"], np.arange(0.05, 0.51, 0.05)) and len(th["vsd"]) == 10
    assert th["vsd"][2] == 0.15000000000000002 and th["vsd"][6] == 0.35000000000000003   # np.arange's own fp64 values
    assert np.array_equal(th["mssd"], np.arange(0.05, 0.51, 0.05) * 120.0)
    assert th["mspd"].tolist() == [5.0, 10.0, 15.0, 20.0, 25.0, 30.0, 35.0, 40.0, 45.0, 50.0]
    assert np.array_equal(eb.correct_thresholds(1.0, 1280)["mspd"], np.arange(5, 51, 5) * 2.0)
    assert eb.correct_thresholds(1.0, 720)["mspd"][0] == 5 * (720 / 640.0)
    assert len(eb.VSD_TAUS) == 10 and eb.VSD_TAUS[-1] == np.arange(0.05, 0.51, 0.05)[-1]


def test_vsd_errors_from_counts():
    c = np.array([[10, 8, 3, 0], [0, 0, 0, 0], [4, 4, 4, 1]])
    e = eb.vsd_errors(c)
    assert e.tolist() == [[(3 + 2) / 10.0, 2 / 10.0], [1.0, 1.0], [1.0, 0.25]]


# ------------------------------------------------------------------------------------------------ csv and time
CSV_HEAD = "scene_id,im_id,obj_id,score,R,t,time\n"
ROW = "{s},{i},{o},{sc},1 0 0 0 1 0 0 0 1,1.5 -2 800,{tm}\n"


def test_csv_parsing(tmp_path):
    p = tmp_path / "r.csv"
    p.write_text(CSV_HEAD + ROW.format(s=1, i=3, o=5, sc=0.25, tm=1.5) + ROW.format(s=1, i=3, o=6, sc=0.75, tm=1.5)
                 + ROW.format(s=2, i=4, o=5, sc=1, tm=0.5) + "\n")
    rows = eb.load_results_csv(str(p))
    assert [(r["scene_id"], r["im_id"], r["obj_id"], r["score"]) for r in rows] == [(1, 3, 5, 0.25), (1, 3, 6, 0.75), (2, 4, 5, 1.0)]
    assert np.array_equal(rows[0]["R"], np.eye(3)) and rows[0]["t"].tolist() == [1.5, -2.0, 800.0]
    assert eb.average_time_per_image(rows) == 1.0
    bad = tmp_path / "bad.csv"
    bad.write_text("scene_id,im_id,obj_id,score,R,t\n")
    with pytest.raises(ValueError):
        eb.load_results_csv(str(bad))


def test_csv_written_by_prepare_bop_submission_parses(tmp_path):
    import json
    from foundpose_amd import eval_util
    d = tmp_path / "out"
    (d / "5").mkdir(parents=True)
    e = {"scene_id": "1", "img_id": "3", "obj_id": "5", "inst_id": "0", "hypothesis_id": "0", "score": "0.5",
         "R": np.eye(3).tolist(), "t": [[1.0], [2.0], [700.0]], "time": {"a": 0.25}, "cnos_time": 0.5}
    (d / "5" / "estimated-poses.json").write_text(json.dumps([e]))
    rows = eb.load_results_csv(eval_util.prepare_bop_submission(str(d), "lmo", [5]))
    assert len(rows) == 1 and rows[0]["t"].tolist() == [1.0, 2.0, 700.0] and rows[0]["time"] == 0.75


def test_time_mismatch_raises_and_negative_time_reports_minus_one(tmp_path):
    p = tmp_path / "r.csv"
    p.write_text(CSV_HEAD + ROW.format(s=1, i=3, o=5, sc=0.2, tm=1.5) + ROW.format(s=1, i=3, o=6, sc=0.2, tm=1.7))
    with pytest.raises(ValueError, match="not the same"):
        eb.average_time_per_image(eb.load_results_csv(str(p)))
    p.write_text(CSV_HEAD + ROW.format(s=1, i=3, o=5, sc=0.2, tm=-1) + ROW.format(s=1, i=4, o=6, sc=0.2, tm=1.7))
    assert eb.average_time_per_image(eb.load_results_csv(str(p))) == -1.0


# ------------------------------------------------------------------------------------------------ the VSD restatement
# One image row, 4 pixels, cx = cy = 0 and f = 1000: pixel k lies at xs = k / 1000 (dist = d sqrt(1 + xs^2), within 8e-6 of d).
K = np.array([[1000.0, 0, 0], [0, 1000.0, 0], [0, 0, 1]])
DIAM = 100.0


def _row(*v):
    return np.array([v], np.float32)


def test_vsd_ref_occlusion_within_and_beyond_delta():
    gt = _row(500, 500, 500, 500)
    test = _row(500, 490, 480, 0)       # visible, occluded by 10 mm (within delta), by 20 mm (beyond), no measurement
    c = vsd_ref.vsd_counts(test, gt, gt, K, 15.0, DIAM, TAUS)
    assert c.tolist() == [3, 3] + [0] * 10                # pixel 2 is in neither mask
    assert vsd_ref.vsd(test, gt, gt, K, 15.0, DIAM, TAUS).tolist() == [0.0] * 10
    # the estimate 32 mm behind: not visible by itself where the test is, but visible wherever the GT is
    est = _row(532, 532, 532, 532)
    c = vsd_ref.vsd_counts(test, est, gt, K, 15.0, DIAM, TAUS)
    assert c.tolist() == [3, 3] + [3] * 6 + [0] * 4       # |dist| / 100 = 0.32: counted for taus 0.05 .. 0.3
    assert vsd_ref.vsd(test, est, gt, K, 15.0, DIAM, TAUS).tolist() == [1.0] * 6 + [0.0] * 4
    # with delta 25, pixel 2 (20 mm behind the occluder) becomes visible for the GT, and so for the estimate
    assert vsd_ref.vsd_counts(test, est, gt, K, 25.0, DIAM, TAUS)[:2].tolist() == [4, 4]


def test_vsd_ref_estimate_in_front_of_the_scene():
    gt = _row(500, 500, 0, 0)
    test = _row(500, 500, 600, 600)
    est = _row(0, 500, 520, 560)        # pixel 2: 80 mm in front of the scene (visible); pixel 3: 40 mm in front
    c = vsd_ref.vsd_counts(test, est, gt, K, 15.0, DIAM, TAUS)
    # union: pixels 0 (GT), 1 (both), 2, 3 (estimate) -> 4; intersection: pixel 1, error 0
    assert c.tolist() == [4, 1] + [0] * 10
    assert vsd_ref.vsd(test, est, gt, K, 15.0, DIAM, TAUS).tolist() == [0.75] * 10
    est_behind = _row(0, 500, 700, 0)  # 100 mm behind the scene: hidden
    assert vsd_ref.vsd_counts(test, est_behind, gt, K, 15.0, DIAM, TAUS)[:2].tolist() == [2, 1]


def test_vsd_ref_zero_depth_test_pixels_and_empty_union():
    gt = _row(500, 500, 0, 0)
    est = _row(0, 520, 520, 0)
    hole = _row(0, 0, 0, 0)             # no measurement anywhere: every rendered pixel is visible
    c = vsd_ref.vsd_counts(hole, est, gt, K, 15.0, DIAM, TAUS)
    assert c.tolist() == [3, 1] + [1] * 4 + [0] * 6       # pixel 1: 0.2 (1 + 5e-7) >= 0.05 .. 0.2
    empty = _row(0, 0, 0, 0)
    assert vsd_ref.vsd_counts(_row(500, 500, 500, 500), empty, empty, K, 15.0, DIAM, TAUS).tolist() == [0] * 12
    assert vsd_ref.vsd(_row(500, 500, 500, 500), empty, empty, K, 15.0, DIAM, TAUS).tolist() == [1.0] * 10


def test_vsd_ref_distance_is_exact_at_the_principal_point():
    # at (cx, cy) the distance is the depth itself: |532 - 500| / 100 = 0.32 exactly in fp64; elsewhere slightly more
    K2 = np.array([[600.0, 0, 2], [0, 600.0, 0], [0, 0, 1]])
    d = vsd_ref.dist_im(_row(532, 532, 532), K2)
    assert d[0, 2] == 532.0 and d[0, 0] > d[0, 1] > 532.0


def test_geometry_only_ply_loading_ignores_a_texture(tmp_path):
    from foundpose_amd import renderer, synthetic
    m = synthetic.make_blob_mesh(6, 6, radius=20.0, seed=1)
    p = tmp_path / "plain.ply"
    renderer.save_ply(str(p), m, binary=False)
    text = p.read_text().replace("format ascii 1.0\n", "format ascii 1.0\ncomment TextureFile obj_000001.png\n")
    (tmp_path / "tex.ply").write_text(text)
    with pytest.raises(NotImplementedError):
        renderer.load_ply(str(tmp_path / "tex.ply"))          # the default is unchanged
    g = renderer.load_ply(str(tmp_path / "tex.ply"), geometry_only=True)
    assert np.array_equal(g.vertices, renderer.load_ply(str(p)).vertices) and np.array_equal(g.faces, m.faces)
