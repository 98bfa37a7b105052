"""CPU: the annotated half of the evaluator -- symmetry expansion, the BOP ground-truth loader, the metrics table and the
extended estimated-poses.json entry (/root/reference/utils/eval_util.py:316-516, utils/data_util.py:105-151)."""
import json
import os

import numpy as np
import pytest

from foundpose_amd import eval_util, infer, ops
from foundpose_amd._lib import FoundPoseNativeError
from foundpose_amd.crop_util import PinholePlaneCameraModel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLIP_X = [1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 4.0, 0, 0, 0, 1]


def _check_rigid(syms):
    for s in syms:
        R = s["R"]
        assert R.shape == (3, 3) and s["t"].shape == (3, 1)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12


def test_symmetry_expansion_counts_and_geometry():
    assert len(eval_util.get_symmetry_transformations({"diameter": 1.0}, 0.01)) == 1
    d = eval_util.get_symmetry_transformations({"symmetries_discrete": [FLIP_X, np.diag([-1.0, -1, 1, 1]).ravel().tolist()]}, 0.01)
    assert len(d) == 3 and np.array_equal(d[0]["R"], np.eye(3)) and np.array_equal(d[0]["t"], np.zeros((3, 1)))
    assert np.array_equal(d[1]["R"], np.reshape(FLIP_X, (4, 4))[:3, :3]) and np.array_equal(d[1]["t"], [[0], [0], [4.0]])   # the 4x4 round-trips
    _check_rigid(d)
    axis, offset = np.array([0.3, -0.5, 0.8]), np.array([2.0, -1.0, 5.0])
    c = eval_util.get_symmetry_transformations({"symmetries_continuous": [{"axis": axis.tolist(), "offset": offset.tolist()}]}, 0.01)
    assert len(c) == int(np.ceil(np.pi / 0.01)) - 1 == 314
    _check_rigid(c)
    u = axis / np.linalg.norm(axis)
    for s in c:
        assert np.abs(s["R"] @ u - u).max() < 1e-12                                   # the axis is fixed ...
        assert np.abs(s["R"] @ (offset + 7 * u) + s["t"].ravel() - (offset + 7 * u)).max() < 1e-9   # ... through the offset
        assert np.abs(s["R"] - np.eye(3)).max() > 1e-3                                # the identity is not in the list
    both = eval_util.get_symmetry_transformations({"symmetries_discrete": [FLIP_X],
                                                    "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 0.01)
    assert len(both) == 2 * 314
    _check_rigid(both)
    assert all(np.abs(s["R"] - np.eye(3)).max() > 1e-3 or np.abs(s["t"]).max() > 1e-3 for s in both)
    coarse = eval_util.get_symmetry_transformations({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, np.pi / 4)
    assert len(coarse) == 3 and np.allclose(coarse[1]["R"], [[-1, 0, 0], [0, -1, 0], [0, 0, 1]])   # steps of 2 pi / 4


def test_bop_ground_truth_loader(tmp_path):
    from PIL import Image
    split = tmp_path / "test"
    sdir = split / "000002"
    (sdir / "rgb").mkdir(parents=True)
    (sdir / "mask_visib").mkdir()
    Image.fromarray(np.full((20, 30, 3), 7, np.uint8)).save(sdir / "rgb" / "000005.png")
    (sdir / "scene_camera.json").write_text(json.dumps({"5": {"cam_K": [100, 0, 15, 0, 110, 10, 0, 0, 1]}}))
    R = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    (sdir / "scene_gt.json").write_text(json.dumps({"5": [{"cam_R_m2c": np.ravel(R).tolist(), "cam_t_m2c": [1.5, -2, 300], "obj_id": 4},
                                                          {"cam_R_m2c": np.eye(3).ravel().tolist(), "cam_t_m2c": [0, 0, 500], "obj_id": 9}]}))
    (sdir / "scene_gt_info.json").write_text(json.dumps({"5": [{"bbox_obj": [3, 4, 10, 6], "visib_fract": 0.75},
                                                               {"bbox_obj": [0, 0, 5, 5], "visib_fract": 0.0}]}))
    m = np.zeros((20, 30), np.uint8)
    m[4:10, 3:13] = 255
    Image.fromarray(m).save(sdir / "mask_visib" / "000005_000000.png")
    Image.fromarray(np.zeros((20, 30), np.uint8)).save(sdir / "mask_visib" / "000005_000001.png")
    targets = [{"scene_id": 2, "im_id": 5, "obj_id": 4, "inst_count": 1}]
    frame, = list(infer.load_bop_frames(str(split), targets, 4, with_gt=True))
    a, b = frame["gt_annos"]
    assert (a.lid, b.lid) == (4, 9)
    assert np.array_equal(a.boxes_amodal, [3, 4, 13, 10]) and float(a.visibilities) == 0.75 and float(b.visibilities) == 0.0
    assert a.masks_modal.dtype == np.uint8 and np.array_equal(a.masks_modal, m // 255) and a.masks_modal.sum() == 60
    assert np.array_equal(a.pose.R, R) and np.array_equal(a.pose.t, [[1.5], [-2], [300]])   # m2w = m2c under the identity camera
    assert np.array_equal(frame["camera"].T_world_from_eye, np.eye(4))
    plain, = list(infer.load_bop_frames(str(split), targets, 4))
    assert "gt_annos" not in plain and set(plain) == {"scene_id", "im_id", "image", "camera"}


def _state():
    """A fixed evaluator state: three detections of objects 1 and 5."""
    rng = np.random.default_rng(5)
    ev = eval_util.PoseEvaluator([1, 5])
    for i, lid in enumerate((1, 5, 1)):
        ev.result_ids.append((3, 10 + i, lid, i, 0))
        ev.obj_ids.append(lid)
        ev.R.append(np.eye(3))
        ev.t.append(np.array([[1.0], [2.0], [300.0 + i]]))
        ev.score.append(0.25 * (i + 1))
        ev.time.append({"prep": 0.5})
        ev.mssd.append(float(rng.uniform(1, 30)))
        ev.mspd.append(float(rng.uniform(1, 30)))
        ev.mssd_n.append(ev.mssd[-1] / 100.0)
        ev.inliers_gt_err.append({"10": float(rng.uniform())})
        ev.inliers_est_err.append({"10": float(rng.uniform())})
        ev.inliers_gt.append(np.arange(i + 2))
        ev.inliers_est.append(np.arange(i + 1))
        ev.point_errors.append(rng.uniform(0, 9, 40))
        ev.rotation_errors.append(np.array(rng.uniform(0, 20)))
        ev.translation_errors.append(np.array(rng.uniform(0, 20)))
        ev.template_ori_err.append(float(rng.uniform(0, 20)))
        ev.detection_times[(3, 10 + i)] = 0.125
    return ev


def test_save_metrics_is_the_references_table(tmp_path):
    tabulate = pytest.importorskip("tabulate").tabulate
    ev = _state()
    ev.save_metrics(str(tmp_path / "m.tsv"), 10.0)
    # eval_util.py:400-516, line by line
    sel = {lid: np.where(np.array(ev.obj_ids) == lid)[0] for lid in (1, 5)}
    per = lambda f: [f(s) for s in sel.values()]
    mssd, mssd_n, mspd = (per(lambda s, k=k: np.nanmean(np.array(getattr(ev, k))[s])) for k in ("mssd", "mssd_n", "mspd"))
    ig, ie = (per(lambda s, k=k: np.nanmean([getattr(ev, k)[i]["10"] for i in s])) for k in ("inliers_gt_err", "inliers_est_err"))
    pe = lambda q: per(lambda s: np.nanpercentile(np.array(list(np.array(ev.point_errors)[s])), q))
    pr = lambda k, q: per(lambda s: np.nanpercentile(np.array(getattr(ev, k))[s], q))
    tpl = per(lambda s: np.nanmean(np.array(ev.template_ori_err)[s]))
    num = per(len)
    allp = np.concatenate(ev.point_errors, axis=0)
    table = [["mssd", np.nanmean(ev.mssd), np.nanmean(mssd), 0, 0] + mssd, ["mssd_n", np.nanmean(ev.mssd_n), np.nanmean(mssd_n), 0, 0] + mssd_n,
             ["mspd", np.nanmean(ev.mspd), np.nanmean(mspd), 0, 0] + mspd,
             ["inliers_gt", np.nanmean([e["10"] for e in ev.inliers_gt_err]), np.nanmean(ig), 0, 0] + ig,
             ["inliers_est", np.nanmean([e["10"] for e in ev.inliers_est_err]), np.nanmean(ie), 0, 0] + ie,
             ["Point_p50", np.percentile(allp, 50), 0, 0, 0] + pe(50), ["Point_p95", np.percentile(allp, 95), 0, 0, 0] + pe(95),
             ["Rot_p50", np.percentile(ev.rotation_errors, 50), 0, 0, 0] + pr("rotation_errors", 50),
             ["Rot_p95", np.percentile(ev.rotation_errors, 95), 0, 0, 0] + pr("rotation_errors", 95),
             ["Trans_p50", np.percentile(ev.translation_errors, 50), 0, 0, 0] + pr("translation_errors", 50),
             ["Trans_p95", np.percentile(ev.translation_errors, 95), 0, 0, 0] + pr("translation_errors", 95),
             ["Tpl_ori_err", np.mean(ev.template_ori_err), 0, 0, 0] + tpl, ["num_obj", np.sum(num), np.mean(num), 0, 0] + num]
    want = tabulate(table, headers=["", "overall", "pmean", "sym", "nonsym", "1", "5"], tablefmt="tsv", floatfmt=".2f", numalign=None, stralign=None)
    assert open(tmp_path / "m.tsv", "rb").read() == want.encode("utf-8")


def test_results_json_extended_and_plain_entries(tmp_path):
    ev = _state()
    ev.save_results_json(str(tmp_path / "e.json"))
    got = json.load(open(tmp_path / "e.json"))
    ref = json.load(open(os.path.join(GOLDEN, "pose_eval_estimated-poses.json")))   # written by the reference's save_results_json
    assert [set(e) for e in got] == [set(ref[0])] * 3
    for k in ref[0]:
        assert type(got[0][k]) is type(ref[0][k]), k
    assert got[1]["inliers_gt"] == 3 and got[1]["inliers_est"] == 2 and got[1]["mssd_n"] == pytest.approx(got[1]["mssd"] / 100)
    # without ground truth (mssd empty): exactly today's entry
    plain = eval_util.PoseEvaluator()
    cam = PinholePlaneCameraModel(64, 64, (100.0, 100.0), (32.0, 32.0), np.eye(4))
    plain.detection_times[(1, 2)] = 0.25
    plain.update_without_anno(1, 2, 0, 0, np.zeros((4, 3)) + [0, 0, 500.0], 7, np.eye(3), np.array([0, 0, 0.0]), cam, cam, {"prep": 0.1},
                              {"nn_vertex_ids": np.array([0, 1]), "coord_2d": np.array([[32.0, 32.0], [50.0, 32.0]]), "coord_2d_ids": np.array([0, 1])})
    plain.save_results_json(str(tmp_path / "p.json"))
    e, = json.load(open(tmp_path / "p.json"))
    assert set(e) == {"scene_id", "img_id", "obj_id", "inst_id", "hypothesis_id", "score", "R", "t", "time", "cnos_time"} and e["score"] == "0.5"


def test_pose_errors_refuses_cpu_tensors():
    import torch
    z = torch.zeros(4, 12, dtype=torch.float64)
    with pytest.raises(FoundPoseNativeError, match="CPU tensor"):
        ops.pose_errors(torch.zeros(5, 3, dtype=torch.float64), z[:1], z[:1], z, z, [[0, 5, 0, 4]])


def test_rotation_error_restates_scipy():
    Rotation = pytest.importorskip("scipy.spatial.transform").Rotation
    rng = np.random.default_rng(6)
    for _ in range(50):
        A, B = Rotation.random(random_state=rng).as_matrix(), Rotation.random(random_state=rng).as_matrix()
        want = np.rad2deg(Rotation.from_matrix(A.dot(B.T)).magnitude())
        assert abs(eval_util.rotation_error_deg(A, B) - want) < 1e-9
