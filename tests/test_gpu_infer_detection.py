"""task "detection" through both drivers on the planted split of tests/test_gpu_depth_refine.py (the module-scoped `driver_split`), with
count-free targets -- a set of images -- and one detection listed twice.  Every listed detection gets a csv row without num_preds_factor,
detection_min_score / detection_max_per_object drop exactly the rows they should, infer and infer_batched write the same csv, pose_nms
removes the duplicate as in the localization run, and the csv goes through eval_bop24.evaluate_bop24.  The split's correspondences are
exact and its "models" are the bank's vertices: this shows that the task is WIRED, not that it is accurate.  The kernels of the score are
checked in tests/test_gpu_detection_ap.py, the evaluator in tests/test_gpu_bop24_eval.py."""

import json
import os

import numpy as np
import pytest

from foundpose_amd import eval_bop19, eval_bop24, infer
from tests.test_gpu_depth_refine import _drive, driver_split  # noqa: F401  (the module-scoped fixture and the driver runner)
from tests.test_gpu_infer_batched import IM_IDS, _csv
from tests.test_gpu_infer_pose_nms import CSV, DUP, _doubled

pytestmark = pytest.mark.gpu

IMAGES = {(1, im) for im in IM_IDS}     # the count-free targets: images only


def _run(tmp_path, tag, ex, split, opts, batch=0, targets=IMAGES, device_masks=False):
    """tests/test_gpu_depth_refine._drive with count-free targets (_drive's own are the localization task's table) -> (csv lines without
    `time`, csv rows)."""
    d = str(tmp_path / tag)
    if batch:
        infer.infer_batched(opts, iter([split.frame(f, None) for f in range(3)]), split.dets, split.repres, d, batch_detections=batch, extractor=ex,
                            num_target_insts=targets, device_masks=device_masks)
    else:
        infer.infer(opts, lambda lid: iter([split.frame(f, [lid]) for f in range(3)]), split.dets, split.repres, d, extractor=ex, num_target_insts=targets)
    return _csv(d), eval_bop19.load_results_csv(os.path.join(d, CSV))


def _keys(rows):
    return sorted((r["scene_id"], r["im_id"], r["obj_id"]) for r in rows)


@pytest.fixture(scope="module")
def plain(driver_split, tmp_path_factory):
    """The detection run every case compares with: infer() on the split with DUP's detection listed twice, every option at its default.
    -> (directory, csv lines without `time`, csv rows, the doubled split, the options)."""
    ex, split, opts, _ = driver_split
    split, dopts = _doubled(split), opts._replace(task="detection")
    tmp = tmp_path_factory.mktemp("detection")
    lines, rows = _run(tmp, "plain", ex, split, dopts)
    return str(tmp / "plain"), lines, rows, split, dopts


def test_every_listed_detection_gets_a_row_in_both_drivers(tmp_path, driver_split, plain):
    ex = driver_split[0]
    _, lines, rows, split, dopts = plain
    # 4 + 2 planted instances and the duplicate, with num_preds_factor 1: the localization run needs factor 2 for the seventh
    # (the empty detection of object 2 in image 3 has no mask pixel and gets no pose in either task)
    listed = sorted(k for k, v in split.dets.items() for _ in v if k != (1, IM_IDS[0], 2))
    assert dopts.num_preds_factor == 1.0 and len(rows) == 7 and _keys(rows) == listed and _keys(rows).count(DUP) == 2
    # infer and infer_batched (batch 1 and 4; the masks made on the host and on the device) write the same csv up to `time`
    for tag, batch, dm in (("b1", 1, False), ("b4", 4, False), ("b4_dm", 4, True)):
        assert _run(tmp_path, tag, ex, split, dopts, batch=batch, device_masks=dm)[0] == lines, tag
    # the localization task's table is an image list here: its counts and object ids are not read (_drive passes that table)
    _drive(tmp_path, "table", ex, split, dopts, None)
    assert _csv(str(tmp_path / "table")) == lines


def test_the_options_drop_exactly_the_rows_they_name(tmp_path, driver_split, plain):
    ex = driver_split[0]
    _, lines, rows, split, dopts = plain
    # image 3 holds two detections of object 1, scored 0.9 and 0.8: a minimum between them drops exactly the second one's row
    first = (1, IM_IDS[0], 1)
    assert sorted(d["score"] for d in split.dets[first]) == [pytest.approx(0.8), pytest.approx(0.9)]
    gone = [i for i, r in enumerate(rows) if (r["scene_id"], r["im_id"], r["obj_id"]) == first][1]
    mlines, _ = _run(tmp_path, "min", ex, split, dopts._replace(detection_min_score=0.85))
    assert mlines[1:] == [line for i, line in enumerate(lines[1:]) if i != gone]
    # a minimum nothing reaches: a csv without a row
    assert _run(tmp_path, "none", ex, split, dopts._replace(detection_min_score=0.95))[1] == []
    # at most one per (image, object): the best of image 3's two, the first of the twins (equal scores keep the file's order)
    twin = [i for i, r in enumerate(rows) if (r["scene_id"], r["im_id"], r["obj_id"]) == DUP][1]
    oopts = dopts._replace(detection_max_per_object=1)
    olines, orows = _run(tmp_path, "one", ex, split, oopts)
    assert len(orows) == 5 and olines[1:] == [line for i, line in enumerate(lines[1:]) if i not in (gone, twin)]
    assert _run(tmp_path, "one_b4_dm", ex, split, oopts, batch=4, device_masks=True)[0] == olines     # the device path selects by the same rule
    # an image that is no target gets no pose
    _, trows = _run(tmp_path, "two_images", ex, split, dopts, targets={(1, IM_IDS[0]), (1, IM_IDS[2])})
    assert {r["im_id"] for r in trows} == {IM_IDS[0], IM_IDS[2]} and len(trows) == 4


def test_pose_nms_removes_the_duplicate_and_the_csv_is_scored(tmp_path, driver_split, plain):
    from PIL import Image

    from foundpose_amd.renderer import Mesh, save_ply
    ex, split0, _, _ = driver_split
    plain_dir, lines, rows, split, dopts = plain
    twins = [i for i, r in enumerate(rows) if (r["scene_id"], r["im_id"], r["obj_id"]) == DUP]
    second = sorted(twins, key=lambda i: rows[i]["score"], reverse=True)[1]
    for tag, batch in (("nms", 0), ("nms_b4", 4)):
        nlines, _ = _run(tmp_path, tag, ex, split, dopts._replace(frame_select_type="pose_nms"), batch=batch)
        assert nlines[1:] == [line for i, line in enumerate(lines[1:]) if i != second], tag
        decisions = json.load(open(str(tmp_path / tag / "pose-nms.json")))
        assert [d["keep"] for d in decisions] == [i != second for i in range(7)], tag

    # ---- the split written as a BOP tree: cameras, the planted poses as ground truth, one image per frame for its width, the bank's
    # vertices as models -- and the csv of every detection scored by the BOP24 evaluator
    root = tmp_path / "synth"
    sdir = root / "test" / "000001"
    os.makedirs(str(sdir / "rgb"))
    os.makedirs(str(root / "models"))
    cams, gts, infos = {}, {}, {}
    for f, im in enumerate(IM_IDS):
        cam = split0.cams[f]
        Image.fromarray(split0.images[f]).save(str(sdir / "rgb" / f"{im:06d}.png"))
        cams[str(im)] = {"cam_K": [cam.f[0], 0.0, cam.c[0], 0.0, cam.f[1], cam.c[1], 0.0, 0.0, 1.0], "depth_scale": 1.0}
        annos = [a for (f2, lid), al in sorted(split0.annos.items()) if f2 == f for a in al]
        gts[str(im)] = [{"cam_R_m2c": np.asarray(a.pose.R).ravel().tolist(), "cam_t_m2c": np.asarray(a.pose.t).ravel().tolist(), "obj_id": a.lid} for a in annos]
        infos[str(im)] = [{"visib_fract": 0.9} for _ in annos]
    for name, obj in (("scene_camera.json", cams), ("scene_gt.json", gts), ("scene_gt_info.json", infos)):
        (sdir / name).write_text(json.dumps(obj))
    info = {}
    for lid in (1, 2):
        v = split0.repres[lid].vertices.cpu().numpy().astype(np.float32)
        save_ply(str(root / "models" / f"obj_{lid:06d}.ply"), Mesh(v, np.array([[0, 1, 2]], np.int32), np.ones_like(v), np.zeros_like(v)))
        info[str(lid)] = {"diameter": float(2.0 * np.linalg.norm(v, axis=1).max())}
    (root / "models" / "models_info.json").write_text(json.dumps(info))
    (root / "test_targets_bop24.json").write_text(json.dumps([{"scene_id": 1, "im_id": im} for im in IM_IDS]))
    out = eval_bop24.evaluate_bop24(os.path.join(plain_dir, CSV), str(root / "test"))
    print({k: out[k] for k in ("bop24_average_precision", "bop24_average_precision_mssd", "bop24_average_precision_mspd")})
    assert out["num_target_images"] == 3 and out["num_estimates_evaluated"] == 7 and out["num_gt_instances"] == 6 == out["num_valid_gt_instances"]
    assert sum(po["num_estimates"] for po in out["per_object"].values()) == 7
    for po in out["per_object"].values():    # every estimate is a true positive, a false positive or ignored, at every threshold
        assert all(sum(t) == po["num_estimates"] for t in po["totals_mssd"] + po["totals_mspd"])
    assert 0.0 <= out["bop24_average_precision"] <= 1.0
