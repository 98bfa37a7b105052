"""GPU: gt_info.write_gt_info on a BOP tree from synthetic.make_bop_eval_scene plus one hand-edited image whose instances leave the
image: scene_gt_info.json against the restatement applied to renders the test fetches itself, the PNG masks, the targets, the evaluators
end to end on the written files, depth_from_gt on a tree without depth/, the refusals."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from foundpose_amd import eval_bop19 as eb, eval_coco, gt_info, ops, synthetic
from foundpose_amd.eval_bop19 import _Camera
from foundpose_amd.infer_pose_util import binary_mask_to_rle
from foundpose_amd.renderer import HipRasterizer, load_ply
from tests import gt_info_ref as ref

pytestmark = pytest.mark.gpu
W, H = 64, 48
EXTRA_IM = 3


def _window_camera(K, T):
    Kw = K.copy()
    Kw[0, 2] += W
    Kw[1, 2] += H
    return _Camera(Kw, 3 * W, 3 * H, np.linalg.inv(T))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The fixture's three images (two objects, an occluder strip and a 20 x 20 hole each), a fourth image written by hand whose three
    instances of object 1 sit half outside the image, wholly outside it but inside the 3W x 3H window, and beyond the window; nine pixels
    of a depth image where one instance is the surface seen are punched out.  Then the tool, once."""
    root = tmp_path_factory.mktemp("gt_info")
    meta = synthetic.make_bop_eval_scene(str(root), num_images=3, num_objects=2, width=W, height=H, mesh_res=12, gts_per_image=2, depth_scale=0.1, seed=7)
    sd = os.path.join(meta["split_dir"], "000001")
    K = meta["K"]
    gts, cams = json.load(open(os.path.join(sd, "scene_gt.json"))), json.load(open(os.path.join(sd, "scene_camera.json")))
    z = 2000.0
    at = lambda u: [(u - K[0, 2]) / K[0, 0] * z, 0.0, z]            # the translation whose centre projects to column u, on the row of cy
    gts[str(EXTRA_IM)] = [{"cam_R_m2c": np.eye(3).ravel().tolist(), "cam_t_m2c": at(u), "obj_id": 1} for u in (0.0, -32.0, -400.0)]
    cams[str(EXTRA_IM)] = dict(cams["0"])
    json.dump(gts, open(os.path.join(sd, "scene_gt.json"), "w"))
    json.dump(cams, open(os.path.join(sd, "scene_camera.json"), "w"))
    Image.fromarray(np.full((H, W), 30000, np.uint16)).save(os.path.join(sd, "depth", f"{EXTRA_IM:06d}.png"))     # a plane at 3000 mm
    ras = HipRasterizer("cuda")
    for lid in meta["diameters"]:
        ras.add_object_model(lid, mesh=load_ply(os.path.join(meta["models_dir"], f"obj_{lid:06d}.ply")))
    # the hole: nine pixels where an instance is the nearest surface (its render equals the stored depth to the PNG's step), punched out of
    # the depth image of the instance that has the most of them
    best = None
    for im in range(3):
        u16 = np.array(Image.open(os.path.join(sd, "depth", f"{im:06d}.png")))
        stored = u16.astype(np.float32) * np.float32(0.1)
        for g, e in enumerate(gts[str(im)]):
            cam = _window_camera(K, eb._m2c(e["cam_R_m2c"], e["cam_t_m2c"]))        # the render the tool will make
            r = ras.render_views(int(e["obj_id"]), [cam], with_color=False)["depth"][0, H:2 * H, W:2 * W].cpu().numpy()
            ys, xs = np.nonzero((r > 0) & (np.abs(r - stored) < 0.2))
            if best is None or len(ys) > len(best[2]):
                best = (im, g, list(zip(ys.tolist(), xs.tolist())), u16, stored)
    hole_im, hole_g, front, u16, stored = best
    assert len(front) >= 9
    punched = front[:9]
    for y, x in punched:
        u16[y, x] = 0
    Image.fromarray(u16).save(os.path.join(sd, "depth", f"{hole_im:06d}.png"))
    os.remove(os.path.join(sd, "scene_gt_info.json"))
    os.remove(os.path.join(os.path.dirname(meta["split_dir"]), "test_targets_bop19.json"))
    summary = gt_info.write_gt_info(meta["split_dir"], meta["models_dir"], targets="bop19")
    return dict(meta=meta, sd=sd, gts=gts, cams=cams, ras=ras, summary=summary, punched=punched, unpunched=stored, hole=(hole_im, hole_g),
                info=json.load(open(os.path.join(sd, "scene_gt_info.json"))))


def _instances(tree):
    for im in sorted(int(k) for k in tree["gts"]):
        for g, e in enumerate(tree["gts"][str(im)]):
            yield im, g, int(e["obj_id"]), eb._m2c(e["cam_R_m2c"], e["cam_t_m2c"])


def _depth(tree, im):
    return eb.load_depth(os.path.join(tree["sd"], "depth", f"{im:06d}.png"), tree["cams"][str(im)]["depth_scale"])


def test_written_files_equal_the_restatement_on_renders_fetched_here(tree):
    K, info = tree["meta"]["K"], tree["info"]
    assert list(info) == ["0", "1", "2", "3"] and [len(v) for v in info.values()] == [2, 2, 2, 3]
    fracts = []
    for im, g, lid, T in _instances(tree):
        r = tree["ras"].render_views(lid, [_window_camera(K, T)], with_color=False)
        large, box = r["depth"][0].cpu().numpy(), r["boxes"][0].cpu().numpy()
        test = _depth(tree, im)
        row, mask, visib = ref.gt_visibility(test, large, K, 15.0, W, H)
        rec = info[str(im)][g]
        print(im, g, rec)
        assert rec == ref.record(row) and list(rec) == list(ref.record(row)), (im, g)          # key for key, in the toolkit's order
        if rec["px_count_visib"] > 0:    # bbox_obj is the renderer's silhouette box, moved into image coordinates
            assert rec["bbox_obj"] == [int(box[0]) - W, int(box[1]) - H, int(box[2] - box[0]), int(box[3] - box[1])]
        # the PNGs decode to the kernel's masks, which are the restatement's
        _, k_mask, k_visib = ops.gt_visibility(torch.from_numpy(test)[None].cuda(), r["depth"], [(0,) + gt_info.scan_box(box) + (W, H)],
                                               [(K[0, 0], K[1, 1], K[0, 2], K[1, 2], 15.0)])
        for sub, kern, want in (("mask", k_mask, mask), ("mask_visib", k_visib, visib)):
            png = Image.open(os.path.join(tree["sd"], sub, f"{im:06d}_{g:06d}.png"))
            assert png.mode == "L" and png.size == (W, H)
            assert np.array_equal(np.asarray(png), kern[0].cpu().numpy()) and np.array_equal(np.asarray(png), want)
        fracts.append(rec["visib_fract"])
    assert any(0.0 < f < 1.0 for f in fracts[:6])                     # the fixture's occluders
    # the hand-made image: half outside, outside the image but inside the window, beyond the window
    half, margin, beyond = info[str(EXTRA_IM)]
    assert 0.3 < half["visib_fract"] < 0.7 and half["bbox_obj"][0] < 0 and half["bbox_visib"][0] == 0
    assert margin["px_count_all"] > 0 and margin["px_count_visib"] == 0 and margin["visib_fract"] == 0.0
    assert margin["bbox_obj"] == [-1] * 4 and margin["bbox_visib"] == [-1] * 4
    assert beyond == {"bbox_obj": [-1] * 4, "bbox_visib": [-1] * 4, "px_count_all": 0, "px_count_valid": 0, "px_count_visib": 0, "visib_fract": 0.0}
    s = tree["summary"]
    assert (s["num_scenes"], s["num_images"], s["num_instances"]) == (1, 4, 9) and s["delta"] == 15.0
    assert s["num_instances_below_min_visib"] == sum(f < 0.1 for f in fracts)
    assert s["device_seconds"]["render"] > 0 and s["device_seconds"]["gt_visibility"] > 0 and s["wall_seconds"] > 0


def test_a_hole_changes_px_count_valid_and_not_px_count_visib(tree):
    K = tree["meta"]["K"]
    im, g = tree["hole"]
    lid, T = [(l, t) for i, j, l, t in _instances(tree) if (i, j) == (im, g)][0]
    large = tree["ras"].render_views(lid, [_window_camera(K, T)], with_color=False)["depth"][0].cpu().numpy()
    filled = ref.record(ref.gt_visibility(tree["unpunched"], large, K, 15.0, W, H)[0])
    rec = tree["info"][str(im)][g]
    assert rec["px_count_valid"] == filled["px_count_valid"] - len(tree["punched"])
    assert rec["px_count_visib"] == filled["px_count_visib"] and rec["px_count_all"] == filled["px_count_all"]
    assert rec["bbox_visib"] == filled["bbox_visib"]


def test_targets_agree_with_the_written_fractions(tree):
    written = json.load(open(os.path.join(os.path.dirname(tree["meta"]["split_dir"]), "test_targets_bop19.json")))
    inst = [(1, im, lid, tree["info"][str(im)][g]["visib_fract"]) for im, g, lid, _ in _instances(tree)]
    assert written == ref.targets_bop19(inst) and tree["summary"]["targets"].endswith("test_targets_bop19.json")
    assert {"scene_id": 1, "im_id": EXTRA_IM, "obj_id": 1, "inst_count": 1} in written
    assert sum(t["inst_count"] for t in written) == sum(v >= 0.1 for *_, v in inst)


def test_evaluators_run_on_the_written_files(tree, tmp_path):
    """scene_gt_info.json, the masks and the targets all come from the tool (the fixture deleted what make_bop_eval_scene wrote): the
    GT poses score AR = 1, detections made of the written visible masks score AP = 1."""
    split = tree["meta"]["split_dir"]
    ests, dets = [], []
    for im, g, lid, T in _instances(tree):
        rec = tree["info"][str(im)][g]
        if rec["visib_fract"] >= 0.1:
            ests.append((1, im, lid, 1.0, T, 0.1))
        m = np.asarray(Image.open(os.path.join(tree["sd"], "mask_visib", f"{im:06d}_{g:06d}.png")))
        if m.any():
            dets.append({"scene_id": 1, "image_id": im, "category_id": lid, "bbox": rec["bbox_visib"], "score": 1.0, "segmentation": binary_mask_to_rle(m > 0)})
    synthetic.write_bop_results_csv(str(tmp_path / "gt.csv"), ests)
    s = eb.evaluate_bop19(str(tmp_path / "gt.csv"), split)
    assert s["bop19_average_recall"] == 1.0 and s["num_target_instances"] == len(ests) >= 5
    c = eval_coco.evaluate_coco(dets, split, iou_type="segm")
    assert c["coco_average_precision"] == 1.0 and c["num_gt_instances"] == 9 and c["num_ignored_gt_instances"] >= 2


def test_a_second_run_is_refused_and_touches_nothing(tree):
    split = tree["meta"]["split_dir"]
    files = [os.path.join(dp, f) for dp, _, fs in os.walk(os.path.dirname(split)) for f in fs]
    before = {p: os.stat(p).st_mtime_ns for p in files}
    assert sum(p.endswith(".png") and "mask" in p for p in files) == 18
    with pytest.raises(FileExistsError):
        gt_info.write_gt_info(split, tree["meta"]["models_dir"], targets="bop19")
    with pytest.raises(FileExistsError):
        gt_info.main(["--dataset-dir", split, "--models-dir", tree["meta"]["models_dir"], "--no-masks"])
    assert {p: os.stat(p).st_mtime_ns for p in files} == before
    assert sorted(os.path.join(dp, f) for dp, _, fs in os.walk(os.path.dirname(split)) for f in fs) == sorted(files)


def test_command_line_mirrors_into_an_output_dir(tree, tmp_path, capsys):
    split = tree["meta"]["split_dir"]
    out = tmp_path / "mirror" / "test"
    assert gt_info.main(["--dataset-dir", split, "--models-dir", tree["meta"]["models_dir"], "--output-dir", str(out), "--no-masks",
                         "--targets", "bop24", "--scenes", "1"]) == 0
    assert json.load(open(out / "000001" / "scene_gt_info.json")) == tree["info"]
    assert sorted(os.listdir(out / "000001")) == ["scene_gt_info.json"]
    assert json.load(open(tmp_path / "mirror" / "test_targets_bop24.json")) == [{"scene_id": 1, "im_id": im} for im in range(4)]
    assert capsys.readouterr().out.rstrip().endswith(gt_info.NOT_PINNED)
    # another tolerance gives other numbers: at 1 000 mm the 40 mm occluders hide nothing
    tight = tmp_path / "tight"
    gt_info.write_gt_info(split, tree["meta"]["models_dir"], delta=1000.0, output_dir=str(tight), write_masks=False)
    wide = json.load(open(tight / "000001" / "scene_gt_info.json"))
    assert all(b["px_count_visib"] >= a["px_count_visib"] for k in wide for a, b in zip(tree["info"][k], wide[k]))
    assert any(b["px_count_visib"] > a["px_count_visib"] for k in wide for a, b in zip(tree["info"][k], wide[k]))


def _rgb_only_tree(root, meta, translations):
    sd = root / "rgbonly" / "test" / "000001"
    os.makedirs(sd / "rgb")
    Image.new("RGB", (W, H)).save(sd / "rgb" / "000000.png")
    json.dump({"0": [{"cam_R_m2c": np.eye(3).ravel().tolist(), "cam_t_m2c": list(t), "obj_id": 1} for t in translations]}, open(sd / "scene_gt.json", "w"))
    json.dump({"0": {"cam_K": meta["K"].ravel().tolist(), "depth_scale": 1.0}}, open(sd / "scene_camera.json", "w"))
    return str(root / "rgbonly" / "test"), sd


def test_depth_from_gt_lets_the_instances_occlude_each_other(tree, tmp_path):
    meta = tree["meta"]
    z = 20.0 * meta["diameters"][1]                                       # the silhouette's radius stays below 15 px: inside the image
    split, sd = _rgb_only_tree(tmp_path, meta, [(40.0, 0.0, z + 600.0), (0.0, 0.0, z)])
    with pytest.raises(FileNotFoundError, match="depth-from-gt"):
        gt_info.write_gt_info(split, meta["models_dir"])
    assert not os.path.exists(sd / "scene_gt_info.json")
    s = gt_info.write_gt_info(split, meta["models_dir"], depth_from_gt=True)
    far, near = json.load(open(sd / "scene_gt_info.json"))["0"]
    assert near["visib_fract"] == 1.0 and near["px_count_visib"] == near["px_count_all"] == near["px_count_valid"] > 100
    assert 0.0 < far["visib_fract"] < 1.0 and far["px_count_valid"] == far["px_count_all"]
    assert s["depth_from_gt"] and not os.path.exists(sd / "depth")        # no depth image is ever written
    m_far, m_near = (np.asarray(Image.open(sd / "mask_visib" / f"000000_{g:06d}.png")) > 0 for g in (0, 1))
    assert not (m_far & m_near).any() and m_far.sum() == far["px_count_visib"]


def test_a_pose_inside_the_near_plane_is_refused_by_name(tree, tmp_path):
    meta = tree["meta"]
    split, sd = _rgb_only_tree(tmp_path, meta, [(0.0, 0.0, 900.0), (0.0, 0.0, 60.0)])
    with pytest.raises(ValueError, match=r"instance 1 \(scene 1, image 0, object 1\)"):
        gt_info.write_gt_info(split, meta["models_dir"], depth_from_gt=True)
    assert sorted(os.listdir(sd)) == ["rgb", "scene_camera.json", "scene_gt.json"]
