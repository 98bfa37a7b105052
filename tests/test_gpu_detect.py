"""GPU end to end, built like tests/test_gpu_onboarding.py: two meshes -> gen_templates -> detector banks -> frames
of noise with templates of both objects pasted where their masks are -> label_proposals / the detect command line -> a detections file
that load_detections_in_bop_format and infer_batched take.  It holds with any backbone weights, because a pasted proposal's cut-out IS its
template's cut-out bit for bit: with detector_topk = 1 it scores 1 against its own template.  (Seeds 7 and 11 for the two blobs and 1234 for
the weights: the noise proposals and the other object's templates stay below 1 - 1e-4 with them; the scores are printed.)"""
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import detect, detect_util as du, eval_bop19, feature_util, gen_repre, gen_templates, infer, infer_pose_util, repre_util, synthetic
from foundpose_amd.crop_util import PinholePlaneCameraModel
from foundpose_amd.renderer import save_ply
from foundpose_amd.vit_config import ARCHS

pytestmark = pytest.mark.gpu
DET_NAME = "dinov2_version=vits14-reg_stride=14_facet=token_layer=11_norm=1"          # the final normalised CLS token of the small model
POSE_NAME = "dinov2_version=vits14-reg_stride=14_facet=token_layer=9_logbin=0_norm=1"  # tests/test_gpu_onboarding.py's
W, H = 480, 360
# (image id, object, template, x0, y0): where each template's 224 x 224 frame is pasted
PLANTED = [(3, 1, 5, 10, 20), (3, 2, 12, 250, 100), (4, 2, 3, 30, 70), (4, 1, 16, 245, 5)]


def _dataset(root):
    d = os.path.join(root, "synth")
    os.makedirs(os.path.join(d, "models"))
    for lid, seed in ((1, 7), (2, 11)):
        save_ply(os.path.join(d, "models", f"obj_{lid:06d}.ply"), synthetic.make_blob_mesh(50, 50, radius=55.0, seed=seed))
    with open(os.path.join(d, "models", "models_info.json"), "w") as f:
        json.dump({"1": {"diameter": 200.0}, "2": {"diameter": 200.0}}, f)
    with open(os.path.join(d, "camera.json"), "w") as f:
        json.dump({"cx": 325.26, "cy": 242.05, "fx": 572.41, "fy": 573.57, "width": 640, "height": 480, "depth_scale": 1.0}, f)


class World:
    def __init__(self, root):
        self.root = root
        _dataset(root)
        topts = gen_templates.load_opts({"gen_templates_opts": {"version": "v1", "object_dataset": "synth", "object_lids": None,
                                                                "min_num_viewpoints": 9, "num_inplane_rotations": 2, "crop_size": [224, 224]}})
        self.held = gen_templates.synthesize_templates(topts, root, root, (450.0, 550.0), return_templates=True)
        self.weights = os.path.join(root, "dinov2_vits14_reg4_pretrain.pth")
        torch.save(synthetic.make_vit_state_dict(ARCHS["vits14-reg"], seed=1234), self.weights)
        self.ex = feature_util.make_feature_extractor(DET_NAME, weights=self.weights, precision="fp32").to("cuda")
        self.opts = du.load_opts({"detect_opts": {"version": "v1", "templates_version": "v1", "object_dataset": "synth", "object_lids": [1, 2],
                                                  "detector_extractor_name": DET_NAME, "detector_crop_size": 56, "detector_topk": 1,
                                                  "detector_min_score": 1 - 1e-4, "detector_batch": 4}})
        self.banks = {lid: du.build_detector_bank(self.ex, self.held[lid]["rgb"], self.held[lid]["mask"], 56) for lid in (1, 2)}
        rng = np.random.default_rng(3)
        self.images = {im: rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for im in (3, 4)}
        self.proposals = []
        masks = {}
        for im, lid, t, x0, y0 in PLANTED:
            rgb = self.held[lid]["rgb"][t].permute(1, 2, 0).cpu().numpy()
            on = self.held[lid]["mask"][t].cpu().numpy() != 0
            self.images[im][y0:y0 + 224, x0:x0 + 224][on] = rgb[on]
            m = np.zeros((H, W), np.uint8)
            m[y0:y0 + 224, x0:x0 + 224] = on
            masks[(im, lid)] = m
        blob = np.zeros((H, W), np.uint8)
        blob[300:350, 60:200] = 1                                  # noise only: below both pasted templates of either image
        for im, lids in ((3, (1, 2)), (4, (2, 1))):
            ms = [masks[(im, lids[0])], masks[(im, lids[1])]] + ([masks[(im, lids[0])]] if im == 3 else []) + [blob] \
                + ([np.zeros((H, W), np.uint8)] if im == 3 else [])
            for m in ms:   # category_id / score / bbox of a segmenter's file are ignored: planted wrong on purpose
                self.proposals.append({"scene_id": 1, "image_id": im, "category_id": 99, "score": 0.5, "bbox": [0, 0, 1, 1], "time": 0.25,
                                       "segmentation": infer_pose_util.binary_mask_to_rle(m)})
        # image 3: [object 1, object 2, object 1 again, noise, empty]; image 4: [object 2, object 1, noise]
        self.want = {3: ["kept", "kept", "suppressed", "low_score", "empty"], 4: ["kept", "kept", "low_score"]}
        self.planted_of = {3: [(1, 5), (2, 12), (1, 5)], 4: [(2, 3), (1, 16)]}

    def of_image(self, im):
        return [p for p in self.proposals if p["image_id"] == im]

    def label(self, im, **kw):
        return du.label_proposals(self.opts._replace(**kw), self.images[im], self.of_image(im), self.banks, self.ex)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(str(tmp_path_factory.mktemp("detect")))


def test_a_pasted_template_is_its_template_bit_for_bit(world):
    for im, lid, t, x0, y0 in PLANTED:
        tpl = (world.held[lid]["rgb"][t:t + 1].permute(0, 2, 3, 1).float() / 255.0).contiguous()
        tm = (world.held[lid]["mask"][t:t + 1] != 0).to(torch.uint8).contiguous()
        want, ws, wb, wa = du.crops_of_masks(tpl, tm, 56)
        frame = infer._to_device_image(world.images[im])[None].contiguous()
        m = torch.zeros(1, H, W, dtype=torch.uint8, device="cuda")
        m[0, y0:y0 + 224, x0:x0 + 224] = tm[0]
        got, gs, gb, ga = du.crops_of_masks(frame, m, 56)
        assert torch.equal(got, want) and int(gs[0]) == 0 == int(ws[0]) and int(ga[0]) == int(wa[0])
        assert (gb[0].cpu() - wb[0].cpu()).tolist() == [x0, y0, x0, y0]


def test_every_pasted_proposal_gets_its_object_and_template(world):
    for im in (3, 4):
        dets, decs = world.label(im, detector_min_score=0.0, detector_nms_thresh=1.0)
        for d in decs:
            print(f"image {im} proposal {d['proposal']}: {d['decision']} object {d['category_id']} template {d['template_id']} score {d['score']}")
        for d, (lid, t) in zip(decs, world.planted_of[im]):
            assert (d["category_id"], d["template_id"]) == (lid, t) and d["score"] >= 1 - 1e-5, d
        noise = decs[len(world.planted_of[im])]
        assert noise["score"] < 1 - 1e-4, "the noise blob is as close to a template as a template is to itself: pick other seeds"


def test_exactly_the_pasted_ones_survive_and_every_proposal_has_a_reason(world):
    for im in (3, 4):
        dets, decs = world.label(im)
        assert [d["decision"] for d in decs] == world.want[im]
        kept = sorted((k[2], tuple(d["bbox"])) for k, ds in dets.items() for d in ds)
        want = []
        for (lid, t), (im2, _, _, x0, y0) in zip(world.planted_of[im][:2], [p_ for p_ in PLANTED if p_[0] == im]):
            ys, xs = np.nonzero(world.held[lid]["mask"][t].cpu().numpy())
            want.append((lid, (int(x0 + xs.min()), int(y0 + ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1))))
        assert kept == sorted(want) and set(dets) == {(1, im, 1), (1, im, 2)}
        for k, ds in dets.items():
            for d in ds:
                assert d["time"] > 0.25 and d["segmentation"] in [p_["segmentation"] for p_ in world.of_image(im)]
    dets, decs = world.label(3)
    assert decs[2]["suppressed_by"] == 0 and decs[0]["suppressed_by"] == -1      # the twin falls to its first copy
    assert decs[4]["area"] == 0 and decs[4]["bbox"] == [0, 0, 0, 0]
    # the options that drop: everything is small below 10^6 pixels; one detection per image
    assert {d["decision"] for d in world.label(3, detector_min_area=10 ** 6)[1]} == {"small"}
    one = world.label(3, detector_max_per_image=1)[1]
    assert sorted(d["decision"] for d in one) == ["empty", "kept", "low_score", "max_per_image", "suppressed"]
    with pytest.raises(ValueError, match="canvas"):
        du.label_proposals(world.opts, world.images[3][:, :470], world.of_image(3), world.banks, world.ex)
    with pytest.raises(ValueError, match="detector_crop_size"):
        world.label(3, detector_crop_size=28)


def _strip_time(records):
    return json.dumps([{k: v for k, v in r.items() if k != "time"} for r in records])


def test_the_vit_batch_does_not_change_a_byte(world):
    outs = []
    for b in (1, 4):
        recs = []
        for im in (3, 4):
            recs += du.detections_to_list(world.label(im, detector_batch=b)[0])
        outs.append(_strip_time(recs))
    assert outs[0] == outs[1] and len(json.loads(outs[0])) == 4


def test_the_command_line_writes_what_the_calls_return_and_infer_takes_it(world, tmp_path):
    from PIL import Image
    split = tmp_path / "split"
    os.makedirs(split / "000001" / "rgb")
    for im, img in world.images.items():
        Image.fromarray(img).save(split / "000001" / "rgb" / f"{im:06d}.png")
    (tmp_path / "detect.json").write_text(json.dumps({"detect_opts": world.opts._asdict()}))
    (tmp_path / "proposals.json").write_text(json.dumps(world.proposals))
    common = ["--opts", str(tmp_path / "detect.json"), "--output-path", world.root, "--precision", "fp32", "--weights", world.weights]
    detect.main(["onboard"] + common)
    for lid in (1, 2):
        disk = du.load_detector_bank(repre_util.get_object_repre_dir_path(os.path.join(world.root, "object_repre"), "v1", "synth", lid))
        assert torch.equal(disk["descs"], world.banks[lid]["descs"]) and disk["crop_size"] == 56 and disk["extractor_name"] == du.extractor_name_of(world.ex)
        assert disk["template_ids"].tolist() == list(range(18))
    out = tmp_path / "out" / "detections.json"
    detect.main(["run"] + common + ["--proposals", str(tmp_path / "proposals.json"), "--dataset-dir", str(split), "--output", str(out)])
    memory = []
    for im in (3, 4):
        memory += du.detections_to_list(world.label(im)[0])
    assert _strip_time(json.loads(out.read_text())) == _strip_time(memory)
    decisions = json.loads((tmp_path / "out" / "detector-decisions.json").read_text())
    assert [d["decision"] for d in decisions] == world.want[3] + world.want[4]
    assert [d["proposal"] for d in decisions] == list(range(8)) and decisions[2]["suppressed_by"] == 0
    # the file is a CNOS file: the loader keys it by the planted (scene, image, object)
    loaded = infer_pose_util.load_detections_in_bop_format(str(out))
    assert sorted(loaded) == [(1, 3, 1), (1, 3, 2), (1, 4, 1), (1, 4, 2)] and all(len(v) == 1 for v in loaded.values())
    # ... and infer_batched, task "detection", estimates one pose per detection of the file (wiring only: not accuracy)
    ro = gen_repre.load_opts({"gen_repre_opts": {"version": "v1", "templates_version": "v1", "object_dataset": "synth", "object_lids": [1, 2],
                                                 "extractor_name": POSE_NAME, "pca_components": 64, "cluster_num": 32,
                                                 "template_desc_opts": {"desc_type": "tfidf"}}})
    pose_ex = feature_util.make_feature_extractor(POSE_NAME, weights=world.weights, precision="fp32").to("cuda")
    repres = {lid: repre_util.load_object_repre(gen_repre.generate_repre(ro, "synth", lid, world.root, extractor=pose_ex, templates=world.held[lid]))
              for lid in (1, 2)}
    for lid in (1, 2):   # onboarding the pose bank leaves the detector bank beside it
        assert os.path.exists(os.path.join(repre_util.get_object_repre_dir_path(os.path.join(world.root, "object_repre"), "v1", "synth", lid), "detector.pth"))
    iopts = infer.load_opts({"infer_opts": {"version": "v1", "object_dataset": "synth", "repre_version": "v1", "object_lids": [1, 2], "crop_rel_pad": 0.2,
                                            "crop_size": [224, 224], "extractor_name": POSE_NAME, "grid_cell_size": 14.0, "pnp_ransac_iter": 400,
                                            "vis_results": False, "task": "detection"}})
    cam = PinholePlaneCameraModel(W, H, (572.0, 572.0), (W / 2.0, H / 2.0), np.eye(4))
    frames = [{"scene_id": 1, "im_id": im, "image": world.images[im], "camera": cam} for im in (3, 4)]
    odir = str(tmp_path / "poses")
    infer.infer_batched(iopts, iter(frames), loaded, repres, odir, batch_detections=4, extractor=pose_ex, num_target_insts={(1, 3), (1, 4)})
    rows = eval_bop19.load_results_csv(os.path.join(odir, "coarse_synth-estimated-poses.csv"))
    assert sorted((r["scene_id"], r["im_id"], r["obj_id"]) for r in rows) == sorted(loaded)
