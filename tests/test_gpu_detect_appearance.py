"""GPU end to end with the appearance score, on the world of tests/test_gpu_detect.py: two blobs, the small ViT with
seed 1234 at fp32, crops of 56 pixels (4 x 4 patches).  A pasted template's cut-out and mask ARE its template's, so its patch descriptors
and its patch coverage are the template's bit for bit: every valid patch finds itself at similarity 1, whatever the weights.  The other
claims -- a half-masked copy keeps its object, the noise blob stays below -- hold for these seeds; the scores are printed."""
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import detect, detect_util as du, infer_pose_util, repre_util
from tests.test_gpu_detect import H, W, World

pytestmark = pytest.mark.gpu
MODE = "semantic_appearance"
OLD_KEYS = {"proposal", "decision", "category_id", "score", "template_id", "area", "bbox", "suppressed_by"}


class AppearanceWorld(World):
    def __init__(self, root):
        super().__init__(root)
        self.plain_banks = self.banks
        self.banks = {lid: du.build_detector_bank(self.ex, self.held[lid]["rgb"], self.held[lid]["mask"], 56, with_patches=True) for lid in (1, 2)}
        self.plain_opts = self.opts
        self.opts = self.opts._replace(detector_score_type=MODE)
        self.min_cover = du.min_cover_pixels(self.opts.detector_patch_min_cover, 14)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return AppearanceWorld(str(tmp_path_factory.mktemp("detect_appearance")))


def _proposal(im, mask):
    return {"scene_id": 1, "image_id": im, "time": 0.25, "segmentation": infer_pose_util.binary_mask_to_rle(mask)}


def test_the_patch_bank_is_the_plain_bank_plus_two_tables(world):
    for lid in (1, 2):
        b, plain = world.banks[lid], world.plain_banks[lid]
        assert torch.equal(b["descs"], plain["descs"]) and b["template_ids"].tolist() == plain["template_ids"].tolist()
        T = int(b["descs"].shape[0])
        assert tuple(b["patch_descs"].shape) == (T, 16, world.ex.arch.dim) and b["patch_descs"].dtype == torch.float32
        assert tuple(b["patch_cover"].shape) == (T, 16) and b["patch_cover"].dtype == torch.int32 and b["patch_size"] == 14
        norms = b["patch_descs"].double().norm(dim=2)
        assert float((norms - 1).abs().max()) < 1e-5
        assert int(b["patch_cover"].min()) >= 0 and int(b["patch_cover"].max()) <= 196 and bool((b["patch_cover"] >= world.min_cover).any(1).all())
    bs = du.bank_set(world.banks)
    assert tuple(bs.patch_descs.shape) == (36, 16, world.ex.arch.dim) and tuple(bs.patch_cover.shape) == (36, 16)
    assert du.bank_set(world.plain_banks).patch_descs is None
    assert du.bank_set({1: world.banks[1], 2: world.plain_banks[2]}).patch_descs is None   # only when every bank has them


def test_a_pasted_template_finds_every_one_of_its_patches(world):
    for im in (3, 4):
        dets, decs = world.label(im, detector_min_score=0.0, detector_nms_thresh=1.0)
        for d in decs:
            print(f"image {im} proposal {d['proposal']}: {d['decision']} object {d['category_id']} template {d['template_id']} score {d['score']} "
                  f"semantic {d['semantic_score']} appearance {d['appearance_score']} valid patches {d['valid_patches']}")
        for d, (lid, t) in zip(decs, world.planted_of[im]):
            want_valid = int((world.banks[lid]["patch_cover"][t] >= world.min_cover).sum())
            assert (d["category_id"], d["template_id"]) == (lid, t), d
            assert d["appearance_score"] >= 1 - 1e-5 and d["semantic_score"] >= 1 - 1e-5 and d["score"] >= 1 - 1e-5, d
            assert d["valid_patches"] == want_valid and 0 < want_valid <= 16, d
        noise = decs[len(world.planted_of[im])]
        pasted = min(d["score"] for d in decs[:len(world.planted_of[im])])
        assert noise["score"] < pasted and noise["score"] < 1 - 1e-4, "the noise blob scores like a pasted template: pick other seeds"
        assert set(decs[0]) == OLD_KEYS | {"semantic_score", "appearance_score", "valid_patches"}
    # the empty proposal of image 3: no crop, no valid patch
    empty = world.label(3)[1][4]
    assert empty["decision"] == "empty" and empty["valid_patches"] == 0 and empty["appearance_score"] is None


def _box_hw(world, lid, t):
    ys, xs = np.nonzero(world.held[lid]["mask"][t].cpu().numpy())
    return int(ys.max() - ys.min() + 1), int(xs.max() - xs.min() + 1)


def _whole_and_left_half(world, lid, t, x0=10, y0=20):
    """Template t of object lid pasted into a noise frame of its own, offered whole and with only its left half masked."""
    rgb = world.held[lid]["rgb"][t].permute(1, 2, 0).cpu().numpy()
    on = world.held[lid]["mask"][t].cpu().numpy() != 0
    image = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    image[y0:y0 + 224, x0:x0 + 224][on] = rgb[on]
    xs = np.nonzero(on.any(0))[0]
    half = on.copy()
    half[:, (xs.min() + xs.max() + 1) // 2:] = False            # the left half of the object's box
    full_m, half_m = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    full_m[y0:y0 + 224, x0:x0 + 224] = on
    half_m[y0:y0 + 224, x0:x0 + 224] = half
    _, decs = du.label_proposals(world.opts._replace(detector_min_score=0.0, detector_nms_thresh=1.0), image,
                                 [_proposal(7, full_m), _proposal(7, half_m)], world.banks, world.ex)
    return decs


HALVED = (2, 0)   # (object, template)


def test_a_half_masked_copy_keeps_its_object_with_fewer_valid_patches(world):
    """Which template is pasted and halved.  The cut-out keeps the aspect and scales the LONGER side of the box to the crop.  Where the box
    is at least as tall as it is wide, its left half is still scaled by the height -- the same pixels at the same scale, half as many of
    them -- so fewer patches are covered: 6 or 7 against 8 to 12 for all eight such templates of this world.  Where the box is wider than
    tall, halving the width RAISES the scale (up to twice) and the half can cover MORE patches than the whole: 12 against 8 for object 1's
    template 5, a box of 79 x 132.  So the halved template is one whose box is at least as tall as wide, which the test checks.
    Which object the half gets is decided by the CLS score alone (the appearance score is taken against the winner's best template: it
    changes the score, never the label), and with random weights that is a property of the seeds: of the eight tall templates the four
    of object 2 keep their object (semantic 0.87 to 0.95) and the four of object 1 go to object 2 (0.87 to 0.95 as well).  Like the seeds
    of the noise blob, HALVED is one for which it holds; pick another if the weights change.  The scores are printed: the whole scores 1.0
    in both parts, the half 0.90 and 0.59."""
    lid, t = HALVED
    h, w = _box_hw(world, lid, t)
    assert h >= w, "halve a template whose box is at least as tall as wide (see above)"
    full, got = _whole_and_left_half(world, lid, t)
    print(f"half-masked copy of object {lid} template {t} (box {h} x {w}): object {got['category_id']} template {got['template_id']} semantic "
          f"{got['semantic_score']} appearance {got['appearance_score']} combined {got['score']} valid patches {got['valid_patches']} "
          f"(whole: {full['valid_patches']}, combined {full['score']})")
    assert full["category_id"] == lid and full["template_id"] == t and full["score"] >= 1 - 1e-5
    assert got["category_id"] == lid
    assert 0 < got["valid_patches"] < full["valid_patches"]
    assert got["score"] == float(np.float32((np.float32(got["semantic_score"]) + np.float32(got["appearance_score"])) * np.float32(0.5)))


def test_the_patch_tables_round_trip_bit_for_bit(world, tmp_path):
    d = str(tmp_path / "repre")
    path = du.save_detector_bank(world.banks[1], d)
    assert sorted(os.listdir(d)) == sorted([du.DETECTOR_PATCH_FILE, du.DETECTOR_FILE]) and path.endswith(du.DETECTOR_FILE)
    disk = du.load_detector_bank(d, with_patches=True)
    for k in ("descs", "patch_descs", "patch_cover"):
        assert torch.equal(disk[k], world.banks[1][k]) and disk[k].is_cuda and disk[k].dtype == world.banks[1][k].dtype
    assert disk["patch_size"] == 14 and disk["crop_size"] == 56 and disk["template_ids"].tolist() == list(range(18))
    plain = du.load_detector_bank(d)                             # detector.pth keeps its format and its loader
    assert set(plain) == {"descs", "template_ids", "extractor_name", "crop_size"}
    d2 = str(tmp_path / "plain")
    du.save_detector_bank(world.plain_banks[1], d2)
    assert os.listdir(d2) == [du.DETECTOR_FILE]
    with pytest.raises(FileNotFoundError, match="detect onboard"):
        du.load_detector_bank(d2, with_patches=True)
    # tables of another extractor are not paired with this detector.pth; a plain bank saved over the pair takes the stale tables away
    assert torch.load(os.path.join(d, du.DETECTOR_PATCH_FILE), weights_only=True)["extractor_name"] == world.banks[1]["extractor_name"]
    other = dict(world.banks[1], extractor_name=world.banks[1]["extractor_name"].replace("layer=11", "layer=10"))
    d3 = str(tmp_path / "mixed")
    du.save_detector_bank(other, d3)
    du.save_detector_bank({k: v for k, v in other.items() if not k.startswith("patch_")}, d3)
    assert os.listdir(d3) == [du.DETECTOR_FILE]
    du.save_detector_bank(other, d3)
    torch.save(dict(torch.load(os.path.join(d3, du.DETECTOR_FILE), weights_only=True), extractor_name=world.banks[1]["extractor_name"]),
               os.path.join(d3, du.DETECTOR_FILE))
    with pytest.raises(ValueError, match="not written together"):
        du.load_detector_bank(d3, with_patches=True)


def test_banks_without_patches_are_refused_by_name(world):
    with pytest.raises(ValueError, match="detect onboard"):
        du.label_proposals(world.opts, world.images[3], world.of_image(3), world.plain_banks, world.ex)


def _strip_time(dets):
    return json.dumps([{k: v for k, v in r.items() if k != "time"} for r in du.detections_to_list(dets)])


def test_the_default_mode_is_what_it_was(world):
    assert world.plain_opts.detector_score_type == "semantic"
    for im in (3, 4):
        old = du.label_proposals(world.plain_opts, world.images[im], world.of_image(im), world.plain_banks, world.ex)
        new = du.label_proposals(world.plain_opts._replace(detector_score_type="semantic", detector_patch_min_cover=0.9), world.images[im],
                                 world.of_image(im), world.banks, world.ex)
        assert old[1] == new[1] and _strip_time(old[0]) == _strip_time(new[0])
        assert all(set(d) == OLD_KEYS for d in old[1]) and [d["decision"] for d in old[1]] == world.want[im]


def test_the_command_line_runs_end_to_end_in_the_new_mode(world, tmp_path):
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
        rdir = repre_util.get_object_repre_dir_path(os.path.join(world.root, "object_repre"), "v1", "synth", lid)
        disk = du.load_detector_bank(rdir, with_patches=True)
        for k in ("descs", "patch_descs", "patch_cover"):
            assert torch.equal(disk[k], world.banks[lid][k])
    out = tmp_path / "out" / "detections.json"
    detect.main(["run"] + common + ["--proposals", str(tmp_path / "proposals.json"), "--dataset-dir", str(split), "--output", str(out)])
    memory = []
    for im in (3, 4):
        memory += du.detections_to_list(world.label(im)[0])
    strip = lambda recs: json.dumps([{k: v for k, v in r.items() if k != "time"} for r in recs])
    assert strip(json.loads(out.read_text())) == strip(memory)
    decisions = json.loads((tmp_path / "out" / "detector-decisions.json").read_text())
    assert [d["decision"] for d in decisions] == world.want[3] + world.want[4]
    assert all({"semantic_score", "appearance_score", "valid_patches"} <= set(d) for d in decisions)
    loaded = infer_pose_util.load_detections_in_bop_format(str(out))
    assert sorted(loaded) == [(1, 3, 1), (1, 3, 2), (1, 4, 1), (1, 4, 2)] and all(len(v) == 1 for v in loaded.values())
    assert all(d["score"] >= 1 - 1e-4 for v in loaded.values() for d in v)
