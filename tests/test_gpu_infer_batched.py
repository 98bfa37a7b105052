"""infer.infer_batched against infer.infer on one synthetic split: the frame-major, cross-object driver must write
the per-object driver's results -- every field of estimated-poses.json except the run times, and the BOP csv except its time column --
whatever the batch size, in fp32 and in the shipped bf16, with featuremetric refinement and ground-truth evaluation, without cropping,
and across a change of image size.  The comparison is exact: a pose depends on (seed, frame, object, instance) and on nothing else.

The split (in the style of tests/test_gpu_infer_driver.py::_scene): frames (1, 3), (1, 4), (1, 5) of one size; object 1 in all three, twice
in the first; object 2 in the last two; every instance's own crop is a template of its object's bank, with vertices from a planted pose.
Object 2 is also a target of the first frame, where its only detection has an empty mask; object 3 (a copy of object 2's bank) is a target
of the first frame and has no detection at all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from foundpose_amd import bank_builder, crop_util, eval_util, feature_util, infer, infer_pose_util, repre_util, workload
from tests.test_gpu_infer_driver import NAME

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T = 480, 640, 16
# (frame, object lid, box xywh), in detection-score order within a (frame, object)
INSTANCES = [(0, 1, [60, 50, 170, 150]), (0, 1, [380, 240, 150, 180]), (1, 1, [200, 120, 160, 170]), (2, 1, [90, 260, 180, 150]),
             (1, 2, [420, 60, 150, 160]), (2, 2, [330, 90, 170, 190])]
SLOTS = {1: [3, 7, 10, 13], 2: [2, 9]}
IM_IDS = [3, 4, 5]
TARGETS = {1: {(1, 3): 2, (1, 4): 1, (1, 5): 1}, 2: {(1, 3): 1, (1, 4): 1, (1, 5): 1}, 3: {(1, 3): 1}}
SEED_STATE = 4321


def _im_id(f):
    return IM_IDS[f] if f < len(IM_IDS) else 6 + f


def _opts(**kw):
    d = {"version": "v1", "object_dataset": "synth", "repre_version": "v1", "object_lids": [1, 2, 3], "crop_rel_pad": 0.2, "crop_size": [224, 224],
         "use_detections": True, "extractor_name": NAME, "grid_cell_size": 14.0, "match_template_type": "tfidf", "match_top_n_templates": 5,
         "match_feat_matching_type": "cyclic_buddies", "match_top_k_buddies": 300, "pnp_type": "opencv", "pnp_ransac_iter": 400,
         "pnp_inlier_thresh": 10.0, "final_pose_type": "best_coarse", "num_preds_factor": 1, "vis_results": False}
    d.update(kw)
    return d


def _mask(box, shape):
    x, y, w, h = box
    m = np.zeros(shape, np.uint8)
    m[y + 10:y + h - 10, x + 10:x + w - 10] = 1
    return m


def _build(ex, instances, frame_sizes, slots, crop=True):
    """-> images, cameras, CNOS detections, {lid: repre}, {(frame, lid): [GtAnnotation]} with the planted poses."""
    g = torch.Generator().manual_seed(0)
    images = [(torch.rand(h, w, 3, generator=g) * 255).to(torch.uint8).numpy() for h, w in frame_sizes]
    cams = [crop_util.PinholePlaneCameraModel(w, h, (600.0, 600.0), (w / 2.0, h / 2.0), np.eye(4)) for h, w in frame_sizes]
    dets, planted = [], {1: [], 2: []}
    for f, lid, box in instances:
        m = _mask(box, frame_sizes[f])
        score = 0.9 - 0.1 * sum(1 for f2, l2, _ in instances[:instances.index((f, lid, box))] if (f2, l2) == (f, lid))
        dets.append({"scene_id": 1, "image_id": _im_id(f), "category_id": lid, "bbox": box, "score": score, "time": 0.25,
                     "segmentation": infer_pose_util.binary_mask_to_rle(m)})
        img_f = torch.from_numpy(images[f]).cuda().float() / 255.0
        if crop:
            x, y, w, h = box
            c, cm, cc = crop_util.crop_detections(img_f, torch.from_numpy(m[None]).cuda(), [[x, y, x + w, y + h]], cams[f], (224, 224), 0.2)
            planted[lid].append((f, box, m, c[0], cm[0], cc[0]))
        else:
            planted[lid].append((f, box, m, img_f.permute(2, 0, 1), torch.from_numpy(m).cuda(), cams[f]))
    dets.append({"scene_id": 1, "image_id": IM_IDS[0], "category_id": 2, "bbox": [5, 5, 40, 40], "score": 0.7, "time": 0.25,     # a target whose
                 "segmentation": infer_pose_util.binary_mask_to_rle(np.zeros(frame_sizes[0], np.uint8))})                    # detection is empty
    repres, annos = {}, {}
    for lid in (1, 2):
        size = tuple(planted[lid][0][3].shape[-2:])
        tpl = torch.rand(T, 3, *size, generator=g).cuda()
        tmask = torch.zeros(T, *size, dtype=torch.uint8).cuda()
        tmask[:, size[0] // 5:size[0] - size[0] // 6, size[1] // 7:size[1] - size[1] // 9] = 1
        for (f, box, m, c, cm, cc), s in zip(planted[lid], slots[lid]):
            tpl[s], tmask[s] = c, cm
        feats, f2t, pts = bank_builder.extract_template_features(ex, tpl, tmask)
        verts = torch.randn(feats.shape[0], 3, generator=g).cuda() * 50.0
        R = workload._random_rotations(len(planted[lid]), g)
        for i, ((f, (x, y, w, h), m, c, cm, cc), s) in enumerate(zip(planted[lid], slots[lid])):
            rows = f2t == s
            K = torch.tensor([[cc.f[0], 0, cc.c[0]], [0, cc.f[1], cc.c[1]], [0, 0, 1.0]], dtype=torch.float64)
            t = torch.tensor([10.0 - 7 * i, -20.0 + 9 * i, 900.0 + 60 * i], dtype=torch.float64)
            verts[rows] = workload.planted_vertices(pts[rows], K, R[i], t).cuda()
            T_m2c = np.eye(4)
            T_m2c[:3, :3], T_m2c[:3, 3] = R[i].numpy(), t.numpy()
            T_m2w = cc.T_world_from_eye @ T_m2c
            annos.setdefault((f, lid), []).append(infer.GtAnnotation("synth", lid, infer.GtPose(T_m2w[:3, :3], T_m2w[:3, 3:]), m,
                                                                     np.array([x, y, x + w, y + h]), np.asarray(0.9)))
        repres[lid] = bank_builder.build_object_repre(feats, f2t, verts, T, pca_components=128, cluster_num=64, cluster_iters=10)
        repres[lid].feat_opts = repre_util.FeatureOpts(extractor_name=NAME)
    repres[3] = repres[2]
    return images, cams, dets, repres, annos


class Split:
    """One built split, shared by the cases of a module run (nothing in it is modified by a run)."""

    def __init__(self, ex, instances=INSTANCES, frame_sizes=((H, W),) * 3, slots=SLOTS, crop=True, targets=TARGETS):
        self.images, self.cams, dets, self.repres, self.annos = _build(ex, instances, frame_sizes, slots, crop)
        self.targets = targets
        self.raw_dets = dets
        self.dets = {}
        for d in dets:
            self.dets.setdefault((d["scene_id"], d["image_id"], d["category_id"]), []).append({k: d[k] for k in ("bbox", "segmentation", "score", "time")})

    def frame(self, f, lids=None, with_gt=False):
        fr = {"scene_id": 1, "im_id": _im_id(f), "image": self.images[f], "camera": self.cams[f]}
        if with_gt:
            fr["gt_annos"] = [a for (f2, lid), al in sorted(self.annos.items()) if f2 == f and (lids is None or lid in lids) for a in al]
        return fr

    def run_both(self, tmp, tag, opts, ex, batch_sizes, with_gt=False, eval_models=None, targets=None):
        """infer() once, infer_batched() per batch size -> (output directory of infer(), [(batch size, output directory of infer_batched)])."""
        n = len(self.images)
        targets = self.targets if targets is None else targets
        per_object = lambda lid: iter([self.frame(f, [lid], with_gt) for f in range(n)])
        ref_dir = str(tmp / f"{tag}_ref")
        ref_paths = infer.infer(opts, per_object, self.dets, self.repres, ref_dir, extractor=ex, num_target_insts=targets, eval_models=eval_models)
        outs = []
        for bs in batch_sizes:
            d = str(tmp / f"{tag}_b{bs}")
            paths = infer.infer_batched(opts, iter([self.frame(f, None, with_gt) for f in range(n)]), self.dets, self.repres, d, batch_detections=bs,
                                        extractor=ex, num_target_insts=targets, eval_models=eval_models)
            assert [os.path.relpath(p, d) for p in paths] == [os.path.relpath(p, ref_dir) for p in ref_paths]
            outs.append((bs, d))
        return ref_dir, outs


def _entries(d, lid):
    return [{k: v for k, v in e.items() if k != "time"} for e in json.load(open(os.path.join(d, str(lid), "estimated-poses.json")))]


def _csv(d):
    rows = open(os.path.join(d, "coarse_synth-estimated-poses.csv")).read().splitlines()
    return [r.rsplit(",", 1)[0] for r in rows]


def _assert_same(ref_dir, outs, counts):
    for lid, want_n in counts.items():
        want = _entries(ref_dir, lid)
        assert len(want) == want_n, (lid, len(want))
        for bs, d in outs:
            got = _entries(d, lid)
            assert len(got) == len(want), (bs, lid)
            for a, b in zip(got, want):
                assert a == b, (bs, lid, a["img_id"], a["inst_id"], [k for k in b if a.get(k) != b[k]])
    for bs, d in outs:
        assert _csv(d) == _csv(ref_dir), bs


@pytest.fixture(scope="module")
def ex32():
    return feature_util.make_feature_extractor(NAME, random_init_seed=SEED_STATE, precision="fp32").to("cuda")


@pytest.fixture(scope="module")
def split(ex32):
    return Split(ex32)


def test_fp32_batched_equals_per_object_for_every_batch_size(tmp_path, ex32, split):
    """Batch size 4: batches straddle frames and objects, the last one is short; 1: a batch per detection; 64: the whole split at once."""
    ref_dir, outs = split.run_both(tmp_path, "fp32", infer.load_opts({"infer_opts": _opts()}), ex32, (4, 1, 64))
    _assert_same(ref_dir, outs, {1: 4, 2: 2, 3: 0})
    e = json.load(open(os.path.join(outs[0][1], "1", "estimated-poses.json")))
    assert [(x["img_id"], x["inst_id"]) for x in e] == [("3", "0"), ("3", "1"), ("4", "0"), ("5", "0")]      # frame order, then instance order
    assert set(e[0]["time"]) == {"prep", "feat_extract", "grid_sample", "proj", "corresp", "pose_coarse", "final_select"}


def test_bf16_batched_equals_per_object(tmp_path, split):
    ex = feature_util.make_feature_extractor(NAME, random_init_seed=SEED_STATE, precision="bf16").to("cuda")
    ref_dir, outs = split.run_both(tmp_path, "bf16", infer.load_opts({"infer_opts": _opts()}), ex, (4, 1, 64))
    _assert_same(ref_dir, outs, {1: 4, 2: 2, 3: 0})


def test_featuremetric_and_ground_truth_evaluation_are_equal_too(tmp_path, ex32, split):
    rng = np.random.default_rng(3)
    model = lambda: eval_util.EvalModel(rng.normal(size=(200, 3)) * 40.0, [{"R": np.eye(3), "t": np.zeros((3, 1))}], 120.0)
    opts = infer.load_opts({"infer_opts": _opts(final_pose_type="featuremetric", refine_iters=10, object_lids=[1, 2])})
    ref_dir, outs = split.run_both(tmp_path, "fm", opts, ex32, (4, 64), with_gt=True, eval_models={1: model(), 2: model()},
                                   targets={lid: TARGETS[lid] for lid in (1, 2)})
    _assert_same(ref_dir, outs, {1: 4, 2: 2})
    e = json.load(open(os.path.join(outs[0][1], "2", "estimated-poses.json")))
    assert all({"mssd", "mspd", "inliers_gt", "inliers_est"} <= set(x) and "pose_refine" in x["time"] for x in e)


def test_without_cropping(tmp_path, ex32):
    """crop=False: the frames themselves go to the extractor (sides are multiples of the patch size)."""
    sizes = ((224, 336),) * 3
    inst = [(0, 1, [20, 30, 150, 160]), (0, 1, [180, 20, 140, 180]), (1, 1, [60, 40, 160, 150]), (2, 1, [150, 30, 170, 170]),
            (1, 2, [10, 50, 150, 150]), (2, 2, [30, 20, 140, 190])]
    sp = Split(ex32, inst, sizes, crop=False)
    opts = infer.load_opts({"infer_opts": {k: v for k, v in _opts(crop=False).items() if k not in ("crop_size", "crop_rel_pad")}})
    ref_dir, outs = sp.run_both(tmp_path, "nocrop", opts, ex32, (4, 64))
    _assert_same(ref_dir, outs, {1: 4, 2: 2, 3: 0})
    # a frame that does not tile into patches is refused like in the per-object driver
    bad = dict(sp.frame(0), image=np.zeros((230, 336, 3), np.uint8), camera=crop_util.PinholePlaneCameraModel(336, 230, (600.0, 600.0), (168.0, 115.0), np.eye(4)))
    dets = {(1, IM_IDS[0], 1): [{"bbox": [30, 40, 120, 160], "score": 0.9, "time": 0.1,
                                 "segmentation": infer_pose_util.binary_mask_to_rle(_mask([30, 40, 120, 160], (230, 336)))}]}
    with pytest.raises(AssertionError, match="not a multiple of patch size"):
        infer.infer_batched(opts, iter([bad]), dets, sp.repres, str(tmp_path / "bad"), batch_detections=4, extractor=ex32, num_target_insts=sp.targets)


def test_a_frame_of_another_size_flushes_on_its_own(tmp_path, ex32, monkeypatch):
    sizes = ((H, W),) * 3 + ((360, 500),)
    inst = INSTANCES + [(3, 1, [40, 60, 160, 150]), (3, 2, [260, 120, 170, 160])]
    slots = {1: SLOTS[1] + [15], 2: SLOTS[2] + [12]}
    targets = {lid: dict(t) for lid, t in TARGETS.items()}
    targets[1][(1, 9)] = targets[2][(1, 9)] = 1
    sp = Split(ex32, inst, sizes, slots, targets=targets)
    seen = []
    real = infer.plan_flush
    monkeypatch.setattr(infer, "plan_flush", lambda q: seen.append([(e.frame_no, e.size) for e in q]) or real(q))
    ref_dir, outs = sp.run_both(tmp_path, "size", infer.load_opts({"infer_opts": _opts()}), ex32, (64,))
    _assert_same(ref_dir, outs, {1: 5, 2: 3, 3: 0})
    assert [len(b) for b in seen] == [6, 2] and {f for f, _ in seen[1]} == {3} and {s for _, s in seen[1]} == {(500, 360)}


def test_cli_batched_writes_the_same_file(tmp_path, ex32, split):
    """`python -m foundpose_amd.infer ... --batch-detections 4` on the split written to disk, in a process of its own, against the in-process
    per-object run; and --vis with it is refused before anything is loaded."""
    from PIL import Image
    from foundpose_amd import synthetic
    from foundpose_amd.vit_config import ARCHS
    sd = synthetic.make_vit_state_dict(ARCHS["vits14-reg"], seed=SEED_STATE)
    torch.save(sd, tmp_path / "weights.pth")
    root = tmp_path / "synth"
    (root / "test" / "000001" / "rgb").mkdir(parents=True)
    cam_json = {}
    for f, im in enumerate(IM_IDS):
        Image.fromarray(split.images[f]).save(root / "test" / "000001" / "rgb" / f"{im:06d}.png")
        c = split.cams[f]
        cam_json[str(im)] = {"cam_K": [c.f[0], 0, c.c[0], 0, c.f[1], c.c[1], 0, 0, 1], "depth_scale": 1.0}
    (root / "test" / "000001" / "scene_camera.json").write_text(json.dumps(cam_json))
    (root / "test_targets_bop19.json").write_text(json.dumps([{"scene_id": s, "im_id": i, "obj_id": lid, "inst_count": n}
                                                                for lid, t in sorted(TARGETS.items()) for (s, i), n in sorted(t.items())]))
    (tmp_path / "cnos.json").write_text(json.dumps(split.raw_dets))
    (tmp_path / "opts.json").write_text(json.dumps({"infer_opts": _opts()}))
    for lid, r in split.repres.items():
        repre_util.save_object_repre(r, repre_util.get_object_repre_dir_path(str(tmp_path / "object_repre"), "v1", "synth", lid))
    argv = [sys.executable, "-m", "foundpose_amd.infer", "--opts", str(tmp_path / "opts.json"), "--dataset-dir", str(root / "test"), "--detections",
            str(tmp_path / "cnos.json"), "--repre-dir", str(tmp_path / "object_repre"), "--precision", "fp32", "--weights", str(tmp_path / "weights.pth"),
            "--batch-detections", "4"]
    bad = subprocess.run(argv + ["--output-dir", str(tmp_path / "out_vis"), "--vis"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "per-object driver" in bad.stderr and not (tmp_path / "out_vis").exists()
    run = subprocess.run(argv + ["--output-dir", str(tmp_path / "out_cli")], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, run.stderr[-2000:]
    # the reference: the per-object driver in this process, on the files' content (the weights file holds the state dict of seed SEED_STATE,
    # which is what random_init_seed=SEED_STATE builds ex32 from)
    ex = feature_util.make_feature_extractor(NAME, state_dict=sd, precision="fp32").to("cuda")
    ref_dir = str(tmp_path / "out_ref")
    loaded = {lid: repre_util.load_object_repre(repre_util.get_object_repre_dir_path(str(tmp_path / "object_repre"), "v1", "synth", lid)) for lid in (1, 2, 3)}
    infer.infer(infer.load_opts(str(tmp_path / "opts.json")), lambda lid: iter([split.frame(f) for f in range(3)]),
                infer_pose_util.load_detections_in_bop_format(str(tmp_path / "cnos.json")), loaded, ref_dir, extractor=ex, num_target_insts=TARGETS)
    _assert_same(ref_dir, [(4, str(tmp_path / "out_cli"))], {1: 4, 2: 2, 3: 0})
