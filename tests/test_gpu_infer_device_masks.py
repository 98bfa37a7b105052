"""infer.infer_batched(device_masks=True) on the synthetic split of tests/test_gpu_infer_batched.py: with the
detections' masks decoded, opened and cropped on the device the batched driver must still write what the per-object driver writes with its
host masks -- every field of estimated-poses.json but the times, and the csv -- whatever the batch size, with ground truth, with
coarse_select_type "mask_verify" (which reads the masks on the device), without cropping, and for detections made on a padded canvas."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import eval_util, feature_util, infer, infer_pose_util as ipu
from tests.test_gpu_infer_batched import H, IM_IDS, NAME, SEED_STATE, TARGETS, W, Split, _assert_same, _opts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex32():
    return feature_util.make_feature_extractor(NAME, random_init_seed=SEED_STATE, precision="fp32").to("cuda")


@pytest.fixture(scope="module")
def split(ex32):
    return Split(ex32)


def _per_object(sp, tmp, tag, opts, ex, dets=None, with_gt=False, eval_models=None, targets=None):
    d = str(tmp / tag)
    n = len(sp.images)
    infer.infer(opts, lambda lid: iter([sp.frame(f, [lid], with_gt) for f in range(n)]), sp.dets if dets is None else dets, sp.repres, d, extractor=ex,
                num_target_insts=sp.targets if targets is None else targets, eval_models=eval_models)
    return d


def _batched(sp, tmp, tag, opts, ex, bs, dets=None, with_gt=False, eval_models=None, targets=None, device_masks=True):
    d = str(tmp / tag)
    n = len(sp.images)
    infer.infer_batched(opts, iter([sp.frame(f, None, with_gt) for f in range(n)]), sp.dets if dets is None else dets, sp.repres, d, batch_detections=bs,
                        extractor=ex, num_target_insts=sp.targets if targets is None else targets, eval_models=eval_models, device_masks=device_masks)
    return d


def test_every_batch_size_writes_the_per_object_drivers_results(tmp_path, ex32, split, monkeypatch):
    """Batch sizes 1, 4 and 64 -- and no full-frame mask is made on the host: select_instances and open_mask_3x3 are never called."""
    opts = infer.load_opts({"infer_opts": _opts()})
    ref = _per_object(split, tmp_path, "ref", opts, ex32)

    def never(*a, **k):
        raise AssertionError("the host mask path ran")
    monkeypatch.setattr(infer, "select_instances", never)
    monkeypatch.setattr(ipu, "open_mask_3x3", never)
    outs = [(bs, _batched(split, tmp_path, f"b{bs}", opts, ex32, bs)) for bs in (1, 4, 64)]
    _assert_same(ref, outs, {1: 4, 2: 2, 3: 0})     # object 2's empty-mask detection and detection-free object 3 are dropped as before


def test_with_ground_truth_and_evaluation(tmp_path, ex32, split):
    """The 0.05 IoU filter, the choice of gt_anno (two annotations of object 1 in the first frame) and the evaluator's mask_iou from device counts
    and device masks."""
    rng = np.random.default_rng(3)
    model = lambda: eval_util.EvalModel(rng.normal(size=(200, 3)) * 40.0, [{"R": np.eye(3), "t": np.zeros((3, 1))}], 120.0)
    models = {1: model(), 2: model()}
    opts = infer.load_opts({"infer_opts": _opts(object_lids=[1, 2])})
    targets = {lid: TARGETS[lid] for lid in (1, 2)}
    ref = _per_object(split, tmp_path, "ref", opts, ex32, with_gt=True, eval_models=models, targets=targets)
    outs = [(bs, _batched(split, tmp_path, f"b{bs}", opts, ex32, bs, with_gt=True, eval_models=models, targets=targets)) for bs in (4, 64)]
    _assert_same(ref, outs, {1: 4, 2: 2})
    e = json.load(open(os.path.join(outs[0][1], "1", "estimated-poses.json")))
    assert all({"mssd", "mspd", "inliers_gt", "inliers_est"} <= set(x) for x in e)


def test_with_mask_verify(tmp_path, ex32, split):
    opts = infer.load_opts({"infer_opts": _opts(coarse_select_type="mask_verify", mask_verify_grid=32, mask_verify_max_points=500)})
    ref = _per_object(split, tmp_path, "ref", opts, ex32)
    _assert_same(ref, [(4, _batched(split, tmp_path, "b4", opts, ex32, 4))], {1: 4, 2: 2, 3: 0})


def test_without_cropping(tmp_path, ex32):
    sizes = ((224, 336),) * 3
    inst = [(0, 1, [20, 30, 150, 160]), (0, 1, [180, 20, 140, 180]), (1, 1, [60, 40, 160, 150]), (2, 1, [150, 30, 170, 170]),
            (1, 2, [10, 50, 150, 150]), (2, 2, [30, 20, 140, 190])]
    sp = Split(ex32, inst, sizes, crop=False)
    opts = infer.load_opts({"infer_opts": {k: v for k, v in _opts(crop=False).items() if k not in ("crop_size", "crop_rel_pad")}})
    ref = _per_object(sp, tmp_path, "ref", opts, ex32)
    _assert_same(ref, [(4, _batched(sp, tmp_path, "b4", opts, ex32, 4))], {1: 4, 2: 2, 3: 0})


def test_a_mask_the_opening_empties_is_dropped_by_both_paths(tmp_path, ex32, split):
    """One more detection of object 1 in the second frame, a 2-pixel-wide bar in the interior: decoded it has 240 pixels, opened none, so it gets
    no pose on either path (the frame's target count is raised to 2, so the detection is among the chosen ones)."""
    bar = np.zeros((H, W), np.uint8)
    bar[200:320, 300:302] = 1
    det = {"bbox": [300, 200, 2, 120], "score": 0.5, "time": 0.25, "segmentation": ipu.binary_mask_to_rle(bar)}
    dets = copy.deepcopy(split.dets)
    dets[(1, IM_IDS[1], 1)].append(det)
    targets = {lid: dict(t) for lid, t in TARGETS.items()}
    targets[1][(1, IM_IDS[1])] = 2
    inst = ipu.instances_on_device({1: [det]}, (W, H))[1][0]
    assert inst["mask_area"] == 0 and not inst["input_mask_modal"].any() and int(ipu.rle_to_binary_mask(det["segmentation"]).sum()) == 240
    opts = infer.load_opts({"infer_opts": _opts()})
    ref = _per_object(split, tmp_path, "ref", opts, ex32, dets=dets, targets=targets)
    _assert_same(ref, [(4, _batched(split, tmp_path, "b4", opts, ex32, 4, dets=dets, targets=targets))], {1: 4, 2: 2, 3: 0})


def _on_canvas(dets, pad_h, pad_w):
    """The detections re-encoded on a canvas pad_w wider and pad_h taller, the frame centred in it."""
    dy, dx = pad_h // 2, pad_w // 2
    out = {}
    for key, lst in dets.items():
        out[key] = []
        for d in lst:
            m = ipu.rle_to_binary_mask(d["segmentation"])
            big = np.zeros((m.shape[0] + pad_h, m.shape[1] + pad_w), np.uint8)
            big[dy:dy + m.shape[0], dx:dx + m.shape[1]] = m
            x, y, w, h = d["bbox"]
            out[key].append(dict(d, bbox=[x + dx, y + dy, w, h], segmentation=ipu.binary_mask_to_rle(big)))
    return out


def test_detections_on_a_padded_canvas(tmp_path, ex32, split):
    """A canvas 8 wider and 6 taller than the frames, boxes shifted by (+4, +3): the host path and the device path both write what the unpadded
    run writes."""
    opts = infer.load_opts({"infer_opts": _opts()})
    padded = _on_canvas(split.dets, 6, 8)
    assert padded[(1, IM_IDS[0], 1)][0]["segmentation"]["size"] == [H + 6, W + 8] and padded[(1, IM_IDS[0], 1)][0]["bbox"] == [64, 53, 170, 150]
    ref = _per_object(split, tmp_path, "ref", opts, ex32)
    outs = [("host", _per_object(split, tmp_path, "host", opts, ex32, dets=padded)),
            ("device", _batched(split, tmp_path, "device", opts, ex32, 4, dets=padded)),
            ("batched host", _batched(split, tmp_path, "bhost", opts, ex32, 4, dets=padded, device_masks=False))]
    _assert_same(ref, outs, {1: 4, 2: 2, 3: 0})


def test_a_canvas_one_pixel_wider_is_refused(tmp_path, ex32, split):
    opts = infer.load_opts({"infer_opts": _opts()})
    with pytest.raises(ValueError, match="odd number of pixels"):
        _batched(split, tmp_path, "odd", opts, ex32, 4, dets=_on_canvas(split.dets, 0, 1))


def test_instances_equal_the_host_path_with_ground_truth():
    """instances_on_device against _instance_from_detection, detection by detection: the mask's bits, its area, the box, the chosen annotation
    (first maximum; annotation 0 when nothing overlaps) and the IoU as the same double -- for partial overlaps, none, ties, an empty mask and
    two canvas sizes in one frame."""
    rng = np.random.default_rng(11)
    h, w = 60, 84
    yy, xx = np.mgrid[:h, :w]
    disc = lambda cy, cx, r: ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).astype(np.uint8)

    class Anno:
        def __init__(self, m):
            self.masks_modal = m
    annos = {1: [Anno(disc(30, 20, 12)), Anno(disc(30, 60, 12)), Anno(disc(30, 60, 12))], 2: [Anno(disc(10, 10, 6))], 3: []}

    def det(m, score, pad=(0, 0)):
        big = np.zeros((h + pad[0], w + pad[1]), np.uint8)
        big[pad[0] // 2:pad[0] // 2 + h, pad[1] // 2:pad[1] // 2 + w] = m
        ys, xs = np.nonzero(big) if big.any() else (np.array([0]), np.array([0]))
        return {"bbox": [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)], "score": score, "time": 0.5,
                "segmentation": ipu.binary_mask_to_rle(big)}
    preds = {1: [det(disc(28, 24, 10), 0.9), det(disc(33, 58, 11) | (rng.random((h, w)) < 0.03), 0.8), det(disc(50, 40, 4), 0.7),
                 det(np.zeros((h, w), np.uint8), 0.6), det(disc(30, 40, 25), 0.5, pad=(4, 2))],
             2: [det(disc(12, 11, 7), 0.9, pad=(4, 2)), det(disc(45, 70, 8), 0.8)],
             3: [det(disc(20, 20, 9), 0.9)]}
    got = ipu.instances_on_device(preds, (w, h), annos)
    assert list(got) == [1, 2, 3]
    for lid, plist in preds.items():
        assert len(got[lid]) == len(plist)
        for g, p_ in zip(got[lid], plist):
            want = ipu._instance_from_detection(p_, (w, h), annos[lid])
            assert set(g) == set(want) | {"mask_area"}
            assert g["input_mask_modal"].is_cuda and g["input_mask_modal"].dtype == torch.uint8
            assert torch.equal(g["input_mask_modal"].cpu(), torch.from_numpy(want["input_mask_modal"]))
            assert g["mask_area"] == int(want["input_mask_modal"].sum())
            assert np.array_equal(g["input_box_amodal"], want["input_box_amodal"]) and g["input_box_amodal"].dtype == want["input_box_amodal"].dtype
            assert g["gt_anno"] is want["gt_anno"] and g["gt_iou"] == want["gt_iou"] and g["time"] == want["time"]
    assert got[1][0]["gt_anno"] is annos[1][0] and got[1][1]["gt_anno"] is annos[1][1] and 0 < got[1][1]["gt_iou"] < 1     # the first of two equal maxima
    assert got[1][2]["gt_anno"] is annos[1][0] and got[1][2]["gt_iou"] == 0.0 and got[3][0]["gt_anno"] is None              # no overlap / no annotation
