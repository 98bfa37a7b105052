"""CNOS-style detection from class-agnostic mask proposals: every proposal of a segmenter is cut out of the frame,
described by the DINOv2 CLS token, scored per object against the CLS descriptors of that object's templates (the mean of the best few
cosine similarities), labelled with the best object and thinned by non-maximum suppression on the tight boxes.  The result has the form of
a CNOS detections file, which infer / infer_batched take as they are.

This stage is the project's own restatement of CNOS's published behaviour (its second half; the segmenter stays outside); the reference
tree has no counterpart.  Every step runs on the device -- ops.detection_masks, ops.mask_boxes, ops.proposal_crops, the ViT,
ops.normalize_rows, ops.proposal_scores, ops.proposal_rank, ops.box_iou, ops.pose_nms_greedy -- with ONE read-back per image.  There is no
CPU path: CPU tensors are refused."""

import json
import os
import time
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, infer_pose_util, ops

MAX_GROUP = 256   # candidates of one (image, object) that reach the suppression: fp_pose_nms_greedy's limit
DETECTOR_FILE = "detector.pth"


class DetectOpts(NamedTuple):
    """Options of the detector ({"detect_opts": {...}}).  version / templates_version / object_dataset / object_lids name the templates and
    the object_repre directories as gen_repre's options do; they are needed by the command line only."""
    version: str = ""
    templates_version: str = ""
    object_dataset: str = ""
    object_lids: Optional[List[int]] = None
    detector_extractor_name: str = "dinov2_version=vitl14-reg_stride=14_facet=token_layer=23_norm=1"   # the final normalised CLS token
    detector_crop_size: int = 224
    detector_topk: int = 5              # similarities averaged per (proposal, object): CNOS's "avg_5"
    detector_min_score: float = 0.2     # proposals whose best object scores below this are dropped
    detector_nms_thresh: float = 0.25   # two detections of one object conflict at a box overlap >= this
    detector_min_area: int = 0          # proposals of fewer pixels are dropped
    detector_max_per_image: int = 100
    detector_batch: int = 32            # crops per ViT forward
    detector_template_stride: int = 1   # every n-th template enters the detector bank


def load_opts(path_or_dict) -> DetectOpts:
    """{"detect_opts": {...}} or the bare dict; unknown keys are an error, as for InferOpts."""
    d = path_or_dict
    if not isinstance(d, dict):
        with open(path_or_dict) as f:
            d = json.load(f)
    return check_opts(DetectOpts(**dict(d.get("detect_opts", d))))


def check_opts(opts: DetectOpts) -> DetectOpts:
    def integer(name, lo, hi=None):
        v = getattr(opts, name)
        if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
            raise ValueError(f"{name} must be an integer in [{lo}, {'inf' if hi is None else hi}], got {v!r}")
    integer("detector_crop_size", 1, _lib.PROPOSAL_MAX_SIZE)
    integer("detector_topk", 1, _lib.PROPOSAL_MAX_K)
    integer("detector_min_area", 0)
    integer("detector_max_per_image", 1)
    integer("detector_batch", 1)
    integer("detector_template_stride", 1)
    for name in ("detector_min_score", "detector_nms_thresh"):
        v = getattr(opts, name)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            raise ValueError(f"{name} must be a number, got {v!r}")
    if not 0.0 < opts.detector_nms_thresh <= 1.0:
        raise ValueError(f"detector_nms_thresh must be in (0, 1], got {opts.detector_nms_thresh!r}")
    return opts


# ---------------------------------------------------------------------------------------------------- descriptors
def _require_device(name: str, t) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} is a device tensor (got {'a CPU tensor' if isinstance(t, torch.Tensor) else type(t).__name__}); there is no CPU path")


def cls_descriptors(extractor, crops: torch.Tensor, batch: int) -> torch.Tensor:
    """crops f32 [P, 3, S, S] in [0, 1] -> L2-normalised CLS descriptors f32 [P, D], `batch` crops per forward.  Nothing is read back."""
    _require_device("crops", crops)
    out = []
    for b0 in range(0, int(crops.shape[0]), batch):
        _, cls = extractor.forward_tokens(crops[b0:b0 + batch])
        out.append(cls.clone() if getattr(extractor, "use_graph", False) else cls)   # (a graph replay hands out its static buffer)
    cls = torch.cat(out) if out else torch.zeros(0, extractor.arch.dim, dtype=torch.float32, device=crops.device)
    return ops.normalize_rows(cls)


def crops_of_masks(images: torch.Tensor, masks: torch.Tensor, crop_size: int, image_index: Optional[torch.Tensor] = None):
    """The cut-outs of `masks` uint8 [P, H, W] out of `images` f32 [n_img, H, W, 3]: -> (crops, status, boxes, area), the three steps the
    query side and the template side share (ops.mask_boxes, ops.proposal_crops)."""
    boxes, area = ops.mask_boxes(masks)
    crops, status = ops.proposal_crops(images, masks, boxes, crop_size, image_index)
    return crops, status, boxes, area


def extractor_name_of(extractor) -> str:
    """The canonical name of an extractor's configuration (feature_util.make_feature_extractor parses it back)."""
    return (f"dinov2_version={extractor.version}_stride={extractor.stride}_facet={extractor.facet}_layer={extractor.layer}"
            f"_norm={int(bool(extractor.apply_norm))}")


def build_detector_bank(extractor, templates_u8: torch.Tensor, masks: torch.Tensor, crop_size: int, template_stride: int = 1,
                        batch: int = 32) -> Dict[str, Any]:
    """The detector bank of one object: templates_u8 uint8 [T, 3, h, w] and masks [T, h, w] (0 / non-zero), on the device.  Every
    template_stride-th template is cut out by its own mask exactly as a proposal is cut out of a frame -- mask_boxes, proposal_crops, CLS,
    normalize_rows -- so a template pasted into a frame gets the template's own descriptor bit for bit.
    -> {"descs" f32 [T', D] normalised (device), "template_ids" int64 [T'], "extractor_name", "crop_size"}."""
    _require_device("templates_u8", templates_u8)
    _require_device("masks", masks)
    if templates_u8.dim() != 4 or templates_u8.shape[1] != 3 or templates_u8.dtype != torch.uint8 or masks.dim() != 3 \
            or masks.shape[0] != templates_u8.shape[0] or tuple(masks.shape[1:]) != tuple(templates_u8.shape[2:]):
        raise ValueError(f"build_detector_bank: templates uint8 [T, 3, h, w] and masks [T, h, w] are needed, got {tuple(templates_u8.shape)} "
                         f"{templates_u8.dtype} and {tuple(masks.shape)}")
    if isinstance(template_stride, bool) or not isinstance(template_stride, int) or template_stride < 1:
        raise ValueError(f"template_stride must be an integer >= 1, got {template_stride!r}")
    ids = torch.arange(0, int(templates_u8.shape[0]), template_stride)
    sel = ids.to(templates_u8.device)
    images = (templates_u8[sel].permute(0, 2, 3, 1).to(torch.float32) / 255.0).contiguous()   # HWC in [0, 1]: _to_device_image's arithmetic
    m = (masks[sel] != 0).to(torch.uint8).contiguous()
    descs = []
    for b0 in range(0, int(ids.shape[0]), batch):   # (crops of `batch` templates at a time: the crop stack never outgrows a ViT batch)
        crops, _, _, _ = crops_of_masks(images[b0:b0 + batch], m[b0:b0 + batch], crop_size)
        descs.append(cls_descriptors(extractor, crops, batch))
    return {"descs": torch.cat(descs) if descs else torch.zeros(0, extractor.arch.dim, dtype=torch.float32, device=templates_u8.device),
            "template_ids": ids.clone(), "extractor_name": extractor_name_of(extractor), "crop_size": int(crop_size)}


def save_detector_bank(bank: Dict[str, Any], repre_dir: str) -> str:
    """-> <repre_dir>/detector.pth, beside repre.pth (which is not touched)."""
    os.makedirs(repre_dir, exist_ok=True)
    path = os.path.join(repre_dir, DETECTOR_FILE)
    torch.save({"descs": bank["descs"].detach().cpu(), "template_ids": bank["template_ids"].cpu(), "extractor_name": bank["extractor_name"],
                "crop_size": int(bank["crop_size"])}, path)
    return path


def load_detector_bank(repre_dir: str, device: str = "cuda") -> Dict[str, Any]:
    path = os.path.join(repre_dir, DETECTOR_FILE)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: run `python -m foundpose_amd.detect onboard` for this object")
    d = torch.load(path, map_location="cpu", weights_only=True)
    d["descs"] = d["descs"].to(device, torch.float32).contiguous()
    return d


class BankSet(NamedTuple):
    """The detector banks of all objects as fp_proposal_scores takes them."""
    lids: List[int]               # object o of the device tables is lids[o]
    descs: torch.Tensor           # f32 [N, D] on the device: the objects' rows back to back
    obj_off: torch.Tensor         # int32 [O + 1] on the device
    template_ids: List[np.ndarray]   # per object: the template id of each of its rows
    max_templates: int
    crop_size: int


def bank_set(banks: Dict[int, Dict[str, Any]]) -> BankSet:
    """{lid: detector bank} -> the device tables, objects in ascending lid order.  Banks of different crop sizes or widths are refused."""
    if not banks:
        raise ValueError("no detector bank")
    lids = sorted(banks)
    sizes = {int(banks[l]["crop_size"]) for l in lids}
    dims = {int(banks[l]["descs"].shape[1]) for l in lids}
    if len(sizes) != 1 or len(dims) != 1:
        raise ValueError(f"the detector banks disagree: crop sizes {sorted(sizes)}, descriptor widths {sorted(dims)}")
    for l in lids:
        _require_device(f"the descriptors of object {l}", banks[l]["descs"])
    counts = [int(banks[l]["descs"].shape[0]) for l in lids]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    descs = torch.cat([banks[l]["descs"].to(torch.float32) for l in lids]).contiguous()
    return BankSet(lids, descs, _lib.upload_async(torch.from_numpy(off), descs.device), [np.asarray(banks[l]["template_ids"]).astype(np.int64) for l in lids],
                   max(max(counts), 1), sizes.pop())


# ---------------------------------------------------------------------------------------------------- one image
def _proposal_key(p_: Dict[str, Any]) -> Tuple[int, int]:
    return int(p_.get("scene_id", 0)), int(p_.get("image_id", 0))


def label_proposals(opts: DetectOpts, image, proposals: Sequence[Dict[str, Any]], banks, extractor):
    """The detections of ONE image.  image: HWC uint8 or float in [0, 1] (numpy or tensor; infer._to_device_image's inputs); proposals:
    CNOS-shaped records of which "segmentation" (COCO RLE on a canvas of the image's size), "scene_id", "image_id" and "time" are read and
    "category_id", "score", "bbox" are ignored; banks: {lid: detector bank} or a bank_set() of them.
    Steps: masks (ops.detection_masks, no opening) -> boxes and areas -> crops -> CLS in chunks of detector_batch -> scores -> per proposal
    the first of: "small" (area < detector_min_area), "empty" (no pixel), "no_object", "low_score" (best score < detector_min_score),
    "group_limit" (rank >= 256 in its (image, object) group: score descending, equal scores in input order) -> box overlaps of all pairs
    of a group and greedy suppression at overlap >= detector_nms_thresh ("suppressed") -> the best detector_max_per_image by score, equal
    scores in input order ("max_per_image") -> "kept".  One read-back.  A dropped proposal still rides through the crops and the ViT: the
    batch is not compacted, that would need a second read-back.
    -> (detections: {(scene_id, image_id, category_id): [{"bbox" [x, y, w, h] of the tight box, "segmentation" (the proposal's own RLE,
    unchanged), "score", "time" (the proposal's own plus this call's wall time)}]} in the form of load_detections_in_bop_format, kept
    detections in score order; decisions: one per proposal {"proposal", "decision", "category_id", "score", "template_id", "area", "bbox",
    "suppressed_by"})."""
    from .infer import _to_device_image
    t0 = time.perf_counter()
    opts = check_opts(opts)
    bs = banks if isinstance(banks, BankSet) else bank_set(banks)
    if bs.crop_size != opts.detector_crop_size:
        raise ValueError(f"the detector banks were cut at {bs.crop_size} pixels, detector_crop_size is {opts.detector_crop_size}")
    if len(proposals) == 0:
        return {}, []
    if len(proposals) > _lib.PROPOSAL_MAX_RANKED:
        raise ValueError(f"{len(proposals)} proposals in one image: at most {_lib.PROPOSAL_MAX_RANKED}")
    img = _to_device_image(image)
    if img.dim() != 3 or img.shape[2] != 3:
        raise ValueError(f"the image must be [H, W, 3], got {tuple(img.shape)}")
    H, W = int(img.shape[0]), int(img.shape[1])
    counts, run_off, canvas = infer_pose_util.pack_rle(proposals)   # (refuses proposals of different canvases)
    if tuple(canvas) != (H, W):
        raise ValueError(f"the proposals lie on a canvas of {canvas[1]} x {canvas[0]}, the image is {W} x {H}")
    P, O = len(proposals), len(bs.lids)
    dev = img.device
    table = _lib.upload_async(torch.from_numpy(np.concatenate([counts, run_off])), dev)
    masks, _ = ops.detection_masks(table[:counts.size], table[counts.size:], (H, W), (H, W), open3x3=False)
    image_index = torch.zeros(P, dtype=torch.int32, device=dev)
    crops, status, boxes, area = crops_of_masks(img.contiguous()[None], masks, opts.detector_crop_size, image_index)
    desc_n = cls_descriptors(extractor, crops, opts.detector_batch)
    _, best_obj, best_score, best_tpl = ops.proposal_scores(desc_n, bs.descs, bs.obj_off, bs.max_templates, opts.detector_topk)
    decision, order, group_off, pair_off, pairs, ranked = ops.proposal_rank(best_obj, best_score, area, status, boxes, O, opts.detector_min_area,
                                                                            float(opts.detector_min_score), MAX_GROUP)
    overlap, pstatus = ops.box_iou(ranked, pairs)
    keep, by = ops.pose_nms_greedy(group_off, pair_off, pairs, overlap, pstatus, P, float(opts.detector_nms_thresh))
    sat = extractor.saturation_snapshot() if hasattr(extractor, "saturation_snapshot") else None
    ints = [decision, order, keep, by, best_obj, best_tpl, area, boxes.flatten(), best_score.view(torch.int32)]
    back = torch.cat(ints + ([sat.to(torch.int32).flatten()] if sat is not None else [])).cpu().numpy()   # the image's one read-back
    decision, order, keep, by, best_obj, best_tpl, area = (back[i * P:(i + 1) * P] for i in range(7))
    boxes_h = back[7 * P:11 * P].reshape(P, 4)
    score_h = back[11 * P:12 * P].view(np.float32)
    if sat is not None:
        extractor.report_saturation(int(back[12 * P]), int(back[12 * P + 1]))
    return _select(opts, proposals, bs, decision, order, keep, by, best_obj, best_tpl, area, boxes_h, score_h, t0)


def _select(opts, proposals, bs, decision, order, keep, by, best_obj, best_tpl, area, boxes, score, t0):
    """The host half of label_proposals: names for the device's decisions, the cut at detector_max_per_image, the records."""
    P = len(proposals)
    names = [_lib.PROPOSAL_DECISIONS[int(d)] for d in decision]
    suppressed_by = [-1] * P
    survivors = []
    for place in range(P):
        p = int(order[place])
        if p < 0:
            break   # behind the last candidate
        if keep[place]:
            survivors.append(p)
        else:
            names[p], suppressed_by[p] = "suppressed", int(order[int(by[place])])
    survivors.sort(key=lambda p: (-float(score[p]), p))   # score descending, equal scores in input order
    for p in survivors[:opts.detector_max_per_image]:
        names[p] = "kept"
    for p in survivors[opts.detector_max_per_image:]:
        names[p] = "max_per_image"
    elapsed = time.perf_counter() - t0
    detections: Dict[Tuple[int, int, int], List[Dict[str, Any]]] = {}
    decisions = []
    for p, p_ in enumerate(proposals):
        o = int(best_obj[p])
        lid = bs.lids[o] if 0 <= o < len(bs.lids) else None
        x1, y1, x2, y2 = (int(v) for v in boxes[p])
        tpl = int(bs.template_ids[o][int(best_tpl[p])]) if lid is not None and 0 <= int(best_tpl[p]) < len(bs.template_ids[o]) else -1
        s = float(score[p])
        decisions.append({"proposal": p, "decision": names[p], "category_id": lid, "score": s if np.isfinite(s) else None, "template_id": tpl,
                          "area": int(area[p]), "bbox": [x1, y1, x2 - x1, y2 - y1], "suppressed_by": suppressed_by[p]})
    for p in survivors[:opts.detector_max_per_image]:
        p_ = proposals[p]
        key = _proposal_key(p_) + (decisions[p]["category_id"],)
        detections.setdefault(key, []).append({"bbox": decisions[p]["bbox"], "segmentation": p_["segmentation"], "score": decisions[p]["score"],
                                               "time": float(p_.get("time", 0.0)) + elapsed})
    return detections, decisions


def detections_to_list(detections: Dict[Tuple[int, int, int], List[Dict[str, Any]]]) -> List[Dict[str, Any]]:
    """The detections dict -> the record list of a CNOS file (load_detections_in_bop_format reads it back into the same dict)."""
    return [{"scene_id": k[0], "image_id": k[1], "category_id": k[2], "bbox": d["bbox"], "score": d["score"], "time": d["time"],
             "segmentation": d["segmentation"]} for k, ds in detections.items() for d in ds]
