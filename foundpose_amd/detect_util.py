"""CNOS-style detection from class-agnostic mask proposals: every proposal of a segmenter is cut out of the frame,
described by the DINOv2 CLS token, scored per object against the CLS descriptors of that object's templates (the mean of the best few
cosine similarities), labelled with the best object and thinned by non-maximum suppression on the tight boxes.  The result has the form of
a CNOS detections file, which infer / infer_batched take as they are.

This stage is the project's own restatement of CNOS's published behaviour (its second half; the segmenter stays outside); the reference
tree has no counterpart.  Every step runs on the device -- ops.detection_masks, ops.mask_boxes, ops.proposal_crops, the ViT,
ops.normalize_rows, ops.proposal_scores, ops.proposal_rank, ops.box_iou, ops.pose_nms_greedy -- with ONE read-back per image.  There is no
CPU path: CPU tensors are refused.

detector_score_type "semantic_appearance"  adds the patch-descriptor score of CNOS's later versions and of SAM-6D:
ops.proposal_patch_cover says which ViT patches of the cut-out the mask covers, ops.proposal_appearance gives every covered patch its best
cosine match among the covered patches of the proposal's best template and averages them, and the mean of the two scores is what the
threshold, the ranking and the detections file see.  The default, "semantic", is the path it was."""

import json
import math
import os
import time
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, infer_pose_util, ops

MAX_GROUP = 256   # candidates of one (image, object) that reach the suppression: fp_pose_nms_greedy's limit
DETECTOR_FILE = "detector.pth"
DETECTOR_PATCH_FILE = "detector_patches.pth"   # the patch tables of the appearance score (section 25), beside detector.pth
SCORE_TYPES = ("semantic", "semantic_appearance")


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
    detector_score_type: str = "semantic"   # "semantic": the CLS score alone; "semantic_appearance": its mean with the patch score (section 25)
    detector_patch_min_cover: float = 0.5   # a patch counts when the mask covers at least this share of its pixels, in (0, 1]


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
    if opts.detector_score_type not in SCORE_TYPES:
        raise ValueError(f"detector_score_type must be one of {SCORE_TYPES}, got {opts.detector_score_type!r}")
    v = opts.detector_patch_min_cover
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < v <= 1.0:
        raise ValueError(f"detector_patch_min_cover must be a number in (0, 1], got {v!r}")
    return opts


def min_cover_pixels(cover: float, patch_size: int) -> int:
    """detector_patch_min_cover as the pixel count fp_proposal_appearance takes: max(1, ceil(cover * patch_size^2))."""
    return max(1, int(math.ceil(float(cover) * patch_size * patch_size)))


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


def patch_descriptors(extractor, crops: torch.Tensor, batch: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """cls_descriptors' sibling for the appearance score: crops f32 [P, 3, S, S] -> (L2-normalised CLS descriptors f32 [P, D], L2-normalised
    patch descriptors f32 [P, Np, D] in token order) from the same forwards.  Nothing is read back."""
    _require_device("crops", crops)
    graph = getattr(extractor, "use_graph", False)   # (a graph replay hands out its static buffers)
    cls_out, patch_out = [], []
    for b0 in range(0, int(crops.shape[0]), batch):
        fmap, cls = extractor.forward_tokens(crops[b0:b0 + batch])
        cls_out.append(cls.clone() if graph else cls)
        patch_out.append(fmap.clone() if graph else fmap)
    if not cls_out:
        g = int(crops.shape[2]) // patch_size_of(extractor)
        D = extractor.arch.dim
        return (torch.zeros(0, D, dtype=torch.float32, device=crops.device), torch.zeros(0, g * g, D, dtype=torch.float32, device=crops.device))
    patches = torch.cat(patch_out)
    P, Np, D = (int(v) for v in patches.shape)
    return ops.normalize_rows(torch.cat(cls_out)), ops.normalize_rows(patches.reshape(P * Np, D)).view(P, Np, D)


def patch_size_of(extractor) -> int:
    """The side of a ViT patch in crop pixels; the appearance score needs one token per patch cell (stride = patch size)."""
    ps = int(extractor.patch_size)
    if int(getattr(extractor, "stride", ps)) != ps:
        raise ValueError(f"the appearance score needs an extractor of stride = patch size ({ps}), got stride {extractor.stride}")
    return ps


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
                        batch: int = 32, with_patches: bool = False) -> Dict[str, Any]:
    """The detector bank of one object: templates_u8 uint8 [T, 3, h, w] and masks [T, h, w] (0 / non-zero), on the device.  Every
    template_stride-th template is cut out by its own mask exactly as a proposal is cut out of a frame -- mask_boxes, proposal_crops, CLS,
    normalize_rows -- so a template pasted into a frame gets the template's own descriptor bit for bit.
    -> {"descs" f32 [T', D] normalised (device), "template_ids" int64 [T'], "extractor_name", "crop_size"}.
    with_patches: also "patch_descs" f32 [T', Np, D] (the normalised patch tokens of the same forwards), "patch_cover" int32 [T', Np]
    (ops.proposal_patch_cover of the template's own mask) and "patch_size", by the calls the query side uses: a pasted template's patches
    are its template's bit for bit.  The patch table takes T' Np D 4 bytes -- 1 MB per template at ViT-L and 224 pixels -- and
    detector_template_stride is the lever."""
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
    descs, pdescs, pcover = [], [], []
    ps = patch_size_of(extractor) if with_patches else 0
    if with_patches and int(crop_size) % ps:
        raise ValueError(f"the appearance score needs a crop size that is a multiple of the patch size {ps}, got {crop_size}")
    for b0 in range(0, int(ids.shape[0]), batch):   # (crops of `batch` templates at a time: the crop stack never outgrows a ViT batch)
        crops, _, boxes, _ = crops_of_masks(images[b0:b0 + batch], m[b0:b0 + batch], crop_size)
        if with_patches:
            cls_n, patches_n = patch_descriptors(extractor, crops, batch)
            descs.append(cls_n)
            pdescs.append(patches_n)
            pcover.append(ops.proposal_patch_cover(m[b0:b0 + batch], boxes, crop_size, ps))
        else:
            descs.append(cls_descriptors(extractor, crops, batch))
    dev, D = templates_u8.device, extractor.arch.dim
    bank = {"descs": torch.cat(descs) if descs else torch.zeros(0, D, dtype=torch.float32, device=dev),
            "template_ids": ids.clone(), "extractor_name": extractor_name_of(extractor), "crop_size": int(crop_size)}
    if with_patches:
        Np = (int(crop_size) // ps) ** 2
        bank["patch_descs"] = torch.cat(pdescs) if pdescs else torch.zeros(0, Np, D, dtype=torch.float32, device=dev)
        bank["patch_cover"] = torch.cat(pcover) if pcover else torch.zeros(0, Np, dtype=torch.int32, device=dev)
        bank["patch_size"] = ps
    return bank


def save_detector_bank(bank: Dict[str, Any], repre_dir: str) -> str:
    """-> <repre_dir>/detector.pth, beside repre.pth (which is not touched).  A bank with patch tables also writes them, to
    <repre_dir>/detector_patches.pth: detector.pth keeps its format.  A bank without them REMOVES a detector_patches.pth that an earlier
    onboarding left there: its tables belong to another detector.pth (other weights or another precision do not show in any field)."""
    os.makedirs(repre_dir, exist_ok=True)
    path = os.path.join(repre_dir, DETECTOR_FILE)
    ppath = os.path.join(repre_dir, DETECTOR_PATCH_FILE)
    torch.save({"descs": bank["descs"].detach().cpu(), "template_ids": bank["template_ids"].cpu(), "extractor_name": bank["extractor_name"],
                "crop_size": int(bank["crop_size"])}, path)
    if "patch_descs" in bank:
        torch.save({"patch_descs": bank["patch_descs"].detach().cpu(), "patch_cover": bank["patch_cover"].detach().cpu(),
                    "patch_size": int(bank["patch_size"]), "template_ids": bank["template_ids"].cpu(), "extractor_name": bank["extractor_name"],
                    "crop_size": int(bank["crop_size"])}, ppath)
    elif os.path.exists(ppath):
        os.remove(ppath)
    return path


def load_detector_bank(repre_dir: str, device: str = "cuda", with_patches: bool = False) -> Dict[str, Any]:
    path = os.path.join(repre_dir, DETECTOR_FILE)
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: run `python -m foundpose_amd.detect onboard` for this object")
    d = torch.load(path, map_location="cpu", weights_only=True)
    d["descs"] = d["descs"].to(device, torch.float32).contiguous()
    if with_patches:
        ppath = os.path.join(repre_dir, DETECTOR_PATCH_FILE)
        if not os.path.exists(ppath):
            raise FileNotFoundError(f"{ppath} is missing: run `python -m foundpose_amd.detect onboard` with detector_score_type "
                                    f"\"semantic_appearance\" for this object")
        e = torch.load(ppath, map_location="cpu", weights_only=True)
        if e["template_ids"].tolist() != d["template_ids"].tolist() or int(e["crop_size"]) != int(d["crop_size"]) \
                or e.get("extractor_name") != d["extractor_name"]:
            raise ValueError(f"{ppath} and {path} were not written together: onboard the object again")
        d["patch_descs"] = e["patch_descs"].to(device, torch.float32).contiguous()
        d["patch_cover"] = e["patch_cover"].to(device, torch.int32).contiguous()
        d["patch_size"] = int(e["patch_size"])
    return d


class BankSet(NamedTuple):
    """The detector banks of all objects as fp_proposal_scores takes them."""
    lids: List[int]               # object o of the device tables is lids[o]
    descs: torch.Tensor           # f32 [N, D] on the device: the objects' rows back to back
    obj_off: torch.Tensor         # int32 [O + 1] on the device
    template_ids: List[np.ndarray]   # per object: the template id of each of its rows
    max_templates: int
    crop_size: int
    patch_descs: Optional[torch.Tensor] = None   # f32 [N, Np, D] on the device, rows as descs: only when every bank has patch tables
    patch_cover: Optional[torch.Tensor] = None   # int32 [N, Np]


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
    pd = pc = None
    if all("patch_descs" in banks[l] and "patch_cover" in banks[l] for l in lids):
        shapes = {tuple(banks[l]["patch_descs"].shape[1:]) for l in lids}
        if len(shapes) != 1:
            raise ValueError(f"the detector banks disagree: patch tables of {sorted(shapes)}")
        for l in lids:
            _require_device(f"the patch descriptors of object {l}", banks[l]["patch_descs"])
            _require_device(f"the patch coverage of object {l}", banks[l]["patch_cover"])
        pd = torch.cat([banks[l]["patch_descs"].to(torch.float32) for l in lids]).contiguous()
        pc = torch.cat([banks[l]["patch_cover"].to(torch.int32) for l in lids]).contiguous()
    return BankSet(lids, descs, _lib.upload_async(torch.from_numpy(off), descs.device), [np.asarray(banks[l]["template_ids"]).astype(np.int64) for l in lids],
                   max(max(counts), 1), sizes.pop(), pd, pc)


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
    With detector_score_type "semantic_appearance" (banks with patch tables; else ValueError): behind the scores, the patch coverage of
    every cut-out, the patch descriptors of the same forwards and ops.proposal_appearance; "score" is then the mean of the CLS score and
    the appearance score everywhere -- threshold, ranking, suppression order, records -- and a decision also holds "semantic_score",
    "appearance_score" (None unless the appearance status is 0) and "valid_patches".  Still one read-back.
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
    appearance = opts.detector_score_type == "semantic_appearance"
    if appearance and (bs.patch_descs is None or bs.patch_cover is None):
        raise ValueError("detector_score_type \"semantic_appearance\" needs detector banks with patch tables: run `python -m foundpose_amd.detect "
                         "onboard` with this option (build_detector_bank / load_detector_bank with_patches=True)")
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
    extra = []
    if appearance:
        ps = patch_size_of(extractor)
        if opts.detector_crop_size % ps or (opts.detector_crop_size // ps) ** 2 != int(bs.patch_descs.shape[1]):
            raise ValueError(f"the detector banks hold {int(bs.patch_descs.shape[1])} patches per template, a crop of {opts.detector_crop_size} pixels "
                             f"at patch size {ps} does not")
        q_cover = ops.proposal_patch_cover(masks, boxes, opts.detector_crop_size, ps, image_index, 1)
        desc_n, patches_n = patch_descriptors(extractor, crops, opts.detector_batch)
        _, best_obj, semantic, best_tpl = ops.proposal_scores(desc_n, bs.descs, bs.obj_off, bs.max_templates, opts.detector_topk)
        best_score, app, n_valid, app_status, _, _ = ops.proposal_appearance(patches_n, q_cover, bs.patch_descs, bs.patch_cover, bs.obj_off, best_obj, best_tpl,
                                                                             semantic, min_cover_pixels(opts.detector_patch_min_cover, ps))
        extra = [semantic.view(torch.int32), app.view(torch.int32), n_valid, app_status]   # ride in the image's one read-back
    else:
        desc_n = cls_descriptors(extractor, crops, opts.detector_batch)
        _, best_obj, best_score, best_tpl = ops.proposal_scores(desc_n, bs.descs, bs.obj_off, bs.max_templates, opts.detector_topk)
    decision, order, group_off, pair_off, pairs, ranked = ops.proposal_rank(best_obj, best_score, area, status, boxes, O, opts.detector_min_area,
                                                                            float(opts.detector_min_score), MAX_GROUP)
    overlap, pstatus = ops.box_iou(ranked, pairs)
    keep, by = ops.pose_nms_greedy(group_off, pair_off, pairs, overlap, pstatus, P, float(opts.detector_nms_thresh))
    sat = extractor.saturation_snapshot() if hasattr(extractor, "saturation_snapshot") else None
    ints = [decision, order, keep, by, best_obj, best_tpl, area, boxes.flatten(), best_score.view(torch.int32)] + extra
    back = torch.cat(ints + ([sat.to(torch.int32).flatten()] if sat is not None else [])).cpu().numpy()   # the image's one read-back
    decision, order, keep, by, best_obj, best_tpl, area = (back[i * P:(i + 1) * P] for i in range(7))
    boxes_h = back[7 * P:11 * P].reshape(P, 4)
    score_h = back[11 * P:12 * P].view(np.float32)
    n_cols = 12 + len(extra)
    if sat is not None:
        extractor.report_saturation(int(back[n_cols * P]), int(back[n_cols * P + 1]))
    if not appearance:
        return _select(opts, proposals, bs, decision, order, keep, by, best_obj, best_tpl, area, boxes_h, score_h, t0)
    return _select(opts, proposals, bs, decision, order, keep, by, best_obj, best_tpl, area, boxes_h, score_h, t0,
                   semantic=back[12 * P:13 * P].view(np.float32), appearance=back[13 * P:14 * P].view(np.float32), valid_patches=back[14 * P:15 * P],
                   appearance_status=back[15 * P:16 * P])


def _select(opts, proposals, bs, decision, order, keep, by, best_obj, best_tpl, area, boxes, score, t0, *, semantic=None, appearance=None,
            valid_patches=None, appearance_status=None):
    """The host half of label_proposals: names for the device's decisions, the cut at detector_max_per_image, the records.  With the
    appearance score `score` is the combined one and the records also name its two parts."""
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
        if semantic is not None:
            sem = float(semantic[p])
            decisions[-1].update({"semantic_score": sem if np.isfinite(sem) else None,
                                  "appearance_score": float(appearance[p]) if int(appearance_status[p]) == 0 else None,
                                  "valid_patches": int(valid_patches[p])})
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
