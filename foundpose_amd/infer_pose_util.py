"""Detections in, object instances out: the input side of the driver, with the reference's function names
(/root/reference/utils/infer_pose_util.py:24-151).  CNOS/BOP detection files are JSON lists of
{scene_id, image_id, category_id, bbox [x, y, w, h], segmentation (COCO RLE), score, time}.

The reference decodes the RLE with bop_toolkit's pycoco_utils and opens the mask with cv2.morphologyEx; neither package
is a dependency here: the RLE codec is restated (uncompressed counts lists as CNOS writes them, and COCO's compressed
strings), the 3x3 opening is two pooling passes with cv2's border rules (erosion ignores the outside, dilation too)."""

import json
from collections import defaultdict
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops


def load_detections_in_bop_format(path: str) -> Dict[Tuple[int, int, int], List[Dict[str, Any]]]:
    with open(path) as f:
        pred_mask_list = json.load(f)
    detections = defaultdict(list)
    for pred in pred_mask_list:
        key = (pred["scene_id"], pred["image_id"], pred["category_id"])
        detections[key].append({"bbox": pred["bbox"], "segmentation": pred["segmentation"], "score": pred["score"], "time": pred["time"]})
    return detections


def _decode_compressed_counts(s: str) -> List[int]:
    """COCO's LEB128-like string form of the run lengths (pycocotools rleFrString)."""
    counts, p, m = [], 0, 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if m > 2:
            x += counts[m - 2]
        counts.append(x)
        m += 1
    return counts


def rle_to_binary_mask(rle: Dict[str, Any]) -> np.ndarray:
    """COCO RLE {"counts", "size": [h, w]} -> bool [h, w]; runs alternate 0/1 starting with 0, column-major."""
    h, w = rle["size"]
    counts = rle["counts"]
    if isinstance(counts, (str, bytes)):
        counts = _decode_compressed_counts(counts.decode() if isinstance(counts, bytes) else counts)
    flat = np.zeros(h * w, dtype=bool)
    pos, val = 0, False
    for c in counts:
        if val:
            flat[pos:pos + c] = True
        pos += c
        val = not val
    return flat.reshape((h, w), order="F")


def binary_mask_to_rle(mask: np.ndarray) -> Dict[str, Any]:
    """Inverse of rle_to_binary_mask (uncompressed counts), the form CNOS result files use."""
    flat = np.asarray(mask).astype(bool).ravel(order="F")
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    edges = np.concatenate([[0], change, [flat.size]])
    counts = np.diff(edges).tolist()
    if flat.size and flat[0]:
        counts = [0] + counts
    return {"counts": counts, "size": [int(mask.shape[0]), int(mask.shape[1])]}


def open_mask_3x3(mask: np.ndarray) -> np.ndarray:
    """cv2.morphologyEx(mask, MORPH_OPEN, 3x3 rect): erosion then dilation; pixels outside the image never win (cv2's
    default border value for each of the two passes)."""
    m = torch.as_tensor(np.asarray(mask) != 0, dtype=torch.float32)[None, None]
    er = 1.0 - torch.nn.functional.max_pool2d(torch.nn.functional.pad(1.0 - m, (1, 1, 1, 1), value=0.0), 3, 1)
    di = torch.nn.functional.max_pool2d(torch.nn.functional.pad(er, (1, 1, 1, 1), value=0.0), 3, 1)
    return di[0, 0].numpy().astype(np.uint8)


def mask_iou(a: np.ndarray, b: np.ndarray) -> float:
    a, b = np.asarray(a).astype(bool), np.asarray(b).astype(bool)
    union = np.logical_or(a, b).sum()
    return float(np.logical_and(a, b).sum() / union) if union else 0.0


def _centre_crop_offsets(canvas_wh: Tuple[int, int], image_wh: Tuple[int, int]) -> np.ndarray:
    """(dx, dy) of an image that was centre-cropped out of the detector's canvas (e.g. to a multiple of the ViT patch size); the image can
    never be larger than the canvas the masks were predicted on."""
    canvas, image = np.asarray(canvas_wh, np.int64), np.asarray(image_wh, np.int64)
    if np.any(image > canvas):
        raise ValueError("Image is larger than mask.")
    return (canvas - image) // 2


def _best_overlap(mask: np.ndarray, annos: Sequence[Any]) -> Tuple[Optional[Any], float]:
    """The annotation whose modal mask overlaps `mask` most (first one on ties, annotation 0 when nothing overlaps) and that IoU; all IoUs in
    one vectorised pass over the stacked annotation masks."""
    if len(annos) == 0:
        return None, 0.0
    m = np.asarray(mask).astype(bool)
    stack = np.stack([np.asarray(a.masks_modal).astype(bool) for a in annos])
    inter = np.logical_and(stack, m[None]).reshape(len(annos), -1).sum(1)
    union = np.logical_or(stack, m[None]).reshape(len(annos), -1).sum(1)
    ious = np.where(union > 0, inter / np.maximum(union, 1), 0.0)
    best = int(np.argmax(ious)) if float(ious.max()) > 0.0 else 0    # argmax returns the first maximum, like a strict `>` scan
    return annos[best], float(ious[best]) if float(ious.max()) > 0.0 else 0.0


def _box_in_image(pred: Dict[str, Any], dx, dy) -> np.ndarray:
    """A CNOS box (x, y, w, h) on the detector's canvas -> (x1, y1, x2, y2) in the image, dtype of the input kept."""
    x, y, w, h = np.array(pred["bbox"])
    box = np.array(pred["bbox"])
    box[:] = (x - dx, y - dy, x - dx + w, y - dy + h)
    return box


def _instance_from_detection(pred: Dict[str, Any], image_size: Tuple[int, int], gt_object_annos: Sequence[Any]) -> Dict[str, Any]:
    """One CNOS detection -> the instance record of the driver: opened modal mask and amodal box, both moved into the (possibly
    centre-cropped) image, plus the best-overlapping annotation when ground truth is given."""
    mask = open_mask_3x3(rle_to_binary_mask(pred["segmentation"]).astype(np.uint8))
    dx, dy = _centre_crop_offsets((mask.shape[1], mask.shape[0]), image_size)
    # (the reference slices [shift:-shift], which empties the mask when the shift is 0; a zero shift is a no-op here)
    mask = mask[dy:mask.shape[0] - dy, dx:mask.shape[1] - dx]
    box = _box_in_image(pred, dx, dy)
    gt_anno, gt_iou = _best_overlap(mask, gt_object_annos)
    return {"input_box_amodal": box, "input_mask_modal": mask, "gt_anno": gt_anno, "gt_iou": gt_iou, "time": pred["time"]}


def get_instances_for_pose_estimation(bop_chunk_id: int, bop_im_id: int, obj_id: int, use_detections: bool, detections: Dict[Any, Any],
                                      max_num_preds: int, gt_object_annos: Sequence[Any], image_size: Tuple[int, int]) -> List[Dict[str, Any]]:
    """Per-instance dicts {input_box_amodal (x1, y1, x2, y2), input_mask_modal uint8 [H, W], gt_anno, gt_iou, time}: the interface of
    /root/reference/utils/infer_pose_util.py:44-151.  With detections: the max_num_preds best-scoring ones of (scene, image, object) -- a
    single detection is kept whatever max_num_preds says, as in the reference -- else one instance per ground-truth annotation."""
    if not use_detections:
        return [{"input_box_amodal": np.array(a.boxes_amodal).copy(), "input_mask_modal": np.array(a.masks_modal).copy(), "gt_anno": a}
                for a in gt_object_annos]
    preds = detections.get((bop_chunk_id, bop_im_id, obj_id))
    if preds is None:
        return []
    return [_instance_from_detection(p_, image_size, gt_object_annos) for p_ in _top_predictions(preds, max_num_preds)]


def _top_predictions(preds: Sequence[Dict[str, Any]], max_num_preds: int) -> Sequence[Dict[str, Any]]:
    """The max_num_preds best-scoring detections, best first; a single detection is kept whatever max_num_preds says."""
    if len(preds) > 1:
        order = sorted(range(len(preds)), key=lambda i: preds[i]["score"], reverse=True)   # stable: equal scores keep their file order
        preds = [preds[i] for i in order[:max_num_preds]]
    return preds


# ---------------------------------------------------------------------------------------------------- masks decoded on the device
def pack_rle(preds: Sequence[Dict[str, Any]]) -> Tuple[np.ndarray, np.ndarray, Tuple[int, int]]:
    """The run lengths of detections that share one canvas, for ops.detection_masks: -> (counts int32 [R_total], the runs back to back;
    run_off int32 [len(preds) + 1], where each detection's runs start; (hc, wc)).  A detection is a CNOS record (its "segmentation" is
    read) or the RLE dict itself; compressed COCO strings are expanded on the host.  Refused: no detection, a negative run, a detection
    whose runs add up to more than 2^31 - 1, detections of different sizes (the caller groups by size)."""
    if len(preds) == 0:
        raise ValueError("pack_rle: no detection")
    runs, size = [], None
    for i, p_ in enumerate(preds):
        rle = p_.get("segmentation", p_)
        counts = rle["counts"]
        if isinstance(counts, (str, bytes)):
            counts = _decode_compressed_counts(counts.decode() if isinstance(counts, bytes) else counts)
        c = np.asarray(counts, dtype=np.int64).reshape(-1)
        if c.size and int(c.min()) < 0:
            raise ValueError(f"pack_rle: detection {i} has a negative run length ({int(c.min())})")
        if int(c.sum()) > 2**31 - 1:
            raise ValueError(f"pack_rle: the runs of detection {i} add up to {int(c.sum())} (at most 2^31 - 1)")
        hw = (int(rle["size"][0]), int(rle["size"][1]))
        if size is not None and hw != size:
            raise ValueError(f"pack_rle: detection {i} is on a canvas of {hw}, the ones before it on {size}: pack one size at a time")
        size = hw
        runs.append(c)
    run_off = np.zeros(len(runs) + 1, np.int64)
    np.cumsum([c.size for c in runs], out=run_off[1:])
    if int(run_off[-1]) > 2**31 - 1:
        raise ValueError(f"pack_rle: {int(run_off[-1])} runs in one pack (at most 2^31 - 1)")
    return np.concatenate(runs).astype(np.int32), run_off.astype(np.int32), size


def _device_crop_offsets(canvas_hw: Tuple[int, int], image_size: Tuple[int, int]) -> np.ndarray:
    """_centre_crop_offsets for the device path, which also refuses an odd difference: the host path's [dy : hc - dy] slice then returns a
    mask one pixel larger than the image -- an accident, not a contract."""
    hc, wc = canvas_hw
    d = _centre_crop_offsets((wc, hc), image_size)
    if (wc - image_size[0]) % 2 or (hc - image_size[1]) % 2:
        raise ValueError(f"The mask canvas ({wc} x {hc}) and the image ({image_size[0]} x {image_size[1]}) differ by an odd number of pixels: "
                         f"the image is no centre crop of the canvas.")
    return d


def instances_on_device(preds_by_lid: Dict[int, Sequence[Dict[str, Any]]], image_size: Tuple[int, int],
                        gt_annos_by_lid: Optional[Dict[int, Sequence[Any]]] = None) -> Dict[int, List[Dict[str, Any]]]:
    """_instance_from_detection for ONE frame and all its objects with the masks made on the device (ops.detection_masks, DESIGN.md section
    19): {lid: [detection]} (already the chosen ones, best first) -> {lid: [instance]} in the same order.  An instance has the keys of the host
    path; its "input_mask_modal" is a device uint8 [H, W] view into the frame's stack -- the host path's bits -- and "mask_area" its number of
    set pixels.  One pack, one upload and one launch sequence per distinct canvas size; one read-back per frame (the areas and, with ground
    truth, the overlap counts).  gt_annos_by_lid: the annotations each object's detections are compared with; "gt_anno" / "gt_iou" follow
    _best_overlap's rule on the integer counts, so they are the host path's values.  image_size is (width, height)."""
    W, H = int(image_size[0]), int(image_size[1])
    flat = [(lid, p_) for lid, preds in preds_by_lid.items() for p_ in preds]
    out: Dict[int, List[Dict[str, Any]]] = {lid: [] for lid in preds_by_lid}
    if not flat:
        return out
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, (_, p_) in enumerate(flat):
        groups.setdefault((int(p_["segmentation"]["size"][0]), int(p_["segmentation"]["size"][1])), []).append(i)
    offsets = {hw: _device_crop_offsets(hw, (W, H)) for hw in groups}     # every refusal comes before the first launch
    packs = {hw: pack_rle([flat[i][1] for i in idx]) for hw, idx in groups.items()}
    masks: List[Optional[torch.Tensor]] = [None] * len(flat)
    areas: List[Optional[torch.Tensor]] = [None] * len(flat)
    for hw, idx in groups.items():
        counts, run_off, _ = packs[hw]
        table = _lib.upload_async(torch.from_numpy(np.concatenate([counts, run_off])), "cuda")
        stack, area = ops.detection_masks(table[:counts.size], table[counts.size:], hw, (H, W), open3x3=True)
        for j, i in enumerate(idx):
            masks[i], areas[i] = stack[j], area[j:j + 1]
    back = [torch.cat(areas).to(torch.int64)]
    annos_of = {lid: list((gt_annos_by_lid or {}).get(lid, ())) for lid in preds_by_lid}
    with_gt = [lid for lid in preds_by_lid if len(preds_by_lid[lid]) and len(annos_of[lid])]
    if with_gt:   # the annotation masks of the objects at hand go up once; inter[d, a] per object, exact integer sums
        host = np.stack([np.asarray(a.masks_modal).astype(bool) for lid in with_gt for a in annos_of[lid]])
        gt = torch.from_numpy(host).cuda()
        a0 = 0
        for lid in with_gt:
            g = gt[a0:a0 + len(annos_of[lid])]
            a0 += len(annos_of[lid])
            m = torch.stack([masks[i] for i, (l2, _) in enumerate(flat) if l2 == lid]).bool()
            back.append((m[:, None] & g[None]).flatten(2).sum(-1).flatten())
            back.append(g.flatten(1).sum(-1))
    back = torch.cat(back).cpu().numpy()            # the frame's one read-back
    area_h, pos = back[:len(flat)], len(flat)
    overlap = {}
    for lid in with_gt:
        d, a = len(preds_by_lid[lid]), len(annos_of[lid])
        inter = back[pos:pos + d * a].reshape(d, a)
        gt_area = back[pos + d * a:pos + d * a + a]
        pos += d * a + a
        overlap[lid] = (inter, gt_area)
    seen = {lid: 0 for lid in preds_by_lid}
    for i, (lid, p_) in enumerate(flat):
        dx, dy = offsets[(int(p_["segmentation"]["size"][0]), int(p_["segmentation"]["size"][1]))]
        gt_anno, gt_iou = (annos_of[lid][0], 0.0) if len(annos_of[lid]) else (None, 0.0)
        if lid in overlap:
            inter = overlap[lid][0][seen[lid]]
            union = int(area_h[i]) + overlap[lid][1] - inter
            ious = np.where(union > 0, inter / np.maximum(union, 1), 0.0)     # _best_overlap's rule, on the device's counts
            if float(ious.max()) > 0.0:
                gt_anno, gt_iou = annos_of[lid][int(np.argmax(ious))], float(ious[int(np.argmax(ious))])
        seen[lid] += 1
        out[lid].append({"input_box_amodal": _box_in_image(p_, dx, dy), "input_mask_modal": masks[i], "gt_anno": gt_anno, "gt_iou": gt_iou,
                         "time": p_["time"], "mask_area": int(area_h[i])})
    return out
