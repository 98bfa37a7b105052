"""The COCO average precision of a detections file, on the MI355X: what BOP's 2D detection and 2D segmentation tasks measure (DESIGN.md
section 24).

    python -m foundpose_amd.eval_coco --detections detections.json --dataset-dir <datasets>/lmo/test [--targets ../test_targets_bop19.json] \\
        [--iou-type segm|bbox] [--bbox-type amodal|modal] [--min-visib 0.1] [--max-dets 100] --output scores.json

AP over IoU 0.50:0.05:0.95 of the detections `detect` (or CNOS itself) wrote, on masks or on boxes.  Restates the published behaviour of
pycocotools' COCOeval (evaluateImg and accumulate for instances without iscrowd, one area range); neither pycocotools nor bop_toolkit is
installed here, so nothing is pinned against their code: the yardstick is tests/coco_ref.py.  The run lengths are decoded by
fp_detection_masks, detections and ground truth are packed to bits by fp_mask_pack, fp_group_mask_iou (or fp_group_box_iou) intersects every
detection with every instance of the same object in the same image, fp_coco_match applies COCO's matching rule for the ten thresholds and
fp_detection_ap accumulates precision and recall per object (csrc/coco_eval.hip, csrc/detection_ap.hip).  The overlaps are never read back;
the host reads files, sorts, builds the tables and averages.
"""

import argparse
import json
import math
import os
import time
from collections import defaultdict
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .device_timer import DeviceTimer
from .eval_bop19 import _read_json
from .eval_bop24 import REC_THR, ap_objects, target_images
from .group_tables import MAX_GROUP_GT, MAX_THS, check_groups, int32_table, upload

IOU_THS = np.linspace(0.5, 0.95, 10)     # COCO's thresholds as pycocotools makes them
MAX_DETS_LIMIT = 256                      # detections of one (image, object) that the matching takes
IOU_TYPES, BBOX_TYPES = ("segm", "bbox"), ("amodal", "modal")


# ---------------------------------------------------------------------------------------------------------- the matching launch
def match_groups(overlap, est_off, gt_off, pair_off, gt_ignore, ths=IOU_THS):
    """fp_coco_match with its host tables checked first (ValueError before any launch): overlap f64 [P] ON THE DEVICE (ops.group_mask_iou's
    or ops.group_box_iou's output, not read back); est_off / gt_off / pair_off [NG + 1] ascending, group g owning E_g estimates (in rank
    order), G_g <= 256 GT instances (the non-ignored ones first) and the E_g G_g rows of overlap from pair_off[g]; gt_ignore [G_total];
    ths [T], 1 <= T <= 16, every threshold in (0, 1].  -> (flag int8 [N_est, T], matched_gt int32 [N_est, T]) on the device."""
    import torch

    from . import ops
    if not isinstance(overlap, torch.Tensor) or not overlap.is_cuda:
        raise ValueError("match_groups: overlap is a device tensor (the overlaps are not read back); there is no CPU path")
    if overlap.dtype != torch.float64 or overlap.dim() != 1 or not overlap.is_contiguous():
        raise ValueError(f"match_groups: overlap must be a contiguous float64 [P] tensor, got {overlap.dtype} {tuple(overlap.shape)}")
    gt_ignore = int32_table("gt_ignore", gt_ignore)
    est_off, gt_off, pair_off, _ = check_groups("match_groups", est_off, gt_off, pair_off, gt_ignore.size, int(overlap.shape[0]), "overlap", "gt_ignore")
    ths = check_thresholds(ths)
    d_est, d_gt, d_pair, d_ign = upload([est_off, gt_off, pair_off, gt_ignore], np.int32, overlap.device)
    d_ths, = upload([ths], np.float64, overlap.device)
    return ops.coco_match(d_est, d_gt, d_pair, overlap, d_ign, d_ths, int(est_off[-1]))


def check_thresholds(ths) -> np.ndarray:
    ths = np.ascontiguousarray(np.asarray(ths, np.float64))
    if ths.ndim != 1 or not 1 <= ths.size <= MAX_THS:
        raise ValueError(f"ths must be [T] with 1 <= T <= {MAX_THS}, got {ths.shape}")
    if not np.all((ths > 0.0) & (ths <= 1.0)):    # false for a NaN
        raise ValueError(f"every IoU threshold must lie in (0, 1], got {ths.tolist()}")
    return ths


def check_options(iou_type: str, bbox_type: str, min_visib: float, max_dets: int, image_block: int) -> None:
    if iou_type not in IOU_TYPES:
        raise ValueError(f"iou_type must be one of {IOU_TYPES}, got {iou_type!r}")
    if bbox_type not in BBOX_TYPES:
        raise ValueError(f"bbox_type must be one of {BBOX_TYPES}, got {bbox_type!r}")
    if not (isinstance(min_visib, (int, float)) and 0.0 <= float(min_visib) <= 1.0):
        raise ValueError(f"min_visib must lie in [0, 1], got {min_visib!r}")
    if not (isinstance(max_dets, (int, np.integer)) and 1 <= int(max_dets) <= MAX_DETS_LIMIT):
        raise ValueError(f"max_dets must lie in [1, {MAX_DETS_LIMIT}], got {max_dets!r}")
    if not (isinstance(image_block, (int, np.integer)) and int(image_block) >= 1):
        raise ValueError(f"image_block must be >= 1, got {image_block!r}")


# ---------------------------------------------------------------------------------------------------------- inputs
def detection_records(detections: Union[str, Sequence[Dict[str, Any]], Dict[Tuple[int, int, int], Sequence[Dict[str, Any]]]]) -> List[Dict[str, Any]]:
    """A CNOS detections file, its record list, or the dict load_detections_in_bop_format makes of it -> records {scene_id, image_id,
    category_id, bbox, score, segmentation} in input order (a dict: key by key)."""
    if isinstance(detections, (str, os.PathLike)):
        detections = _read_json(os.fspath(detections))
    if isinstance(detections, dict):
        return [dict(d, scene_id=int(k[0]), image_id=int(k[1]), category_id=int(k[2])) for k, ds in detections.items() for d in ds]
    return [dict(d, scene_id=int(d["scene_id"]), image_id=int(d["image_id"]), category_id=int(d["category_id"])) for d in detections]


def image_size(split_dir: str, scene_id: int, im_id: int) -> Tuple[int, int]:
    """(W, H) of a test image, from the header of rgb/<im>.png, rgb/<im>.jpg, gray/<im>.tif or depth/<im>.png (the first that exists)."""
    from PIL import Image
    sd = os.path.join(split_dir, f"{scene_id:06d}")
    for sub, ext in (("rgb", "png"), ("rgb", "jpg"), ("gray", "tif"), ("depth", "png")):
        p = os.path.join(sd, sub, f"{im_id:06d}.{ext}")
        if os.path.exists(p):
            with Image.open(p) as im:
                return int(im.size[0]), int(im.size[1])
    raise FileNotFoundError(f"{sd}: no rgb, gray or depth image {im_id:06d}: the masks' canvas is checked against the image size")


def read_mask(path: str) -> np.ndarray:
    """mask_visib/<im>_<gt>.png -> uint8 [H, W] of 0 / 1 (non-zero is set)."""
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.ndim == 3:
        a = a.max(axis=2)
    return (a != 0).astype(np.uint8)


def build_tables(records: Sequence[Dict[str, Any]], images: Sequence[Tuple[int, int]], infos: Dict[int, Any], gts: Dict[int, Any],
                 bbox_type: str = "amodal", min_visib: float = 0.1, max_dets: int = 100, unseen=frozenset()) -> Dict[str, Any]:
    """The host side of the protocol for the images `images`: everything the launches read but the pixels.  records: detection_records';
    gts / infos: scene_gt.json / scene_gt_info.json per scene; unseen: {(scene, im, gt id)} whose visible mask is empty.  An instance is
    ignored when visib_fract < min_visib, when it is in `unseen` or when its box (bbox_obj for "amodal", bbox_visib for "modal") is the -1
    sentinel.  -> dict: groups [(scene, im, obj)] sorted, the ones with a detection only; est_rows: the records in group-then-rank order
    (score descending, equal scores in input order, at most max_dets of a group); est_off / gt_off / pair_off; gt_ignore and gt_ids [(scene,
    im, gt id)] in layout order, every group's non-ignored instances first; gt_boxes f64 [G, 4]; n_valid / n_ignored {obj: count} over ALL
    instances of the images; num_other (records of other images), num_cut (beyond max_dets)."""
    img_set = set(images)
    per = defaultdict(list)
    num_other = 0
    for i, r in enumerate(records):
        key = (r["scene_id"], r["image_id"], r["category_id"])
        if key[:2] not in img_set:
            num_other += 1
            continue
        s = float(r["score"])
        if math.isnan(s):
            raise ValueError(f"detection {i}: the score is NaN, the detections cannot be ranked")
        per[key].append(i)
    box_key = "bbox_obj" if bbox_type == "amodal" else "bbox_visib"
    gt_of = defaultdict(list)     # (scene, im, obj) -> [(ignored, gt id, box)], the non-ignored first
    n_valid, n_ignored = defaultdict(int), defaultdict(int)
    for s, im in images:
        ents, ivs = gts[s].get(str(im), []), infos[s].get(str(im), [])
        for g, e in enumerate(ents):
            lid = int(e["obj_id"])
            box = [float(v) for v in ivs[g][box_key]]
            ign = float(ivs[g]["visib_fract"]) < min_visib or (s, im, g) in unseen or all(v == -1.0 for v in box)
            gt_of[(s, im, lid)].append((int(ign), g, box))
            (n_ignored if ign else n_valid)[lid] += 1
    for insts in gt_of.values():
        insts.sort(key=lambda t: t[0])        # stable: scene_gt order inside each half
    groups = sorted(per)
    est_rows: List[int] = []
    est_off, gt_off, pair_off, gt_ignore, gt_ids, gt_boxes = [0], [0], [0], [], [], []
    num_cut = 0
    for key in groups:
        ranked = sorted(per[key], key=lambda i: float(records[i]["score"]), reverse=True)   # stable: among equal scores the earlier record wins
        num_cut += max(len(ranked) - max_dets, 0)
        ranked = ranked[:max_dets]
        insts = gt_of.get(key, [])
        if len(insts) > MAX_GROUP_GT:
            raise ValueError(f"scene {key[0]} image {key[1]} has {len(insts)} GT instances of object {key[2]} (at most {MAX_GROUP_GT})")
        est_rows += ranked
        gt_ignore += [t[0] for t in insts]
        gt_ids += [(key[0], key[1], t[1]) for t in insts]
        gt_boxes += [t[2] for t in insts]
        est_off.append(est_off[-1] + len(ranked))
        gt_off.append(gt_off[-1] + len(insts))
        pair_off.append(pair_off[-1] + len(ranked) * len(insts))
    if pair_off[-1] > 2**31 - 1:
        raise ValueError(f"{pair_off[-1]} (detection, GT) pairs: more than one block holds; lower image_block")
    return {"groups": groups, "est_rows": np.array(est_rows, np.int64), "est_off": np.array(est_off, np.int64), "gt_off": np.array(gt_off, np.int64),
            "pair_off": np.array(pair_off, np.int64), "gt_ignore": np.array(gt_ignore, np.int64), "gt_ids": gt_ids,
            "gt_boxes": np.array(gt_boxes, np.float64).reshape(-1, 4), "n_valid": dict(n_valid), "n_ignored": dict(n_ignored),
            "num_other": num_other, "num_cut": num_cut}


def rank_objects(records: Sequence[Dict[str, Any]], est_rows: np.ndarray, extra_objects=()) -> Tuple[List[int], np.ndarray, np.ndarray]:
    """-> (obj_ids sorted, obj_off [O + 1], order): per object the rows of the estimate table in global rank order, score descending and
    equal scores in table order (by image, then by rank within the image: the order in which pycocotools concatenates the images)."""
    pos_of = defaultdict(list)
    for pos, i in enumerate(est_rows):
        pos_of[records[int(i)]["category_id"]].append(pos)
    obj_ids = sorted(set(pos_of) | {int(o) for o in extra_objects})
    obj_off, order = [0], []
    for lid in obj_ids:
        order += sorted(pos_of.get(lid, []), key=lambda p: float(records[int(est_rows[p])]["score"]), reverse=True)
        obj_off.append(len(order))
    return obj_ids, np.array(obj_off, np.int64), np.array(order, np.int64)


def summarize(ap: np.ndarray, totals: np.ndarray, n_valid: Sequence[int], ths: np.ndarray) -> Dict[str, Any]:
    """ap [O, T], totals [O, T, 3] -> AP (the mean over thresholds and over the objects with n_valid > 0; the others hold -1 and are left
    out), AP50 / AP75 (the columns at those thresholds, -1 without one), AR (true positives over n_valid, the same mean).  Without any such
    object every number is 0."""
    ap, n_valid = np.asarray(ap, np.float64), np.asarray(n_valid, np.int64)
    has = n_valid > 0
    T = len(ths)
    if not has.any():
        return {"ap": 0.0, "ap50": 0.0, "ap75": 0.0, "ar": 0.0, "columns": np.zeros(T), "recall": np.zeros((0, T))}
    cols = ap[has].mean(axis=0)
    recall = totals[has, :, 0].astype(np.float64) / n_valid[has, None].astype(np.float64)

    def at(v):
        k = np.flatnonzero(np.isclose(ths, v))
        return float(cols[k[0]]) if k.size else -1.0
    return {"ap": float(ap[has].mean()), "ap50": at(0.5), "ap75": at(0.75), "ar": float(recall.mean()), "columns": cols, "recall": recall}


# ---------------------------------------------------------------------------------------------------------- evaluation
def evaluate_coco(detections, split_dir: str, targets: Union[None, str, Sequence[Dict[str, int]]] = None, iou_type: str = "segm",
                  bbox_type: str = "amodal", min_visib: float = 0.1, max_dets: int = 100, image_block: int = 32, device: str = "cuda",
                  details: bool = False) -> Dict[str, Any]:
    """COCO AP of `detections` (a CNOS file, its record list or load_detections_in_bop_format's dict) against the split `split_dir`
    (<datasets>/<dataset>/<split>).  targets: a test_targets json path or its list of {scene_id, im_id} (default <split_dir>/../
    test_targets_bop19.json; other keys are ignored, detections on other images are dropped and counted).  iou_type "segm": masks against
    mask_visib/<im>_<gt>.png; "bbox": the detections' bbox against bbox_obj ("amodal") or bbox_visib ("modal") of scene_gt_info.json.  An
    instance with visib_fract < min_visib, an empty visible mask (segm) or a -1 box is IGNORED: it is not counted and a detection matched to
    it is dropped.  At most max_dets (<= 256) detections of an (image, object) are taken, the best first.  One decode / pack / overlap /
    match chain per block of `image_block` images of one size.  details: also the tables and the device's flags.  -> the scores dict
    (DESIGN.md section 24)."""
    import torch

    from . import _lib, ops
    from .infer_pose_util import pack_rle
    check_options(iou_type, bbox_type, min_visib, max_dets, image_block)
    root = os.path.dirname(os.path.abspath(split_dir))
    if targets is None or isinstance(targets, str):
        targets = _read_json(targets or os.path.join(root, "test_targets_bop19.json"))
    t_start = time.perf_counter()
    records = detection_records(detections)
    images = target_images(targets)
    gts, infos = {}, {}
    for s in sorted({s for s, _ in images}):
        sd = os.path.join(split_dir, f"{s:06d}")
        gts[s] = _read_json(os.path.join(sd, "scene_gt.json"))
        infos[s] = _read_json(os.path.join(sd, "scene_gt_info.json"))
    ths = check_thresholds(IOU_THS)
    T = int(ths.size)
    dev = torch.device(device)
    host = defaultdict(float)
    timer = DeviceTimer()
    timed = timer.timed

    # ---- the blocks: consecutive target images of one size, image_block at most
    segm = iou_type == "segm"
    with_dets = {(r["scene_id"], r["image_id"]) for r in records}
    sizes = {k: image_size(split_dir, *k) for k in images if k in with_dets} if segm else {}
    blocks: List[List[Tuple[int, int]]] = []
    block_size = None     # an image without a detection has no pair: it fits any block
    for k in images:
        size = sizes.get(k)
        if blocks and len(blocks[-1]) < image_block and (size is None or block_size is None or size == block_size):
            blocks[-1].append(k)
            block_size = block_size or size
        else:
            blocks.append([k])
            block_size = size

    flags, matcheds, est_rows_all, tables = [], [], [], []
    n_valid, n_ignored = defaultdict(int), defaultdict(int)
    img_set = set(images)
    num_other = sum(1 for r in records if (r["scene_id"], r["image_id"]) not in img_set)
    num_cut = num_pairs = 0
    for blk in blocks:
        t0 = time.perf_counter()
        unseen, gt_masks = set(), {}
        if segm:   # the visible masks of the block's instances; an empty one makes its instance ignored, so they come before the tables
            for s, im in blk:
                for g in range(len(gts[s].get(str(im), []))):
                    m = read_mask(os.path.join(split_dir, f"{s:06d}", "mask_visib", f"{im:06d}_{g:06d}.png"))
                    gt_masks[(s, im, g)] = m
                    if not m.any():
                        unseen.add((s, im, g))
        host["read_gt"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        tb = build_tables(records, blk, infos, gts, bbox_type, min_visib, max_dets, unseen)
        for lid, n in tb["n_valid"].items():
            n_valid[lid] += n
        for lid, n in tb["n_ignored"].items():
            n_ignored[lid] += n
        num_cut += tb["num_cut"]
        est_rows_all.append(tb["est_rows"])
        P, NE, NGT = int(tb["pair_off"][-1]), int(tb["est_off"][-1]), int(tb["gt_off"][-1])
        num_pairs += P
        host["tables"] += time.perf_counter() - t0
        if NE == 0:
            continue
        preds = [records[int(i)] for i in tb["est_rows"]]
        if segm:
            for r in preds:    # the run lengths must cover the image exactly, as in detect_util.label_proposals
                w, h = sizes[(r["scene_id"], r["image_id"])]
                if tuple(int(v) for v in r["segmentation"]["size"]) != (h, w):
                    raise ValueError(f"a detection of scene {r['scene_id']} image {r['image_id']} lies on a canvas of {r['segmentation']['size'][1]} x "
                                     f"{r['segmentation']['size'][0]}, the image is {w} x {h}")
        d_est, d_gt, d_pair = upload([tb["est_off"], tb["gt_off"], tb["pair_off"]], np.int32, dev)
        if P == 0:
            overlap = torch.zeros(0, dtype=torch.float64, device=dev)
        elif segm:
            t0 = time.perf_counter()
            counts, run_off, (H, W) = pack_rle(preds)     # (refuses detections of different canvases)
            for k in tb["gt_ids"]:
                if gt_masks[k].shape != (H, W):
                    raise ValueError(f"mask_visib of scene {k[0]} image {k[1]} instance {k[2]} is {gt_masks[k].shape[1]} x {gt_masks[k].shape[0]}, the image is {W} x {H}")
            gt_stack = np.stack([gt_masks[k] for k in tb["gt_ids"]]) if NGT else np.zeros((0, H, W), np.uint8)
            host["pack_host"] += time.perf_counter() - t0
            table = _lib.upload_async(torch.from_numpy(np.concatenate([counts, run_off])), dev)
            d_gtm = _lib.upload_async(torch.from_numpy(gt_stack), dev)      # one upload of the block's GT masks
            det_masks, _ = timed("decode", ops.detection_masks, table[:counts.size], table[counts.size:], (H, W), (H, W), open3x3=False)
            words_a, _ = timed("pack", ops.mask_pack, det_masks)
            words_b, _ = timed("pack", ops.mask_pack, d_gtm)
            del det_masks, d_gtm
            _, overlap, _ = timed("overlap", ops.group_mask_iou, words_a, words_b, d_est, d_gt, d_pair, P)
        else:
            boxes_a = np.array([[float(v) for v in r["bbox"]] for r in preds], np.float64).reshape(-1, 4)
            d_a, d_b = upload([boxes_a, tb["gt_boxes"]], np.float64, dev)
            overlap, _ = timed("overlap", ops.group_box_iou, d_a.reshape(-1, 4), d_b.reshape(-1, 4), d_est, d_gt, d_pair, P)
        flag, matched = timed("match", match_groups, overlap, tb["est_off"], tb["gt_off"], tb["pair_off"], tb["gt_ignore"], ths)
        flags.append(flag)
        if details:
            matcheds.append(matched)
            tables.append(dict(tb, overlap=overlap.cpu().numpy()))

    # ---- precision / recall per object and threshold over all images: one launch, the flags as the matching left them on the device
    t0 = time.perf_counter()
    est_rows = np.concatenate(est_rows_all) if est_rows_all else np.zeros(0, np.int64)
    obj_ids, obj_off, order = rank_objects(records, est_rows, set(n_valid) | set(n_ignored))
    nv = np.array([n_valid.get(lid, 0) for lid in obj_ids], np.int64)
    host["tables"] += time.perf_counter() - t0
    flag = torch.cat(flags) if flags else torch.zeros(0, T, dtype=torch.int8, device=dev)
    if T % 2:   # fp_detection_ap takes an even number of columns: a copy of the last one rides along and is dropped
        flag = torch.cat([flag, flag[:, -1:]], dim=1)
    ap_d, q_d, totals_d = timed("ap", ap_objects, flag.contiguous(), obj_off, order, nv)
    ap, totals = ap_d.cpu().numpy()[:, :T], totals_d.cpu().numpy()[:, :T]
    dev_s = timer.seconds()

    s = summarize(ap, totals, nv, ths)
    out = {"coco_average_precision": s["ap"], "coco_average_precision_50": s["ap50"], "coco_average_precision_75": s["ap75"],
           f"coco_average_recall_{int(max_dets)}": s["ar"], "coco_average_recall": s["ar"],
           "iou_type": iou_type, "bbox_type": bbox_type if not segm else None, "iou_thresholds": ths.tolist(), "ap_per_threshold": s["columns"].tolist(),
           "min_visib_fract": float(min_visib), "max_dets": int(max_dets), "num_recall_thresholds": int(REC_THR.size),
           "num_target_images": len(images), "num_detections": len(records), "num_detections_evaluated": int(est_rows.size),
           "num_detections_of_other_images": int(num_other), "num_detections_beyond_max_dets": int(num_cut),
           "num_gt_instances": int(sum(n_valid.values()) + sum(n_ignored.values())), "num_ignored_gt_instances": int(sum(n_ignored.values())),
           "num_pairs": int(num_pairs), "num_ignored_detections": totals[:, :, 2].sum(0).tolist() if len(obj_ids) else [0] * T,
           "per_object": {}, "device_seconds": dev_s, "host_seconds": dict(host, total=time.perf_counter() - t_start)}
    for o, lid in enumerate(obj_ids):
        has = int(nv[o]) > 0
        out["per_object"][str(lid)] = {
            "average_precision": float(ap[o].mean()) if has else -1.0, "ap": ap[o].tolist(),
            "average_recall": float((totals[o, :, 0] / float(nv[o])).mean()) if has else -1.0,
            "num_valid_instances": int(nv[o]), "num_ignored_instances": int(n_ignored.get(lid, 0)),
            "num_detections": int(obj_off[o + 1] - obj_off[o]), "totals": totals[o].tolist()}   # (tp, fp, ignored) per threshold
    if details:
        out["tables"] = {"blocks": tables, "est_rows": est_rows, "obj_ids": obj_ids, "obj_off": obj_off, "order": order, "n_valid": nv,
                         "flag": flag.cpu().numpy()[:, :T], "matched_gt": (torch.cat(matcheds).cpu().numpy() if matcheds else np.zeros((0, T), np.int32)),
                         "ap": ap, "q": q_d.cpu().numpy()[:, :T], "totals": totals}
    return out


def main(argv: Optional[Sequence[str]] = None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--detections", required=True, help="CNOS detections json (what detect writes)")
    ap.add_argument("--dataset-dir", required=True, help="BOP split directory (<datasets>/<dataset>/<split>)")
    ap.add_argument("--targets", default=None, help="test targets json (default: <dataset-dir>/../test_targets_bop19.json); only scene_id / im_id are read")
    ap.add_argument("--iou-type", default="segm", choices=IOU_TYPES, help="masks (BOP's 2D segmentation task) or boxes (2D detection)")
    ap.add_argument("--bbox-type", default="amodal", choices=BBOX_TYPES, help="bbox: the GT box, bbox_obj (amodal) or bbox_visib (modal)")
    ap.add_argument("--min-visib", type=float, default=0.1, help="a GT instance less visible than this is ignored (0: every instance counts)")
    ap.add_argument("--max-dets", type=int, default=100, help="detections taken per (image, object), the best first")
    ap.add_argument("--image-block", type=int, default=32, help="images per decode / overlap / match chain")
    ap.add_argument("--output", required=True, help="scores JSON")
    args = ap.parse_args(argv)
    t0 = time.perf_counter()
    scores = evaluate_coco(args.detections, args.dataset_dir, args.targets, args.iou_type, args.bbox_type, args.min_visib, args.max_dets,
                           args.image_block)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(scores, f, indent=2)
    print(f"coco_average_precision {scores['coco_average_precision']:.4f} (AP50 {scores['coco_average_precision_50']:.4f}, AP75 "
          f"{scores['coco_average_precision_75']:.4f}, AR {scores['coco_average_recall']:.4f}; {args.iou_type}) over "
          f"{scores['num_gt_instances'] - scores['num_ignored_gt_instances']} instances and {scores['num_detections_evaluated']} detections in "
          f"{time.perf_counter() - t0:.1f} s -> {args.output}")


if __name__ == "__main__":
    main()
