"""The inference driver (/root/reference/scripts/infer.py:55-100, 290-816) over the MI355X path: options with the
reference's names and defaults, CNOS detections in, `estimated-poses.json` per object out.

What differs from the reference loop, by design: the instances of an image go through the crop producer, the extractor,
the matching and the PnP tail as ONE batch on the device (the reference handles them one at a time on the CPU), the
ground-truth evaluation (opt-in: eval_models / --eval-gt) is one fp_pose_errors launch per frame, and the result pictures
(opt-in: renderer= / --vis, with vis_results; vis_util) are composited on the device, one tile per
estimated pose and one summary per frame; the HTML branches are not part of this path.

  python -m foundpose_amd.infer --opts configs/infer/lmo.json --dataset-dir <bop split dir> --detections <cnos json> \\
         --repre-dir <output>/object_repre --output-dir <output>/inference [--vis [--models-dir <models>]] [--batch-detections 32 [--device-masks]]

--batch-detections N (N >= 1) runs infer_batched instead: one pass over the images, N detections per batch across frames and objects, the
same poses; --device-masks with it makes the detections' masks on the device instead of on the host (section 19).

"task": "detection" in the options runs the BOP24 6D detection task instead of 6D localization (section 21): the targets (default
test_targets_bop24.json) name images only, and every detection of every object gets a pose; eval_bop24 scores the csv.
"""

import argparse
import functools
import json
import math
import os
import time
from typing import Any, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import crop_util, engine as fe, eval_bop19, eval_util, feature_util, infer_pose_util, multiview, pnp_util, pose_nms, refine_util, repre_util, vis_util
from .bank import DeviceBank


class InferOpts(NamedTuple):
    """Options of scripts/infer.py:55-100 (same names, same defaults)."""
    version: str
    repre_version: str
    object_dataset: str
    object_lids: Optional[List[int]] = None
    max_sym_disc_step: float = 0.01
    crop: bool = True
    crop_rel_pad: float = 0.2
    crop_size: Tuple[int, int] = (420, 420)
    use_detections: bool = True
    num_preds_factor: float = 1.0
    min_visibility: float = 0.1
    extractor_name: str = "dinov2_vitl14"
    grid_cell_size: float = 1.0
    max_num_queries: int = 1000000
    match_template_type: str = "tfidf"
    match_top_n_templates: int = 5
    match_feat_matching_type: str = "cyclic_buddies"
    match_top_k_buddies: int = 300
    pnp_type: str = "opencv"
    pnp_ransac_iter: int = 1000
    pnp_required_ransac_conf: float = 0.99
    pnp_inlier_thresh: float = 10.0
    pnp_refine_lm: bool = True
    final_pose_type: str = "best_coarse"
    save_estimates: bool = True
    vis_results: bool = True
    vis_corresp_top_n: int = 100
    vis_feat_map: bool = True
    vis_for_paper: bool = True
    debug: bool = True
    refine_iters: int = 30          # final_pose_type="featuremetric": Levenberg-Marquardt iterations (refine_util)
    depth_refine_iters: int = 30    # final_pose_type="depth" / "featuremetric_depth": iterations against the frame's depth
    depth_refine_max_dist: float = 0.0   # ... its truncation distance tau in mm; 0: a tenth of the diagonal of the bounding box of repre.vertices
    depth_refine_weight: float = 1.0     # final_pose_type="featuremetric_depth_joint": w_d of E_f + w_d E_d (refine_iters iterations)
    depth_pnp_inlier_thresh: float = 0.0   # pnp_type="kabsch_depth": the 3D inlier threshold in mm; 0: 0.05 x the diagonal of the bounding box of repre.vertices
    coarse_select_type: str = "inliers"    # which coarse hypothesis goes on: "inliers" (the most correspondence inliers), "depth_verify" (every hypothesis checked against the frame's depth) or "mask_verify" (... against the detection's mask, no depth needed; section 18)
    depth_verify_thresh: float = 0.0       # coarse_select_type="depth_verify": the tolerance tau in mm; 0: 0.02 x the diagonal of the bounding box of repre.vertices
    depth_verify_max_points: int = 16384   # ... and the number of model points placed at each hypothesis, at most
    mask_verify_grid: int = 64             # coarse_select_type="mask_verify": the side G of the silhouette's cell grid, in [8, 128]
    mask_verify_max_points: int = 16384    # ... and the number of model points placed at each hypothesis, at most
    frame_select_type: str = "none"        # what is done with the poses of a frame TOGETHER once all are estimated: "none" or "pose_nms" (duplicate poses suppressed by their 3D overlap)
    pose_nms_thresh: float = 0.3           # frame_select_type="pose_nms": two poses conflict when either's sample lies in the other's occupied cells by this fraction, in (0, 1]
    pose_nms_grid: int = 16                # ... the side G of the occupancy grid over the model's bounding sphere, in [8, 32]
    pose_nms_max_points: int = 4096        # ... the number of model points of each sample, at most
    pose_nms_cross_object: bool = False    # ... compare poses of different objects too
    task: str = "localization"             # "localization": the targets say how many instances each (image, object) has and num_preds_factor x that many detections get a pose; "detection": the targets name images only and every detection of every object gets one (BOP24 6D detection)
    detection_min_score: float = 0.0       # task="detection": detections scored below this get no pose
    detection_max_per_object: int = 16     # ... and at most this many of one (image, object), best first; >= 1
    scene_select_type: str = "none"        # what is done with the poses of a static SCENE together, after frame_select_type: "none" or "multiview" (the estimates of one object from several calibrated views fused into one world pose)
    scene_fuse_match_thresh: float = 1.0   # scene_select_type="multiview": an estimate joins a cluster whose seed lies within this x the object's diameter, > 0
    scene_fuse_huber_px: float = 10.0      # ... the Huber delta of the reprojection error in pixels, > 0
    scene_fuse_points: int = 64            # ... the number of model points per member view, in [1, 4096]
    scene_fuse_min_views: int = 2          # ... the smallest cluster that is refined, >= 2
    scene_fuse_iters: int = 20             # ... Levenberg-Marquardt iterations, in [0, 1000]
    mask_refine_iters: int = 30            # final_pose_type="mask" / "featuremetric_mask": iterations against the detection's mask, in [0, 1000]
    mask_refine_huber_px: float = 8.0      # ... the Huber delta of both residuals in pixels, > 0 (this default and the two below rest on no measurement)
    mask_refine_max_points: int = 4096     # ... the number of model points placed at the pose, at most
    mask_refine_max_contour: int = 1024    # ... the number of contour pixels of the mask that pull on the model, at most


FINAL_POSE_TYPES = ("best_coarse", "featuremetric", "depth", "featuremetric_depth")
JOINT_POSE_TYPES = ("featuremetric_depth_joint",)   # features and depth in one objective (refine_util.refine_best_coarse_rgbd); a final pose type too
MASK_POSE_TYPES = ("mask", "featuremetric_mask")   # the final pose is refined against the detection's own mask (refine_util.refine_best_coarse_mask): no depth; final pose types too
DEPTH_POSE_TYPES = ("depth", "featuremetric_depth") + JOINT_POSE_TYPES   # the final pose is refined against the frame's "depth"
DEPTH_PNP_TYPES = ("kabsch_depth",)   # the coarse poses are solved on the frame's "depth" (pnp_util.solve_kabsch_ransac_batch)
COARSE_SELECT_TYPES = ("inliers", "depth_verify", "mask_verify")
DEPTH_SELECT_TYPES = ("depth_verify",)   # the coarse hypotheses are checked against the frame's "depth" (pnp_util.verify_poses_depth)
MASK_SELECT_TYPES = ("mask_verify",)     # ... against the detection's own mask (pnp_util.verify_poses_mask): no depth
FRAME_SELECT_TYPES = ("none", "pose_nms")
SCENE_SELECT_TYPES = ("none", "multiview")
TASKS = ("localization", "detection")


def _scene_fuse_opts(opts: "InferOpts") -> multiview.FuseOpts:
    return multiview.FuseOpts(opts.scene_fuse_match_thresh, opts.scene_fuse_huber_px, opts.scene_fuse_points, opts.scene_fuse_min_views,
                              opts.scene_fuse_iters)


def load_opts(path_or_dict) -> InferOpts:
    """configs/infer/*.json: {"infer_opts": {...}}; unknown keys are an error, like NamedTuple construction in the reference."""
    d = path_or_dict
    if not isinstance(d, dict):
        with open(path_or_dict) as f:
            d = json.load(f)
    d = dict(d.get("infer_opts", d))
    if "crop_size" in d:
        d["crop_size"] = tuple(d["crop_size"])
    return InferOpts(**d)


def _check_driver_opts(opts: InferOpts):
    """The options both drivers refuse, before any device work.  -> (refine, check_max_queries)."""
    if opts.match_template_type != "tfidf":
        raise ValueError(f"Unknown matching type '{opts.match_template_type}'.")
    if opts.match_feat_matching_type != "cyclic_buddies":
        raise ValueError(f"Unknown feature matching type ({opts.match_feat_matching_type}).")
    if opts.final_pose_type not in FINAL_POSE_TYPES + JOINT_POSE_TYPES + MASK_POSE_TYPES:
        raise ValueError(f"Unknown final pose type {opts.final_pose_type}")
    if opts.pnp_type not in pnp_util.PNP_TYPES:
        raise ValueError(f"Unknown PnP type '{opts.pnp_type}' (one of {', '.join(pnp_util.PNP_TYPES)})")
    if isinstance(opts.depth_pnp_inlier_thresh, bool) or not isinstance(opts.depth_pnp_inlier_thresh, (int, float)) \
            or not 0 <= opts.depth_pnp_inlier_thresh < float("inf"):
        raise ValueError(f"depth_pnp_inlier_thresh must be a finite number >= 0 (mm; 0: a twentieth of the model's bounding-box diagonal), "
                         f"got {opts.depth_pnp_inlier_thresh!r}")
    if opts.coarse_select_type not in COARSE_SELECT_TYPES:
        raise ValueError(f"Unknown coarse select type '{opts.coarse_select_type}' (one of {', '.join(COARSE_SELECT_TYPES)})")
    if isinstance(opts.depth_verify_thresh, bool) or not isinstance(opts.depth_verify_thresh, (int, float)) \
            or not 0 <= opts.depth_verify_thresh < float("inf"):
        raise ValueError(f"depth_verify_thresh must be a finite number >= 0 (mm; 0: a fiftieth of the model's bounding-box diagonal), "
                         f"got {opts.depth_verify_thresh!r}")
    if isinstance(opts.depth_verify_max_points, bool) or not isinstance(opts.depth_verify_max_points, int) or opts.depth_verify_max_points < 1:
        raise ValueError(f"depth_verify_max_points must be an integer >= 1, got {opts.depth_verify_max_points!r}")
    if isinstance(opts.mask_verify_grid, bool) or not isinstance(opts.mask_verify_grid, int) \
            or not pnp_util.VERIFY_MIN_GRID <= opts.mask_verify_grid <= pnp_util.VERIFY_MAX_GRID:
        raise ValueError(f"mask_verify_grid must be an integer in [{pnp_util.VERIFY_MIN_GRID}, {pnp_util.VERIFY_MAX_GRID}], got {opts.mask_verify_grid!r}")
    if isinstance(opts.mask_verify_max_points, bool) or not isinstance(opts.mask_verify_max_points, int) or opts.mask_verify_max_points < 1:
        raise ValueError(f"mask_verify_max_points must be an integer >= 1, got {opts.mask_verify_max_points!r}")
    if opts.frame_select_type not in FRAME_SELECT_TYPES:
        raise ValueError(f"Unknown frame select type '{opts.frame_select_type}' (one of {', '.join(FRAME_SELECT_TYPES)})")
    if isinstance(opts.pose_nms_thresh, bool) or not isinstance(opts.pose_nms_thresh, (int, float)) \
            or not (math.isfinite(opts.pose_nms_thresh) and 0 < opts.pose_nms_thresh <= 1):
        raise ValueError(f"pose_nms_thresh must be a finite number in (0, 1], got {opts.pose_nms_thresh!r}")
    if isinstance(opts.pose_nms_grid, bool) or not isinstance(opts.pose_nms_grid, int) \
            or not pose_nms.MIN_GRID <= opts.pose_nms_grid <= pose_nms.MAX_GRID:
        raise ValueError(f"pose_nms_grid must be an integer in [{pose_nms.MIN_GRID}, {pose_nms.MAX_GRID}], got {opts.pose_nms_grid!r}")
    if isinstance(opts.pose_nms_max_points, bool) or not isinstance(opts.pose_nms_max_points, int) or opts.pose_nms_max_points < 1:
        raise ValueError(f"pose_nms_max_points must be an integer >= 1, got {opts.pose_nms_max_points!r}")
    if not isinstance(opts.pose_nms_cross_object, bool):
        raise ValueError(f"pose_nms_cross_object must be true or false, got {opts.pose_nms_cross_object!r}")
    if opts.scene_select_type not in SCENE_SELECT_TYPES:
        raise ValueError(f"Unknown scene select type '{opts.scene_select_type}' (one of {', '.join(SCENE_SELECT_TYPES)})")
    try:
        multiview.check_opts(_scene_fuse_opts(opts))
    except ValueError as e:
        raise ValueError(f"scene_fuse_{e}") from None
    if opts.task not in TASKS:
        raise ValueError(f"Unknown task '{opts.task}' (one of {', '.join(TASKS)})")
    if isinstance(opts.detection_min_score, bool) or not isinstance(opts.detection_min_score, (int, float)) or not math.isfinite(opts.detection_min_score):
        raise ValueError(f"detection_min_score must be a finite number, got {opts.detection_min_score!r}")
    if isinstance(opts.detection_max_per_object, bool) or not isinstance(opts.detection_max_per_object, int) or opts.detection_max_per_object < 1:
        raise ValueError(f"detection_max_per_object must be an integer >= 1, got {opts.detection_max_per_object!r}")
    if opts.task == "detection":
        if opts.num_preds_factor != 1.0:
            raise ValueError(f"task 'detection' has no instance counts to multiply: num_preds_factor must be 1.0, got {opts.num_preds_factor!r} "
                             f"(detection_max_per_object bounds the poses of an (image, object))")
        if not opts.use_detections:
            raise ValueError("task 'detection' estimates a pose for every detection: use_detections must be true")
    # the best coarse pose refined on the projected feature map (refine_util): the engine keeps the map
    refine = opts.final_pose_type in ("featuremetric", "featuremetric_depth", "featuremetric_mask") + JOINT_POSE_TYPES
    if refine and (not isinstance(opts.refine_iters, int) or opts.refine_iters < 0):
        raise ValueError(f"refine_iters must be an integer >= 0, got {opts.refine_iters!r}")
    if opts.final_pose_type in DEPTH_POSE_TYPES and (not isinstance(opts.depth_refine_iters, int) or opts.depth_refine_iters < 0):
        raise ValueError(f"depth_refine_iters must be an integer >= 0, got {opts.depth_refine_iters!r}")
    if not opts.depth_refine_max_dist >= 0:
        raise ValueError(f"depth_refine_max_dist must be >= 0 (mm; 0: a tenth of the model's bounding-box diagonal), got {opts.depth_refine_max_dist!r}")
    if isinstance(opts.depth_refine_weight, bool) or not isinstance(opts.depth_refine_weight, (int, float)) \
            or not 0 <= opts.depth_refine_weight < float("inf"):
        raise ValueError(f"depth_refine_weight must be a finite number >= 0, got {opts.depth_refine_weight!r}")
    if isinstance(opts.mask_refine_iters, bool) or not isinstance(opts.mask_refine_iters, int) or not 0 <= opts.mask_refine_iters <= 1000:
        raise ValueError(f"mask_refine_iters must be an integer in [0, 1000], got {opts.mask_refine_iters!r}")
    if isinstance(opts.mask_refine_huber_px, bool) or not isinstance(opts.mask_refine_huber_px, (int, float)) \
            or not (math.isfinite(opts.mask_refine_huber_px) and opts.mask_refine_huber_px > 0):
        raise ValueError(f"mask_refine_huber_px must be a finite number > 0, got {opts.mask_refine_huber_px!r}")
    if isinstance(opts.mask_refine_max_points, bool) or not isinstance(opts.mask_refine_max_points, int) or opts.mask_refine_max_points < 1:
        raise ValueError(f"mask_refine_max_points must be an integer >= 1, got {opts.mask_refine_max_points!r}")
    if isinstance(opts.mask_refine_max_contour, bool) or not isinstance(opts.mask_refine_max_contour, int) or opts.mask_refine_max_contour < 1:
        raise ValueError(f"mask_refine_max_contour must be an integer >= 1, got {opts.mask_refine_max_contour!r}")
    # scripts/infer.py:482-485 subsamples the query points with torch.randperm when a mask yields more than max_num_queries of them
    # (default 1 000 000: never for a crop).  The batched path keeps every point; an option value that could trigger the subsampling
    # is refused instead of being ignored (crop=False: checked per frame against the image's own grid).
    def check_max_queries(size_wh):
        max_points = int(size_wh[0] // opts.grid_cell_size) * int(size_wh[1] // opts.grid_cell_size)
        if opts.max_num_queries < max_points:
            raise NotImplementedError(f"max_num_queries={opts.max_num_queries} could subsample the {max_points} grid points of a {size_wh[0]}x{size_wh[1]} input: not on the batched path")
    if opts.crop:
        check_max_queries(opts.crop_size)
    return refine, check_max_queries


def _annotated(inst, eval_model) -> bool:
    return eval_model is not None and getattr(inst.get("gt_anno"), "pose", None) is not None


def _frame_targets(opts: InferOpts, object_lid: int, frame: Dict[str, Any],
                   num_target_insts: Optional[Dict[Tuple[int, int], int]]) -> Optional[Tuple[List[Any], int]]:
    """(the object's annotations in the frame, its number of target instances), or None when the frame is not one of this object's.
    task "detection": a frame is every object's when the targets name it (or there are none); the count is not read (0 is returned) and a
    frame whose annotations show none of this object goes on with an empty list -- a pose estimated there is a false positive that must
    reach the csv."""
    scene_id, im_id = frame["scene_id"], frame["im_id"]
    if opts.task == "detection":
        if num_target_insts is not None and (scene_id, im_id) not in num_target_insts:
            return None
        annos = [a for a in (frame.get("gt_annos") or [])
                 if getattr(a, "lid", object_lid) == object_lid and not np.isnan(getattr(a, "visibilities", 1.0))
                 and getattr(a, "visibilities", 1.0) > opts.min_visibility]
        return annos, 0
    # number of target instances (infer.py:308-321): from the test targets when given -- frames that are not a target of
    # this object, or whose count is 0, are skipped -- otherwise the number of ground-truth annotations of the frame
    # ground-truth annotations of this object that are sufficiently visible (infer.py:286-305): a frame that HAS annotations but
    # none of them qualifies is skipped; a frame without annotations (sample.objects_anno is None) goes on with an empty list
    object_annos = []
    if frame.get("gt_annos") is not None:
        object_annos = [a for a in frame["gt_annos"]
                        if getattr(a, "lid", object_lid) == object_lid and not np.isnan(getattr(a, "visibilities", 1.0))
                        and getattr(a, "visibilities", 1.0) > opts.min_visibility]
        if len(object_annos) == 0:
            return None
    if num_target_insts is not None:
        if (scene_id, im_id) not in num_target_insts:
            return None
        n_target = int(num_target_insts[(scene_id, im_id)])
    else:
        n_target = len(object_annos)     # infer.py:317: no targets and no annotations -> 0 -> the frame is skipped
    if n_target == 0:
        return None
    return object_annos, n_target


def detection_predictions(opts: InferOpts, preds: Optional[Sequence[Dict[str, Any]]]) -> List[Dict[str, Any]]:
    """task "detection": the detections of one (scene, image, object) that get a pose -- those with score >= detection_min_score, best first
    (equal scores in file order), at most detection_max_per_object.  No instance count is involved."""
    preds = preds or []
    order = sorted((i for i in range(len(preds)) if preds[i]["score"] >= opts.detection_min_score), key=lambda i: preds[i]["score"], reverse=True)
    return [preds[i] for i in order[:opts.detection_max_per_object]]


def detection_targets(num_target_insts, lids: Sequence[int]) -> Optional[Dict[int, Dict[Tuple[int, int], int]]]:
    """task "detection": the drivers' num_target_insts -- None, a collection of (scene_id, im_id), or the localization task's {lid:
    {(scene_id, im_id): count}}, whose counts and object ids are not read -- as {lid: {(scene_id, im_id): 0}} with EVERY target image under
    EVERY object of the run."""
    if num_target_insts is None:
        return None
    if isinstance(num_target_insts, dict) and all(isinstance(v, dict) for v in num_target_insts.values()):
        images = [k for v in num_target_insts.values() for k in v]
    else:
        images = list(num_target_insts)
    images = list(dict.fromkeys((int(s), int(i)) for s, i in images))
    return {lid: dict.fromkeys(images, 0) for lid in lids}


def select_instances(opts: InferOpts, object_lid: int, frame: Dict[str, Any], detections: Dict[Any, Any],
                     num_target_insts: Optional[Dict[Tuple[int, int], int]], eval_model: Optional[eval_util.EvalModel],
                     detection_times: Dict[Tuple[int, int], float]) -> List[Tuple[int, Dict[str, Any]]]:
    """The instances of `object_lid` in one frame that get a pose: [(instance id, instance)] in instance order, empty when the frame is not
    one of this object's.  Both drivers select with this function (infer_batched's device_masks path: with
    select_instances_device, the same rules).  detection_times (PoseEvaluator.detection_times) receives the
    detector's time of the frame."""
    scene_id, im_id, cam = frame["scene_id"], frame["im_id"], frame["camera"]
    tgt = _frame_targets(opts, object_lid, frame, num_target_insts)
    if tgt is None:
        return []
    object_annos, n_target = tgt
    if opts.task == "detection":   # the chosen detections stand in for the file's: get_instances_for_pose_estimation keeps all of them, in this order
        chosen = detection_predictions(opts, detections.get((scene_id, im_id, object_lid)))
        detections, max_num_preds = ({(scene_id, im_id, object_lid): chosen} if chosen else {}), len(chosen)
    else:
        max_num_preds = int(opts.num_preds_factor * n_target)
    instances = infer_pose_util.get_instances_for_pose_estimation(
        scene_id, im_id, object_lid, opts.use_detections, detections, max_num_preds, object_annos, (cam.width, cam.height))
    kept = []
    for inst_j, inst in enumerate(instances):
        detection_times[(scene_id, im_id)] = inst.get("time", 0) if opts.use_detections else 0
        if opts.task == "detection" and _annotated(inst, eval_model) and inst["gt_iou"] < 0.05:
            inst = dict(inst, gt_anno=None)   # no annotation is this detection's: it is kept and recorded without one, not dropped
        # infer.py:770-777: a detection that hardly overlaps its ground-truth annotation is not evaluated (applied on the
        # evaluation path only: the annotation-free entries stay what they were)
        if opts.use_detections and _annotated(inst, eval_model) and infer_pose_util.mask_iou(inst["input_mask_modal"], inst["gt_anno"].masks_modal) < 0.05:
            continue
        if inst["input_mask_modal"].sum() > cam.width * cam.height:  # infer.py:388-392
            continue
        if inst["input_mask_modal"].sum() == 0:
            continue
        kept.append((inst_j, inst))
    return kept


def select_instances_device(opts: InferOpts, lids: Sequence[int], frame: Dict[str, Any], detections: Dict[Any, Any],
                            num_target_insts: Optional[Dict[int, Dict[Tuple[int, int], int]]],
                            eval_models: Optional[Dict[int, Optional[eval_util.EvalModel]]],
                            detection_times_by_lid: Dict[int, Dict[Tuple[int, int], float]]) -> Dict[int, List[Tuple[int, Dict[str, Any]]]]:
    """select_instances for ALL objects of a frame at once, the detections' masks decoded and opened on the device
    (infer_pose_util.instances_on_device): {lid: [(instance id, instance)]}, for every lid what select_instances
    returns -- the same targets, the same detections in the same order, the same three filters, evaluated from the masks' areas and their
    overlap counts instead of the masks -- except that "input_mask_modal" is a uint8 [H, W] tensor on the device.  use_detections=False
    keeps the host path: those masks are annotations, not run lengths."""
    if not opts.use_detections:
        return {lid: select_instances(opts, lid, frame, detections, None if num_target_insts is None else num_target_insts.get(lid, {}),
                                      None if eval_models is None else eval_models.get(lid), detection_times_by_lid[lid]) for lid in lids}
    scene_id, im_id, cam = frame["scene_id"], frame["im_id"], frame["camera"]
    preds_by_lid, annos_by_lid = {}, {}
    for lid in lids:
        tgt = _frame_targets(opts, lid, frame, None if num_target_insts is None else num_target_insts.get(lid, {}))
        preds = None if tgt is None else detections.get((scene_id, im_id, lid))
        if opts.task == "detection":
            preds = detection_predictions(opts, preds) or None
        if preds is not None:
            annos_by_lid[lid] = tgt[0]
            preds_by_lid[lid] = preds if opts.task == "detection" else infer_pose_util._top_predictions(preds, int(opts.num_preds_factor * tgt[1]))
    instances = infer_pose_util.instances_on_device(preds_by_lid, (cam.width, cam.height), annos_by_lid)
    kept = {lid: [] for lid in lids}
    for lid, insts in instances.items():
        eval_model = None if eval_models is None else eval_models.get(lid)
        for inst_j, inst in enumerate(insts):
            detection_times_by_lid[lid][(scene_id, im_id)] = inst.get("time", 0)
            if opts.task == "detection" and _annotated(inst, eval_model) and inst["gt_iou"] < 0.05:
                inst = dict(inst, gt_anno=None)
            if _annotated(inst, eval_model) and inst["gt_iou"] < 0.05:   # (gt_iou is mask_iou with the chosen annotation: one quotient of the same integers)
                continue
            if inst["mask_area"] > cam.width * cam.height:
                continue
            if inst["mask_area"] == 0:
                continue
            kept[lid].append((inst_j, inst))
    return kept


def _to_device_image(img) -> torch.Tensor:
    """A frame's image (HWC uint8 or float [0,1], numpy or tensor) -> float32 [H, W, 3] in [0,1] on the device."""
    if not isinstance(img, torch.Tensor):
        arr = np.asarray(img)
        img = torch.from_numpy(arr if arr.flags.writeable else arr.copy())   # (PIL hands out read-only arrays)
    return (img.to("cuda", torch.float32) / 255.0) if img.dtype == torch.uint8 else img.to("cuda", torch.float32)


def _bbox_diagonal_fraction(repre, fraction: float) -> float:
    """fraction x the diagonal of the bounding box of repre.vertices (mm), computed on the host."""
    v = repre.vertices.detach().cpu().numpy().astype(np.float64)
    return fraction * float(np.linalg.norm(v.max(0) - v.min(0)))


def depth_refine_tau(opts: InferOpts, repre) -> float:
    """The truncation distance of the depth refinement for one object (mm), computed once per object on the host."""
    return float(opts.depth_refine_max_dist) if opts.depth_refine_max_dist > 0 else _bbox_diagonal_fraction(repre, 0.1)


def depth_pnp_tau(opts: InferOpts, repre) -> float:
    """The 3D inlier threshold of pnp_type "kabsch_depth" for one object (mm), computed once per object on the host."""
    return float(opts.depth_pnp_inlier_thresh) if opts.depth_pnp_inlier_thresh > 0 else _bbox_diagonal_fraction(repre, 0.05)


def depth_verify_tau(opts: InferOpts, repre) -> float:
    """The tolerance of coarse_select_type "depth_verify" for one object (mm), computed once per object on the host."""
    return float(opts.depth_verify_thresh) if opts.depth_verify_thresh > 0 else _bbox_diagonal_fraction(repre, 0.02)


def _check_frame_depth(frame: Dict[str, Any], why: str = "the final pose type refines against depth") -> None:
    """A frame that has work under a depth pose type, a depth PnP type or a depth select type must carry "depth" of the camera's size: refused by name otherwise."""
    cam, d = frame["camera"], frame.get("depth")
    where = f"scene {frame['scene_id']} image {frame['im_id']}"
    if d is None:
        raise ValueError(f"{where}: {why}, but the frame carries no \"depth\"")
    if tuple(d.shape) != (cam.height, cam.width):
        raise ValueError(f"{where}: depth is {tuple(d.shape)}, the camera's image is ({cam.height}, {cam.width})")


def _depth_reason(opts: InferOpts) -> str:
    if opts.pnp_type in DEPTH_PNP_TYPES:
        return f"pnp_type '{opts.pnp_type}' solves the coarse poses on depth"
    if opts.coarse_select_type in DEPTH_SELECT_TYPES:
        return f"coarse_select_type '{opts.coarse_select_type}' checks the coarse poses against depth"
    return "the final pose type refines against depth"


def _frame_depth(frame: Dict[str, Any], why: str = "the final pose type refines against depth") -> torch.Tensor:
    """A frame's "depth" (float32 mm [H, W], numpy or tensor, 0 = no measurement) on the device."""
    _check_frame_depth(frame, why)
    d = frame["depth"]
    if not isinstance(d, torch.Tensor):
        arr = np.asarray(d)
        d = torch.from_numpy(arr if arr.flags.writeable else arr.copy())
    return d.to("cuda", torch.float32)


def _stage_times(eng, n: int, t0: float, t1: float, t2: float, t3: float, t4: float, t5: Optional[float]) -> Dict[str, float]:
    """The reference's per-detection `times` keys (infer.py:464-633, persisted by eval_util.py:327).  The detections between t0 and t5
    ran as ONE batch of n, so every instance is charged its share of the batch; the four stages inside infer_batch come
    from HIP events on the stream (their sum is the device time of t1..t2, the host-side remainder is in feat_extract)."""
    st = eng.stage_times()
    dev_sum = sum(st.values())
    times = {"prep": (t1 - t0) / n,
             "feat_extract": (st.get("feat_extract", 0.0) + max(0.0, (t2 - t1) - dev_sum)) / n,
             "grid_sample": st.get("grid_sample", 0.0) / n, "proj": st.get("proj", 0.0) / n, "corresp": st.get("corresp", 0.0) / n,
             "pose_coarse": (t3 - t2) / n, "final_select": (t4 - t3) / n}
    if t5 is not None:
        times["pose_refine"] = (t5 - t4) / n
    return times


def _refine_final(opts: InferOpts, res, best, bank: DeviceBank, det_obj, frame_cams, cams, crop_size, depth, image_index, taus, masks=None):
    """The final pose of a batch for the refining pose types: featuremetric in the cameras PnP solved in, then / or against the frames' depth
    in the frames' own cameras, or on both in one objective in the frames' cameras, or (after the optional featuremetric stage) against the detections' `masks` in the frames' cameras (refine_util).  Its time is times["pose_refine"].  -> (R [n, 3, 3], t [n, 3]) numpy, in the solve cameras."""
    pose = best
    if opts.final_pose_type in JOINT_POSE_TYPES:
        pose = refine_util.refine_best_coarse_rgbd(res, best, bank, det_obj, frame_cams, cams, crop_size, depth, image_index, taus,
                                                   opts.depth_refine_weight, opts.refine_iters)
        return pose["R"].cpu().numpy(), pose["t"].cpu().numpy()
    if opts.final_pose_type in ("featuremetric", "featuremetric_depth", "featuremetric_mask"):
        ref = refine_util.refine_best_coarse(res, best, bank, det_obj, cams, crop_size, opts.refine_iters)
        pose = dict(best, R=ref["R"], t=ref["t"])
    if opts.final_pose_type in DEPTH_POSE_TYPES:
        pose = refine_util.refine_best_coarse_depth(res, pose, bank, det_obj, frame_cams, cams, depth, image_index, taus, opts.depth_refine_iters)
    if opts.final_pose_type in MASK_POSE_TYPES:
        pose = refine_util.refine_best_coarse_mask(pose, bank, det_obj, frame_cams, cams, masks, opts.mask_refine_huber_px, opts.mask_refine_iters,
                                                   opts.mask_refine_max_points, opts.mask_refine_max_contour)
    return pose["R"].cpu().numpy(), pose["t"].cpu().numpy()


def _record_poses(evaluator: eval_util.PoseEvaluator, opts: InferOpts, object_lid: int, repre, vertices: np.ndarray,
                  eval_model: Optional[eval_util.EvalModel], res, records, times: Dict[str, float]) -> None:
    """The found poses of ONE object out of a batch into its evaluator, in the order given.  records: (row of the detection in `res`,
    scene_id, im_id, instance id, instance, the frame's camera, the camera PnP solved in, id of the best correspondence set, R, t)."""
    pending = []   # consecutive annotated hypotheses: evaluated in one launch, recorded in instance order

    def flush():
        if pending:
            evaluator.update_batch(pending)
            pending.clear()
    for b, scene_id, im_id, inst_j, inst, cam, crop_cam, cid, R, t in records:
        corr_all = res.corresp_list(b)
        c = corr_all[cid]
        corresp_np = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
        T_m2c = np.eye(4)
        T_m2c[:3, :3], T_m2c[:3, 3] = R, t
        T_m2w = crop_cam.T_world_from_eye @ T_m2c  # infer.py:661-666
        if _annotated(inst, eval_model):   # infer.py:806-835
            pred_mask = inst["input_mask_modal"]
            if isinstance(pred_mask, torch.Tensor):   # infer_batched's device_masks path: only an evaluated mask ever reaches the host
                pred_mask = pred_mask.cpu().numpy()
            bank_cams = repre.template_cameras_cam_from_model   # (a bank without template cameras: no template orientation error)
            tpl_cams = [bank_cams[int(cc["template_id"])] for cc in corr_all] if len(bank_cams) else []
            pending.append(dict(scene_id=scene_id, im_id=im_id, inst_id=inst_j, hypothesis_id=0, base_image=None, object_repre_vertices=vertices,
                                obj_lid=object_lid, object_pose_m2w=(T_m2w[:3, :3], T_m2w[:3, 3:]), object_pose_m2w_gt=inst["gt_anno"].pose,
                                orig_camera_c2w=cam, camera_c2w=crop_cam, pred_mask=pred_mask, gt_mask=inst["gt_anno"].masks_modal,
                                corresp=corresp_np, retrieved_templates_camera_m2c=tpl_cams, time_per_inst=times,
                                object_mesh_vertices=eval_model.pts, object_syms=eval_model.syms, object_diameter=eval_model.diameter,
                                inlier_radius=opts.pnp_inlier_thresh))
            continue
        flush()
        evaluator.update_without_anno(scene_id, im_id, inst_j, 0, vertices, object_lid, T_m2w[:3, :3], T_m2w[:3, 3], cam, crop_cam, times, corresp_np,
                                      inlier_radius=10)
    flush()


# ---------------------------------------------------------------------------------------------------- one flush for both drivers
class QueuedDetection(NamedTuple):
    """One kept instance waiting for its batch."""
    frame_no: int                   # running number of its frame in the stream
    size: Tuple[int, int]           # (width, height) of that frame's image
    obj: int                        # object index: the position of its lid in the sorted lids = its object in the DeviceBank
    group_index: int                # its index among the kept instances of its own (frame, object) group
    inst_id: int = 0
    inst: Optional[Dict[str, Any]] = None
    frame: Optional[Dict[str, Any]] = None   # the frame itself: alive as long as a queued detection refers to it


def iter_batches(entries: Iterable[QueuedDetection], batch_detections: int):
    """The flush rule: a batch goes out when `batch_detections` are queued, when the next detection's frame has another image size than the
    queued ones (one batch is one stack of images), and when the stream ends.  Lazy: nothing is read ahead of the batch being filled."""
    if batch_detections < 1:
        raise ValueError(f"batch_detections must be >= 1, got {batch_detections}")
    queue: List[QueuedDetection] = []
    for e in entries:
        if queue and e.size != queue[0].size:
            yield queue
            queue = []
        queue.append(e)
        if len(queue) == batch_detections:
            yield queue
            queue = []
    if queue:
        yield queue


class FlushPlan(NamedTuple):
    order: List[int]             # batch row -> position in the queue: the queue stable-sorted by object index
    det_obj: List[int]           # batch row -> object index (ascending)
    image_index: List[int]       # batch row -> position of its frame in `frames`
    pair_group_index: List[int]  # batch row -> group_index of the detection (the RANSAC sampler key of slot j is group_index * n + j)
    frames: List[int]            # frame_no of the images to stack, in queue order


def plan_flush(queue: Sequence[QueuedDetection]) -> FlushPlan:
    """Rows of one batch: the engine takes detections grouped by object, so the queue is stable-sorted by object index (within an object
    the order stays frame, then instance); every row remembers which of the batch's stacked images it reads and its sampler key group."""
    order = sorted(range(len(queue)), key=lambda i: queue[i].obj)   # sorted() is stable
    frames = list(dict.fromkeys(e.frame_no for e in queue))
    slot = {f: i for i, f in enumerate(frames)}
    return FlushPlan(order, [queue[i].obj for i in order], [slot[queue[i].frame_no] for i in order], [queue[i].group_index for i in order], frames)


def single_group_plan(n: int) -> FlushPlan:
    """plan_flush of the per-object driver's queue -- the n kept instances of ONE (frame 0, object 0) group, in order -- without the sort."""
    return FlushPlan(list(range(n)), [0] * n, [0] * n, list(range(n)), [0])


def _extractor_on_device(opts: InferOpts, extractor, precision: str, weights: Optional[str]):
    if extractor is None:  # infer.py:125-128; the checkpoint: weights=, $FOUNDPOSE_DINOV2_WEIGHTS or the torch hub cache, else this raises
        extractor = feature_util.make_feature_extractor(opts.extractor_name, precision=precision, weights=weights).to("cuda")
    return extractor


class _Pipeline:
    """What a driver call sets up once and every flush reads, over `repres` in bank order (models, vertices and the taus: one per object).
    Everything a driver refuses is refused here (_check_driver_opts), before any device work."""

    def __init__(self, opts: InferOpts, extractor, repres: Sequence[repre_util.FeatureBasedObjectRepre],
                 models: Sequence[Optional[eval_util.EvalModel]], seed: int, precision: str = "bf16", weights: Optional[str] = None) -> None:
        self.opts, self.models, self.seed = opts, list(models), seed
        self.refine, self.check_max_queries = _check_driver_opts(opts)
        self.use_depth = opts.final_pose_type in DEPTH_POSE_TYPES        # the final pose is refined against depth,
        self.depth_pnp = opts.pnp_type in DEPTH_PNP_TYPES                # the coarse poses are solved on it,
        self.verify = opts.coarse_select_type in DEPTH_SELECT_TYPES      # the coarse hypotheses are checked against it
        self.mask_verify = opts.coarse_select_type in MASK_SELECT_TYPES  # ... or against the detection's mask
        self.mask_refine = opts.final_pose_type in MASK_POSE_TYPES       # the final pose is refined against the detection's mask: no depth
        self.extractor = _extractor_on_device(opts, extractor, precision, weights)
        self.bank = DeviceBank(list(repres))
        self.eng = fe.FoundPoseEngine(self.extractor, self.bank, opts.grid_cell_size, opts.match_top_n_templates, opts.match_top_k_buddies, tie_order="torch")
        self.eng.record_stage_times = True
        self.vertices = [r.vertices.cpu().numpy() for r in repres]
        self.taus = [depth_refine_tau(opts, r) for r in repres] if self.use_depth else None
        self.pnp_taus = [depth_pnp_tau(opts, r) for r in repres] if self.depth_pnp else None
        self.verify_taus = [depth_verify_tau(opts, r) for r in repres] if self.verify else None


def _check_frame_work(pipe: _Pipeline, frame: Dict[str, Any]) -> None:
    """A frame whose first kept detection is being queued: it must carry the depth the options read and, with crop=False (infer.py:355-357,
    411-416: the whole image and the modal mask of every instance go to the extractor unchanged), tile into patches -- the backbone's patch
    embedding asserts it in the reference as well -- and have no more grid points than max_num_queries."""
    opts = pipe.opts
    if pipe.use_depth or pipe.depth_pnp or pipe.verify:
        _check_frame_depth(frame, _depth_reason(opts))
    if not opts.crop:
        h, w = np.shape(frame["image"])[:2]
        ps = pipe.extractor.patch_size
        if h % ps or w % ps:
            raise AssertionError(f"Input image height {h} / width {w} is not a multiple of patch size {ps} (crop=False)")
        pipe.check_max_queries((frame["camera"].width, frame["camera"].height))


class _Flush(NamedTuple):
    """What one flush leaves behind; every per-detection field is in batch order (FlushPlan.order)."""
    rows: List[QueuedDetection]
    crops: torch.Tensor
    crop_masks: torch.Tensor
    cams: List[Any]                  # the cameras the poses are solved in: the crop cameras, or the frames' own with crop=False
    res: Any                         # the engine's MatchResult
    best: Dict[str, torch.Tensor]    # the coarse selection (on the device)
    found: List[bool]
    cid: List[int]                   # id of the best correspondence set
    R: np.ndarray                    # the final poses, in `cams`
    t: np.ndarray
    refined: bool                    # a refinement ran: R, t are not best's, and times has "pose_refine"
    times: Dict[str, float]


def _run_flush(pipe: _Pipeline, queue: Sequence[QueuedDetection], plan: FlushPlan, *, device_masks: bool = False,
               keep_feature_map: bool = False) -> _Flush:
    """One batch through upload, crop cameras and warp, the engine, the coarse poses, their verification, the selection and the refinement:
    the body of both drivers.  device_masks: the queue's masks are uint8 tensors on the device already; keep_feature_map: the engine keeps
    the projected feature map even where no refinement needs it (for the pictures)."""
    opts, eng, bank = pipe.opts, pipe.eng, pipe.bank
    t0 = time.perf_counter()
    dets = [queue[i] for i in plan.order]
    by_no = {e.frame_no: e.frame for e in queue}
    images = torch.stack([_to_device_image(by_no[f]["image"]) for f in plan.frames])
    if device_masks:   # views into their frames' stacks: nothing is uploaded
        masks = torch.stack([e.inst["input_mask_modal"] for e in dets])
    else:
        masks = torch.from_numpy(np.stack([e.inst["input_mask_modal"] for e in dets]).astype(np.uint8)).cuda()
    src_cams = [e.frame["camera"] for e in dets]
    if opts.crop:
        cams = []
        for e in dets:
            b = e.inst["input_box_amodal"].tolist()
            box = crop_util.calc_crop_box(crop_util.AlignedBox2f(b[0], b[1], b[2], b[3]), make_square=True)
            cams.append(crop_util.construct_crop_camera(box, e.frame["camera"], tuple(opts.crop_size), opts.crop_rel_pad))
        crops, crop_masks = crop_util.warp_crops(images, masks, src_cams, cams, plan.image_index)
    else:   # crop=False: every detection gets its frame's whole image and solves in the frame's own camera (_check_frame_work)
        crops = images[torch.as_tensor(plan.image_index, device=images.device)].permute(0, 3, 1, 2).contiguous()
        crop_masks, cams = masks, src_cams
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    res = eng.infer_batch(crops, crop_masks, plan.det_obj, keep_feature_map=pipe.refine or keep_feature_map)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    n_slots = int(res.counts.shape[1])
    keys = [[g * n_slots + j for j in range(n_slots)] for g in plan.pair_group_index]

    @functools.lru_cache(maxsize=None)   # made once, on first need: the upload is part of the stage that asks first
    def depth():   # the depth images of the flush, stacked like its RGB images and read through plan.image_index
        return torch.stack([_frame_depth(by_no[f], _depth_reason(opts)) for f in plan.frames])
    depth_kw = {}
    if pipe.depth_pnp:
        depth_kw = dict(frame_cameras=src_cams, depth=depth(), image_index=plan.image_index, depth_inlier_thresh_mm=[pipe.pnp_taus[o] for o in plan.det_obj])
    poses = pnp_util.estimate_poses(res, cams, opts.pnp_type, opts.pnp_ransac_iter, opts.pnp_inlier_thresh, opts.pnp_required_ransac_conf,
                                    opts.pnp_refine_lm, seed=pipe.seed, pair_keys=keys, **depth_kw)
    checked = None
    if pipe.verify:   # every hypothesis against its frame's depth; part of pose_coarse
        checked = pnp_util.verify_poses_depth(poses, bank, plan.det_obj, cams, src_cams, depth(), plan.image_index,
                                              [pipe.verify_taus[o] for o in plan.det_obj], max_points=opts.depth_verify_max_points)
    elif pipe.mask_verify:   # ... or against its detection's mask in its frame's image; part of pose_coarse
        checked = pnp_util.verify_poses_mask(poses, bank, plan.det_obj, cams, src_cams, masks,
                                             max_points=opts.mask_verify_max_points, grid=opts.mask_verify_grid)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    best = pnp_util.select_best_coarse(poses) if checked is None else pnp_util.select_best_verified(poses, checked)
    found, cid = best["found"].cpu().tolist(), best["corresp_id"].cpu().tolist()
    Rb, tb = best["R"].cpu().numpy(), best["t"].cpu().numpy()
    t4 = time.perf_counter()
    t5 = None
    if pipe.refine or pipe.use_depth or pipe.mask_refine:   # infer.py:619: the refined pose of the best coarse pose is the final pose
        Rb, tb = _refine_final(opts, res, best, bank, plan.det_obj, src_cams, cams, (crops.shape[-1], crops.shape[-2]),
                               depth() if pipe.use_depth else None, plan.image_index,
                               [pipe.taus[o] for o in plan.det_obj] if pipe.use_depth else None, masks if pipe.mask_refine else None)
        t5 = time.perf_counter()
    return _Flush(dets, crops, crop_masks, cams, res, best, found, cid, Rb, tb, t5 is not None, _stage_times(eng, len(dets), t0, t1, t2, t3, t4, t5))


def infer_object(opts: InferOpts, object_lid: int, repre: repre_util.FeatureBasedObjectRepre, frames: Iterable[Dict[str, Any]],
                 detections: Dict[Any, Any], extractor=None, num_target_insts: Optional[Dict[Tuple[int, int], int]] = None,
                 precision: str = "bf16", seed: int = 0, weights: Optional[str] = None,
                 eval_model: Optional[eval_util.EvalModel] = None, renderer=None, output_dir: Optional[str] = None,
                 frame_poses: Optional[Dict[Tuple[int, int], List[Tuple[int, np.ndarray]]]] = None) -> eval_util.PoseEvaluator:
    """One object over a stream of frames (the body of infer.py's per-object loop).  A frame is
    {"scene_id", "im_id", "image": HWC uint8 or float [0,1] (numpy or tensor), "camera": PinholePlaneCameraModel (c2w)} and, for the
    depth-reading options (the final pose types of DEPTH_POSE_TYPES, pnp_type "kabsch_depth", coarse_select_type "depth_verify"), "depth":
    float32 mm [H, W] (numpy or tensor, 0 = no measurement).
    eval_model (eval_util.load_eval_model): instances whose annotation carries a ground-truth `pose` (model -> world) are
    evaluated against it (PoseEvaluator.update_batch, one launch per frame, inlier radius opts.pnp_inlier_thresh as in
    infer.py:831); without it, or for annotations without a pose, the driver records what it always has.
    renderer (a HipRasterizer holding this object's mesh under `object_lid`) together with opts.vis_results: one picture per estimated
    pose is written to vis_util.tile_path(output_dir, ...) and its share of the time recorded as times["vis"]; frame_poses, when
    given, collects (object_lid, T_m2c in the frame's own camera) per (scene_id, im_id) for the frame summaries.  Without a renderer
    nothing of this runs, whatever vis_results says."""
    vis = renderer is not None and bool(opts.vis_results)
    if vis:   # refused before any device work
        vis_util.check_opts(opts)
        if output_dir is None:
            raise ValueError("pictures need an output_dir")
    pipe = _Pipeline(opts, extractor, [repre], [eval_model], seed, precision, weights)
    evaluator = eval_util.PoseEvaluator()
    vis_templates = repre.templates.cuda() if vis else None

    for frame in frames:
        scene_id, im_id, cam = frame["scene_id"], frame["im_id"], frame["camera"]
        kept = select_instances(opts, object_lid, frame, detections, num_target_insts, eval_model, evaluator.detection_times)
        if not kept:
            continue
        _check_frame_work(pipe, frame)
        n = len(kept)
        queue = [QueuedDetection(0, (cam.width, cam.height), 0, i, inst_j, inst, frame) for i, (inst_j, inst) in enumerate(kept)]
        fl = _run_flush(pipe, queue, single_group_plan(n), keep_feature_map=vis)
        cams, res, best, found, cid, Rb, tb, times = fl.cams, fl.res, fl.best, fl.found, fl.cid, fl.R, fl.t, fl.times
        if vis:   # compositing on the device, one copy of the batch's tiles to pinned memory, PNG encoding on the host
            tv = time.perf_counter()
            to_T = lambda R, t: np.block([[np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3, 1)], [np.array([[0.0, 0.0, 0.0, 1.0]])]])
            coarse = [to_T(best["R"][b].cpu().numpy(), best["t"][b].cpu().numpy()) if found[b] else None for b in range(n)] if fl.refined else [None] * n
            final = [to_T(Rb[b], tb[b]) if found[b] else None for b in range(n)]
            gt_pose = [getattr(inst.get("gt_anno"), "pose", None) for _, inst in kept]
            gt = [None if p is None else np.linalg.inv(cams[b].T_world_from_eye) @ to_T(p.R, p.t) for b, p in enumerate(gt_pose)]
            tiles, vis_records = vis_util.vis_inference_results_batch(
                fl.crops, fl.crop_masks, cams, res, found, cid, coarse, final, repre, renderer, object_lid, extractor=pipe.extractor,
                poses_gt=gt if any(g is not None for g in gt) else None, draw_coarse=fl.refined, vis_corresp_top_n=opts.vis_corresp_top_n,
                vis_feat_map=opts.vis_feat_map, vis_for_paper=opts.vis_for_paper, templates=vis_templates)
            host = vis_util.tiles_to_host(tiles)
            for b, (inst_j, _) in enumerate(kept):
                if found[b]:
                    vis_util.write_png(vis_util.tile_path(output_dir, scene_id, im_id, object_lid, inst_j, 0), host[b])
                    for note in vis_records[b]["notes"]:
                        print(f"vis: scene {scene_id} image {im_id} object {object_lid} instance {inst_j}: {note}")
            times["vis"] = (time.perf_counter() - tv) / n
        records = []
        for b, (inst_j, inst) in enumerate(kept):
            if not found[b]:
                continue
            if vis and frame_poses is not None:
                T_m2c = np.eye(4)
                T_m2c[:3, :3], T_m2c[:3, 3] = Rb[b], tb[b]
                frame_poses.setdefault((scene_id, im_id), []).append((object_lid, np.linalg.inv(cam.T_world_from_eye) @ (cams[b].T_world_from_eye @ T_m2c)))
            records.append((b, scene_id, im_id, inst_j, inst, cam, cams[b], cid[b], Rb[b], tb[b]))
        _record_poses(evaluator, opts, object_lid, repre, pipe.vertices[0], eval_model, res, records, times)
    return evaluator


def _select_frame_poses(opts: InferOpts, repres: Dict[int, repre_util.FeatureBasedObjectRepre], lids: Sequence[int], csv_path: str) -> List[str]:
    """frame_select_type "pose_nms" (DESIGN.md section 20), after the per-object estimated-poses.json files and the csv of every pose are
    written: the poses of each frame compared with each other (pose_nms.suppress_duplicates, samples from the repres' vertices), the csv
    written again with the kept rows only -- the stage's wall time, divided equally over the images that have rows, added to their `time`
    -- and every row's decision written to pose-nms.json beside it.  -> the paths written besides the csv."""
    _check_driver_opts(opts)
    rows = eval_bop19.load_results_csv(csv_path)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    samples = pose_nms.samples_from_vertices({lid: repres[lid].vertices for lid in lids}, opts.pose_nms_max_points)
    result = pose_nms.suppress_duplicates(rows, samples, opts.pose_nms_thresh, opts.pose_nms_grid, opts.pose_nms_cross_object)
    torch.cuda.synchronize()
    images = {(r["scene_id"], r["im_id"]) for r in rows}
    share = (time.perf_counter() - t0) / max(len(images), 1)
    pose_nms.write_results_csv(csv_path, [dict(r, time=r["time"] + share) for i, r in enumerate(rows) if result["keep"][i]])
    path = os.path.join(os.path.dirname(csv_path), "pose-nms.json")
    with open(path, "w") as f:
        json.dump(pose_nms.decision_records(rows, result), f, indent=1)
    return [path]


def _fuse_scene_poses(opts: InferOpts, scene_cameras, scene_models, csv_path: str) -> List[str]:
    """scene_select_type "multiview" (DESIGN.md section 37), after the csv is written and after frame_select_type has had its turn with it
    (a frame's duplicates are gone before views are matched): the rows of every scene whose images all carry cam_R_w2c / cam_t_w2c fused
    (multiview.fuse_results), the csv written again -- same rows, same order; the stage's wall time, divided equally over the images that
    have rows, added to their `time` --, and every row's and cluster's record written to scene-fuse.json beside it.  A run without camera
    poses leaves the csv's bytes as they are and the file says why.  -> the paths written besides the csv."""
    _check_driver_opts(opts)
    rows = eval_bop19.load_results_csv(csv_path)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    present = {r["obj_id"] for r in rows}
    if scene_models is None or any(lid not in scene_models for lid in present):
        raise ValueError("scene_select_type 'multiview' needs the objects' models (diameter and symmetries: models_info.json and the meshes of "
                         f"--models-dir); missing for {sorted(present - set(scene_models or {}))}")
    fused, report = multiview.fuse_results(rows, scene_cameras or {}, scene_models, _scene_fuse_opts(opts))
    torch.cuda.synchronize()
    if any(r["fused"] for r in report["rows"]):   # nothing fused: the csv keeps its bytes, its times included
        images = {(r["scene_id"], r["im_id"]) for r in rows}
        share = (time.perf_counter() - t0) / max(len(images), 1)
        pose_nms.write_results_csv(csv_path, [dict(r, time=r["time"] + share) for r in fused])
    path = os.path.join(os.path.dirname(csv_path), "scene-fuse.json")
    multiview.write_report(path, report)
    return [path]


def _write_results(opts: InferOpts, lids: Sequence[int], evaluators: Sequence[eval_util.PoseEvaluator],
                   repres: Dict[int, repre_util.FeatureBasedObjectRepre], output_dir: str, scene_cameras=None, scene_models=None) -> List[str]:
    """The files of a run, once every pose is estimated (save_estimates): <output_dir>/<lid>/estimated-poses.json per object (infer.py:813-816),
    the BOP csv, what frame_select_type "pose_nms" does with it and then what scene_select_type "multiview" does.  -> their paths, in this order."""
    paths = []
    if opts.save_estimates:
        for lid, ev in zip(lids, evaluators):
            paths.append(os.path.join(output_dir, str(lid), "estimated-poses.json"))
            ev.save_results_json(paths[-1])
        csv_path = eval_util.prepare_bop_submission(output_dir, opts.object_dataset, lids)
        paths.append(csv_path)
        if opts.frame_select_type == "pose_nms":
            paths.extend(_select_frame_poses(opts, repres, lids, csv_path))
        if opts.scene_select_type == "multiview":
            paths.extend(_fuse_scene_poses(opts, scene_cameras, scene_models, csv_path))
    return paths


def infer(opts: InferOpts, frames_by_object, detections, repres: Dict[int, repre_util.FeatureBasedObjectRepre], output_dir: str, extractor=None,
          precision: str = "bf16", num_target_insts: Optional[Dict[int, Dict[Tuple[int, int], int]]] = None, weights: Optional[str] = None,
          eval_models: Optional[Dict[int, eval_util.EvalModel]] = None, renderer=None, scene_cameras=None, scene_models=None) -> List[str]:
    """All objects: `frames_by_object(lid)` yields the frames that show object `lid`; one estimated-poses.json per object
    under <output_dir>/<lid>/ (infer.py:813-816), then the BOP19 csv.
    num_target_insts: {object lid: {(scene_id, im_id): inst_count}} from test_targets_bop19.json -- the number of poses to
    estimate per (image, object) is num_preds_factor x inst_count (infer.py:308-346); frames without an entry are skipped.
    eval_models: {object lid: eval_util.EvalModel} -- evaluate the hypotheses of frames whose annotations carry a pose.
    scene_cameras / scene_models: with opts.scene_select_type "multiview" (DESIGN.md section 37), {scene_id: the scene's scene_camera.json}
    and {object lid: eval_util.EvalModel}; read by nothing else.
    renderer: a HipRasterizer holding the mesh of every object under its lid -- with opts.vis_results, one picture per estimated pose
    (<output_dir>/<lid>/<scene>_<im>_<lid>_<inst>_0.png) and, after all objects, one summary per frame (<output_dir>/vis/<scene>_<im>.png)
    with every final pose in the frame's own camera.  Without it no picture is made and nothing else changes.
    opts.task "detection" (DESIGN.md section 21): num_target_insts only names the target images -- a collection of (scene_id, im_id), or
    the dict above with its counts and object ids unread (detection_targets) -- and in each of them every detection of every object with
    score >= detection_min_score gets a pose, at most detection_max_per_object per object; `frames_by_object(lid)` then yields every
    target image."""
    lids = list(opts.object_lids) if opts.object_lids is not None else sorted(repres)
    if opts.task == "detection":
        num_target_insts = detection_targets(num_target_insts, lids)
    if renderer is not None and not opts.vis_results:
        print("vis_results is false in the options: no pictures are written")
        renderer = None
    if renderer is not None:
        vis_util.check_opts(opts)
    frame_poses: Dict[Tuple[int, int], List[Tuple[int, np.ndarray]]] = {}
    extractor = _extractor_on_device(opts, extractor, precision, weights)   # one for all objects
    evaluators = [infer_object(opts, lid, repres[lid], frames_by_object(lid), detections, extractor,
                               num_target_insts=None if num_target_insts is None else num_target_insts.get(lid, {}),
                               eval_model=None if eval_models is None else eval_models.get(lid), renderer=renderer, output_dir=output_dir,
                               frame_poses=frame_poses if renderer is not None else None) for lid in lids]
    paths = _write_results(opts, lids, evaluators, repres, output_dir, scene_cameras, scene_models)
    if renderer is not None and frame_poses:   # the frames are read again rather than kept: one image in memory at a time
        done = set()
        for lid in lids:
            for frame in frames_by_object(lid):
                key = (frame["scene_id"], frame["im_id"])
                if key in done or key not in frame_poses:
                    continue
                done.add(key)
                pic, _, notes = vis_util.vis_frame_summary(frame["image"], frame["camera"], [(o, T, None) for o, T in frame_poses[key]], renderer)
                for note in notes:
                    print(f"vis: scene {key[0]} image {key[1]}: {note}")
                p = vis_util.summary_path(output_dir, *key)
                vis_util.write_png(p, vis_util.tiles_to_host(pic))
                paths.append(p)
    return paths


# ---------------------------------------------------------------------------------------------------- frame-major, cross-object batches
def infer_batched(opts: InferOpts, frames: Iterable[Dict[str, Any]], detections, repres: Dict[int, repre_util.FeatureBasedObjectRepre],
                  output_dir: str, *, batch_detections: int = 32, extractor=None, precision: str = "bf16",
                  num_target_insts: Optional[Dict[int, Dict[Tuple[int, int], int]]] = None, weights: Optional[str] = None,
                  eval_models: Optional[Dict[int, eval_util.EvalModel]] = None, seed: int = 0, renderer=None,
                  device_masks: bool = False, scene_cameras=None, scene_models=None) -> List[str]:
    """infer() for a whole split in ONE pass over its frames: the kept instances of every (frame, object) are queued and go through the
    crop producer, the engine and the PnP tail `batch_detections` at a time, across frames and objects (one DeviceBank of all objects).
    `frames` yields each image once (load_bop_frames_all); `gt_annos` may hold annotations of several objects.  The poses, scores and
    files are those of infer(): the instances are selected by the same function and go through the same flush (_run_flush), in which a
    detection's crop and the engine's results do not depend on the batch, and RANSAC's sampler is keyed by the pair's index in its own
    (frame, object) group -- the per-object driver's whole batch -- instead of its place in the batch.  Pictures are not made here: infer() /
    infer_object() write them.
    device_masks: the detections' run lengths are decoded, opened and cropped on the device (select_instances_device)
    instead of on the host; the masks are the same bits and so is everything written.
    scene_cameras / scene_models: as in infer()."""
    if batch_detections < 1:
        raise ValueError(f"batch_detections must be >= 1, got {batch_detections}")
    if renderer is not None:
        raise NotImplementedError("result pictures are written by the per-object driver (infer.infer / infer.infer_object, batch_detections=0): "
                                  "the batched driver makes none")
    lids = sorted(opts.object_lids) if opts.object_lids is not None else sorted(repres)
    models = [None if eval_models is None else eval_models.get(l) for l in lids]
    pipe = _Pipeline(opts, extractor, [repres[l] for l in lids], models, seed, precision, weights)
    if opts.task == "detection":   # the targets name images only (infer()'s note): every target image under every object
        num_target_insts = detection_targets(num_target_insts, lids)
    evaluators = [eval_util.PoseEvaluator() for _ in lids]

    def entries():
        for frame_no, frame in enumerate(frames):
            cam, checked = frame["camera"], False
            kept_by_lid = None
            if device_masks:
                kept_by_lid = select_instances_device(opts, lids, frame, detections, num_target_insts, dict(zip(lids, models)),
                                                      {lid: evaluators[o].detection_times for o, lid in enumerate(lids)})
            for o, lid in enumerate(lids):
                if kept_by_lid is not None:
                    kept = kept_by_lid[lid]
                else:
                    kept = select_instances(opts, lid, frame, detections, None if num_target_insts is None else num_target_insts.get(lid, {}),
                                            models[o], evaluators[o].detection_times)
                if kept and not checked:   # (only a frame that has work is checked)
                    _check_frame_work(pipe, frame)
                    checked = True
                for i, (inst_j, inst) in enumerate(kept):
                    yield QueuedDetection(frame_no, (cam.width, cam.height), o, i, inst_j, inst, frame)

    for queue in iter_batches(entries(), batch_detections):
        fl = _run_flush(pipe, queue, plan_flush(queue), device_masks=device_masks and opts.use_detections)
        for o, lid in enumerate(lids):   # rows are grouped by object, and within an object in frame, then instance order
            records = [(b, e.frame["scene_id"], e.frame["im_id"], e.inst_id, e.inst, e.frame["camera"], fl.cams[b], fl.cid[b], fl.R[b], fl.t[b])
                       for b, e in enumerate(fl.rows) if e.obj == o and fl.found[b]]
            if records:
                _record_poses(evaluators[o], opts, lid, repres[lid], pipe.vertices[o], models[o], fl.res, records, fl.times)
    return _write_results(opts, lids, evaluators, repres, output_dir, scene_cameras, scene_models)


# ---------------------------------------------------------------------------------------------------- BOP split on disk
class GtAnnotation(NamedTuple):
    """structs.ObjectAnnotation, the fields data_util.prepare_sample fills (utils/data_util.py:105-151)."""
    dataset: str
    lid: int
    pose: Any = None                # GtPose (model -> world) or None
    masks_modal: Optional[np.ndarray] = None
    boxes_amodal: Optional[np.ndarray] = None
    visibilities: Optional[np.ndarray] = None


class GtPose(NamedTuple):
    R: np.ndarray   # 3x3
    t: np.ndarray   # 3x1 (mm)


def load_gt_annotations(scene_dir: str, im_id: int, camera, scene_gt: Dict[str, Any], scene_gt_info: Dict[str, Any], dataset: str = "") -> Optional[List[GtAnnotation]]:
    """The annotations of one image as data_util.prepare_sample builds them: scene_gt.json (cam_R_m2c, cam_t_m2c, obj_id)
    -> the m2w pose T_world_from_eye [R | t]; scene_gt_info.json bbox_obj (x, y, w, h) -> boxes_amodal (x1, y1, x2, y2),
    visib_fract -> visibilities; mask_visib/<im>_<gt>.png / 255 -> masks_modal (uint8).  None when the image has none."""
    from PIL import Image
    gts = scene_gt.get(str(im_id), [])
    if not len(gts) or not len(scene_gt_info):
        return None
    annos = []
    for gt_id, gt in enumerate(gts):
        info = scene_gt_info[str(im_id)][gt_id]
        mask = np.asarray(Image.open(os.path.join(scene_dir, "mask_visib", f"{im_id:06d}_{gt_id:06d}.png"))) / 255.0
        box = info["bbox_obj"]
        T_m2c = np.eye(4)
        T_m2c[:3, :3] = np.array(gt["cam_R_m2c"], np.float64).reshape(3, 3)
        T_m2c[:3, 3] = np.array(gt["cam_t_m2c"], np.float64).reshape(3)
        T_m2w = np.matmul(camera.T_world_from_eye, T_m2c)
        annos.append(GtAnnotation(dataset=dataset, lid=int(gt["obj_id"]), pose=GtPose(T_m2w[:3, :3], T_m2w[:3, 3:]),
                                  masks_modal=np.array(mask, dtype=np.uint8), boxes_amodal=np.array([box[0], box[1], box[0] + box[2], box[1] + box[3]]),
                                  visibilities=np.asarray(info["visib_fract"])))
    return annos


class _SplitReader:
    """The images of a BOP split with their cameras (and annotations): <split>/<scene:06d>/rgb/<im:06d>.{png,jpg} + scene_camera.json (cam_K)."""

    def __init__(self, split_dir: str, with_gt: bool, with_depth: bool = False) -> None:
        self.split_dir, self.with_gt, self.with_depth = split_dir, with_gt, with_depth
        self.cams: Dict[int, Dict[str, Any]] = {}
        self.gts: Dict[int, Tuple[Dict[str, Any], Dict[str, Any]]] = {}

    def frame(self, sid: int, iid: int) -> Dict[str, Any]:
        from PIL import Image
        sdir = os.path.join(self.split_dir, f"{sid:06d}")
        if sid not in self.cams:
            with open(os.path.join(sdir, "scene_camera.json")) as f:
                self.cams[sid] = json.load(f)
        K = np.array(self.cams[sid][str(iid)]["cam_K"], np.float64).reshape(3, 3)
        path = next(p for p in (os.path.join(sdir, "rgb", f"{iid:06d}.png"), os.path.join(sdir, "rgb", f"{iid:06d}.jpg"),
                                os.path.join(sdir, "gray", f"{iid:06d}.tif")) if os.path.exists(p))
        image = np.asarray(Image.open(path).convert("RGB"))
        camera = crop_util.PinholePlaneCameraModel(image.shape[1], image.shape[0], (K[0, 0], K[1, 1]), (K[0, 2], K[1, 2]), np.eye(4))
        frame = {"scene_id": sid, "im_id": iid, "image": image, "camera": camera}
        if self.with_depth:   # depth/<im>.png in depth_scale units -> float32 mm, what the BOP evaluation reads (eval_bop19.load_depth)
            from .eval_bop19 import load_depth
            frame["depth"] = load_depth(os.path.join(sdir, "depth", f"{iid:06d}.png"), float(self.cams[sid][str(iid)].get("depth_scale", 1.0)))
        if self.with_gt:
            if sid not in self.gts:
                with open(os.path.join(sdir, "scene_gt.json")) as f, open(os.path.join(sdir, "scene_gt_info.json")) as g:
                    self.gts[sid] = (json.load(f), json.load(g))
            frame["gt_annos"] = load_gt_annotations(sdir, iid, camera, *self.gts[sid])
        return frame


def load_bop_frames(split_dir: str, targets: Sequence[Dict[str, int]], object_lid: int, with_gt: bool = False, with_depth: bool = False):
    """Frames of a BOP split that show `object_lid` according to test_targets_bop19.json entries
    ({"scene_id", "im_id", "obj_id", "inst_count"}): <split>/<scene:06d>/rgb/<im:06d>.{png,jpg} + scene_camera.json (cam_K).
    with_gt: each frame also carries "gt_annos" from scene_gt.json, scene_gt_info.json and mask_visib/ (load_gt_annotations).
    with_depth: and "depth", float32 mm [H, W], from depth/<im:06d>.png and the frame's depth_scale (eval_bop19.load_depth)."""
    reader = _SplitReader(split_dir, with_gt, with_depth)
    for tgt in targets:
        if tgt.get("obj_id", object_lid) == object_lid:   # an entry without obj_id (test_targets_bop24.json) is every object's
            yield reader.frame(tgt["scene_id"], tgt["im_id"])


def load_bop_frames_all(split_dir: str, targets: Sequence[Dict[str, int]], with_gt: bool = False, with_depth: bool = False):
    """Every image the targets name, ONCE, whatever the number of objects targeted in it, in the order of its first entry (the stream of
    infer_batched).  with_gt: "gt_annos" holds the annotations of all objects of the image.  with_depth: "depth" as in load_bop_frames."""
    reader = _SplitReader(split_dir, with_gt, with_depth)
    seen = set()
    for tgt in targets:
        key = (tgt["scene_id"], tgt["im_id"])
        if key not in seen:
            seen.add(key)
            yield reader.frame(*key)


def main(argv: Optional[Sequence[str]] = None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--opts", required=True, help="options JSON ({'infer_opts': {...}}, e.g. the reference's configs/infer/lmo.json)")
    ap.add_argument("--dataset-dir", required=True, help="BOP split directory (<datasets>/<dataset>/<split>)")
    ap.add_argument("--targets", default=None, help="test_targets_bop19.json (default: <dataset-dir>/../test_targets_bop19.json); with \"task\": "
                    "\"detection\" in the options: test_targets_bop24.json (the default then), of which only scene_id / im_id are read")
    ap.add_argument("--detections", required=True, help="CNOS detections in the BOP format")
    ap.add_argument("--repre-dir", required=True, help="<output>/object_repre (repre.pth under <version>/<dataset>/<lid>/)")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f16", "f16x3", "f16f8", "fp32"])
    ap.add_argument("--weights", default=None, help="DINOv2 checkpoint: a .pth with the upstream key names, or a directory holding the upstream file "
                    "(dinov2_vitl14_pretrain.pth, dinov2_vits14_reg4_pretrain.pth, ...); default $FOUNDPOSE_DINOV2_WEIGHTS, then the torch hub cache. "
                    "Without a checkpoint the run fails: there is no random-weight fallback")
    ap.add_argument("--eval-gt", action="store_true", help="evaluate the poses against the split's ground truth (scene_gt.json, scene_gt_info.json, "
                    "mask_visib/): MSSD, MSPD and the inlier counts go into estimated-poses.json")
    ap.add_argument("--models-dir", default=None, help="with --eval-gt / --vis: models_info.json and obj_XXXXXX.ply (default: <dataset root>/models)")
    ap.add_argument("--vis", action="store_true", help="write the result pictures (when vis_results is true in the options): one tile per estimated pose, "
                    "<output-dir>/<lid>/<scene>_<im>_<lid>_<inst>_0.png (pose contours, retrieved templates, matches), and one summary per frame, "
                    "<output-dir>/vis/<scene>_<im>.png; the object meshes come from --models-dir")
    ap.add_argument("--batch-detections", type=int, default=0, help="N >= 1: one pass over the split's images, N detections per batch across frames and "
                    "objects (infer_batched; same poses, no pictures); 0 (default): one object after the other, one batch per (image, object)")
    ap.add_argument("--device-masks", action="store_true", help="with --batch-detections N >= 1: decode, open and crop the detections' masks on the "
                    "device instead of on the host (same masks, same poses)")
    args = ap.parse_args(argv)
    if args.batch_detections < 0:
        ap.error("--batch-detections must be >= 0")
    if args.batch_detections >= 1 and args.vis:
        ap.error("--vis needs the per-object driver: drop --batch-detections (or pass 0)")
    if args.device_masks and args.batch_detections < 1:
        ap.error("--device-masks needs the batched driver: pass --batch-detections N (N >= 1)")
    opts = load_opts(args.opts)
    with_depth = (opts.final_pose_type in DEPTH_POSE_TYPES or opts.pnp_type in DEPTH_PNP_TYPES
                  or opts.coarse_select_type in DEPTH_SELECT_TYPES)   # the depth pose / PnP / select types read depth/<im>.png beside every image
    # the checkpoint is resolved before anything else is read: a missing one must fail in seconds, not after the banks are loaded
    extractor = feature_util.make_feature_extractor(opts.extractor_name, precision=args.precision, weights=args.weights)
    detection_task = opts.task == "detection"
    with open(args.targets or os.path.join(os.path.dirname(os.path.abspath(args.dataset_dir)),
                                           "test_targets_bop24.json" if detection_task else "test_targets_bop19.json")) as f:
        targets = json.load(f)
    detections = infer_pose_util.load_detections_in_bop_format(args.detections)
    if detection_task:   # an image list: each image once, object ids and instance counts dropped; the objects come from the options or the detections
        targets = [{"scene_id": s, "im_id": i} for s, i in dict.fromkeys((int(t["scene_id"]), int(t["im_id"])) for t in targets)]
        lids = opts.object_lids or sorted({k[2] for k in detections})
        if not lids:
            ap.error("task 'detection': no object_lids in the options and no detection to take the objects from")
    else:
        lids = opts.object_lids or sorted({t["obj_id"] for t in targets})
    repres = {lid: repre_util.load_object_repre(repre_util.get_object_repre_dir_path(args.repre_dir, opts.repre_version, opts.object_dataset, lid)) for lid in lids}
    n_inst: Dict[int, Dict[Tuple[int, int], int]] = {}
    for t in targets:
        if detection_task:
            for lid in lids:
                n_inst.setdefault(lid, {})[(t["scene_id"], t["im_id"])] = 0
        else:
            n_inst.setdefault(t["obj_id"], {})[(t["scene_id"], t["im_id"])] = t["inst_count"]
    eval_models = None
    models_dir = args.models_dir or os.path.join(os.path.dirname(os.path.abspath(args.dataset_dir)), "models")
    renderer = None
    if args.vis and opts.vis_results:
        from .renderer import HipRasterizer
        vis_util.check_opts(opts)
        renderer = HipRasterizer("cuda")
        for lid in lids:
            renderer.add_object_model(lid, os.path.join(models_dir, f"obj_{lid:06d}.ply"))
    elif args.vis:
        print("vis_results is false in the options: no pictures are written")
    if args.eval_gt:
        with open(os.path.join(models_dir, "models_info.json")) as f:
            models_info = json.load(f)
        eval_models = {lid: eval_util.load_eval_model(models_dir, lid, opts.max_sym_disc_step, models_info) for lid in lids}
    scene_cameras = scene_models = None
    if opts.scene_select_type == "multiview":   # the models come from the directory --eval-gt resolves; a missing models_info.json raises
        scene_cameras = multiview.load_scene_cameras(args.dataset_dir, {int(t["scene_id"]) for t in targets})
        scene_models = eval_models if eval_models is not None else multiview.load_models(models_dir, lids, opts.max_sym_disc_step)
    if args.batch_detections >= 1:
        out = infer_batched(opts._replace(object_lids=list(lids)), load_bop_frames_all(args.dataset_dir, targets, with_gt=args.eval_gt, with_depth=with_depth), detections, repres,
                            args.output_dir, batch_detections=args.batch_detections, extractor=extractor.to("cuda"), precision=args.precision,
                            num_target_insts=n_inst, eval_models=eval_models, device_masks=args.device_masks, scene_cameras=scene_cameras,
                            scene_models=scene_models)
        print("\n".join(out))
        return
    out = infer(opts._replace(object_lids=list(lids)), lambda lid: load_bop_frames(args.dataset_dir, targets, lid, with_gt=args.eval_gt, with_depth=with_depth), detections,
                repres, args.output_dir, extractor=extractor.to("cuda"), precision=args.precision, num_target_insts=n_inst, eval_models=eval_models,
                renderer=renderer, scene_cameras=scene_cameras, scene_models=scene_models)
    print("\n".join(out))


if __name__ == "__main__":
    main()
