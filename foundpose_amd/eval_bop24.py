"""The BOP24 average precision of a results csv for the 6D DETECTION task, on the MI355X: AP = mean(AP_MSSD, AP_MSPD) (DESIGN.md
section 21).

    python -m foundpose_amd.eval_bop24 --result-csv coarse_lmo-estimated-poses.csv --dataset-dir <datasets>/lmo/test \\
        [--targets ../test_targets_bop24.json] [--models-dir ../models_eval or ../models] --output scores.json

The task's targets name images only: every estimate of a target image counts, there are no instance counts and no top-n.  Restates the
published behaviour of bop_toolkit_lib's eval_bop24_pose.py (eval_calc_scores in detection mode, score.calc_pose_detection_scores); the
toolkit is not installed here, so nothing is pinned against its code.  MSSD / MSPD of every (estimate, GT instance of the same object in the
image) come from fp_pose_errors and stay on the device; fp_detection_match matches every (image, object) group for the 2 x 10 thresholds
and fp_detection_ap accumulates precision and recall per object (csrc/detection_ap.hip).  The host sorts, builds the tables and averages.
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
from .eval_bop19 import MSPD_THS, MSSD_THS, _m2c, _read_json, average_time_per_image, correct_thresholds, load_results_csv
from .group_tables import MAX_GROUP_GT, MAX_REC, MAX_THS, check_groups, int32_table, offsets, upload

MIN_VISIB_FRACT = 0.1                    # a GT instance is valid when at least this fraction of it is visible
REC_THR = np.linspace(0, 1, 101)         # the recall thresholds precision is interpolated at


# ---------------------------------------------------------------------------------------------------------- the two launches
def match_groups(err, est_off, gt_off, pair_off, gt_valid, group_tab, ths):
    """fp_detection_match with its host tables checked first (ValueError before any launch): err f64 [P, 2] ON THE DEVICE (ops.pose_errors'
    first output); est_off / gt_off / pair_off [NG + 1] ascending, group g owning E_g estimates (in rank order), G_g <= 256 GT instances and
    the E_g G_g rows of err from pair_off[g]; gt_valid [G_total]; group_tab [NG] rows of ths [NTAB, 2, T], 1 <= T <= 16.
    -> (flag int8 [N_est, 2 T], matched_gt int32 [N_est, 2 T]) on the device, N_est = est_off[-1]."""
    import torch

    from . import ops
    if not isinstance(err, torch.Tensor) or not err.is_cuda:
        raise ValueError("match_groups: err is a device tensor (the errors are not read back); there is no CPU path")
    if err.dtype != torch.float64 or err.dim() != 2 or err.shape[1] != 2 or not err.is_contiguous():
        raise ValueError(f"match_groups: err must be a contiguous float64 [P, 2] tensor, got {err.dtype} {tuple(err.shape)}")
    gt_valid = int32_table("gt_valid", gt_valid)
    est_off, gt_off, pair_off, NG = check_groups("match_groups", est_off, gt_off, pair_off, gt_valid.size, int(err.shape[0]), "err", "gt_valid")
    group_tab = int32_table("group_tab", group_tab, NG)
    ths = np.ascontiguousarray(np.asarray(ths, np.float64))
    if ths.ndim != 3 or ths.shape[1] != 2 or not 1 <= ths.shape[2] <= MAX_THS:
        raise ValueError(f"match_groups: ths must be [NTAB, 2, T] with 1 <= T <= {MAX_THS}, got {ths.shape}")
    if NG and (ths.shape[0] < 1 or int(group_tab.min()) < 0 or int(group_tab.max()) >= ths.shape[0]):
        raise ValueError(f"match_groups: group_tab must index the {ths.shape[0]} rows of ths")
    d_est, d_gt, d_pair, d_valid, d_tab = upload([est_off, gt_off, pair_off, gt_valid, group_tab], np.int32, err.device)
    d_ths, = upload([ths], np.float64, err.device)
    return ops.detection_match(d_est, d_gt, d_pair, err, d_valid, d_tab, d_ths.reshape(ths.shape), int(est_off[-1]))


def ap_objects(flag, obj_off, order, n_valid, rec_thr=None):
    """fp_detection_ap with its host tables checked first: flag int8 [N_est, 2 T] ON THE DEVICE as match_groups returned it; obj_off [O + 1]
    ascending; order [N] rows of flag, per object in global rank order; n_valid [O]; rec_thr [R] (default linspace(0, 1, 101)), 1 <= R <=
    128.  -> (ap f64 [O, 2 T], q f64 [O, 2 T, R], totals int32 [O, 2 T, 3]) on the device."""
    import torch

    from . import ops
    if not isinstance(flag, torch.Tensor) or not flag.is_cuda:
        raise ValueError("ap_objects: flag is a device tensor (match_groups' output, not read back); there is no CPU path")
    if flag.dtype != torch.int8 or flag.dim() != 2 or flag.shape[1] % 2 or not 1 <= flag.shape[1] // 2 <= MAX_THS or not flag.is_contiguous():
        raise ValueError(f"ap_objects: flag must be a contiguous int8 [N_est, 2 T] tensor with 1 <= T <= {MAX_THS}, got {flag.dtype} {tuple(flag.shape)}")
    obj_off, order = offsets("obj_off", obj_off), int32_table("order", order)
    n_valid = int32_table("n_valid", n_valid, obj_off.size - 1)
    rec_thr = np.ascontiguousarray(np.asarray(REC_THR if rec_thr is None else rec_thr, np.float64))
    if rec_thr.ndim != 1 or not 1 <= rec_thr.size <= MAX_REC:
        raise ValueError(f"ap_objects: 1 <= R <= {MAX_REC} recall thresholds are needed, got {rec_thr.shape}")
    if int(obj_off[-1]) > order.size:
        raise ValueError(f"ap_objects: obj_off reaches {int(obj_off[-1])}, order has {order.size} entries")
    if order.size and (int(order.min()) < 0 or int(order.max()) >= int(flag.shape[0])):
        raise ValueError(f"ap_objects: order must index the {int(flag.shape[0])} rows of flag")
    d_off, d_order, d_valid = upload([obj_off, order, n_valid], np.int32, flag.device)
    d_thr, = upload([rec_thr], np.float64, flag.device)
    return ops.detection_ap(d_off, d_order, flag, d_valid, d_thr)


def summarize(ap: np.ndarray, n_valid: Sequence[int], num_ths: int) -> Dict[str, Any]:
    """ap [O, 2 T] -> the task's numbers: per column the mean over the objects with n_valid > 0 (others hold -1 and are left out), AP_MSSD /
    AP_MSPD the mean over the T thresholds, AP their mean.  Without any such object every number is 0."""
    ap = np.asarray(ap, np.float64)
    has = np.asarray(n_valid) > 0
    cols = ap[has].mean(axis=0) if has.any() else np.zeros(2 * num_ths)
    mssd, mspd = float(np.mean(cols[:num_ths])), float(np.mean(cols[num_ths:]))
    return {"ap": float(np.mean([mssd, mspd])), "ap_mssd": mssd, "ap_mspd": mspd, "columns": cols}


# ---------------------------------------------------------------------------------------------------------- inputs
def target_images(targets: Sequence[Dict[str, int]]) -> List[Tuple[int, int]]:
    """The (scene_id, im_id) of a targets list, once each, sorted: obj_id / inst_count keys are ignored, so a BOP19 file is an image list."""
    return sorted({(int(t["scene_id"]), int(t["im_id"])) for t in targets})


def image_width(split_dir: str, scene_id: int, im_id: int) -> int:
    """The width of a test image, from the header of rgb/<im>.png, rgb/<im>.jpg, gray/<im>.tif or depth/<im>.png (the first that exists)."""
    from PIL import Image
    sd = os.path.join(split_dir, f"{scene_id:06d}")
    for sub, ext in (("rgb", "png"), ("rgb", "jpg"), ("gray", "tif"), ("depth", "png")):
        p = os.path.join(sd, sub, f"{im_id:06d}.{ext}")
        if os.path.exists(p):
            with Image.open(p) as im:
                return int(im.size[0])
    raise FileNotFoundError(f"{sd}: no rgb, gray or depth image {im_id:06d}: the MSPD thresholds need the image width")


def build_tables(rows: Sequence[Dict[str, Any]], images: Sequence[Tuple[int, int]], gts: Dict[int, Any], infos: Dict[int, Any],
                 diameters: Dict[int, float], width_of: Dict[Tuple[int, int], int]) -> Dict[str, Any]:
    """The host side of the protocol: everything the two launches read but the errors.  rows: the csv; images: the target images; gts /
    infos: scene_gt.json / scene_gt_info.json per scene.  -> dict with obj_ids, n_valid [O], the groups (sorted by scene, image, object;
    `est_rows` the csv rows in group-then-rank order), est_off / gt_off / pair_off, gt_valid, group_tab, ths, obj_off, order, and per group
    the GT poses for the error launch."""
    img_set = set(images)
    per = defaultdict(list)
    for i, r in enumerate(rows):
        if (r["scene_id"], r["im_id"]) in img_set:
            if math.isnan(r["score"]):
                raise ValueError(f"csv row {i}: the score is NaN, the estimates cannot be ranked")
            per[(r["scene_id"], r["im_id"], r["obj_id"])].append(i)
    gt_of = defaultdict(list)     # (scene, im, obj) -> [(gt id, 4x4 m2c, valid)]
    n_valid = defaultdict(int)
    n_gt = 0
    for s, im in images:
        ents, ivs = gts[s].get(str(im), []), infos[s].get(str(im), [])
        for g, e in enumerate(ents):
            lid = int(e["obj_id"])
            ok = float(ivs[g]["visib_fract"]) >= MIN_VISIB_FRACT
            gt_of[(s, im, lid)].append((g, _m2c(e["cam_R_m2c"], e["cam_t_m2c"]), ok))
            n_valid[lid] += int(ok)
            n_gt += 1
    obj_ids = sorted({k[2] for k in per} | set(n_valid))
    groups = sorted(per)
    est_rows: List[int] = []
    est_off, gt_off, pair_off, gt_valid, group_tab = [0], [0], [0], [], []
    tabs: Dict[Tuple[int, int], int] = {}
    ths = []
    for key in groups:
        ranked = sorted(per[key], key=lambda i: rows[i]["score"], reverse=True)   # stable: among equal scores the earlier row wins
        insts = gt_of.get(key, [])
        if len(insts) > MAX_GROUP_GT:
            raise ValueError(f"scene {key[0]} image {key[1]} has {len(insts)} GT instances of object {key[2]} (at most {MAX_GROUP_GT})")
        est_rows += ranked
        gt_valid += [int(v) for _, _, v in insts]
        est_off.append(est_off[-1] + len(ranked))
        gt_off.append(gt_off[-1] + len(insts))
        pair_off.append(pair_off[-1] + len(ranked) * len(insts))
        tk = (key[2], width_of[key[:2]])
        if tk not in tabs:
            if key[2] not in diameters:
                raise ValueError(f"object {key[2]} has estimates but no entry in models_info.json")
            tabs[tk] = len(ths)
            th = correct_thresholds(diameters[key[2]], tk[1])
            ths.append(np.stack([th["mssd"], th["mspd"]]))
        group_tab.append(tabs[tk])
    if pair_off[-1] > 2**31 - 1:
        raise ValueError(f"{pair_off[-1]} (estimate, GT) pairs: more than one evaluation holds")
    # per object: its rows of the estimate table in global rank order (score descending, equal scores in csv order)
    pos_of = defaultdict(list)
    for pos, i in enumerate(est_rows):
        pos_of[rows[i]["obj_id"]].append(pos)
    obj_off, order = [0], []
    for lid in obj_ids:
        by_csv = sorted(pos_of.get(lid, []), key=lambda p: est_rows[p])
        order += sorted(by_csv, key=lambda p: rows[est_rows[p]]["score"], reverse=True)
        obj_off.append(len(order))
    return {"obj_ids": obj_ids, "n_valid": np.array([n_valid.get(lid, 0) for lid in obj_ids], np.int64), "groups": groups,
            "est_rows": np.array(est_rows, np.int64), "est_off": np.array(est_off, np.int64), "gt_off": np.array(gt_off, np.int64),
            "pair_off": np.array(pair_off, np.int64), "gt_valid": np.array(gt_valid, np.int64), "group_tab": np.array(group_tab, np.int64),
            "ths": np.stack(ths) if ths else np.zeros((1, 2, len(MSSD_THS))), "obj_off": np.array(obj_off, np.int64),
            "order": np.array(order, np.int64), "gt_poses": {k: [T for _, T, _ in gt_of.get(k, [])] for k in groups}, "num_gt": n_gt}


# ---------------------------------------------------------------------------------------------------------- evaluation
def evaluate_bop24(result_csv: str, split_dir: str, targets: Union[None, str, Sequence[Dict[str, int]]] = None,
                   models_dir: Optional[str] = None, dataset: str = "", device: str = "cuda", image_block: int = 32, details: bool = False,
                   timing: bool = False) -> Dict[str, Any]:
    """BOP24 6D detection scores of `result_csv` against the split `split_dir` (<datasets>/<dataset>/<split>).  targets: a
    test_targets_bop24.json path or its list of {scene_id, im_id} (default <split_dir>/../test_targets_bop24.json; other keys are ignored,
    rows of other images too); models_dir: models_info.json + obj_XXXXXX.ply (default ../models_eval when it exists, else ../models);
    dataset: its name, recorded in the result (default the parent directory's name).  One fp_pose_errors launch per block of
    `image_block` images.  details: also the tables and the device's flags; timing: also device-event times.  -> the scores dict
    (DESIGN.md section 21)."""
    import torch

    from . import eval_util
    from .renderer import load_ply
    root = os.path.dirname(os.path.abspath(split_dir))
    if targets is None or isinstance(targets, str):
        targets = _read_json(targets or os.path.join(root, "test_targets_bop24.json"))
    if models_dir is None:
        models_dir = os.path.join(root, "models_eval")
        if not os.path.isdir(models_dir):
            models_dir = os.path.join(root, "models")
    dataset = dataset or os.path.basename(root)
    if image_block < 1:
        raise ValueError(f"image_block must be >= 1, got {image_block!r}")

    rows = load_results_csv(result_csv)
    avg_time = average_time_per_image(rows)
    images = target_images(targets)
    cams, gts, infos = {}, {}, {}
    for s in sorted({s for s, _ in images}):
        sd = os.path.join(split_dir, f"{s:06d}")
        cams[s] = _read_json(os.path.join(sd, "scene_camera.json"))
        gts[s] = _read_json(os.path.join(sd, "scene_gt.json"))
        infos[s] = _read_json(os.path.join(sd, "scene_gt_info.json"))
    models_info = _read_json(os.path.join(models_dir, "models_info.json"))
    diameters = {int(k): float(v["diameter"]) for k, v in models_info.items()}
    with_rows = {(r["scene_id"], r["im_id"]) for r in rows}
    width_of = {k: image_width(split_dir, *k) for k in images if k in with_rows}
    tb = build_tables(rows, images, gts, infos, diameters, width_of)

    timer = DeviceTimer(timing)
    timed = timer.timed

    # ---- MSSD / MSPD of every estimate x every GT instance of its group: one launch per block of images, nothing read back
    syms, pts_dev = {}, {}
    for lid in sorted({k[2] for k in tb["groups"] if tb["gt_poses"][k]}):
        syms[lid] = eval_util.get_symmetry_transformations(models_info[str(lid)], max_sym_disc_step=0.01)
        pts_dev[lid] = torch.from_numpy(load_ply(os.path.join(models_dir, f"obj_{lid:06d}.ply"), geometry_only=True).vertices.astype(np.float64)).to(device)
    errs = []
    block_of = {k: n // image_block for n, k in enumerate(images)}
    items, current = [], None
    for gi, key in enumerate(tb["groups"]):      # sorted by (scene, image, object): a block's groups are consecutive
        if current is not None and block_of[key[:2]] != current and items:
            errs.append(timed("mssd_mspd", eval_util.pose_errors_device, items, device)[0])
            items = []
        current = block_of[key[:2]]
        K = np.asarray(cams[key[0]][str(key[1])]["cam_K"], np.float64).reshape(3, 3)
        for r in tb["est_rows"][tb["est_off"][gi]:tb["est_off"][gi + 1]]:
            for T in tb["gt_poses"][key]:
                items.append(dict(R_est=rows[r]["R"], t_est=rows[r]["t"], R_gt=T[:3, :3], t_gt=T[:3, 3], K=K, pts=pts_dev[key[2]], syms=syms[key[2]]))
    if items:
        errs.append(timed("mssd_mspd", eval_util.pose_errors_device, items, device)[0])
    err = torch.cat(errs) if len(errs) > 1 else (errs[0] if errs else torch.zeros(0, 2, dtype=torch.float64, device=device))

    # ---- matching per (image, object) and threshold, precision / recall per object and threshold: two launches
    flag, matched = timed("match", match_groups, err, tb["est_off"], tb["gt_off"], tb["pair_off"], tb["gt_valid"], tb["group_tab"], tb["ths"])
    ap_d, q_d, totals_d = timed("ap", ap_objects, flag, tb["obj_off"], tb["order"], tb["n_valid"])
    ap, totals = ap_d.cpu().numpy(), totals_d.cpu().numpy()

    T = len(MSSD_THS)
    s = summarize(ap, tb["n_valid"], T)
    out = {"bop24_average_precision": s["ap"], "bop24_average_precision_mssd": s["ap_mssd"], "bop24_average_precision_mspd": s["ap_mspd"],
           "bop24_average_time_per_image": avg_time, "dataset": dataset,
           "ap_mssd": s["columns"][:T].tolist(), "ap_mspd": s["columns"][T:].tolist(),
           "mssd_thresholds_x_diameter": MSSD_THS.tolist(), "mspd_thresholds_x_width_over_640": MSPD_THS.tolist(),
           "min_visib_fract": MIN_VISIB_FRACT, "num_recall_thresholds": int(REC_THR.size),
           "num_target_images": len(images), "num_estimates_evaluated": int(tb["est_rows"].size),
           "num_estimates_of_other_images": int(len(rows) - tb["est_rows"].size),
           "num_gt_instances": int(tb["num_gt"]), "num_valid_gt_instances": int(tb["n_valid"].sum()),
           "num_ignored_estimates_mssd": totals[:, :T, 2].sum(0).tolist(), "num_ignored_estimates_mspd": totals[:, T:, 2].sum(0).tolist(),
           "per_object": {}}
    for o, lid in enumerate(tb["obj_ids"]):
        nv = int(tb["n_valid"][o])
        out["per_object"][str(lid)] = {
            "average_precision": float(np.mean([ap[o, :T].mean(), ap[o, T:].mean()])) if nv > 0 else -1.0,
            "average_precision_mssd": float(ap[o, :T].mean()) if nv > 0 else -1.0, "average_precision_mspd": float(ap[o, T:].mean()) if nv > 0 else -1.0,
            "ap_mssd": ap[o, :T].tolist(), "ap_mspd": ap[o, T:].tolist(), "num_valid_instances": nv,
            "num_estimates": int(tb["obj_off"][o + 1] - tb["obj_off"][o]),
            "totals_mssd": totals[o, :T].tolist(), "totals_mspd": totals[o, T:].tolist()}   # (tp, fp, ignored) per threshold
    if details:
        out["tables"] = dict(tb, err=err.cpu().numpy(), flag=flag.cpu().numpy(), matched_gt=matched.cpu().numpy(), ap=ap, q=q_d.cpu().numpy(), totals=totals)
    if timing:
        out["device_seconds"] = timer.seconds()
    return out


def main(argv: Optional[Sequence[str]] = None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--result-csv", required=True, help="BOP results csv (what infer / eval_util.prepare_bop_submission writes)")
    ap.add_argument("--dataset-dir", required=True, help="BOP split directory (<datasets>/<dataset>/<split>)")
    ap.add_argument("--targets", default=None, help="test_targets_bop24.json (default: <dataset-dir>/../test_targets_bop24.json); only scene_id / im_id are read")
    ap.add_argument("--models-dir", default=None, help="models_info.json + obj_XXXXXX.ply (default: ../models_eval if it exists, else ../models)")
    ap.add_argument("--dataset", default="", help="dataset name (default: the name of <dataset-dir>'s parent)")
    ap.add_argument("--output", required=True, help="scores JSON")
    args = ap.parse_args(argv)
    t0 = time.perf_counter()
    scores = evaluate_bop24(args.result_csv, args.dataset_dir, args.targets, args.models_dir, args.dataset)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(scores, f, indent=2)
    print(f"bop24_average_precision {scores['bop24_average_precision']:.4f} (mssd {scores['bop24_average_precision_mssd']:.4f}, mspd "
          f"{scores['bop24_average_precision_mspd']:.4f}) over {scores['num_valid_gt_instances']} valid instances and "
          f"{scores['num_estimates_evaluated']} estimates in {time.perf_counter() - t0:.1f} s -> {args.output}")


if __name__ == "__main__":
    main()
