"""ADD / ADD-S scores of a results csv, on the MI355X: the recall at recall_factor x diameter (LM, LM-O) and the area under the accuracy
curve up to auc_max mm (YCB-V, the PoseCNN protocol).

    python -m foundpose_amd.eval_add --result-csv coarse_lmo-estimated-poses.csv --dataset-dir <datasets>/lmo/test \\
        [--targets ../test_targets_bop19.json] [--models-dir ../models_eval or ../models] [--symmetric-ids 10 11] --output scores.json

ADD and ADI of every (kept estimate, GT instance of the same object in the image) come from fp_pose_add_errors (csrc/pose_add.hip: the
nearest neighbour of ADI is brute force in fp64), one launch per block of 32 images; the protocol (top-n, valid GT, matching, recall, AUC)
runs on the host.  Restates the published behaviour of bop_toolkit_lib.pose_error.add / adi and of the YCB-Video toolbox's VOCap; neither
is installed here, so nothing is pinned against their code.
"""

import argparse
import json
import math
import os
import time
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from .eval_bop19 import _m2c, _read_json, load_results_csv, top_n, valid_gt_mask

RECALL_FACTOR = 0.1     # ADD(-S) below this fraction of the diameter is correct
AUC_MAX_MM = 100.0      # the accuracy curve is integrated up to 10 cm
IMAGE_BLOCK = 32        # images per fp_pose_add_errors launch
METRICS = ("add", "adi", "add_s")


# ---------------------------------------------------------------------------------------------------------- the protocol, on the host
def is_symmetric(model_info: Dict[str, Any], obj_id: int, symmetric_ids: Optional[Iterable[int]] = None) -> bool:
    """ADD(-S) of an object is ADI when its models_info entry has a non-empty symmetries_discrete or symmetries_continuous, or when its id is in
    symmetric_ids; else ADD."""
    if symmetric_ids is not None and int(obj_id) in {int(i) for i in symmetric_ids}:
        return True
    return bool(len(model_info.get("symmetries_discrete", ()) or ())) or bool(len(model_info.get("symmetries_continuous", ()) or ()))


def auc(d: Sequence[float], auc_max: float = AUC_MAX_MM) -> float:
    """The area under the accuracy-threshold curve of the errors d up to auc_max, as a fraction of auc_max (the YCB-Video toolbox's VOCap):
    sort d ascending with accuracies k / n; drop d > auc_max; mrec = [0, d.., auc_max], mpre = [0, acc.., last acc]; the running maximum of
    mpre; the sum of (mrec_i - mrec_{i-1}) mpre_i over the i where mrec changes; / auc_max.  0 when nothing is left (inf and NaN are dropped)."""
    d = np.sort(np.asarray(d, np.float64).reshape(-1))          # NaN sorts last
    n = d.size
    keep = d <= auc_max                                         # False for NaN
    if n == 0 or not keep.any():
        return 0.0
    acc = np.arange(1, n + 1, dtype=np.float64) / float(n)
    mrec = np.concatenate([[0.0], d[keep], [float(auc_max)]])
    mpre = np.concatenate([[0.0], acc[keep], [acc[keep][-1]]])
    mpre = np.maximum.accumulate(mpre)
    i = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1
    return float(np.sum((mrec[i] - mrec[i - 1]) * mpre[i]) / float(auc_max))


def match_target(err: np.ndarray) -> np.ndarray:
    """Greedy matching of one target: err [n_est, n_gt] the ADD(-S) error, estimates in descending score order.  Each estimate takes the
    not-yet-matched GT instance with the lowest error (ties to the lower gt index; a NaN counts as +inf), valid or not.
    -> [n_gt] the estimate each GT instance got, -1 for none."""
    err = np.asarray(err, np.float64)
    n_est, n_gt = err.shape
    got = np.full(n_gt, -1, np.int64)
    for e in range(n_est):
        free = np.nonzero(got < 0)[0]
        if free.size == 0:
            break
        row = np.where(np.isnan(err[e, free]), np.inf, err[e, free])
        got[free[int(np.argmin(row))]] = e                      # argmin: the first minimum, so the lower gt index
    return got


def instance_errors(targets: Sequence[Dict[str, Any]], err: np.ndarray, symmetric: Dict[int, bool]) -> Dict[int, np.ndarray]:
    """Per object the [n_valid, 3] (add, adi, add_s) errors of its valid GT instances after matching, +inf for an unmatched one.  targets: per
    target its obj_id, n_est, valid [n_gt] and pair_off (its n_est x n_gt rows of err, row-major); err [P, 2] = (add, adi)."""
    out: Dict[int, List[Tuple[float, float, float]]] = {}
    for t in targets:
        lid, n_est, valid = int(t["obj_id"]), int(t["n_est"]), np.asarray(t["valid"], bool)
        n_gt = valid.size
        e = np.asarray(err[t["pair_off"]:t["pair_off"] + n_est * n_gt], np.float64).reshape(n_est, n_gt, 2)
        col = 1 if symmetric[lid] else 0
        got = match_target(e[:, :, col]) if n_est else np.full(n_gt, -1, np.int64)
        rows = out.setdefault(lid, [])
        for g in np.nonzero(valid)[0]:
            if got[g] < 0:
                rows.append((math.inf, math.inf, math.inf))
            else:
                a, s = float(e[got[g], g, 0]), float(e[got[g], g, 1])
                rows.append((a, s, s if symmetric[lid] else a))
    return {lid: np.array(v, np.float64).reshape(-1, 3) for lid, v in out.items()}


def score(errors: np.ndarray, diameter_of: np.ndarray, recall_factor: float, auc_max: float) -> Dict[str, float]:
    """errors [n, 3] (add, adi, add_s) of n instances with their objects' diameters [n] -> recall of ADD(-S) and the three AUCs."""
    n = errors.shape[0]
    return {"recall_add_s": float(np.count_nonzero(errors[:, 2] < recall_factor * diameter_of)) / n if n else 0.0,
            "auc_add": auc(errors[:, 0], auc_max), "auc_adi": auc(errors[:, 1], auc_max), "auc_add_s": auc(errors[:, 2], auc_max)}


def summarize(per_obj: Dict[int, np.ndarray], diameters: Dict[int, float], recall_factor: float, auc_max: float) -> Dict[str, Any]:
    """instance_errors' tables -> per object, the mean over the objects that have a valid instance, and all instances as one set."""
    objs = {lid: score(e, np.full(e.shape[0], diameters[lid]), recall_factor, auc_max) for lid, e in sorted(per_obj.items())}
    have = [lid for lid, e in sorted(per_obj.items()) if e.shape[0] > 0]
    keys = ("recall_add_s", "auc_add", "auc_adi", "auc_add_s")
    mean = {k: float(np.mean([objs[lid][k] for lid in have])) if have else 0.0 for k in keys}
    all_e = np.concatenate([per_obj[lid] for lid in have]) if have else np.zeros((0, 3))
    all_d = np.concatenate([np.full(per_obj[lid].shape[0], diameters[lid]) for lid in have]) if have else np.zeros(0)
    return {"mean": mean, "all": score(all_e, all_d, recall_factor, auc_max), "per_object": objs}


# ---------------------------------------------------------------------------------------------------------- evaluation
def evaluate_add(result_csv: str, split_dir: str, targets: Union[None, str, Sequence[Dict[str, int]]] = None,
                 models_dir: Optional[str] = None, dataset: str = "", recall_factor: float = RECALL_FACTOR, auc_max: float = AUC_MAX_MM,
                 symmetric_ids: Optional[Iterable[int]] = None, details: bool = False, device: str = "cuda") -> Dict[str, Any]:
    """ADD / ADD-S scores of `result_csv` against the split `split_dir` (<datasets>/<dataset>/<split>).  targets: a localization targets
    file (test_targets_bop19.json) or its list (default <split_dir>/../test_targets_bop19.json; keys other than scene_id / im_id / obj_id /
    inst_count are ignored, rows of non-targets too); models_dir: models_info.json + obj_XXXXXX.ply (default ../models_eval when it exists,
    else ../models); dataset: its name, recorded in the result; recall_factor: the correctness threshold as a fraction of the diameter;
    auc_max: the end of the accuracy curve in mm; symmetric_ids: objects scored by ADI whatever models_info says.  details: also the pair
    tables and the device's error table.  -> the scores dict."""
    if not (isinstance(recall_factor, (int, float)) and math.isfinite(recall_factor) and recall_factor > 0):
        raise ValueError(f"recall_factor must be a positive number, got {recall_factor!r}")
    if not (isinstance(auc_max, (int, float)) and math.isfinite(auc_max) and auc_max > 0):
        raise ValueError(f"auc_max must be a positive number of mm, got {auc_max!r}")
    sym_ids = sorted({int(i) for i in symmetric_ids}) if symmetric_ids is not None else []
    root = os.path.dirname(os.path.abspath(split_dir))
    if targets is None or isinstance(targets, str):
        targets = _read_json(targets or os.path.join(root, "test_targets_bop19.json"))
    if models_dir is None:
        models_dir = os.path.join(root, "models_eval")
        if not os.path.isdir(models_dir):
            models_dir = os.path.join(root, "models")
    dataset = dataset or os.path.basename(root)

    import torch

    from . import ops
    from .renderer import load_ply
    rows = load_results_csv(result_csv)
    tgt: Dict[Tuple[int, int, int], int] = {}
    for t_ in targets:
        key = (int(t_["scene_id"]), int(t_["im_id"]), int(t_["obj_id"]))
        tgt[key] = tgt.get(key, 0) + int(t_["inst_count"])
    for i, r in enumerate(rows):
        if (r["scene_id"], r["im_id"], r["obj_id"]) in tgt and math.isnan(r["score"]):
            raise ValueError(f"csv row {i}: the score is NaN, the estimates cannot be ranked")
    kept = top_n(rows, tgt)
    obj_ids = sorted({k[2] for k in tgt})

    # ---- annotations and models: every object's points in one device array
    gts, infos = {}, {}
    for s in sorted({k[0] for k in tgt}):
        sd = os.path.join(split_dir, f"{s:06d}")
        gts[s] = _read_json(os.path.join(sd, "scene_gt.json"))
        infos[s] = _read_json(os.path.join(sd, "scene_gt_info.json"))
    models_info = _read_json(os.path.join(models_dir, "models_info.json"))
    diam, symmetric, pt_range, verts = {}, {}, {}, []
    n_pts = 0
    for lid in obj_ids:
        if str(lid) not in models_info:
            raise ValueError(f"object {lid} is a target but has no entry in models_info.json")
        diam[lid] = float(models_info[str(lid)]["diameter"])
        symmetric[lid] = is_symmetric(models_info[str(lid)], lid, sym_ids)
        v = load_ply(os.path.join(models_dir, f"obj_{lid:06d}.ply"), geometry_only=True).vertices.astype(np.float64)
        pt_range[lid] = (n_pts, v.shape[0])
        n_pts += v.shape[0]
        verts.append(v)
    pts_dev = torch.from_numpy(np.concatenate(verts)).to(device) if verts else None

    # ---- per target: the kept estimates (score order) x the GT instances of the object; one launch per block of images
    images = sorted({k[:2] for k in tgt})
    block_of = {k: n // IMAGE_BLOCK for n, k in enumerate(images)}
    tabs: List[Dict[str, Any]] = []
    est_p: List[np.ndarray] = []
    gt_p: List[np.ndarray] = []
    ranges: List[Tuple[int, int]] = []
    errs = []
    n_pairs, launched, current = 0, 0, None

    def launch():
        nonlocal launched
        if n_pairs > launched:
            for c0 in range(launched, n_pairs, 65535):           # the call's batch limit
                c1 = min(c0 + 65535, n_pairs)
                dev = torch.from_numpy(np.stack(est_p[c0:c1] + gt_p[c0:c1])).to(device)
                errs.append(ops.pose_add_errors(pts_dev, dev[:c1 - c0], dev[c1 - c0:], np.array(ranges[c0:c1], np.int64)))
            launched = n_pairs

    for key in sorted(tgt):                                       # sorted by (scene, image, object): a block's targets are consecutive
        s, im, lid = key
        if current is not None and block_of[key[:2]] != current:
            launch()
        current = block_of[key[:2]]
        ents, ivs = gts[s].get(str(im), []), infos[s].get(str(im), [])
        gids = [g for g, e in enumerate(ents) if int(e["obj_id"]) == lid]
        est = kept.get(key, [])
        tabs.append({"scene_id": s, "im_id": im, "obj_id": lid, "est_rows": list(est), "gt_ids": gids, "n_est": len(est),
                     "valid": valid_gt_mask([float(ivs[g]["visib_fract"]) for g in gids], tgt[key]), "pair_off": n_pairs})
        for r in est:
            pe = np.concatenate([np.asarray(rows[r]["R"], np.float64).reshape(9), np.asarray(rows[r]["t"], np.float64).reshape(3)])
            for g in gids:
                T = _m2c(ents[g]["cam_R_m2c"], ents[g]["cam_t_m2c"])
                est_p.append(pe)
                gt_p.append(np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]))
                ranges.append(pt_range[lid])
        n_pairs = len(ranges)
    launch()
    err = torch.cat(errs).cpu().numpy() if errs else np.zeros((0, 2))

    per_obj = instance_errors(tabs, err, symmetric)
    s = summarize(per_obj, diam, float(recall_factor), float(auc_max))
    out = {"recall_add_s": s["mean"]["recall_add_s"], "auc_add": s["mean"]["auc_add"], "auc_adi": s["mean"]["auc_adi"],
           "auc_add_s": s["mean"]["auc_add_s"], "all_instances": s["all"], "recall_factor": float(recall_factor), "auc_max_mm": float(auc_max),
           "dataset": dataset, "num_targets": len(tgt), "num_valid_gt_instances": int(sum(e.shape[0] for e in per_obj.values())),
           "num_estimates_evaluated": int(sum(t["n_est"] for t in tabs)), "num_pairs": int(n_pairs),
           "symmetric_objects": [lid for lid in obj_ids if symmetric[lid]], "per_object": {}}
    for lid in obj_ids:
        n = int(per_obj[lid].shape[0]) if lid in per_obj else 0
        po = s["per_object"].get(lid, {})
        out["per_object"][str(lid)] = {"error_type": "adi" if symmetric[lid] else "add", "diameter": diam[lid], "num_valid_instances": n,
                                       **{k: (po[k] if n else -1.0) for k in ("recall_add_s", "auc_add", "auc_adi", "auc_add_s")}}
    if details:
        out["tables"] = {"targets": tabs, "err": err, "symmetric": symmetric, "diameters": diam,
                         "instance_errors": per_obj}
    return out


def main(argv: Optional[Sequence[str]] = None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--result-csv", required=True, help="BOP19 results csv (what infer / eval_util.prepare_bop_submission writes)")
    ap.add_argument("--dataset-dir", required=True, help="BOP split directory (<datasets>/<dataset>/<split>)")
    ap.add_argument("--targets", default=None, help="test_targets_bop19.json (default: <dataset-dir>/../test_targets_bop19.json)")
    ap.add_argument("--models-dir", default=None, help="models_info.json + obj_XXXXXX.ply (default: ../models_eval if it exists, else ../models)")
    ap.add_argument("--dataset", default="", help="dataset name (default: the name of <dataset-dir>'s parent)")
    ap.add_argument("--recall-factor", type=float, default=RECALL_FACTOR, help="ADD(-S) below this fraction of the diameter is correct (default 0.1)")
    ap.add_argument("--auc-max", type=float, default=AUC_MAX_MM, help="end of the accuracy curve in mm (default 100)")
    ap.add_argument("--symmetric-ids", type=int, nargs="*", default=None, help="objects scored by ADI whatever models_info.json says")
    ap.add_argument("--output", required=True, help="scores JSON")
    args = ap.parse_args(argv)
    t0 = time.perf_counter()
    scores = evaluate_add(args.result_csv, args.dataset_dir, args.targets, args.models_dir, args.dataset, args.recall_factor, args.auc_max,
                          args.symmetric_ids)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(scores, f, indent=2)
    print(f"ADD(-S) recall {scores['recall_add_s']:.4f} at {scores['recall_factor']} x diameter, AUC add {scores['auc_add']:.4f} adi "
          f"{scores['auc_adi']:.4f} add-s {scores['auc_add_s']:.4f} over {scores['num_valid_gt_instances']} valid instances in "
          f"{time.perf_counter() - t0:.1f} s -> {args.output}")


if __name__ == "__main__":
    main()
