"""The BOP19 average recall of a results csv, on the MI355X: AR = mean(AR_VSD, AR_MSSD, AR_MSPD).

    python -m foundpose_amd.eval_bop19 --result-csv coarse_lmo-estimated-poses.csv --dataset-dir <datasets>/lmo/test \\
        [--targets ../test_targets_bop19.json] [--models-dir ../models_eval or ../models] [--vsd-delta 15] --output scores.json

Restates the published behaviour of bop_toolkit_lib's eval_bop19_pose.py (eval_calc_errors + eval_calc_scores); the toolkit
is not installed here, so nothing is pinned against its code.  The estimates and the GT instances are rendered once each by
the HIP rasterizer (renderer.HipRasterizer), VSD is counted by fp_vsd_counts (csrc/vsd.hip), MSSD / MSPD come from
fp_pose_errors (eval_util.pose_errors_batch); the protocol (top-n, valid GT, greedy matching, recalls) runs on the host.
"""

import argparse
import csv
import json
import os
import time
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .device_timer import DeviceTimer

VSD_TAUS = np.arange(0.05, 0.51, 0.05)      # misalignment tolerances, fraction of the object diameter
VSD_THS = np.arange(0.05, 0.51, 0.05)       # correctness thresholds on the VSD error
MSSD_THS = np.arange(0.05, 0.51, 0.05)      # x diameter (mm)
MSPD_THS = np.arange(5, 51, 5)              # x image width / 640 (px)
VSD_DELTA = {"itodd": 5.0}                  # mm; every other dataset: 15
DEFAULT_VSD_DELTA = 15.0
NEAR_LIMIT_MM = 100.0                       # the rasterizer's near plane (renderer.NEAR_PLANE_MM)
WINDOW_LIMIT_PX = float(1 << 20)            # projected |u|, |v| beyond this: not rendered (device limit 2^21)
RENDER_CHUNK = 32                           # views per render_views call
MAX_IO_WORKERS = 16


# ---------------------------------------------------------------------------------------------------------- inputs
def load_results_csv(path: str) -> List[Dict[str, Any]]:
    """The BOP19 results csv (scene_id,im_id,obj_id,score,R,t,time; R row-major, 9 values; t in mm) -> rows in file order."""
    rows = []
    with open(path, newline="") as f:
        reader = csv.reader(f)
        header = next(reader, None)
        if header is None or [h.strip() for h in header] != ["scene_id", "im_id", "obj_id", "score", "R", "t", "time"]:
            raise ValueError(f"{path}: not a BOP19 results csv (header {header})")
        for n, rec in enumerate(reader):
            if not rec or all(not x.strip() for x in rec):
                continue
            if len(rec) != 7:
                raise ValueError(f"{path}: row {n + 1} has {len(rec)} fields, 7 expected")
            R = np.array([float(x) for x in rec[4].split()], np.float64)
            t = np.array([float(x) for x in rec[5].split()], np.float64)
            if R.size != 9 or t.size != 3:
                raise ValueError(f"{path}: row {n + 1}: R needs 9 values and t 3")
            rows.append({"scene_id": int(rec[0]), "im_id": int(rec[1]), "obj_id": int(rec[2]), "score": float(rec[3]),
                         "R": R.reshape(3, 3), "t": t.reshape(3), "time": float(rec[6])})
    return rows


def average_time_per_image(rows: Sequence[Dict[str, Any]]) -> float:
    """The mean over images of the per-image time.  Every row of an image must carry the same time (|difference| <= 1 ms),
    else ValueError; -1 when any time is negative."""
    times: Dict[Tuple[int, int], float] = {}
    for r in rows:
        if r["time"] < 0:
            return -1.0
        key = (r["scene_id"], r["im_id"])
        if key in times:
            if abs(times[key] - r["time"]) > 0.001:
                raise ValueError(f"the running time for scene {key[0]} and image {key[1]} is not the same for all estimates")
        else:
            times[key] = r["time"]
    return float(np.mean(list(times.values()))) if times else -1.0


def correct_thresholds(diameter: float, width: int) -> Dict[str, np.ndarray]:
    """The thresholds an error is compared with (strictly below is correct): VSD per tau, MSSD in mm, MSPD in px."""
    return {"vsd": VSD_THS.copy(), "mssd": MSSD_THS * diameter, "mspd": MSPD_THS * (width / 640.0)}


def top_n(rows: Sequence[Dict[str, Any]], targets: Dict[Tuple[int, int, int], int]) -> Dict[Tuple[int, int, int], List[int]]:
    """Per target (scene, im, obj): the indices of its inst_count highest-scored rows, highest first (a stable sort: among
    equal scores the earlier row wins).  Rows of non-targets are ignored."""
    per = defaultdict(list)
    for i, r in enumerate(rows):
        key = (r["scene_id"], r["im_id"], r["obj_id"])
        if key in targets:
            per[key].append(i)
    return {k: sorted(v, key=lambda i: rows[i]["score"], reverse=True)[:targets[k]] for k, v in per.items()}


def valid_gt_mask(visib_fract: Sequence[float], inst_count: int) -> np.ndarray:
    """The inst_count most visible GT instances of a target are valid: visib_fract descending, ties to the lower gt id."""
    order = sorted(range(len(visib_fract)), key=lambda g: (-visib_fract[g], g))
    mask = np.zeros(len(visib_fract), bool)
    mask[order[:inst_count]] = True
    return mask


def match_count(errs: np.ndarray, ths: np.ndarray, valid: np.ndarray) -> np.ndarray:
    """Greedy matching of one target, once per threshold: errs [M, n_est, n_gt] with the estimates in descending score
    order, ths [M].  Each estimate takes the not-yet-matched GT with the lowest error strictly below the threshold (ties
    to the lower gt id), valid or not; a match to an invalid GT uses up the estimate and counts nowhere.
    -> [M] the number of matched valid GT instances."""
    errs = np.asarray(errs, np.float64)
    M, n_est, n_gt = errs.shape
    matched = np.zeros((M, n_gt), bool)
    rows = np.arange(M)
    for e in range(n_est):
        ok = (errs[:, e, :] < ths[:, None]) & ~matched
        best = np.argmin(np.where(ok, errs[:, e, :], np.inf), axis=1)
        hit = ok[rows, best]
        matched[rows[hit], best[hit]] = True
    return (matched & np.asarray(valid, bool)[None, :]).sum(1)


def vsd_errors(counts: np.ndarray) -> np.ndarray:
    """fp_vsd_counts' [P, 2 + T] -> the VSD errors [P, T]: (count_tau + (|union| - |inter|)) / |union|, 1 when the union is
    empty."""
    c = np.asarray(counts, np.int64)
    union, comp = c[:, 0], c[:, 0] - c[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        e = (c[:, 2:] + comp[:, None]).astype(np.float64) / union[:, None].astype(np.float64)
    e[union == 0] = 1.0
    return e


def prescreen(verts: np.ndarray, T_c2m: np.ndarray, K: np.ndarray) -> bool:
    """True when the rasterizer can draw the mesh seen from the camera T_c2m (its T_world_from_eye): every vertex beyond the
    near plane and projected within +-2^20 px.  The eye coordinates follow csrc/render.hip's arithmetic ((w - t) @ R,
    every operation rounded on its own), so the near-plane verdict is the device's."""
    R, t = T_c2m[:3, :3], T_c2m[:3, 3]
    v = np.asarray(verts, np.float32).astype(np.float64)
    d = [v[:, k] - t[k] for k in range(3)]
    eye = [(d[0] * R[0, k] + d[1] * R[1, k]) + d[2] * R[2, k] for k in range(3)]
    z = eye[2]
    if not np.all(z > NEAR_LIMIT_MM):
        return False
    with np.errstate(all="ignore"):
        u = (eye[0] / z) * K[0, 0] + K[0, 2]
        w = (eye[1] / z) * K[1, 1] + K[1, 2]
    return bool(np.all(np.abs(u) <= WINDOW_LIMIT_PX) and np.all(np.abs(w) <= WINDOW_LIMIT_PX))


def load_depth(path: str, depth_scale: float) -> np.ndarray:
    """A BOP depth PNG (uint16) -> float32 mm: float32(d) * float32(depth_scale), as numpy computes it."""
    from PIL import Image
    with Image.open(path) as im:
        d = np.asarray(im)
    return d.astype(np.float32) * np.float32(depth_scale)


class _Camera:
    """What HipRasterizer.render_views reads of a camera (crop_util.PinholePlaneCameraModel's attributes), without its
    rigidity check: an estimate's rotation comes from a csv as it was written."""

    def __init__(self, K: np.ndarray, width: int, height: int, T_c2m: np.ndarray):
        self.width, self.height = int(width), int(height)
        self.f = (float(K[0, 0]), float(K[1, 1]))
        self.c = (float(K[0, 2]), float(K[1, 2]))
        self.T_world_from_eye = T_c2m


def _m2c(R, t) -> np.ndarray:
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return T


def _read_json(path: str):
    with open(path) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------------------- evaluation
def evaluate_bop19(result_csv: str, split_dir: str, targets: Union[None, str, Sequence[Dict[str, int]]] = None,
                   models_dir: Optional[str] = None, dataset: Optional[str] = None, vsd_delta: Optional[float] = None,
                   device: str = "cuda", image_block: int = 32, details: bool = False, timing: bool = False) -> Dict[str, Any]:
    """BOP19 scores of `result_csv` against the split `split_dir` (<datasets>/<dataset>/<split>).  targets: a
    test_targets_bop19.json path or its list (default <split_dir>/../test_targets_bop19.json); models_dir: models_info.json +
    obj_XXXXXX.ply (default ../models_eval when it exists, else ../models); dataset: its name (default the parent directory's
    name; picks the VSD delta, 5 mm for itodd, else 15 mm, unless vsd_delta is given).  Depth images are processed in blocks
    of `image_block`.  details: also the per-(estimate, GT) errors; timing: also device-event times of the renders, VSD and
    MSSD / MSPD.  -> the scores dict."""
    import torch

    from . import eval_util, ops
    from .renderer import HipRasterizer, load_ply
    root = os.path.dirname(os.path.abspath(split_dir))
    if targets is None or isinstance(targets, str):
        targets = _read_json(targets or os.path.join(root, "test_targets_bop19.json"))
    if models_dir is None:
        models_dir = os.path.join(root, "models_eval")
        if not os.path.isdir(models_dir):
            models_dir = os.path.join(root, "models")
    dataset = dataset or os.path.basename(root)
    delta = float(vsd_delta) if vsd_delta is not None else VSD_DELTA.get(dataset, DEFAULT_VSD_DELTA)

    rows = load_results_csv(result_csv)
    avg_time = average_time_per_image(rows)
    tgt: Dict[Tuple[int, int, int], int] = {}
    for t_ in targets:
        key = (int(t_["scene_id"]), int(t_["im_id"]), int(t_["obj_id"]))
        tgt[key] = tgt.get(key, 0) + int(t_["inst_count"])
    kept = top_n(rows, tgt)
    obj_ids = sorted({k[2] for k in tgt})
    insts_per_obj = defaultdict(int)
    for k, n in tgt.items():
        insts_per_obj[k[2]] += n

    # ---- annotations and models
    scenes = sorted({k[0] for k in tgt})
    cams, gts, infos = {}, {}, {}
    for s in scenes:
        sd = os.path.join(split_dir, f"{s:06d}")
        cams[s] = _read_json(os.path.join(sd, "scene_camera.json"))
        gts[s] = _read_json(os.path.join(sd, "scene_gt.json"))
        infos[s] = _read_json(os.path.join(sd, "scene_gt_info.json"))
    models_info = _read_json(os.path.join(models_dir, "models_info.json"))
    meshes, diam, syms, pts_dev = {}, {}, {}, {}
    ras = HipRasterizer(device)
    for lid in obj_ids:
        info = models_info[str(lid)]
        meshes[lid] = load_ply(os.path.join(models_dir, f"obj_{lid:06d}.ply"), geometry_only=True)
        diam[lid] = float(info["diameter"])
        syms[lid] = eval_util.get_symmetry_transformations(info, max_sym_disc_step=0.01)
        pts_dev[lid] = torch.from_numpy(meshes[lid].vertices.astype(np.float64)).to(device)
        ras.add_object_model(lid, mesh=meshes[lid])

    # ---- per target: the kept estimates (score order), the GT instances of the object, the valid ones
    per_t = {}
    for key in sorted(tgt):
        s, im, lid = key
        ents = gts[s][str(im)]
        ivs = infos[s][str(im)]
        gids = [g for g, e in enumerate(ents) if int(e["obj_id"]) == lid]
        K = np.asarray(cams[s][str(im)]["cam_K"], np.float64).reshape(3, 3)
        per_t[key] = {"est": kept.get(key, []), "gid": gids, "K": K,
                      "gt": [_m2c(ents[g]["cam_R_m2c"], ents[g]["cam_t_m2c"]) for g in gids],
                      "valid": valid_gt_mask([float(ivs[g]["visib_fract"]) for g in gids], tgt[key])}
    work = [k for k in sorted(tgt) if per_t[k]["est"] and per_t[k]["gid"]]

    timer = DeviceTimer(timing)
    timed = timer.timed

    # ---- MSSD / MSPD: one fp_pose_errors launch per chunk of (estimate, GT) pairs
    pe_items, pe_where = [], []
    for key in work:
        d = per_t[key]
        d["mssd"] = np.zeros((len(d["est"]), len(d["gid"])))
        d["mspd"] = np.zeros_like(d["mssd"])
        for i, r in enumerate(d["est"]):
            for j, T in enumerate(d["gt"]):
                pe_items.append(dict(R_est=rows[r]["R"], t_est=rows[r]["t"], R_gt=T[:3, :3], t_gt=T[:3, 3], K=d["K"],
                                     pts=pts_dev[key[2]], syms=syms[key[2]]))
                pe_where.append((key, i, j))
    for c0 in range(0, len(pe_items), 512):
        err, _ = timed("mssd_mspd", eval_util.pose_errors_batch, pe_items[c0:c0 + 512], device)
        for (key, i, j), e in zip(pe_where[c0:c0 + 512], err):
            per_t[key]["mssd"][i, j], per_t[key]["mspd"][i, j] = e[0], e[1]

    # ---- VSD: per block of images, the test depths, one render per kept estimate and GT instance, one fp_vsd_counts call
    images = sorted({(k[0], k[1]) for k in work})
    n_unrenderable = 0
    width_of = {}
    taus = VSD_TAUS
    with ThreadPoolExecutor(max_workers=max(1, min(MAX_IO_WORKERS, image_block))) as pool:
        for b0 in range(0, len(images), image_block):
            block = images[b0:b0 + image_block]
            paths = [(os.path.join(split_dir, f"{s:06d}", "depth", f"{im:06d}.png"), float(cams[s][str(im)]["depth_scale"])) for s, im in block]
            depths = list(pool.map(lambda a: load_depth(*a), paths))
            by_size = defaultdict(list)
            for (s, im), dep in zip(block, depths):
                width_of[(s, im)] = dep.shape[1]
                by_size[dep.shape].append(((s, im), dep))
            for (H, W), group in by_size.items():
                n_unrenderable += _vsd_group(group, H, W, work, per_t, rows, meshes, diam, delta, taus, ras, ops, torch, device, timed)

    # ---- matching and recalls
    n_tau, n_th = len(VSD_TAUS), len(VSD_THS)
    tp = {"vsd": np.zeros(n_tau * n_th, np.int64), "mssd": np.zeros(len(MSSD_THS), np.int64), "mspd": np.zeros(len(MSPD_THS), np.int64)}
    tp_obj = {lid: {k: np.zeros_like(v) for k, v in tp.items()} for lid in obj_ids}
    err_details = []
    for key in work:
        d = per_t[key]
        ths = correct_thresholds(diam[key[2]], width_of[key[:2]])
        vsd = d["vsd"]                                             # [n_est, n_gt, n_tau]
        m = {"vsd": match_count(np.repeat(np.moveaxis(vsd, 2, 0), n_th, axis=0), np.tile(ths["vsd"], n_tau), d["valid"]),
             "mssd": match_count(np.broadcast_to(d["mssd"], (len(MSSD_THS),) + d["mssd"].shape), ths["mssd"], d["valid"]),
             "mspd": match_count(np.broadcast_to(d["mspd"], (len(MSPD_THS),) + d["mspd"].shape), ths["mspd"], d["valid"])}
        for k in tp:
            tp[k] += m[k]
            tp_obj[key[2]][k] += m[k]
        if details:
            for i, r in enumerate(d["est"]):
                for j, g in enumerate(d["gid"]):
                    err_details.append({"scene_id": key[0], "im_id": key[1], "obj_id": key[2], "row": r, "gt_id": g,
                                        "score": rows[r]["score"], "vsd": vsd[i, j].tolist(), "mssd": float(d["mssd"][i, j]),
                                        "mspd": float(d["mspd"][i, j]), "renderable": bool(d["renderable"][i])})

    def recalls(t, n):
        return {k: (v / float(n)) if n > 0 else np.zeros(len(v)) for k, v in t.items()}
    rec = recalls(tp, sum(tgt.values()))
    ar = {k: float(np.mean(v)) for k, v in rec.items()}
    out = {"bop19_average_recall": float(np.mean([ar["vsd"], ar["mssd"], ar["mspd"]])),
           "bop19_average_recall_vsd": ar["vsd"], "bop19_average_recall_mssd": ar["mssd"], "bop19_average_recall_mspd": ar["mspd"],
           "bop19_average_time_per_image": avg_time,
           "recall_vsd": rec["vsd"].reshape(n_tau, n_th).tolist(), "recall_mssd": rec["mssd"].tolist(), "recall_mspd": rec["mspd"].tolist(),
           "vsd_taus": VSD_TAUS.tolist(), "vsd_thresholds": VSD_THS.tolist(), "mssd_thresholds_x_diameter": MSSD_THS.tolist(),
           "mspd_thresholds_x_width_over_640": MSPD_THS.tolist(), "vsd_delta": delta,
           "num_targets": len(tgt), "num_target_instances": int(sum(tgt.values())),
           "num_estimates_evaluated": int(sum(len(per_t[k]["est"]) for k in tgt)), "num_unrenderable_estimates": int(n_unrenderable),
           "per_object": {}}
    for lid in obj_ids:
        r = recalls(tp_obj[lid], insts_per_obj[lid])
        a = {k: float(np.mean(v)) for k, v in r.items()}
        out["per_object"][str(lid)] = {"average_recall": float(np.mean([a["vsd"], a["mssd"], a["mspd"]])), "average_recall_vsd": a["vsd"],
                                       "average_recall_mssd": a["mssd"], "average_recall_mspd": a["mspd"], "num_instances": int(insts_per_obj[lid])}
    if details:
        out["errors"] = err_details
    if timing:
        out["device_seconds"] = timer.seconds()
    return out


def _vsd_group(group, H, W, work, per_t, rows, meshes, diam, delta, taus, ras, ops, torch, device, timed) -> int:
    """VSD errors of every (kept estimate, GT) pair of the images in `group` (one viewport size); -> unrenderable count."""
    img_index = {k: n for n, (k, _) in enumerate(group)}
    keys = [k for k in work if k[:2] in img_index]
    test = torch.from_numpy(np.stack([d for _, d in group])).to(device)
    # render requests per object: ("est", key, i) / ("gt", key, j) with the camera
    req = defaultdict(list)
    n_bad = 0
    for key in keys:
        d = per_t[key]
        K = d["K"]
        d["vsd"] = np.ones((len(d["est"]), len(d["gid"]), len(taus)))
        d["renderable"] = np.zeros(len(d["est"]), bool)
        for j, T in enumerate(d["gt"]):
            Tc = np.linalg.inv(T)
            if not prescreen(meshes[key[2]].vertices, Tc, K):
                raise ValueError(f"the GT pose of instance {d['gid'][j]} (scene {key[0]}, image {key[1]}, object {key[2]}) puts a vertex "
                                 f"within {NEAR_LIMIT_MM} mm of the camera or beyond the rasterizer's range")
            req[key[2]].append(("gt", key, j, _Camera(K, W, H, Tc)))
        for i, r in enumerate(d["est"]):
            Tc = np.linalg.inv(_m2c(rows[r]["R"], rows[r]["t"]))
            if prescreen(meshes[key[2]].vertices, Tc, K):
                d["renderable"][i] = True
                req[key[2]].append(("est", key, i, _Camera(K, W, H, Tc)))
            else:
                n_bad += 1   # VSD error 1 for every tau and GT: never VSD-correct
    n = {"est": 0, "gt": 0}
    slot = {}
    for lid in req:
        for kind, key, i, _ in req[lid]:
            slot[(kind, key, i)] = n[kind]
            n[kind] += 1
    if n["est"] == 0:
        return n_bad
    stacks = {k: torch.zeros(max(v, 1), H, W, dtype=torch.float32, device=device) for k, v in n.items()}
    boxes = {}
    for lid, rq in req.items():
        for c0 in range(0, len(rq), RENDER_CHUNK):
            chunk = rq[c0:c0 + RENDER_CHUNK]
            out = timed("render", ras.render_views, lid, [c for *_, c in chunk], with_color=False)
            for b, (kind, key, i, _) in enumerate(chunk):
                stacks[kind][slot[(kind, key, i)]].copy_(out["depth"][b])
            for b, bx in enumerate(out["boxes"].cpu().numpy()):
                boxes[chunk[b][:3]] = bx
    pairs, params, where = [], [], []
    for key in keys:
        d = per_t[key]
        K = d["K"]
        for i in range(len(d["est"])):
            if not d["renderable"][i]:
                continue
            be = boxes[("est", key, i)]
            for j in range(len(d["gid"])):
                bg = boxes[("gt", key, j)]
                x0, y0 = min(be[0], bg[0]), min(be[1], bg[1])
                x1, y1 = max(be[2], bg[2]), max(be[3], bg[3])
                if x0 > x1:   # both renders empty
                    x0, y0, x1, y1 = 0, 0, -1, -1
                pairs.append((img_index[key[:2]], slot[("est", key, i)], slot[("gt", key, j)], x0, y0, x1, y1))
                params.append((K[0, 0], K[1, 1], K[0, 2], K[1, 2], delta, diam[key[2]]))
                where.append((key, i, j))
    if pairs:
        counts = timed("vsd", ops.vsd_counts, test, stacks["est"], stacks["gt"], np.array(pairs, np.int64), np.array(params, np.float64), taus)
        errs = vsd_errors(counts.cpu().numpy())
        for (key, i, j), e in zip(where, errs):
            per_t[key]["vsd"][i, j] = e
    return n_bad


def main(argv: Optional[Sequence[str]] = None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--result-csv", required=True, help="BOP19 results csv (what infer / eval_util.prepare_bop_submission writes)")
    ap.add_argument("--dataset-dir", required=True, help="BOP split directory (<datasets>/<dataset>/<split>)")
    ap.add_argument("--targets", default=None, help="test_targets_bop19.json (default: <dataset-dir>/../test_targets_bop19.json)")
    ap.add_argument("--models-dir", default=None, help="models_info.json + obj_XXXXXX.ply (default: ../models_eval if it exists, else ../models)")
    ap.add_argument("--dataset", default=None, help="dataset name (default: the name of <dataset-dir>'s parent)")
    ap.add_argument("--vsd-delta", type=float, default=None, help="VSD visibility tolerance in mm (default: 5 for itodd, else 15)")
    ap.add_argument("--output", required=True, help="scores JSON")
    args = ap.parse_args(argv)
    t0 = time.perf_counter()
    scores = evaluate_bop19(args.result_csv, args.dataset_dir, args.targets, args.models_dir, args.dataset, vsd_delta=args.vsd_delta)
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as f:
        json.dump(scores, f, indent=2)
    print(f"bop19_average_recall {scores['bop19_average_recall']:.4f} (vsd {scores['bop19_average_recall_vsd']:.4f}, mssd "
          f"{scores['bop19_average_recall_mssd']:.4f}, mspd {scores['bop19_average_recall_mspd']:.4f}) over {scores['num_target_instances']} "
          f"instances in {time.perf_counter() - t0:.1f} s -> {args.output}")


if __name__ == "__main__":
    main()
