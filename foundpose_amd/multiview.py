"""Multi-view pose consensus for static scenes (csrc/multiview.hip).

Every other stage estimates a pose from one image; LM-O, T-LESS, YCB-V, HB and IC-BIN are static scenes photographed from many calibrated
viewpoints (scene_camera.json: cam_R_w2c / cam_t_w2c).  Here the estimates of one scene are lifted into the world, the estimates of one
object from different images that agree up to a symmetry are clustered greedily, and each cluster is refined to one world pose by
Levenberg-Marquardt on the reprojection error against the members' own projections (fp_multiview_refine): the object-level bundle
adjustment of CosyPose (Labbe et al., ECCV 2020) with the cameras known.  No image and no correspondence is read, only the poses, the
cameras and the models, so it runs on any BOP19 results csv:

    python -m foundpose_amd.multiview --result-csv in.csv --dataset-dir <split> --models-dir <models> --output out.csv \\
        [--match-thresh 1.0] [--huber-px 10] [--points 64] [--min-views 2] [--iters 20]

writes the csv -- same rows, same order, same scores -- and <output>.fuse.json with one record per row and one per cluster.
Static scenes only: a scene whose objects move between its images (TUD-L) must not be fused.  The cameras' poses are trusted.  None of
the defaults rests on a measurement on real data (limits)."""

import argparse
import json
import math
import os
from typing import Any, Dict, List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import upload_async

MAX_HYPOTHESES = 65535      # fp_pose_errors' limit of one call
MAX_PROBLEMS = 65535        # fp_multiview_refine's


class FuseOpts(NamedTuple):
    """The options of fuse_results.  None of the defaults rests on a measurement on real data."""
    match_thresh: float = 1.0    # a candidate joins a cluster whose seed lies within match_thresh x the object's diameter (3D, symmetry-aware)
    huber_px: float = 10.0       # the Huber delta of the reprojection error, in pixels
    points: int = 64             # model points per member: the object's stride sample (bank.sample_verify_points' rule)
    min_views: int = 2           # the smallest cluster that is refined
    iters: int = 20              # Levenberg-Marquardt iterations, at most


def check_opts(opts: FuseOpts) -> None:
    for name in ("match_thresh", "huber_px"):
        v = getattr(opts, name)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v > 0):
            raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    for name, lo, hi in (("points", 1, 4096), ("min_views", 2, 1 << 20), ("iters", 0, 1000)):
        v = getattr(opts, name)
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")


def _mat(R, t) -> np.ndarray:
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return T


def _camera_entry(scene_cameras, sid: int, iid: int):
    sc = None if not scene_cameras else scene_cameras.get(sid, scene_cameras.get(str(sid)))
    return None if sc is None else sc.get(str(iid), sc.get(iid))


def camera_pose(entry: Dict[str, Any], sid: int, iid: int) -> Tuple[np.ndarray, np.ndarray]:
    """A scene_camera.json entry -> (T_w2c 4x4 fp64, (fx, fy, cx, cy)).  A cam_R_w2c that is not finite or not a rotation (|R^T R - I| >
    1e-6 or det < 0), a cam_t_w2c or cam_K that is not finite: ValueError naming the image and the key."""
    R, t, K = (np.asarray(entry[k], np.float64).reshape(s) for k, s in (("cam_R_w2c", (3, 3)), ("cam_t_w2c", 3), ("cam_K", (3, 3))))
    if not np.isfinite(R).all() or np.abs(R.T @ R - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0:
        raise ValueError(f"scene {sid} image {iid}: cam_R_w2c is not a finite rotation matrix")
    if not np.isfinite(t).all():
        raise ValueError(f"scene {sid} image {iid}: cam_t_w2c is not finite")
    if not np.isfinite(K).all() or not (K[0, 0] > 0 and K[1, 1] > 0):
        raise ValueError(f"scene {sid} image {iid}: cam_K is not a finite pinhole matrix")
    return _mat(R, t), np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])


def model_sample(pts, points: int) -> np.ndarray:
    """The object's stride sample, bank.sample_verify_points' rule as pose_nms.samples_from_vertices uses it: rows 0, s, 2 s, ... with s =
    ceil(V / points), as the fp32 values the device holds.  -> fp64 [M, 3], M <= points."""
    from . import bank
    v = torch.as_tensor(np.asarray(pts)).reshape(-1, 3)
    return bank.sample_verify_points(v, [(0, int(v.shape[0]))], points)[0].numpy().astype(np.float64)


def _sym_stack(syms) -> np.ndarray:
    return np.stack([_mat(s["R"], np.asarray(s["t"], np.float64).reshape(3)) for s in syms])


def seed_distances(pairs: Sequence[Tuple[np.ndarray, np.ndarray, int]], samples: List[np.ndarray], sym_stacks: List[np.ndarray], device="cuda"):
    """d(i, j) = min over S of max over x of |W_i x - W_j S x| for every pair (W_i, W_j, object index), by ops.pose_errors (the MSSD
    column and its symmetry index; a pair is a hypothesis whose estimate is W_i and whose ground truth is W_j), in as many calls as
    fp_pose_errors' limit of hypotheses asks for.  -> (d fp64 [P], symmetry index int64 [P])."""
    P = len(pairs)
    d, k = np.zeros(P), np.zeros(P, np.int64)
    if P == 0:
        return d, k
    pt_off = np.concatenate([[0], np.cumsum([len(s) for s in samples])])
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(samples))).to(device)
    flat = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]])   # the MSPD column is not read: a projection that divides by 1
    for c0 in range(0, P, MAX_HYPOTHESES):
        part = pairs[c0:c0 + MAX_HYPOTHESES]
        est, gt, ranges, at = [], [], [], 0
        for Wi, Wj, o in part:
            WS = Wj[None] @ sym_stacks[o]
            est.append(Wi[:3].reshape(12)[[0, 1, 2, 4, 5, 6, 8, 9, 10, 3, 7, 11]])
            gt.append(WS[:, :3].reshape(-1, 12)[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 3, 7, 11]])
            ranges.append((pt_off[o], len(samples[o]), at, len(WS)))
            at += len(WS)
        est, gt = np.stack(est), np.concatenate(gt)
        p_est = np.tile(flat.reshape(1, 12), (len(est), 1))
        p_gt = np.tile(flat.reshape(1, 12), (len(gt), 1))
        up = lambda a: upload_async(torch.from_numpy(np.ascontiguousarray(a, np.float64)), device)   # noqa: E731
        err, idx = ops.pose_errors(pts, up(est), up(p_est), up(gt), up(p_gt), np.asarray(ranges, np.int64))
        d[c0:c0 + len(part)] = err[:, 0].cpu().numpy()
        k[c0:c0 + len(part)] = idx[:, 1].cpu().numpy()
    return d, k


def greedy_clusters(cands: Sequence[int], image: Dict[int, int], score: Dict[int, float], dist: Dict[Tuple[int, int], Tuple[float, int]],
                    bar: float) -> List[Dict[str, Any]]:
    """The candidates (input rows) of one (scene, object), by (score descending, row ascending): each joins the cluster that holds no
    candidate of its own image and whose SEED lies within `bar`, the nearest such seed (ties: the older cluster), else it seeds a new
    cluster.  dist[(i, j)] = (d, symmetry index) of candidate i against candidate j, j before i in that order.
    -> [{"seed": row, "members": [(row, symmetry index or -1 for the seed, d)]}] in the order the clusters were seeded."""
    clusters: List[Dict[str, Any]] = []
    for i in sorted(cands, key=lambda i: (-score[i], i)):
        best = None
        for c in clusters:
            if any(image[m] == image[i] for m, _, _ in c["members"]):
                continue
            d, k = dist[(i, c["seed"])]
            if d <= bar and (best is None or d < best[1]):
                best = (c, d, k)
        if best is None:
            clusters.append({"seed": i, "members": [(i, -1, 0.0)]})
        else:
            best[0]["members"].append((i, best[2], best[1]))
    return clusters


def _rotation_deg(Ra, Rb) -> float:
    return float(np.degrees(np.arccos(np.clip(0.5 * (np.trace(np.asarray(Ra) @ np.asarray(Rb).T) - 1.0), -1.0, 1.0))))


def fuse_results(rows: Sequence[Dict[str, Any]], scene_cameras: Dict[Any, Dict[str, Any]], models: Dict[int, Any], opts: FuseOpts = None, device="cuda",
                 **kw) -> Tuple[List[Dict[str, Any]], Dict[str, Any]]:
    """Fuses the rows of a BOP19 results csv (eval_bop19.load_results_csv's dicts) scene by scene.  scene_cameras: {scene_id: the scene's
    scene_camera.json}; models: {obj_id: eval_util.EvalModel} (pts, syms -- the list the evaluators use --, diameter); opts: a FuseOpts, or
    its fields as keywords.  None of the defaults rests on a measurement on real data.
    A scene is fused only when every image its rows name has cam_K, cam_R_w2c and cam_t_w2c (mm); the rows of any other scene pass
    through untouched and the report names the scene.  A member of a cluster of at least min_views whose solve ended with status 0 or 1 gets
    T_w2c W S -- the consensus' symmetry equivalent nearest its own estimate --, every other row keeps its bytes; scores, row order and
    row count never change.  Three device calls per 65535 pairs / clusters: ops.pose_errors for the distances, ops.multiview_refine.
    -> (rows', report): report["rows"][i] = {row, scene_id, im_id, obj_id, cluster, seed_row, views, sym, dist_to_seed_mm, moved_mm,
    moved_deg, fused, reason}, report["clusters"][c] = {cluster, scene_id, obj_id, seed_row, rows, dropped_rows, status, cost_in,
    cost_out, iters_used, inliers}, report["unfused_scenes"] = [{scene_id, reason}]."""
    opts = (opts or FuseOpts())._replace(**kw)
    check_opts(opts)
    out = [dict(r) for r in rows]
    rep_rows = [{"row": i, "scene_id": r["scene_id"], "im_id": r["im_id"], "obj_id": r["obj_id"], "cluster": None, "seed_row": None, "views": 0,
                 "sym": None, "dist_to_seed_mm": None, "moved_mm": 0.0, "moved_deg": 0.0, "fused": False, "reason": None} for i, r in enumerate(rows)]
    report = {"rows": rep_rows, "clusters": [], "unfused_scenes": []}
    scenes: Dict[int, List[int]] = {}
    for i, r in enumerate(rows):
        scenes.setdefault(r["scene_id"], []).append(i)
    # ---- the lift, and the candidates of every (scene, object)
    cam_of: Dict[Tuple[int, int], Tuple[np.ndarray, np.ndarray]] = {}
    W: Dict[int, np.ndarray] = {}
    groups: List[Tuple[int, int, List[int]]] = []
    for sid, members in scenes.items():
        why = None
        for i in members:
            e = _camera_entry(scene_cameras, sid, rows[i]["im_id"])
            if e is None or any(k not in e for k in ("cam_K", "cam_R_w2c", "cam_t_w2c")):
                why = f"image {rows[i]['im_id']} has no cam_K / cam_R_w2c / cam_t_w2c"
                break
        if why is not None:
            report["unfused_scenes"].append({"scene_id": sid, "reason": why})
            for i in members:
                rep_rows[i]["reason"] = "scene not fused: " + why
            continue
        by_obj: Dict[int, List[int]] = {}
        for i in members:
            key = (sid, rows[i]["im_id"])
            if key not in cam_of:
                cam_of[key] = camera_pose(_camera_entry(scene_cameras, *key), *key)
            W[i] = np.linalg.inv(cam_of[key][0]) @ _mat(rows[i]["R"], rows[i]["t"])
            by_obj.setdefault(rows[i]["obj_id"], []).append(i)
        groups.extend((sid, oid, c) for oid, c in by_obj.items())
    if not groups:
        return out, report
    oids = sorted({oid for _, oid, _ in groups})
    for oid in oids:
        if oid not in models:
            raise ValueError(f"no model for object {oid}")
    obj_ix = {oid: o for o, oid in enumerate(oids)}
    samples = [model_sample(models[oid].pts, opts.points) for oid in oids]
    sym_stacks = [_sym_stack(models[oid].syms) for oid in oids]
    # ---- the distances of every later candidate to every earlier one of another image, then the greedy rule on the host
    pair_keys, pairs = [], []
    for sid, oid, cands in groups:
        order = sorted(cands, key=lambda i: (-rows[i]["score"], i))
        for a, i in enumerate(order):
            for j in order[:a]:
                if rows[i]["im_id"] != rows[j]["im_id"]:
                    pair_keys.append((i, j))
                    pairs.append((W[i], W[j], obj_ix[oid]))
    d, k = seed_distances(pairs, samples, sym_stacks, device)
    dist = {key: (float(d[n]), int(k[n])) for n, key in enumerate(pair_keys)}
    image = {i: rows[i]["im_id"] for i in W}
    score = {i: rows[i]["score"] for i in W}
    problems = []
    for sid, oid, cands in groups:
        for c in greedy_clusters(cands, image, score, dist, opts.match_thresh * float(models[oid].diameter)):
            cid = len(report["clusters"])
            rec = {"cluster": cid, "scene_id": sid, "obj_id": oid, "seed_row": c["seed"], "rows": [m for m, _, _ in c["members"]], "dropped_rows": 0,
                   "status": None, "cost_in": None, "cost_out": None, "iters_used": None, "inliers": None}
            report["clusters"].append(rec)
            for m, s, dm in c["members"]:
                rep_rows[m].update(cluster=cid, seed_row=c["seed"], views=len(c["members"]), sym=s, dist_to_seed_mm=dm)
                if len(c["members"]) < opts.min_views:
                    rep_rows[m]["reason"] = "singleton" if len(c["members"]) == 1 else f"fewer than {opts.min_views} views"
            if len(c["members"]) >= opts.min_views:
                problems.append((rec, c, oid))
    # ---- the rows of every problem: member x sampled point, the target the member's own estimate projects it to
    views: Dict[Tuple[int, int], int] = {}
    Y, uv, vi, rb, re_, R0, t0, S_of = [], [], [], [], [], [], [], {}
    at = 0
    for rec, c, oid in problems:
        X, stack = samples[obj_ix[oid]], sym_stacks[obj_ix[oid]]
        rb.append(at)
        for m, s, _ in c["members"]:
            key = (rec["scene_id"], rows[m]["im_id"])
            cam = cam_of[key][1]
            S_of[m] = np.eye(4) if s < 0 else stack[s]
            M = _mat(rows[m]["R"], rows[m]["t"]) @ np.linalg.inv(S_of[m])
            Xc = X @ M[:3, :3].T + M[:3, 3]
            keep = Xc[:, 2] > 1.0
            rec["dropped_rows"] += int((~keep).sum())
            Y.append(X[keep])
            uv.append(np.stack([cam[0] * Xc[keep, 0] / Xc[keep, 2] + cam[2], cam[1] * Xc[keep, 1] / Xc[keep, 2] + cam[3]], 1))
            vi.append(np.full(int(keep.sum()), views.setdefault(key, len(views))))
            at += int(keep.sum())
        re_.append(at)
        R0.append(W[c["seed"]][:3, :3])
        t0.append(W[c["seed"]][:3, 3])
    if problems and at > 0:
        up = lambda a, dt: upload_async(torch.from_numpy(np.ascontiguousarray(a, dt)), device)   # noqa: E731
        keys = sorted(views, key=views.get)
        view_cam = up(np.stack([cam_of[key][1] for key in keys]), np.float64)
        view_T = up(np.stack([np.concatenate([cam_of[key][0][:3, :3].reshape(9), cam_of[key][0][:3, 3]]) for key in keys]), np.float64)
        pts, tgt, vix = up(np.concatenate(Y), np.float32), up(np.concatenate(uv), np.float64), up(np.concatenate(vi), np.int32)
        res = {}
        for c0 in range(0, len(problems), MAX_PROBLEMS):
            sl = slice(c0, c0 + MAX_PROBLEMS)
            part = ops.multiview_refine(pts, tgt, vix, view_cam, view_T, up(rb[sl], np.int32), up(re_[sl], np.int32), up(np.stack(R0[sl]), np.float64),
                                        up(np.stack(t0[sl]), np.float64), float(opts.huber_px), int(opts.iters))
            for key, v in part.items():
                res.setdefault(key, []).append(v.cpu().numpy())
        res = {key: np.concatenate(v) for key, v in res.items()}
    # ---- write back
    for n, (rec, c, oid) in enumerate(problems):
        if at == 0:
            st = 2
            rec.update(status=2, cost_in=0.0, cost_out=0.0, iters_used=0, inliers=0)
        else:
            st = int(res["status"][n])
            rec.update(status=st, cost_in=float(res["cost_in"][n]), cost_out=float(res["cost_out"][n]), iters_used=int(res["iters_used"][n]),
                       inliers=int(res["num_points"][n]))
        for m, _, _ in c["members"]:
            if st == 2:
                rep_rows[m]["reason"] = "fewer than 6 inliers at the seed's pose"
                continue
            T = cam_of[(rec["scene_id"], rows[m]["im_id"])][0] @ _mat(res["R"][n], res["t"][n]) @ S_of[m]
            rep_rows[m].update(fused=True, moved_mm=float(np.linalg.norm(T[:3, 3] - np.asarray(rows[m]["t"], np.float64).reshape(3))),
                               moved_deg=_rotation_deg(T[:3, :3], np.asarray(rows[m]["R"], np.float64).reshape(3, 3)))
            out[m]["R"], out[m]["t"] = T[:3, :3].copy(), T[:3, 3].copy()
    return out, report


# ---------------------------------------------------------------------------------------------------- files
def load_scene_cameras(split_dir: str, scene_ids) -> Dict[int, Dict[str, Any]]:
    """<split>/<scene:06d>/scene_camera.json of every scene named; a scene without the file is left out (it is then not fused)."""
    out = {}
    for sid in sorted(set(scene_ids)):
        path = os.path.join(split_dir, f"{sid:06d}", "scene_camera.json")
        if os.path.exists(path):
            with open(path) as f:
                out[sid] = json.load(f)
    return out


def load_models(models_dir: str, lids, max_sym_disc_step: float = 0.01) -> Dict[int, Any]:
    """{obj_id: eval_util.EvalModel}.  A missing models_info.json raises and names the file: symmetric objects must not be fused as
    asymmetric ones."""
    from . import eval_util
    path = os.path.join(models_dir, "models_info.json")
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: the objects' diameters and symmetries come from it")
    with open(path) as f:
        info = json.load(f)
    return {lid: eval_util.load_eval_model(models_dir, lid, max_sym_disc_step, info) for lid in sorted(set(lids))}


def write_report(path: str, report: Dict[str, Any]) -> None:
    with open(path, "w") as f:
        json.dump(report, f, indent=1)


def main(argv=None) -> None:
    from . import eval_bop19, pose_nms
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--result-csv", required=True, help="a BOP19 results csv")
    ap.add_argument("--dataset-dir", required=True, help="the BOP split directory: <scene:06d>/scene_camera.json with cam_R_w2c / cam_t_w2c")
    ap.add_argument("--models-dir", required=True, help="models_info.json and obj_XXXXXX.ply of every object the csv names")
    ap.add_argument("--output", required=True, help="the csv with the fused poses; <output>.fuse.json gets every row's and every cluster's record")
    d = FuseOpts()
    ap.add_argument("--match-thresh", type=float, default=d.match_thresh)
    ap.add_argument("--huber-px", type=float, default=d.huber_px)
    ap.add_argument("--points", type=int, default=d.points)
    ap.add_argument("--min-views", type=int, default=d.min_views)
    ap.add_argument("--iters", type=int, default=d.iters)
    args = ap.parse_args(argv)
    opts = FuseOpts(args.match_thresh, args.huber_px, args.points, args.min_views, args.iters)
    check_opts(opts)
    rows = eval_bop19.load_results_csv(args.result_csv)
    models = load_models(args.models_dir, {r["obj_id"] for r in rows})
    fused, report = fuse_results(rows, load_scene_cameras(args.dataset_dir, {r["scene_id"] for r in rows}), models, opts)
    pose_nms.write_results_csv(args.output, fused)
    write_report(args.output + ".fuse.json", report)
    n = sum(r["fused"] for r in report["rows"])
    print(f"{n} of {len(rows)} rows fused in {sum(c['status'] in (0, 1) for c in report['clusters'])} clusters -> {args.output}")


if __name__ == "__main__":
    main()
