"""Duplicate poses within a frame: 3D overlap and greedy suppression on the device (csrc/pose_nms.hip).

Every other stage works per detection; two proposals on one physical instance give two nearly identical poses, and both take a target
slot of the BOP evaluation.  Here the poses of one frame are looked at together: for an ordered pair (i, j) fp_pose_overlap measures
which fraction of i's model sample lies in cells of a G x G x G grid that j's sample occupies -- two bodies cannot share space, whatever
their symmetries --, and fp_pose_nms_greedy keeps, in the order of the scores, every pose that conflicts with no kept one.

    python -m foundpose_amd.pose_nms --result-csv in.csv --models-dir <bop root>/<dataset>/models --output out.csv \\
        [--thresh 0.3] [--grid 16] [--max-points 4096] [--cross-object]

writes the kept rows in their input order and <output>.nms.json with one record per input row.  The defaults rest on no measurement
(limits)."""

import argparse
import json
import math
import os
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import upload_async

MIN_GRID, MAX_GRID = 8, 32   # PN_MIN_GRID / PN_MAX_GRID of csrc/kernels.hpp
MAX_GROUP = 256              # PN_MAX_GROUP: poses of one frame


def _host(x, dtype, name: str) -> np.ndarray:
    """A host table as a contiguous numpy array of `dtype` (lists, numpy arrays and CPU tensors); a device tensor is refused, not copied."""
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            raise ValueError(f"{name} is a host table (it is validated on the host and uploaded once), got a tensor on {x.device}")
        x = x.numpy()
    a = np.asarray(x)
    if a.dtype == object or a.dtype.kind not in "biuf":
        raise ValueError(f"{name} must be numeric, got dtype {a.dtype}")
    if np.dtype(dtype).kind == "i" and a.dtype.kind == "f" and a.size:   # (an empty list is float64 to numpy)
        raise ValueError(f"{name} must hold integers, got dtype {a.dtype}")
    return np.ascontiguousarray(a, dtype)


def _check_grid(grid) -> None:
    if isinstance(grid, bool) or not isinstance(grid, int) or not MIN_GRID <= grid <= MAX_GRID:
        raise ValueError(f"grid must be an integer in [{MIN_GRID}, {MAX_GRID}], got {grid!r}")


def _check_thresh(thresh) -> None:
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float)) or not (math.isfinite(thresh) and 0 < thresh <= 1):
        raise ValueError(f"thresh must be a finite number in (0, 1], got {thresh!r}")


def _check_offsets(off: np.ndarray, total: int, name: str, what: str) -> None:
    if off.ndim != 1 or off.size < 1 or off[0] != 0 or off[-1] != total or (np.diff(off) < 0).any():
        raise ValueError(f"{name} must be int32 [F + 1], non-decreasing from 0 to the {total} {what}, got {off.tolist() if off.size <= 16 else off.shape}")


def _overlap_tables(points, ranges, centers, radii, pose_obj, valid, R, t, pairs, grid):
    """Checks pose_overlaps' arguments.  -> (reals, ints, sizes): the fp64 and int32 tables in upload order and (O, N, P)."""
    _check_grid(grid)
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must be a float32 tensor [M_total, 3] on the device, got "
                         f"{(points.dtype, list(points.shape)) if isinstance(points, torch.Tensor) else type(points).__name__}")
    M = int(points.shape[0])
    if M > 1 << 30:
        raise ValueError(f"{M} sampled points: at most 2^30")
    rng = _host(ranges, np.int64, "ranges")
    O = int(rng.shape[0])
    cen, rad = _host(centers, np.float64, "centers"), _host(radii, np.float64, "radii")
    if rng.shape != (O, 2) or cen.shape != (O, 3) or rad.shape != (O,):
        raise ValueError(f"ranges [O, 2], centers [O, 3] and radii [O] of the same O objects, got {rng.shape}, {cen.shape}, {rad.shape}")
    rng = np.clip(rng, 0, M).astype(np.int32)   # the point ranges clamped against M_total
    obj = _host(pose_obj, np.int32, "pose_obj")
    N = int(obj.shape[0]) if obj.ndim == 1 else -1
    ok = _host(valid, np.int32, "valid")
    Rh, th = _host(R, np.float64, "R"), _host(t, np.float64, "t")
    if N < 0 or ok.shape != (N,) or Rh.shape not in ((N, 3, 3), (N, 9)) or th.shape != (N, 3):
        raise ValueError(f"pose_obj [N], valid [N], R [N, 3, 3] and t [N, 3] of the same N poses, got {obj.shape}, {ok.shape}, {Rh.shape}, {th.shape}")
    if N and not ((obj >= 0) & (obj < O)).all():
        bad = int(np.nonzero((obj < 0) | (obj >= O))[0][0])
        raise ValueError(f"pose {bad}: object {int(obj[bad])} outside the samples' [0, {O})")
    pr = _host(pairs, np.int32, "pairs")
    if pr.ndim != 2 or pr.shape[1] != 2:
        if pr.size:
            raise ValueError(f"pairs must be int32 [P, 2], got {pr.shape}")
        pr = pr.reshape(0, 2)
    P = int(pr.shape[0])
    if P and not ((pr >= 0) & (pr < N)).all():
        bad = int(np.nonzero(((pr < 0) | (pr >= N)).any(1))[0][0])
        raise ValueError(f"pair {bad} = {pr[bad].tolist()} names a pose outside [0, {N})")
    if not points.is_cuda:
        raise ValueError(f"points must be a float32 tensor [M_total, 3] on the device, got one on {points.device}")
    return [cen, rad, Rh, th], [rng, obj, ok, pr], (O, N, P)


def _upload_tables(reals: Sequence[np.ndarray], ints: Sequence[np.ndarray], device):
    """One byte buffer, one upload: the fp64 tables followed by the int32 tables, each read back as its own type (the int32 part starts at
    a multiple of 8 bytes).  -> (fp64 views, int32 views) with the tables' own shapes."""
    flat = [np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in list(reals) + list(ints)]
    raw = upload_async(torch.from_numpy(np.concatenate(flat) if flat else np.zeros(0, np.uint8)), device)
    out, at = [], 0
    for a, dt in [(a, torch.float64) for a in reals] + [(a, torch.int32) for a in ints]:
        out.append(raw[at:at + a.nbytes].view(dt).reshape(a.shape))
        at += a.nbytes
    return out[:len(reals)], out[len(reals):]


def pose_overlaps(points: torch.Tensor, ranges, centers, radii, pose_obj, valid, R, t, pairs, grid: int = 16) -> Dict[str, torch.Tensor]:
    """For every ordered pair (i, j) of `pairs`: the fraction of pose i's model sample that lies in space occupied by pose j's model
    (fp_pose_overlap; the contract: include/foundpose_amd.h).
    points f32 [M_total, 3] on the device with per-object ranges [O, 2], centers [O, 3] and radii [O]: bank.sample_verify_points /
    sample_spheres' compact samples (a VerifyPoints' fields); per pose: pose_obj [N] (its object's index), valid [N], R [N, 3, 3], t [N, 3]
    fp64, all poses of a pair in one common coordinate frame; pairs int [P, 2].  Everything but `points` is a host table: checked here and
    sent in one upload.
    -> counts int32 [P, 2] = (n_in, n_cells), overlap f64 [P], status int32 [P] (0 scored, 1 disjoint spheres, 2 skipped), on the device;
    nothing waits for them.  P = 0 returns empty tensors without a launch; a wrong shape, dtype, device, index or grid raises ValueError
    before anything is launched."""
    reals, ints, (_, _, P) = _overlap_tables(points, ranges, centers, radii, pose_obj, valid, R, t, pairs, grid)
    if P == 0:
        dev = points.device
        return {"counts": torch.zeros(0, 2, dtype=torch.int32, device=dev), "overlap": torch.zeros(0, dtype=torch.float64, device=dev),
                "status": torch.zeros(0, dtype=torch.int32, device=dev)}
    (cen, rad, Rd, td), (rng, obj, ok, pr) = _upload_tables(reals, ints, points.device)
    counts, overlap, status = ops.pose_overlap(points, rng, cen, rad, obj, ok, Rd, td, pr, grid)
    return {"counts": counts, "overlap": overlap, "status": status}


def _check_groups(group_off, pair_off, num_pairs: int) -> Tuple[np.ndarray, np.ndarray]:
    go, po = _host(group_off, np.int32, "group_off"), _host(pair_off, np.int32, "pair_off")
    _check_offsets(go, int(go[-1]) if go.ndim == 1 and go.size else 0, "group_off", "poses")
    _check_offsets(po, num_pairs, "pair_off", "pairs")
    if po.shape != go.shape:
        raise ValueError(f"group_off and pair_off describe the same frames: {go.shape[0] - 1} against {po.shape[0] - 1}")
    sizes = np.diff(go)
    if sizes.size and int(sizes.max()) > MAX_GROUP:
        raise ValueError(f"frame {int(sizes.argmax())} has {int(sizes.max())} poses: at most {MAX_GROUP} per frame")
    return go, po


def nms_greedy(group_off, pair_off, pairs, overlap: torch.Tensor, status: torch.Tensor, thresh: float = 0.3) -> Dict[str, torch.Tensor]:
    """Greedy suppression per frame (fp_pose_nms_greedy).  group_off / pair_off int [F + 1] (host): frame f owns the poses
    [group_off[f], group_off[f + 1]) -- IN RANK ORDER, best first, at most 256 -- and the pairs [pair_off[f], pair_off[f + 1]); pairs
    int32 [P, 2] (a host table, or the device tensor an earlier upload left), overlap f64 [P] and status int32 [P] on the device, as
    pose_overlaps returns them (nothing is read back in between).  Two poses of a frame conflict iff a pair of them, in either direction,
    has status 0 and overlap >= thresh.
    -> keep int32 [N] (1 / 0), suppressed_by int32 [N] (the first kept pose in rank order that conflicts, -1 for a kept pose), on the
    device."""
    _check_thresh(thresh)
    for name, x, dt in (("overlap", overlap, torch.float64), ("status", status, torch.int32)):
        if not isinstance(x, torch.Tensor) or x.dtype != dt or x.dim() != 1:
            raise ValueError(f"{name} must be a {dt} tensor [P] on the device, got {(x.dtype, list(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__}")
    P = int(overlap.shape[0])
    if int(status.shape[0]) != P:
        raise ValueError(f"{P} overlaps and {int(status.shape[0])} statuses")
    go, po = _check_groups(group_off, pair_off, P)
    N = int(go[-1])
    on_device = isinstance(pairs, torch.Tensor) and pairs.is_cuda
    if on_device:
        if pairs.dtype != torch.int32 or tuple(pairs.shape) != (P, 2):
            raise ValueError(f"pairs must be int32 [{P}, 2], got {(pairs.dtype, list(pairs.shape))}")
    else:
        pairs = _host(pairs, np.int32, "pairs").reshape(-1, 2)
        if pairs.shape[0] != P:
            raise ValueError(f"{pairs.shape[0]} pairs for {P} overlaps")
        frame_of = np.repeat(np.arange(len(go) - 1), np.diff(po))
        if P and not ((pairs >= go[frame_of][:, None]) & (pairs < go[frame_of + 1][:, None])).all():
            raise ValueError("a pair names a pose outside its own frame")
    if not overlap.is_cuda or not status.is_cuda:
        raise ValueError(f"overlap and status must be on the device, got {overlap.device} and {status.device}")
    dev = overlap.device
    if on_device:
        _, (god, pod) = _upload_tables([], [go, po], dev)
        prd = pairs.contiguous()
    else:
        _, (god, pod, prd) = _upload_tables([], [go, po, pairs], dev)
    keep, by = ops.pose_nms_greedy(god, pod, prd, overlap.contiguous(), status.contiguous(), N, float(thresh))
    return {"keep": keep, "suppressed_by": by}


def frame_pairs(group_off, pose_obj, cross_object: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """The ordered pairs fp_pose_overlap scores: both directions of every unordered pair of poses of one frame -- of the same object only,
    unless cross_object.  group_off [F + 1]: frame f owns the poses [group_off[f], group_off[f + 1]); pose_obj [N].
    -> (pairs int32 [P, 2], pair_off int32 [F + 1]): a frame's pairs are contiguous, (a, b) before (a, b') for b < b'."""
    go, obj = _host(group_off, np.int64, "group_off"), _host(pose_obj, np.int64, "pose_obj")
    _check_offsets(go, int(obj.shape[0]), "group_off", "poses")
    pairs, pair_off = [], [0]
    for b, e in zip(go[:-1], go[1:]):
        n = int(e - b)
        a, c = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        take = a != c
        if not cross_object:
            take &= obj[b:e][a] == obj[b:e][c]
        pairs.append(np.stack([a[take] + b, c[take] + b], 1))
        pair_off.append(pair_off[-1] + int(take.sum()))
    out = np.concatenate(pairs, 0) if pairs else np.zeros((0, 2), np.int64)
    return out.astype(np.int32).reshape(-1, 2), np.asarray(pair_off, np.int32)


def rank_layout(rows: Sequence[Dict[str, Any]]) -> Tuple[np.ndarray, np.ndarray]:
    """Rows grouped by (scene_id, im_id) -- frames in the order of their first row --, and within a frame by score descending, equal scores
    in input order (eval_bop19.top_n's stable sort).  -> (order [N]: the row at each place of the layout, group_off int32 [F + 1])."""
    frames: Dict[Tuple[int, int], List[int]] = {}
    for i, r in enumerate(rows):
        frames.setdefault((r["scene_id"], r["im_id"]), []).append(i)
    order, group_off = [], [0]
    for members in frames.values():
        order.extend(sorted(members, key=lambda i: rows[i]["score"], reverse=True))
        group_off.append(len(order))
    return np.asarray(order, np.int64), np.asarray(group_off, np.int32)


def suppress_duplicates(rows: Sequence[Dict[str, Any]], samples, thresh: float = 0.3, grid: int = 16, cross_object: bool = False) -> Dict[str, np.ndarray]:
    """Greedy duplicate suppression over the rows of a BOP19 results csv (eval_bop19.load_results_csv's dicts: scene_id, im_id, obj_id,
    score, R, t).  Rows are grouped by (scene_id, im_id); by the BOP format a frame's rows are poses in one coordinate frame (its camera's),
    and that frame is the one used.  samples = (a bank.VerifyPoints -- or any tuple with its fields --, {obj_id: object index in it}).
    Two launches, nothing read back in between.
    -> per row, in input order: keep bool [N]; suppressed_by int64 [N], the ROW that suppressed it or -1; overlap f64 [N], the overlap that
    decided (the larger of the two directions between the row and its suppressor; NaN for a kept row)."""
    _check_thresh(thresh)
    _check_grid(grid)
    vp, lid_to_obj = samples
    n_rows = len(rows)
    out = {"keep": np.ones(n_rows, bool), "suppressed_by": np.full(n_rows, -1, np.int64), "overlap": np.full(n_rows, np.nan)}
    if n_rows == 0:
        return out
    for i, r in enumerate(rows):
        if r["obj_id"] not in lid_to_obj:
            raise ValueError(f"row {i}: no point sample for object {r['obj_id']}")
    order, group_off = rank_layout(rows)
    sizes = np.diff(group_off)
    if int(sizes.max()) > MAX_GROUP:
        key = (rows[order[group_off[sizes.argmax()]]]["scene_id"], rows[order[group_off[sizes.argmax()]]]["im_id"])
        raise ValueError(f"scene {key[0]} image {key[1]} has {int(sizes.max())} poses: at most {MAX_GROUP} per frame")
    obj = np.asarray([lid_to_obj[rows[i]["obj_id"]] for i in order], np.int32)
    R = np.stack([np.asarray(rows[i]["R"], np.float64).reshape(3, 3) for i in order])
    t = np.stack([np.asarray(rows[i]["t"], np.float64).reshape(3) for i in order])
    pairs, pair_off = frame_pairs(group_off, obj, cross_object)
    if len(pairs) == 0:   # no two poses to compare: nothing to upload or launch
        return out
    reals, ints, (_, N, _) = _overlap_tables(vp.points, vp.ranges, vp.centers, vp.radii, obj, np.ones(n_rows, np.int32), R, t, pairs, grid)
    dev = vp.points.device
    (cen, rad, Rd, td), (rng, objd, ok, prd, god, pod) = _upload_tables(reals, ints + [group_off, pair_off], dev)
    _, overlap, status = ops.pose_overlap(vp.points, rng, cen, rad, objd, ok, Rd, td, prd, grid)
    keep, by = ops.pose_nms_greedy(god, pod, prd, overlap, status, N, float(thresh))
    keep, by, overlap, status = (x.cpu().numpy() for x in (keep, by, overlap, status))   # the one wait of the stage
    decided = {}   # suppressed pose -> the larger of the two directions between it and its suppressor
    for (a, b), ov, st in zip(pairs.tolist(), overlap.tolist(), status.tolist()):
        if st == 0 and (by[a] == b or by[b] == a):
            lost = a if by[a] == b else b
            decided[lost] = max(decided.get(lost, 0.0), ov)
    for place, row in enumerate(order.tolist()):
        out["keep"][row] = bool(keep[place])
        if by[place] >= 0:
            out["suppressed_by"][row] = int(order[by[place]])
            out["overlap"][row] = decided[place]
    return out


# ---------------------------------------------------------------------------------------------------- files
def write_results_csv(path: str, rows: Sequence[Dict[str, Any]]) -> None:
    """Rows -> a BOP19 results csv, in eval_util.prepare_bop_submission's format (str() of every number: reading the file back with
    eval_bop19.load_results_csv and writing it again gives the same bytes)."""
    lines = ["scene_id,im_id,obj_id,score,R,t,time"]
    for r in rows:
        lines.append("{},{},{},{},{},{},{}".format(
            r["scene_id"], r["im_id"], r["obj_id"], r["score"], " ".join(map(str, np.asarray(r["R"], np.float64).flatten().tolist())),
            " ".join(map(str, np.asarray(r["t"], np.float64).flatten().tolist())), r["time"]))
    with open(path, "wb") as f:
        f.write("\n".join(lines).encode("utf-8"))


def decision_records(rows: Sequence[Dict[str, Any]], result: Dict[str, np.ndarray]) -> List[Dict[str, Any]]:
    """One record per input row: its place in the input, its frame and object, keep, the row that suppressed it (or -1) and the overlap
    that decided (null for a kept row)."""
    return [{"row": i, "scene_id": r["scene_id"], "im_id": r["im_id"], "obj_id": r["obj_id"], "keep": bool(result["keep"][i]),
             "suppressed_by": int(result["suppressed_by"][i]), "overlap": None if result["keep"][i] else float(result["overlap"][i])}
            for i, r in enumerate(rows)]


def samples_from_vertices(vertices_by_lid: Dict[int, Any], max_points: int = 4096, device: str = "cuda"):
    """{obj_id: vertices [V, 3]} -> suppress_duplicates' samples: bank.sample_verify_points' stride sample of every object (rows 0, s,
    2 s, ... with s = ceil(V / max_points)), its sphere, and the obj_id -> object index map."""
    from . import bank
    if isinstance(max_points, bool) or not isinstance(max_points, int) or max_points < 1:
        raise ValueError(f"max_points must be an integer >= 1, got {max_points!r}")
    lids = sorted(vertices_by_lid)
    parts = [torch.as_tensor(np.asarray(vertices_by_lid[l]) if not isinstance(vertices_by_lid[l], torch.Tensor) else vertices_by_lid[l].cpu(),
                             dtype=torch.float32).reshape(-1, 3) for l in lids]
    offs = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in parts])]).tolist()
    pts, ranges = bank.sample_verify_points(torch.cat(parts, 0) if parts else torch.zeros(0, 3), list(zip(offs[:-1], offs[1:])), max_points)
    centers, radii = bank.sample_spheres(pts, ranges)
    return bank.VerifyPoints(pts.to(device).contiguous(), ranges, centers, radii), {l: o for o, l in enumerate(lids)}


def main(argv=None) -> None:
    from . import eval_bop19
    from .renderer import load_ply
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--result-csv", required=True, help="a BOP19 results csv")
    ap.add_argument("--models-dir", required=True, help="obj_XXXXXX.ply of every object the csv names")
    ap.add_argument("--output", required=True, help="the csv of the kept rows; <output>.nms.json gets every row's decision")
    ap.add_argument("--thresh", type=float, default=0.3)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--max-points", type=int, default=4096)
    ap.add_argument("--cross-object", action="store_true", help="compare poses of different objects too")
    args = ap.parse_args(argv)
    rows = eval_bop19.load_results_csv(args.result_csv)
    verts = {lid: load_ply(os.path.join(args.models_dir, f"obj_{lid:06d}.ply"), geometry_only=True).vertices for lid in sorted({r["obj_id"] for r in rows})}
    result = suppress_duplicates(rows, samples_from_vertices(verts, args.max_points), args.thresh, args.grid, args.cross_object)
    write_results_csv(args.output, [r for i, r in enumerate(rows) if result["keep"][i]])
    with open(args.output + ".nms.json", "w") as f:
        json.dump(decision_records(rows, result), f, indent=1)
    print(f"{int(result['keep'].sum())} of {len(rows)} rows kept -> {args.output}")


if __name__ == "__main__":
    main()
