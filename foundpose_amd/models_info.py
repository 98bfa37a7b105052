"""Writes `models_info.json` from the meshes of a models directory: per `obj_XXXXXX.ply` the bounding box and the diameter (the keys of
bop_toolkit's `calc_models_info`) and, on request, a list of POTENTIAL symmetries in the format `eval_util.get_symmetry_transformations`
reads.

    python -m foundpose_amd.models_info --models-dir DIR --output FILE [--object-ids 1 2] [--symmetries] [--sym-thresh MM] [--max-order 12]
                                        [--continuous-steps 36] [--no-prefilter] [--report FILE] [--force]

The diameter is the largest vertex-to-vertex distance (fp_pts_diameter).  The symmetry candidates follow the procedure of the BOP 2020
report: a rigid transformation S is a potential symmetry when the Hausdorff distance between the model's vertices and their image under S
is below eps = max(15 mm, 0.1 diameter); the candidates are rotations about a fixed list of axes through the surface centroid
(fp_directed_hausdorff evaluates them all by brute force, in fp64).  THE RESULT IS A LIST OF POTENTIAL SYMMETRIES THAT A PERSON MUST
REVIEW before it is used for scoring, as BOP's annotators confirmed theirs: the test sees vertices only (no texture, no surface between
them), only the listed axes and only rotations.

Both searches run on the device; there is no CPU path.  The decision logic below -- axis list, fraction set, per-axis decision,
combination and closure -- is pure host code that takes the Hausdorff evaluation as a callable `evaluate(transforms [K, 12], query_stride)
-> h [K]`, so it can be driven by the numpy restatement (tests/models_info_ref.py) as well."""

import argparse
import json
import math
import os
import re
from fractions import Fraction
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .eval_util import _rotation_matrix

Evaluate = Callable[[np.ndarray, int], np.ndarray]

AXIS_MERGE_DEG = 0.1          # an axis within this angle of an earlier one (either sign) is dropped
PRINCIPAL_GAP = 1e-6          # both eigenvalue gaps of the vertex covariance, as a fraction of the largest eigenvalue
SAME_ROTATION = 1e-9          # Frobenius distance below which two rotations are one
MAX_GROUP = 120               # closure is abandoned when more elements than this would be held
PREFILTER_QUERIES = 2048      # the first pass queries about this many vertices


# ---------------------------------------------------------------------------------------------------------------- geometry
def symmetry_centre(vertices: np.ndarray, faces: Optional[np.ndarray]) -> np.ndarray:
    """The area-weighted centroid of the triangles when the mesh has faces of non-zero total area (every symmetry of a surface fixes it,
    whatever the tessellation), else the vertex mean."""
    v = np.asarray(vertices, np.float64)
    if faces is not None and len(faces):
        a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
        area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
        total = float(area.sum())
        if np.isfinite(total) and total > 0.0:
            return ((a + b + c) / 3.0 * area[:, None]).sum(axis=0) / total
    return v.mean(axis=0)


_CUBE_AXES = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1],
                       [1, 1, 0], [1, -1, 0], [1, 0, 1], [1, 0, -1], [0, 1, 1], [0, 1, -1],
                       [1, 1, 1], [1, 1, -1], [1, -1, 1], [1, -1, -1]], np.float64)


def candidate_axes(vertices: np.ndarray) -> np.ndarray:
    """[A, 3] unit axes: the 13 axes of the cube group in the model frame (x, y, z, the six face diagonals, the four body diagonals), then
    the same 13 in the principal frame of the vertex covariance when both eigenvalue gaps exceed 1e-6 of the largest eigenvalue; an axis
    within 0.1 degree of an earlier one (either sign) is dropped."""
    v = np.asarray(vertices, np.float64)
    cube = _CUBE_AXES / np.linalg.norm(_CUBE_AXES, axis=1, keepdims=True)
    cand = list(cube)
    if len(v) >= 3:
        w, E = np.linalg.eigh(np.cov((v - v.mean(axis=0)).T, bias=True))
        if w[2] > 0 and min(w[1] - w[0], w[2] - w[1]) > PRINCIPAL_GAP * w[2]:
            cand += list(cube @ E.T)          # E's columns are the principal directions: axis = E a
    keep: List[np.ndarray] = []
    cos_merge = math.cos(math.radians(AXIS_MERGE_DEG))
    for a in cand:
        a = a / np.linalg.norm(a)
        if all(abs(float(a @ k)) < cos_merge for k in keep):
            keep.append(a)
    return np.array(keep, np.float64)


def angle_fractions(max_order: int, continuous_steps: int) -> List[Fraction]:
    """F = {k/n : 2 <= n <= max_order, 1 <= k < n} u {j/J : 1 <= j < J}, ascending; closed under f -> 1 - f."""
    f = {Fraction(k, n) for n in range(2, max_order + 1) for k in range(1, n)}
    f |= {Fraction(j, continuous_steps) for j in range(1, continuous_steps)}
    return sorted(f)


def rotation_about(fraction, axis: np.ndarray) -> np.ndarray:
    return _rotation_matrix(2.0 * math.pi * float(fraction), axis)


def transform12(R: np.ndarray, centre: np.ndarray) -> np.ndarray:
    """R about `centre` as the kernel's [12] = R row-major | t, t = c - R c."""
    return np.concatenate([R.ravel(), centre - R @ centre])


def transform4x4(R: np.ndarray, centre: np.ndarray) -> List[float]:
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, centre - R @ centre
    return [float(x) for x in m.ravel()]


# ---------------------------------------------------------------------------------------------------------------- evaluation
def symmetric_hausdorff(evaluate: Evaluate, fwd: np.ndarray, bwd: np.ndarray, eps: float, stride: int) -> Tuple[np.ndarray, np.ndarray]:
    """H_k = max(h(fwd_k), h(bwd_k)), bwd_k the inverse of fwd_k: the symmetric Hausdorff distance.  With stride > 1 a first pass queries
    every stride-th vertex only; a subset of the queries gives a lower bound of a directed distance, so a candidate whose bound is >= eps is
    rejected exactly and only the survivors run at stride 1.  -> (H [K], lower_bound [K] bool: the value is the first pass' bound)."""
    fwd, bwd = np.asarray(fwd, np.float64).reshape(-1, 12), np.asarray(bwd, np.float64).reshape(-1, 12)
    k = len(fwd)
    if k == 0:
        return np.zeros(0), np.zeros(0, bool)
    both = np.concatenate([fwd, bwd])
    if stride <= 1:
        h = np.asarray(evaluate(both, 1), np.float64)
        return np.maximum(h[:k], h[k:]), np.zeros(k, bool)
    h = np.asarray(evaluate(both, stride), np.float64)
    H = np.maximum(h[:k], h[k:])
    bound = ~(H < eps)
    live = np.nonzero(~bound)[0]
    if len(live):
        h = np.asarray(evaluate(np.concatenate([fwd[live], bwd[live]]), 1), np.float64)
        H[live] = np.maximum(h[:len(live)], h[len(live):])
    return H, bound


def axis_decision(H: Dict[Fraction, float], eps: float, max_order: int, continuous_steps: int) -> Tuple[bool, List[Fraction]]:
    """One axis, H[f] for every f of angle_fractions -> (continuous, fractions): continuous when H(j/J) < eps for every j, and then no
    discrete entries; else the union over the orders n with H(k/n) < eps for all k, ascending."""
    if all(H[Fraction(j, continuous_steps)] < eps for j in range(1, continuous_steps)):
        return True, []
    passed = set()
    for n in range(2, max_order + 1):
        if all(H[Fraction(k, n)] < eps for k in range(1, n)):
            passed |= {Fraction(k, n) for k in range(1, n)}
    return False, sorted(passed)


def _held(R: np.ndarray, held: Sequence[np.ndarray]) -> bool:
    return bool(len(held)) and bool(np.any(np.linalg.norm((np.asarray(held) - R).reshape(len(held), 9), axis=1) < SAME_ROTATION))


def combine_axes(axes: np.ndarray, decisions: Sequence[Tuple[bool, List[Fraction]]]) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """The per-axis decisions -> (discrete rotations, continuous axes).  Rotations within 1e-9 (Frobenius) of an earlier one or of the
    identity are dropped.  With a continuous axis a, a discrete R is dropped when R a = a or when Q^T R a = a for a kept Q: the toolkit
    composes every discrete entry with every continuous one, so these would be duplicates."""
    cont = [axes[i] for i, (c, _) in enumerate(decisions) if c]
    rots: List[np.ndarray] = []
    for i, (c, fracs) in enumerate(decisions):
        for f in fracs:
            R = rotation_about(f, axes[i])
            if not _held(R, [np.eye(3)] + rots):
                rots.append(R)
    if not cont:
        return rots, cont
    kept: List[np.ndarray] = []
    for R in rots:
        if not any(np.linalg.norm(M @ a - a) < SAME_ROTATION for a in cont for M in [R] + [Q.T @ R for Q in kept]):
            kept.append(R)
    return kept, cont


def close_group(rots: Sequence[np.ndarray], centre: np.ndarray, evaluate: Evaluate, eps: float, stride: int) -> Tuple[List[np.ndarray], Dict[str, Any]]:
    """Closes the set under composition: per round the products of held pairs that are not held yet are verified by the same evaluation (one
    call per round); products that fail are dropped and counted; it stops when a round adds nothing.  When more than 120 elements would be
    held, closure is abandoned and the axis-pass set is returned; the report says so."""
    held = [np.asarray(R, np.float64) for R in rots]
    failed: List[np.ndarray] = []
    report: Dict[str, Any] = {"rounds": [], "axis_pass": len(held), "failed_products": 0, "abandoned": False}
    while True:
        new: List[np.ndarray] = []
        for A in held:
            for B in held:
                P = A @ B
                if not _held(P, [np.eye(3)] + held + new + failed):
                    new.append(P)
            if len(held) + len(new) > 4 * MAX_GROUP:   # far more candidates than a point group has elements: stop collecting
                break
        if not new:
            break
        H, bound = symmetric_hausdorff(evaluate, np.array([transform12(P, centre) for P in new]), np.array([transform12(P.T, centre) for P in new]),
                                       eps, stride)
        ok = [P for P, h in zip(new, H) if h < eps]
        failed += [P for P, h in zip(new, H) if not h < eps]
        report["rounds"].append({"tested": len(new), "passed": len(ok), "failed": len(new) - len(ok),
                                 "values": [{"value": float(h), "lower_bound": bool(b)} for h, b in zip(H, bound)]})
        report["failed_products"] += len(new) - len(ok)
        if len(held) + len(ok) > MAX_GROUP:
            report["abandoned"] = True
            return [np.asarray(R, np.float64) for R in rots], report
        if not ok:
            break
        held += ok
    report["closed"] = len(held)
    return held, report


def object_symmetries(vertices: np.ndarray, faces: Optional[np.ndarray], diameter: float, evaluate: Evaluate, sym_thresh: Optional[float] = None,
                      max_order: int = 12, continuous_steps: int = 36, prefilter: bool = True) -> Tuple[List[List[float]], List[Dict[str, Any]], Dict[str, Any]]:
    """The potential symmetries of one object -> (symmetries_discrete, symmetries_continuous, report)."""
    check_options(sym_thresh, max_order, continuous_steps)
    v = np.asarray(vertices, np.float64)
    eps = float(sym_thresh) if sym_thresh is not None else max(15.0, 0.1 * float(diameter))
    stride = max(1, -(-len(v) // PREFILTER_QUERIES)) if prefilter else 1
    c = symmetry_centre(v, faces)
    axes = candidate_axes(v)
    fracs = angle_fractions(max_order, continuous_steps)
    # 1 - f is in the set with f, and the rotation by 1 - f is the inverse of the rotation by f
    fwd = np.array([transform12(rotation_about(f, a), c) for a in axes for f in fracs])
    bwd = np.array([transform12(rotation_about(1 - f, a), c) for a in axes for f in fracs])
    H, bound = symmetric_hausdorff(evaluate, fwd, bwd, eps, stride)
    H, bound = H.reshape(len(axes), len(fracs)), bound.reshape(len(axes), len(fracs))
    decisions = [axis_decision(dict(zip(fracs, H[i])), eps, max_order, continuous_steps) for i in range(len(axes))]
    rots, cont = combine_axes(axes, decisions)
    report: Dict[str, Any] = {
        "centre": c.tolist(), "eps": eps, "query_stride": stride,
        "axes": [{"axis": axes[i].tolist(), "continuous": decisions[i][0], "fractions": [str(f) for f in decisions[i][1]],
                  "candidates": [{"fraction": str(f), "value": float(H[i, j]), "lower_bound": bool(bound[i, j])} for j, f in enumerate(fracs)]}
                 for i in range(len(axes))],
        "axis_pass": len(rots)}
    if not cont:
        rots, report["closure"] = close_group(rots, c, evaluate, eps, stride)
    report["discrete"], report["continuous"] = len(rots), len(cont)
    return [transform4x4(R, c) for R in rots], [{"axis": a.tolist(), "offset": c.tolist()} for a in cont], report


def check_options(sym_thresh, max_order, continuous_steps) -> None:
    if sym_thresh is not None and not (isinstance(sym_thresh, (int, float)) and not isinstance(sym_thresh, bool) and math.isfinite(sym_thresh)
                                       and sym_thresh > 0):
        raise ValueError(f"sym_thresh must be a finite number > 0 (the model's unit), got {sym_thresh!r}")
    for name, val, lo in (("max_order", max_order, 2), ("continuous_steps", continuous_steps, 2)):
        if isinstance(val, bool) or not isinstance(val, int) or not lo <= val <= 360:
            raise ValueError(f"{name} must be an integer in [{lo}, 360], got {val!r}")


# ---------------------------------------------------------------------------------------------------------------- the tool
def _object_files(models_dir: str, object_ids: Optional[Sequence[int]]) -> List[Tuple[int, str]]:
    if not os.path.isdir(models_dir):
        raise FileNotFoundError(f"{models_dir}: no such models directory")
    found = {int(m.group(1)): os.path.join(models_dir, n) for n in sorted(os.listdir(models_dir)) for m in [re.fullmatch(r"obj_(\d{6})\.ply", n)] if m}
    if object_ids is None:
        if not found:
            raise FileNotFoundError(f"{models_dir}: no obj_XXXXXX.ply")
        return sorted(found.items())
    missing = [i for i in object_ids if int(i) not in found]
    if missing:
        raise FileNotFoundError(f"{models_dir}: no model file for object(s) {missing}")
    return [(int(i), found[int(i)]) for i in object_ids]


def device_evaluator(pts) -> Evaluate:
    """evaluate(transforms, stride) on the device, at most 65 535 transforms per launch."""
    import torch
    from . import ops

    def evaluate(transforms: np.ndarray, stride: int) -> np.ndarray:
        t = np.ascontiguousarray(transforms, np.float64).reshape(-1, 12)
        out = [ops.directed_hausdorff(pts, torch.from_numpy(t[k0:k0 + 65535]).to(pts.device), stride)[0].cpu().numpy()
               for k0 in range(0, len(t), 65535)]
        return np.concatenate(out) if out else np.zeros(0)
    return evaluate


def calc_models_info(models_dir: str, object_ids: Optional[Sequence[int]] = None, symmetries: bool = False, sym_thresh: Optional[float] = None,
                     max_order: int = 12, continuous_steps: int = 36, prefilter: bool = True, report: bool = False):
    """{obj_id: {"min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "diameter"[, "symmetries_discrete"][, "symmetries_continuous"]}}
    for the obj_XXXXXX.ply of `models_dir` (all, or `object_ids`); with report=True -> (that, {obj_id: report}).  `sym_thresh` is in the
    model's unit (default max(15, 0.1 diameter), BOP's rule for models in mm).  The symmetry lists are POTENTIAL symmetries: a person
    reviews them before they are used, as BOP's annotators did.  Runs on the device; raises without the library or the device."""
    import torch
    from . import _lib, ops
    from .renderer import load_ply
    check_options(sym_thresh, max_order, continuous_steps)
    meshes = []
    for oid, path in _object_files(models_dir, object_ids):   # every file is read and checked before any device work
        mesh = load_ply(path, geometry_only=True)
        v = mesh.vertices.astype(np.float64)
        if len(v) < 1:
            raise ValueError(f"{path}: no vertices")
        if not np.all(np.isfinite(v)):
            raise ValueError(f"{path}: non-finite vertices")
        meshes.append((oid, mesh, v))
    _lib.lib()
    if not torch.cuda.is_available():
        raise _lib.FoundPoseNativeError("models_info runs on the MI355X only: no device is available and no CPU path exists")
    info: Dict[int, Dict[str, Any]] = {}
    reports: Dict[int, Dict[str, Any]] = {}
    for oid, mesh, v in meshes:
        pts = torch.from_numpy(np.ascontiguousarray(v)).to("cuda")
        d, pair = ops.pts_diameter(pts)
        lo, hi = v.min(axis=0), v.max(axis=0)
        entry: Dict[str, Any] = {"min_x": float(lo[0]), "min_y": float(lo[1]), "min_z": float(lo[2]),
                                 "size_x": float(hi[0] - lo[0]), "size_y": float(hi[1] - lo[1]), "size_z": float(hi[2] - lo[2]),
                                 "diameter": float(d.cpu()[0])}
        reports[oid] = {"vertices": len(v), "diameter_pair": [int(x) for x in pair.cpu()]}
        if symmetries:
            disc, cont, rep = object_symmetries(v, mesh.faces, entry["diameter"], device_evaluator(pts), sym_thresh, max_order, continuous_steps, prefilter)
            if disc:
                entry["symmetries_discrete"] = disc
            if cont:
                entry["symmetries_continuous"] = cont
            reports[oid].update(rep)
        info[oid] = entry
    return (info, reports) if report else info


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m foundpose_amd.models_info", description=__doc__.split("\n\n")[0])
    ap.add_argument("--models-dir", required=True)
    ap.add_argument("--output", required=True, help="the models_info.json to write")
    ap.add_argument("--object-ids", type=int, nargs="+", default=None)
    ap.add_argument("--symmetries", action="store_true", help="also list potential symmetries (a person reviews them)")
    ap.add_argument("--sym-thresh", type=float, default=None, help="eps in the model's unit (default max(15, 0.1 diameter))")
    ap.add_argument("--max-order", type=int, default=12)
    ap.add_argument("--continuous-steps", type=int, default=36)
    ap.add_argument("--no-prefilter", action="store_true")
    ap.add_argument("--report", default=None, help="write every candidate's value to this JSON file")
    ap.add_argument("--force", action="store_true", help="overwrite an existing output")
    a = ap.parse_args(argv)
    for path in (a.output, a.report):
        if path and os.path.exists(path) and not a.force:
            raise FileExistsError(f"{path} exists; pass --force to overwrite it")
    info, reports = calc_models_info(a.models_dir, a.object_ids, a.symmetries, a.sym_thresh, a.max_order, a.continuous_steps, not a.no_prefilter, report=True)
    with open(a.output, "w") as f:
        json.dump({str(k): v for k, v in info.items()}, f, indent=2)
    if a.report:
        with open(a.report, "w") as f:
            json.dump({str(k): v for k, v in reports.items()}, f, indent=2)
    print(f"{a.output}: {len(info)} object(s)" + ("; the symmetry lists are POTENTIAL symmetries: review them before use" if a.symmetries else ""))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
