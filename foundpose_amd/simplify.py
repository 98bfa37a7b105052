"""Simplifies object meshes on the MI355X by vertex clustering with quadric error positions, and writes a BOP `models_eval` directory.

    python -m foundpose_amd.simplify --models-dir <models> --output-dir <models_eval> (--target-vertices N | --cell-mm c)
        [--object-ids 1 5 ...] [--keep-largest] [--report r.json] [--overwrite]

In the manner of Lindstrom's out-of-core simplification: the vertices are binned into a uniform grid anchored on
the mesh (fp_mesh_cell_keys), every occupied cell becomes one vertex, placed where the summed plane quadrics of the triangles touching the
cell are smallest (fp_mesh_cluster, one wave per cell), and the triangles are re-indexed; those that collapse, and all but the first of
those that land on one vertex set, are dropped.  torch sorts and scans between the kernels, as in reconstruct.extract_mesh.  Every sum has
a fixed order: the output is bit-identical from run to run, and tests/simplify_ref.py restates it in numpy.

What it does not promise: vertex clustering does not keep a mesh manifold (the report counts boundary and non-manifold edges of the
output), nothing is filled, and nothing is guaranteed about self-intersection.  Edge-collapse decimation gives better meshes per vertex;
it is sequential at heart and not what this module does.

models_info.json: the source directory's entries are copied verbatim when it has the file (diameter and reviewed symmetries belong to the
object, not to one mesh of it); otherwise models_info.calc_models_info writes it from the output.  Runs on the device only: without the
library or a device it raises FoundPoseNativeError.
"""

import argparse
import json
import math
import os
import time
from dataclasses import dataclass
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np

from .gt_info import refuse_existing

MAX_DIM = 1 << 20           # FP_MESH_MAX_DIM
MIN_TARGET = 8              # at the bounding-box diagonal at most 2 x 2 x 2 cells are occupied
BISECTION_ROUNDS = 32
LIMITS = ("vertex clustering does not promise a manifold result: boundary_edges and nonmanifold_edges count what the output has; "
          "nothing is filled, and nothing is guaranteed about self-intersection")


@dataclass(frozen=True)
class SimplifyOpts:
    cell_mm: Optional[float] = None          # the cell size; exactly one of cell_mm and target_vertices is given
    target_vertices: Optional[int] = None    # or: the largest number of output vertices, the cell size found by bisection
    eig_eps: float = 1e-3                    # an eigenvalue is kept when it exceeds eig_eps times the largest (Lindstrom's value)
    keep_largest: bool = False               # keep only the largest edge-connected component of the output


def check_options(opts: SimplifyOpts) -> SimplifyOpts:
    if not isinstance(opts, SimplifyOpts):
        raise ValueError(f"opts must be SimplifyOpts, got {type(opts).__name__}")
    if (opts.cell_mm is None) == (opts.target_vertices is None):
        raise ValueError("exactly one of cell_mm and target_vertices must be given")
    if opts.cell_mm is not None and not (isinstance(opts.cell_mm, (int, float)) and not isinstance(opts.cell_mm, bool)
                                         and math.isfinite(opts.cell_mm) and opts.cell_mm > 0):
        raise ValueError(f"cell_mm must be a finite number > 0, got {opts.cell_mm!r}")
    if opts.target_vertices is not None and (isinstance(opts.target_vertices, bool) or not isinstance(opts.target_vertices, int)
                                             or opts.target_vertices < MIN_TARGET):
        raise ValueError(f"target_vertices must be an integer >= {MIN_TARGET}, got {opts.target_vertices!r}")
    if isinstance(opts.eig_eps, bool) or not isinstance(opts.eig_eps, (int, float)) or not math.isfinite(opts.eig_eps) or not 0 <= opts.eig_eps < 1:
        raise ValueError(f"eig_eps must be a number in [0, 1), got {opts.eig_eps!r}")
    if not isinstance(opts.keep_largest, bool):
        raise ValueError(f"keep_largest must be a bool, got {opts.keep_largest!r}")
    return opts


def check_mesh(mesh, where: str = "mesh") -> None:
    """What is checked before any device work: ValueError."""
    v, f = np.asarray(mesh.vertices), np.asarray(mesh.faces)
    if v.ndim != 2 or v.shape[1] != 3 or len(v) < 1:
        raise ValueError(f"{where}: vertices must be [V, 3] with V >= 1, got {v.shape}")
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{where}: non-finite vertices")
    if f.size and (f.ndim != 2 or f.shape[1] != 3):
        raise ValueError(f"{where}: faces must be [F, 3], got {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError(f"{where}: face index outside the vertex range")
    if np.asarray(mesh.colors).shape != v.shape:
        raise ValueError(f"{where}: colors must be {v.shape}, got {np.asarray(mesh.colors).shape}")


def grid_for(vmin: np.ndarray, vmax: np.ndarray, c: float) -> Optional[Tuple[np.ndarray, Tuple[int, int, int]]]:
    """The grid of cell size c anchored on a mesh with these fp64 extremes: origin = min - c / 2 and n = floor((max - origin) / c) + 1 per
    axis, the kernel's operations, so the kernel's clamp never acts.  None when a dimension would exceed 2^20."""
    c = float(c)
    o = vmin - c / 2
    g = (vmax - o) / c
    if not np.all(np.isfinite(g)) or np.any(g >= MAX_DIM):
        return None
    return o, tuple(int(math.floor(x)) + 1 for x in g)


def bbox_diagonal(vmin: np.ndarray, vmax: np.ndarray) -> float:
    d = [float(t) for t in vmax - vmin]
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def choose_cell_mm(vmin: np.ndarray, vmax: np.ndarray, target: int, count_cells) -> float:
    """The cell size for at most `target` occupied cells.  lo = 0, hi = the bounding-box diagonal (at most 8 cells); 32 times: mid =
    (lo + hi) / 2, and a grid beyond the limits or more than `target` cells (count_cells(mid) -> None or the count) sets lo = mid,
    otherwise hi = mid.  -> hi.  Deterministic, and it does not assume that the count is monotone in the cell size."""
    lo, hi = 0.0, bbox_diagonal(vmin, vmax)
    for _ in range(BISECTION_ROUNDS):
        mid = (lo + hi) / 2
        n = count_cells(mid) if mid > 0 else None
        if n is None or n > target:
            lo = mid
        else:
            hi = mid
    if not hi > 0:
        raise ValueError("the mesh has no extent: every vertex is the same point")
    return hi


def cell_counter(verts, vmin: np.ndarray, vmax: np.ndarray):
    """count_cells for choose_cell_mm on the device: keys and torch.unique only."""
    import torch

    from . import ops

    def count_cells(c: float) -> Optional[int]:
        grid = grid_for(vmin, vmax, c)
        if grid is None:
            return None
        return int(torch.unique(ops.mesh_cell_keys(verts, grid[0], c, grid[1])).numel())
    return count_cells


def output_faces(rank, faces):
    """The face rules on the device: rank int64 [V], faces int32 [F, 3] -> int64 [F', 3] over the cells.  A face with two equal cells is
    dropped; among faces with the same vertex set the one with the lowest input index stays, whatever its orientation (a thin plate
    collapses to one sheet); the order is the input's."""
    import torch
    r = rank[faces.long()]
    r = r[(r[:, 0] != r[:, 1]) & (r[:, 1] != r[:, 2]) & (r[:, 0] != r[:, 2])]
    if len(r) == 0:
        return r
    _, inv = torch.unique(torch.sort(r, 1)[0], dim=0, return_inverse=True)
    idx = torch.arange(len(r), device=r.device)
    first = torch.full((int(inv.max()) + 1,), len(r), dtype=torch.int64, device=r.device).scatter_reduce_(0, inv, idx, "amin")
    return r[first[inv] == idx]


def simplify_mesh(mesh, opts: SimplifyOpts, device: str = "cuda"):
    """renderer.Mesh -> (renderer.Mesh, report).  Everything is checked before any device work; a mesh that already has at most
    opts.target_vertices vertices is returned as it is (report["unchanged"])."""
    import torch

    from . import _lib, ops
    from .reconstruct import largest_component, mesh_topology
    from .renderer import Mesh, vertex_normals
    t0 = time.perf_counter()
    opts = check_options(opts)
    check_mesh(mesh)
    v32 = np.ascontiguousarray(mesh.vertices, np.float32)
    faces_in = np.ascontiguousarray(np.asarray(mesh.faces).reshape(-1, 3), np.int32)
    report: Dict[str, Any] = {"vertices_in": len(v32), "triangles_in": len(faces_in), "limits": LIMITS}
    if opts.target_vertices is not None and len(v32) <= opts.target_vertices:
        report.update(unchanged=True, vertices_out=len(v32), triangles_out=len(faces_in), topology=mesh_topology(faces_in),
                      seconds=time.perf_counter() - t0)
        return mesh, report
    if not np.all(np.isfinite(v32)):
        raise ValueError("mesh: a vertex is not finite in float32")
    _lib.lib()
    if not torch.cuda.is_available():
        raise _lib.FoundPoseNativeError("simplify runs on the MI355X only: no device is available and no CPU path exists")
    v64 = v32.astype(np.float64)
    vmin, vmax = v64.min(0), v64.max(0)
    verts = torch.from_numpy(v32).to(device)
    c = float(opts.cell_mm) if opts.cell_mm is not None else choose_cell_mm(vmin, vmax, opts.target_vertices, cell_counter(verts, vmin, vmax))
    grid = grid_for(vmin, vmax, c)
    if grid is None:
        raise ValueError(f"a grid of {c} mm cells over this mesh has a dimension beyond {MAX_DIM}")
    origin, dims = grid
    cols = torch.from_numpy(np.ascontiguousarray(mesh.colors, np.float32)).to(device)
    faces = torch.from_numpy(faces_in).to(device)
    tables = ops.mesh_cluster_tables(ops.mesh_cell_keys(verts, origin, c, dims), faces)
    out = ops.mesh_cluster(verts, cols, faces, tables, origin, c, dims, opts.eig_eps)
    num_cells = len(tables["cells"])
    if len(faces_in):
        f_out = output_faces(tables["rank"], faces).cpu().numpy()
        if opts.keep_largest:
            f_out = f_out[largest_component(f_out, num_cells)]
        if len(f_out) == 0:
            raise ValueError(f"every triangle collapses at a cell size of {c} mm")
        used = np.zeros(num_cells, bool)
        used[f_out.reshape(-1)] = True
        f_out = (np.cumsum(used) - 1)[f_out].astype(np.int32)
    else:
        f_out, used = np.zeros((0, 3), np.int32), np.ones(num_cells, bool)
    pos, col = out["positions"].cpu().numpy()[used], out["colors"].cpu().numpy()[used]
    status, err = out["status"].cpu().numpy()[used], out["err"].cpu().numpy()[used]
    weight = out["quadrics"].cpu().numpy()[used][:, [0, 3, 5]].sum(1)      # trace A = the summed face weights (|n| = 1)
    ok = weight > 0
    result = Mesh(vertices=pos, faces=f_out, colors=col, normals=vertex_normals(pos, f_out))
    report.update(unchanged=False, cell_mm=c, grid_origin=[float(t) for t in origin], grid_dims=list(dims), cells=num_cells,
                  vertices_out=len(pos), triangles_out=len(f_out),
                  status_counts={str(int(s)): int(n) for s, n in zip(*np.unique(status, return_counts=True))},
                  rms_quadric_error_mm=float(np.sqrt(np.mean(np.maximum(err[ok], 0.0) / weight[ok]))) if ok.any() else None,
                  topology=mesh_topology(f_out), seconds=time.perf_counter() - t0)
    return result, report


def simplify_models(models_dir: str, output_dir: str, opts: SimplifyOpts, object_ids: Optional[Sequence[int]] = None,
                    report_path: Optional[str] = None, overwrite: bool = False, device: str = "cuda") -> Dict[int, Dict[str, Any]]:
    """Every obj_XXXXXX.ply of models_dir (or object_ids) -> output_dir, with models_info.json -> {obj_id: report}."""
    import torch

    from . import _lib
    from .models_info import _object_files, calc_models_info
    from .renderer import load_ply, save_ply
    opts = check_options(opts)
    files = _object_files(models_dir, object_ids)
    if os.path.abspath(models_dir) == os.path.abspath(output_dir):
        raise ValueError("output_dir is models_dir: the source meshes would be overwritten")
    info_out = os.path.join(output_dir, "models_info.json")
    refuse_existing([os.path.join(output_dir, os.path.basename(p)) for _, p in files] + [info_out] + ([report_path] if report_path else []), overwrite)
    meshes = []
    for oid, path in files:                      # every file is read and checked before any device work
        textured = False
        try:
            mesh = load_ply(path)
        except NotImplementedError:
            mesh, textured = load_ply(path, geometry_only=True), True
        check_mesh(mesh, path)
        meshes.append((oid, path, mesh, textured))
    info_in = os.path.join(models_dir, "models_info.json")
    source_info = None
    if os.path.exists(info_in):
        with open(info_in) as f:
            source_info = json.load(f)
        missing = [oid for oid, *_ in meshes if str(oid) not in source_info]
        if missing:
            raise ValueError(f"{info_in}: no entry for object(s) {missing}")
    _lib.lib()
    if not torch.cuda.is_available():
        raise _lib.FoundPoseNativeError("simplify runs on the MI355X only: no device is available and no CPU path exists")
    results = [(oid, path, textured) + simplify_mesh(mesh, opts, device) for oid, path, mesh, textured in meshes]
    os.makedirs(output_dir, exist_ok=True)
    reports: Dict[int, Dict[str, Any]] = {}
    for oid, path, textured, mesh, rep in results:
        save_ply(os.path.join(output_dir, os.path.basename(path)), mesh)
        if textured:
            rep["colors"] = "the source is textured: its texture is not read, and the colours are the fallback grey"
        reports[oid] = rep
    if source_info is not None:
        info = {str(oid): source_info[str(oid)] for oid, *_ in meshes}
    else:
        info = {str(k): e for k, e in calc_models_info(output_dir, [oid for oid, *_ in meshes]).items()}
    with open(info_out, "w") as f:
        json.dump(info, f, indent=2)
    if report_path:
        with open(report_path, "w") as f:
            json.dump({str(k): r for k, r in reports.items()}, f, indent=2)
    return reports


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m foundpose_amd.simplify", description=__doc__.split("\n\n")[0])
    ap.add_argument("--models-dir", required=True)
    ap.add_argument("--output-dir", required=True, help="the models_eval directory to write")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--target-vertices", type=int, default=None, help="at most this many vertices per model (>= 8)")
    how.add_argument("--cell-mm", type=float, default=None, help="the cell size of the clustering grid")
    ap.add_argument("--object-ids", type=int, nargs="+", default=None)
    ap.add_argument("--keep-largest", action="store_true", help="keep only the largest connected component of each output")
    ap.add_argument("--report", default=None, help="write the per-object reports to this JSON file")
    ap.add_argument("--overwrite", action="store_true")
    a = ap.parse_args(argv)
    opts = SimplifyOpts(cell_mm=a.cell_mm, target_vertices=a.target_vertices, keep_largest=a.keep_largest)
    reports = simplify_models(a.models_dir, a.output_dir, opts, a.object_ids, a.report, a.overwrite)
    for oid, r in reports.items():
        if r["unchanged"]:
            print(f"obj_{oid:06d}: {r['vertices_in']} vertices, within the target: unchanged")
        else:
            t = r["topology"]
            print(f"obj_{oid:06d}: {r['vertices_in']} -> {r['vertices_out']} vertices, {r['triangles_in']} -> {r['triangles_out']} triangles, "
                  f"cells of {r['cell_mm']:.4g} mm; {t['boundary_edges']} boundary and {t['nonmanifold_edges']} non-manifold edges")
    print(f"{a.output_dir}: {len(reports)} object(s); {LIMITS}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
