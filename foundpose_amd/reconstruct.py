"""Reconstructs an object mesh from posed RGB-D frames: TSDF fusion and marching tetrahedra on the MI355X.

    python -m foundpose_amd.reconstruct --sequence <scene dir> [--sequence <scene dir> ...] --obj-id N --output <models dir>
        [--opts opts.json] [--report report.json] [--overwrite]

Each sequence is a BOP scene directory (`rgb/`, `depth/`, `<mask_dir>/<im>_<gt index>.png`, `scene_gt.json`, `scene_camera.json` with
`depth_scale`): the reference sequences of BOP's model-free tasks, or an object on a turntable in front of a depth camera.  Every
frame that shows object N gives a depth image, a mask and a model -> camera pose; the frames of all sequences are fused in order into
one truncated signed distance volume (fp_tsdf_integrate), a surface is pulled out of it (fp_tsdf_count_triangles,
fp_tsdf_emit_triangles), welded, and written as the vertex-coloured `obj_%06d.ply` that gen_templates, gen_repre, models_info and
detect onboard start from.  There is no CPU path.

Limits: poses and masks are trusted as given; a voxel reads the nearest depth pixel, across depth edges too; surface that no frame
saw stays open (the report says so, nothing is filled); no accuracy on real BOP data is claimed."""

import argparse
import json
import math
import os
import time
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .gt_info import _read_json, refuse_existing

PAD_FRACTION = 0.05                # automatic bounds: 2 tau + this share of the extent on every side
PERCENTILES = (0.5, 99.5)          # ... around these percentiles of the masked depth points, per axis


class ReconstructOpts(NamedTuple):
    voxel_mm: float = 2.0
    trunc_voxels: float = 4.0      # tau = trunc_voxels * voxel_mm
    min_count: int = 2             # a cell takes part when all its corners were seen this often
    bounds: Optional[Tuple[Tuple[float, float, float], Tuple[float, float, float]]] = None   # ((x0, y0, z0), (x1, y1, z1)) mm; None: automatic
    mask_dir: str = "mask_visib"
    keep_largest: bool = True
    frame_batch: int = 32

    @property
    def trunc_mm(self) -> float:
        return float(self.trunc_voxels) * float(self.voxel_mm)


def load_opts(path_or_dict=None) -> ReconstructOpts:
    d = path_or_dict
    if d is None:
        return check_opts(ReconstructOpts())
    if isinstance(d, ReconstructOpts):
        return check_opts(d)
    if not isinstance(d, dict):
        with open(path_or_dict) as f:
            d = json.load(f)
    d = dict(d.get("reconstruct_opts", d))
    if d.get("bounds") is not None:
        d["bounds"] = tuple(tuple(float(v) for v in row) for row in d["bounds"])
    return check_opts(ReconstructOpts(**d))


def check_opts(o: ReconstructOpts) -> ReconstructOpts:
    if not (math.isfinite(o.voxel_mm) and o.voxel_mm > 0 and math.isfinite(o.trunc_voxels) and o.trunc_voxels > 0):
        raise ValueError(f"voxel_mm and trunc_voxels must be finite and > 0, got {o.voxel_mm!r}, {o.trunc_voxels!r}")
    if isinstance(o.min_count, bool) or int(o.min_count) != o.min_count or o.min_count < 1:
        raise ValueError(f"min_count must be an integer >= 1, got {o.min_count!r}")
    if isinstance(o.frame_batch, bool) or int(o.frame_batch) != o.frame_batch or o.frame_batch < 1:
        raise ValueError(f"frame_batch must be an integer >= 1, got {o.frame_batch!r}")
    if o.bounds is not None:
        b = np.asarray(o.bounds, np.float64)
        if b.shape != (2, 3) or not np.all(np.isfinite(b)) or not np.all(b[1] > b[0]):
            raise ValueError(f"bounds must be ((x0, y0, z0), (x1, y1, z1)) with every x1 > x0, got {o.bounds!r}")
    return o


class Frame(NamedTuple):
    depth: np.ndarray      # float32 [H, W] mm, 0 = no measurement
    mask: np.ndarray       # uint8 [H, W], != 0 on the object
    rgb: np.ndarray        # uint8 [H, W, 3]
    cam: Tuple[float, float, float, float]   # fx, fy, cx, cy
    pose: np.ndarray       # float64 [12]: model -> camera R row-major | t (mm)


# ---------------------------------------------------------------------------------------------------------- host logic
def grid_for(lo: np.ndarray, hi: np.ndarray, voxel_mm: float) -> Tuple[Tuple[float, float, float], Tuple[int, int, int]]:
    """The volume over the box [lo, hi]: origin lo, ceil(extent / voxel) voxels per axis, two at least."""
    dims = tuple(int(max(2, math.ceil((float(b) - float(a)) / voxel_mm - 1e-9))) for a, b in zip(lo, hi))
    return tuple(float(v) for v in lo), dims


def fits(dims: Sequence[int]) -> bool:
    from ._lib import TSDF_MAX_DIM, TSDF_MAX_VOXELS
    return max(dims) <= TSDF_MAX_DIM and int(np.prod(np.asarray(dims, np.int64))) <= TSDF_MAX_VOXELS


def padded_box(p_lo: np.ndarray, p_hi: np.ndarray, trunc_mm: float) -> Tuple[np.ndarray, np.ndarray]:
    pad = 2.0 * trunc_mm + PAD_FRACTION * (p_hi - p_lo)
    return p_lo - pad, p_hi + pad


def suggest_voxel(p_lo: np.ndarray, p_hi: np.ndarray, opts: ReconstructOpts) -> float:
    """The smallest voxel size, in steps of 5 %, at which the padded box of these percentiles fits the volume limits."""
    h = float(opts.voxel_mm)
    for _ in range(400):
        h *= 1.05
        lo, hi = padded_box(p_lo, p_hi, opts.trunc_voxels * h)
        if fits(grid_for(lo, hi, h)[1]):
            return h
    raise ValueError("no voxel size fits the volume limits: the masked depth points span too much space")


def largest_component(faces: np.ndarray, num_vertices: int) -> np.ndarray:
    """bool [F]: the faces of the largest edge-connected component (most faces; ties to the one with the lowest vertex)."""
    if len(faces) == 0:
        return np.zeros(0, bool)
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    g = coo_matrix((np.ones(len(e), np.int8), (e[:, 0], e[:, 1])), shape=(num_vertices, num_vertices))
    _, label = connected_components(g, directed=False)
    of_face = label[faces[:, 0]]                 # labels ascend with the lowest vertex of a component
    return of_face == np.argmax(np.bincount(of_face))


def mesh_topology(faces: np.ndarray) -> Dict[str, Any]:
    """Edge statistics of a triangle list: boundary edges lie on one face, a watertight mesh has none and no edge on more than two."""
    if len(faces) == 0:
        return {"boundary_edges": 0, "nonmanifold_edges": 0, "watertight": False}
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64), 1)
    _, cnt = np.unique(e[:, 0] * (int(faces.max()) + 1) + e[:, 1], return_counts=True)
    b, m = int(np.sum(cnt == 1)), int(np.sum(cnt > 2))
    return {"boundary_edges": b, "nonmanifold_edges": m, "watertight": b == 0 and m == 0}


def read_sequence(scene_dir: str, obj_id: int, mask_dir: str) -> List[Frame]:
    """The frames of a BOP scene directory that show object obj_id, in image order (an image with two instances gives two frames)."""
    from PIL import Image

    from .eval_bop19 import load_depth
    gts = {int(k): v for k, v in _read_json(os.path.join(scene_dir, "scene_gt.json")).items()}
    cams = {int(k): v for k, v in _read_json(os.path.join(scene_dir, "scene_camera.json")).items()}
    frames = []
    for im in sorted(gts):
        hits = [(g, e) for g, e in enumerate(gts[im]) if int(e["obj_id"]) == int(obj_id)]
        if not hits:
            continue
        if im not in cams or "depth_scale" not in cams[im]:
            raise ValueError(f"{scene_dir}: image {im} has no camera with a depth_scale in scene_camera.json")
        K = np.asarray(cams[im]["cam_K"], np.float64).reshape(3, 3)
        depth = load_depth(os.path.join(scene_dir, "depth", f"{im:06d}.png"), float(cams[im]["depth_scale"]))
        rgb_path = next((p for p in (os.path.join(scene_dir, "rgb", f"{im:06d}.{x}") for x in ("png", "jpg")) if os.path.exists(p)), None)
        if rgb_path is None:
            raise FileNotFoundError(f"{scene_dir}: no rgb/{im:06d}.png or .jpg")
        with Image.open(rgb_path) as pic:
            rgb = np.array(pic.convert("RGB"), np.uint8, order="C")
        for g, e in hits:
            with Image.open(os.path.join(scene_dir, mask_dir, f"{im:06d}_{g:06d}.png")) as pic:
                mask = np.array(pic.convert("L"), np.uint8, order="C")
            if not (depth.shape == mask.shape == rgb.shape[:2]):
                raise ValueError(f"{scene_dir}: image {im}: depth {depth.shape}, mask {mask.shape} and rgb {rgb.shape[:2]} differ in size")
            pose = np.concatenate([np.asarray(e["cam_R_m2c"], np.float64).reshape(9), np.asarray(e["cam_t_m2c"], np.float64).reshape(3)])
            frames.append(Frame(depth, mask, rgb, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), pose))
    return frames


# ---------------------------------------------------------------------------------------------------------- device work
def _batches(frames: Sequence[Frame], step: int):
    """Consecutive frames of one image size, `step` at most: the order of the frames is the order of the sums."""
    b0 = 0
    while b0 < len(frames):
        b1 = b0 + 1
        while b1 < len(frames) and b1 - b0 < step and frames[b1].depth.shape == frames[b0].depth.shape:
            b1 += 1
        yield frames[b0:b1]
        b0 = b1


def _upload(batch: Sequence[Frame], device):
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    return (up(np.stack([f.depth for f in batch]).astype(np.float32)), up(np.stack([f.mask for f in batch]).astype(np.uint8)),
            up(np.stack([f.rgb for f in batch]).astype(np.uint8)))


def masked_point_percentiles(frames: Sequence[Frame], opts: ReconstructOpts, device="cuda") -> Tuple[np.ndarray, np.ndarray]:
    """The masked depth pixels of all frames, lifted into the model frame with torch on the device (pixel centres at integers,
    X_m = R^T (X_c - t)) -> their 0.5 and 99.5 percentiles per axis (the nearest rank, by a sort)."""
    import torch
    pts = []
    for batch in _batches(frames, opts.frame_batch):
        depth, mask, _ = _upload(batch, device)
        H, W = depth.shape[1:]
        cam = torch.tensor([f.cam for f in batch], dtype=torch.float64, device=device)
        pose = torch.from_numpy(np.stack([f.pose for f in batch])).to(device)
        v, u = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=device), torch.arange(W, dtype=torch.float64, device=device), indexing="ij")
        d = depth.double()
        xc = torch.stack([(u[None] - cam[:, 2, None, None]) / cam[:, 0, None, None] * d, (v[None] - cam[:, 3, None, None]) / cam[:, 1, None, None] * d, d], -1)
        xm = torch.einsum("fji,fhwj->fhwi", pose[:, :9].reshape(-1, 3, 3), xc - pose[:, None, None, 9:])
        pts.append(xm[(mask != 0) & (depth > 0)])
    pts = torch.cat(pts) if pts else torch.zeros(0, 3, dtype=torch.float64, device=device)
    if len(pts) == 0:
        raise ValueError("no masked depth pixel in any frame: the bounds cannot be found (give opts.bounds)")
    s = torch.sort(pts, 0).values
    pick = lambda q: s[int(round(q / 100.0 * (len(s) - 1)))].cpu().numpy()   # noqa: E731
    return pick(PERCENTILES[0]), pick(PERCENTILES[1])


def choose_volume(frames: Sequence[Frame], opts: ReconstructOpts, device="cuda"):
    """-> (origin, dims) of the volume: opts.bounds as given, or the padded percentiles of the masked depth points.  A volume beyond
    the limits raises ValueError and names a voxel size that fits."""
    if opts.bounds is not None:
        lo, hi = (np.asarray(b, np.float64) for b in opts.bounds)
        p_lo = p_hi = None
    else:
        p_lo, p_hi = masked_point_percentiles(frames, opts, device)
        lo, hi = padded_box(p_lo, p_hi, opts.trunc_mm)
    origin, dims = grid_for(lo, hi, opts.voxel_mm)
    if not fits(dims):
        from ._lib import TSDF_MAX_DIM, TSDF_MAX_VOXELS
        hint = (f"voxel_mm >= {suggest_voxel(p_lo, p_hi, opts):.2f} fits" if p_lo is not None
                else f"voxel_mm >= {max(float(np.max(hi - lo)) / TSDF_MAX_DIM, (float(np.prod(hi - lo)) / TSDF_MAX_VOXELS) ** (1 / 3)) * 1.01:.2f} fits")
        raise ValueError(f"a volume of {dims[0]} x {dims[1]} x {dims[2]} voxels of {opts.voxel_mm} mm exceeds {TSDF_MAX_DIM} per axis or "
                         f"{TSDF_MAX_VOXELS} voxels: {hint}")
    return origin, dims


def fuse(frames: Sequence[Frame], opts=None, device="cuda") -> Dict[str, Any]:
    """Fuses the frames, in order, into a new TSDF volume -> the volume (ops.tsdf_new_volume's dict, on the device)."""
    from . import ops
    opts = load_opts(opts)
    if not frames:
        raise ValueError("no frame to fuse")
    origin, dims = choose_volume(frames, opts, device)
    vol = ops.tsdf_new_volume(origin, opts.voxel_mm, dims, device)
    for batch in _batches(frames, opts.frame_batch):
        depth, mask, rgb = _upload(batch, device)
        ops.tsdf_integrate(vol, depth, mask, rgb, np.array([f.cam for f in batch], np.float64), np.stack([f.pose for f in batch]), opts.trunc_mm)
    return vol


def extract_mesh(volume: Dict[str, Any], opts=None):
    """The surface of a fused volume -> renderer.Mesh.  Triangle corners are welded on the device by their edge keys (torch.unique: the
    sorted key order is the vertex order), triangles whose three welded positions are not pairwise distinct are dropped, with
    opts.keep_largest only the largest edge-connected component is kept, vertices no face uses are removed (order kept) and the
    normals are renderer.vertex_normals.  A volume without a surface raises ValueError."""
    import torch

    from . import ops
    from .renderer import Mesh, vertex_normals
    opts = load_opts(opts)
    _, keys, pos, col = ops.tsdf_extract(volume, opts.min_count)
    if len(keys) == 0:
        raise ValueError("the volume holds no surface: no cell with all corners seen min_count times has a sign change")
    uniq, inv = torch.unique(keys, sorted=True, return_inverse=True)
    verts = torch.empty(len(uniq), 3, dtype=torch.float32, device=pos.device)
    cols = torch.empty_like(verts)
    verts[inv], cols[inv] = pos, col             # every corner on one edge carries the same bits: any of them may land
    faces = inv.view(-1, 3)
    p = verts[faces]
    same = lambda a, b: (p[:, a] == p[:, b]).all(1)   # noqa: E731
    faces = faces[~(same(0, 1) | same(1, 2) | same(0, 2))].cpu().numpy()
    verts, cols = verts.cpu().numpy(), cols.clamp(0.0, 1.0).cpu().numpy()
    if opts.keep_largest:
        faces = faces[largest_component(faces, len(verts))]
    if len(faces) == 0:
        raise ValueError("every triangle of the surface is degenerate")
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    verts, cols, faces = verts[used], cols[used], remap[faces].astype(np.int32)
    return Mesh(vertices=verts, faces=faces, colors=cols.astype(np.float32), normals=vertex_normals(verts, faces))


def reconstruct(sequences: Sequence[str], obj_id: int, output_dir: str, opts=None, report_path: Optional[str] = None, overwrite: bool = False,
                device: str = "cuda") -> Dict[str, Any]:
    """Reads the sequences, fuses, extracts and writes <output_dir>/obj_%06d.ply (and the report) -> the report."""
    import torch

    from . import _lib
    from .renderer import save_ply
    t0 = time.perf_counter()
    opts = load_opts(opts)
    out_path = os.path.join(output_dir, f"obj_{int(obj_id):06d}.ply")
    refuse_existing([out_path] + ([report_path] if report_path else []), overwrite)
    frames: List[Frame] = []
    for sd in sequences:
        got = read_sequence(sd, obj_id, opts.mask_dir)
        if not got:
            raise ValueError(f"{sd}: no frame shows object {obj_id}")
        frames += got
    t_read = time.perf_counter()
    _lib.lib()
    if not torch.cuda.is_available():
        raise _lib.FoundPoseNativeError("reconstruct runs on the MI355X only: no device is available and no CPU path exists")
    vol = fuse(frames, opts, device)
    observed = int((vol["sdf_cnt"] >= opts.min_count).sum())
    torch.cuda.synchronize()
    t_fuse = time.perf_counter()
    mesh = extract_mesh(vol, opts)
    t_mesh = time.perf_counter()
    os.makedirs(output_dir, exist_ok=True)
    save_ply(out_path, mesh)
    topo = mesh_topology(mesh.faces)
    lo = np.asarray(vol["origin"])
    report = {"obj_id": int(obj_id), "output": out_path, "sequences": [os.path.abspath(s) for s in sequences], "frames_used": len(frames),
              "opts": opts._asdict(), "bounds": [lo.tolist(), (lo + np.asarray(vol["dims"]) * vol["voxel_mm"]).tolist()],
              "dims": list(vol["dims"]), "observed_voxels": observed, "vertices": int(len(mesh.vertices)), "triangles": int(len(mesh.faces)),
              **topo,
              "note": None if topo["watertight"] else "the surface is open where no frame saw it; nothing is filled",
              "seconds": {"read": t_read - t0, "fuse": t_fuse - t_read, "extract": t_mesh - t_fuse, "total": time.perf_counter() - t0}}
    if report_path:
        with open(report_path, "w") as f:
            json.dump(report, f, indent=1)
    return report


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m foundpose_amd.reconstruct", description=__doc__.split("\n\n")[0])
    ap.add_argument("--sequence", action="append", required=True, help="a BOP scene directory; repeat to fuse several, in order")
    ap.add_argument("--obj-id", type=int, required=True)
    ap.add_argument("--output", required=True, help="the models directory obj_%%06d.ply is written into")
    ap.add_argument("--opts", default=None, help="JSON with ReconstructOpts fields")
    ap.add_argument("--report", default=None, help="write the report to this JSON file")
    ap.add_argument("--overwrite", action="store_true", help="replace an existing output")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    r = reconstruct(a.sequence, a.obj_id, a.output, a.opts, a.report, a.overwrite, a.device)
    print(f"{r['output']}: {r['vertices']} vertices, {r['triangles']} triangles from {r['frames_used']} frame(s) in a volume of "
          f"{r['dims'][0]} x {r['dims'][1]} x {r['dims'][2]} voxels; {r['boundary_edges']} boundary edge(s), "
          f"{'watertight' if r['watertight'] else 'open: ' + str(r['note'])}; {r['seconds']['total']:.2f} s")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
