"""Reconstructs an object mesh from posed RGB-D frames: TSDF fusion and marching tetrahedra on the MI355X.

    python -m foundpose_amd.reconstruct --sequence <scene dir> [--sequence <scene dir> ...] --obj-id N --output <models dir>
        [--opts opts.json] [--report report.json] [--overwrite] [--tracked-poses <dir>]

Each sequence is a BOP scene directory (`rgb/`, `depth/`, `<mask_dir>/<im>_<gt index>.png`, `scene_gt.json`, `scene_camera.json` with
`depth_scale`): the reference sequences of BOP's model-free tasks, or an object on a turntable in front of a depth camera.  Every
frame that shows object N gives a depth image, a mask and a model -> camera pose; the frames of all sequences are fused in order into
one truncated signed distance volume (fp_tsdf_integrate), a surface is pulled out of it (fp_tsdf_count_triangles,
fp_tsdf_emit_triangles), welded, and written as the vertex-coloured `obj_%06d.ply` that gen_templates, gen_repre, models_info and
detect onboard start from.  There is no CPU path.

With opts `pose_source: "track"` one known pose per sequence is enough: the frames are the images of
scene_camera.json, only the first image's scene_gt.json pose is used (and every Nth with `track_anchor_every`), every other frame is
tracked against the volume fused so far (fp_tsdf_track) and fused at its tracked pose; `bounds` must then be given, and
--tracked-poses writes the poses per sequence in scene_gt.json's format.  With `track_color_weight` > 0 a frame
is tracked on shape and on the colour the volume holds (fp_tsdf_track_rgb): for objects whose shape leaves a rotation open.

With opts `fill: "carve"` the fused volume is closed before extraction (fill_volume): whatever no frame saw
empty counts as inside, `fill_plane` declares the half-space of the table empty, the volume's outermost voxel layer is outside, and
`fill_smooth_iters` iterations of a volumetric diffusion (fp_tsdf_diffuse) take the voxel staircase off the invented surface while
`fill_color_iters` iterations carry colour onto it; every vertex between two observed voxels keeps its bits.

Limits: with pose_source "given" poses and masks are trusted as given; a voxel reads the nearest depth pixel, across depth edges too; with
fill "none", the default, surface that no frame saw stays open (the report says so, nothing is filled); fill "carve" closes it with the
visual hull of what the frames carved, so an overhang no frame looked under is filled solid, and a background without valid depth carves
nothing; no accuracy on real BOP data is claimed."""

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
FILL_MAX_ITERS = 4096              # FP_TSDF_DIFFUSE_MAX_ITERS
FILL_SNAP = 2.0 ** -10             # a filled value closer to zero than this becomes this: an exact 0 is outside, and a vertex on a corner collapses its triangle


class ReconstructOpts(NamedTuple):
    voxel_mm: float = 2.0
    trunc_voxels: float = 4.0      # tau = trunc_voxels * voxel_mm
    min_count: int = 2             # a cell takes part when all its corners were seen this often
    bounds: Optional[Tuple[Tuple[float, float, float], Tuple[float, float, float]]] = None   # ((x0, y0, z0), (x1, y1, z1)) mm; None: automatic
    mask_dir: str = "mask_visib"
    keep_largest: bool = True
    frame_batch: int = 32
    pose_source: str = "given"     # "given": every frame's pose comes from scene_gt.json; "track": frames are tracked against the volume (section 30)
    track_anchor_every: int = 0    # 0: only the first frame of a sequence takes its pose from scene_gt.json; N > 0: every Nth frame does too
    track_iters: int = 20          # Levenberg-Marquardt iterations per tracked frame
    track_max_dist_voxels: float = 3.0   # the inlier distance, in voxels (<= trunc_voxels)
    track_min_count: int = 1       # a cell takes part in tracking when all its corners were seen this often
    track_max_points: int = 16384  # cap on the points of a frame
    track_motion: str = "velocity"   # "velocity" or "hold": how a frame's start pose is predicted
    track_min_inlier_share: float = 0.5   # a tracked frame below this share of inliers is lost
    track_max_lost: int = 3        # consecutive lost frames allowed
    fill: str = "none"             # "none": surface no frame saw stays open; "carve": the volume is closed before extraction (section 34); the
                                   # fill fields stand before the two colour fields, which tests/test_tsdf_track_rgb_cpu.py pins as the last
    fill_smooth_iters: int = 4     # diffusion iterations over the distances the fill invents; more iterations erode the filled part
    fill_color_iters: int = 64     # diffusion iterations that carry colour onto voxels without one
    fill_plane: Optional[Tuple[float, float, float, float]] = None   # (a, b, c, d), model frame, mm: a x + b y + c z + d > 0 is known to be empty
    track_color_weight: float = 0.0   # mm per unit of colour; 0: frames are tracked on shape alone, > 0: on shape and colour (section 31)
    track_color_max: float = 0.25  # a colour channel further than this from the volume's colour is an outlier

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
    if isinstance(d.get("fill_plane"), list):
        d["fill_plane"] = tuple(d["fill_plane"])
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
    if o.pose_source not in ("given", "track"):
        raise ValueError(f"pose_source must be 'given' or 'track', got {o.pose_source!r}")
    if o.track_motion not in ("velocity", "hold"):
        raise ValueError(f"track_motion must be 'velocity' or 'hold', got {o.track_motion!r}")
    for name, low, high in (("track_anchor_every", 0, None), ("track_iters", 0, 1000), ("track_min_count", 1, None), ("track_max_points", 1, None),
                            ("track_max_lost", 0, None)):
        v = getattr(o, name)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or v < low or (high is not None and v > high):
            raise ValueError(f"{name} must be an integer >= {low}" + (f" and <= {high}" if high is not None else "") + f", got {v!r}")
    v = o.track_max_dist_voxels
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v > 0):
        raise ValueError(f"track_max_dist_voxels must be finite and > 0, got {v!r}")
    if v > o.trunc_voxels:
        raise ValueError(f"track_max_dist_voxels {v!r} exceeds trunc_voxels {o.trunc_voxels!r}: beyond the truncation distance the volume holds no distance")
    v = o.track_min_inlier_share
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1:
        raise ValueError(f"track_min_inlier_share must lie in [0, 1], got {v!r}")
    v = o.track_color_weight
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v >= 0):
        raise ValueError(f"track_color_weight must be finite and >= 0 (0: shape alone), got {v!r}")
    v = o.track_color_max
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v > 0):
        raise ValueError(f"track_color_max must be finite and > 0, got {v!r}")
    if o.fill not in ("none", "carve"):
        raise ValueError(f"fill must be 'none' or 'carve', got {o.fill!r}")
    for name in ("fill_smooth_iters", "fill_color_iters"):
        v = getattr(o, name)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or v < 0 or v > FILL_MAX_ITERS:
            raise ValueError(f"{name} must be an integer >= 0 and <= {FILL_MAX_ITERS}, got {v!r}")
    if o.fill_plane is not None:
        v = o.fill_plane
        if (not isinstance(v, (tuple, list)) or len(v) != 4 or any(isinstance(c, bool) or not isinstance(c, (int, float)) or not math.isfinite(c) for c in v)
                or not any(c != 0 for c in v[:3])):
            raise ValueError(f"fill_plane must be null or four finite numbers (a, b, c, d) with (a, b, c) != 0, got {v!r}")
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


def read_sequence_tracked(scene_dir: str, obj_id: int, mask_dir: str) -> Tuple[List[Frame], List[Optional[np.ndarray]], List[int]]:
    """Track mode's reader: every image of scene_camera.json, in order -> (frames, given, image ids).  given[k] is the pose of the
    image's first scene_gt.json entry that shows obj_id, or None (Frame.pose is then NaN); the mask is <im>_<gt index>.png when that
    entry exists, else <im>_000000.png.  read_sequence is left as it is."""
    from PIL import Image

    from .eval_bop19 import load_depth
    gt_path = os.path.join(scene_dir, "scene_gt.json")
    gts = {int(k): v for k, v in _read_json(gt_path).items()} if os.path.exists(gt_path) else {}
    cams = {int(k): v for k, v in _read_json(os.path.join(scene_dir, "scene_camera.json")).items()}
    frames, given, ims = [], [], []
    for im in sorted(cams):
        if "depth_scale" not in cams[im]:
            raise ValueError(f"{scene_dir}: image {im} has no depth_scale in scene_camera.json")
        hit = next(((g, e) for g, e in enumerate(gts.get(im, [])) if int(e["obj_id"]) == int(obj_id)), None)
        K = np.asarray(cams[im]["cam_K"], np.float64).reshape(3, 3)
        depth = load_depth(os.path.join(scene_dir, "depth", f"{im:06d}.png"), float(cams[im]["depth_scale"]))
        rgb_path = next((p for p in (os.path.join(scene_dir, "rgb", f"{im:06d}.{x}") for x in ("png", "jpg")) if os.path.exists(p)), None)
        if rgb_path is None:
            raise FileNotFoundError(f"{scene_dir}: no rgb/{im:06d}.png or .jpg")
        with Image.open(rgb_path) as pic:
            rgb = np.array(pic.convert("RGB"), np.uint8, order="C")
        with Image.open(os.path.join(scene_dir, mask_dir, f"{im:06d}_{hit[0] if hit else 0:06d}.png")) as pic:
            mask = np.array(pic.convert("L"), np.uint8, order="C")
        if not (depth.shape == mask.shape == rgb.shape[:2]):
            raise ValueError(f"{scene_dir}: image {im}: depth {depth.shape}, mask {mask.shape} and rgb {rgb.shape[:2]} differ in size")
        pose = None if hit is None else np.concatenate([np.asarray(hit[1]["cam_R_m2c"], np.float64).reshape(9),
                                                        np.asarray(hit[1]["cam_t_m2c"], np.float64).reshape(3)])
        frames.append(Frame(depth, mask, rgb, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), np.full(12, np.nan) if pose is None else pose))
        given.append(pose)
        ims.append(im)
    return frames, given, ims


def predict_pose(history: Sequence[Tuple[int, np.ndarray]], index: int, motion: str) -> np.ndarray:
    """The start pose (4 x 4, fp64, on the host) of frame `index` of a sequence from `history` = [(frame index, T)] of its kept frames:
    "hold" is the last kept pose; "velocity" is T1 T2^-1 T1 of the two frames before it when both were kept, R re-orthonormalised by
    SVD, and "hold" otherwise (before two poses exist, and after a lost frame)."""
    T1 = history[-1][1]
    if motion == "velocity" and len(history) >= 2 and history[-1][0] == index - 1 and history[-2][0] == index - 2:
        T = T1 @ np.linalg.inv(history[-2][1]) @ T1
        U, _, Vt = np.linalg.svd(T[:3, :3])
        T[:3, :3] = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
        T[3] = (0.0, 0.0, 0.0, 1.0)
        return T
    return T1.copy()


def anchor_box_hint(frames: Sequence[Frame], given: Sequence[Optional[np.ndarray]]) -> str:
    """The box of the masked depth points of the frames with a pose, in the model frame (numpy, on the host: a hint for opts.bounds)."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for f, p in zip(frames, given):
        if p is None:
            continue
        v, u = np.nonzero((f.mask != 0) & (f.depth > 0))
        if not len(u):
            continue
        d = f.depth[v, u].astype(np.float64)
        xc = np.stack([(u - f.cam[2]) / f.cam[0] * d, (v - f.cam[3]) / f.cam[1] * d, d], 1)
        xm = (xc - p[9:]) @ p[:9].reshape(3, 3)
        lo, hi = np.minimum(lo, xm.min(0)), np.maximum(hi, xm.max(0))
    if not np.all(np.isfinite(lo)):
        return "no frame with a pose has a masked depth pixel"
    return (f"the masked depth points of the frames with a pose span {np.round(lo, 1).tolist()} .. {np.round(hi, 1).tolist()} mm in the model frame: "
            "start from that box and leave room for the side of the object those frames do not see")


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


def _selected(depth, mask, max_points: int):
    """The flat indices of the pixels a frame is tracked with (lift_points' rule), in row-major order."""
    sel = ((mask != 0) & (depth > 0)).reshape(-1).nonzero()[:, 0]               # row-major order
    step = max(1, -(-int(sel.numel()) // int(max_points)))
    return sel[::step]


def _lift(depth, mask, cam, max_points: int, sel=None):
    """depth fp32 [H, W], mask uint8 [H, W] on the device -> fp32 [P, 3] camera-frame points (lift_points' rule)."""
    import torch
    W = depth.shape[1]
    if sel is None:
        sel = _selected(depth, mask, max_points)
    u, v = (sel % W).double(), torch.div(sel, W, rounding_mode="floor").double()
    d = depth.reshape(-1)[sel].double()
    fx, fy, cx, cy = (float(c) for c in cam)
    return torch.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], 1).float().contiguous()


def _lift_rgb(depth, mask, rgb, cam, max_points: int):
    """_lift, and the colours of the same pixels: rgb uint8 [H, W, 3] on the device -> (fp32 [P, 3] points, fp32 [P, 3] colours =
    uint8 / 255 as an fp32 division: what fp_tsdf_integrate adds to the volume)."""
    import torch
    sel = _selected(depth, mask, max_points)
    colors = rgb.reshape(-1, 3)[sel].to(torch.float32) / torch.tensor(255.0, dtype=torch.float32, device=rgb.device)
    return _lift(depth, mask, cam, max_points, sel), colors.contiguous()


def lift_points(frame: Frame, max_points: int, device="cuda"):
    """The camera-frame points a frame is tracked with, fp32 [P, 3] on the device: the pixels with mask != 0 and depth > 0 in row-major
    order, every ceil(n / max_points)-th of them, X_c = ((u - cx) / fx d, (v - cy) / fy d, d) in fp64 rounded to fp32; pixel centres
    lie at integers, as in masked_point_percentiles."""
    import torch
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)   # noqa: E731
    return _lift(up(frame.depth, np.float32), up(frame.mask, np.uint8), frame.cam, max_points)


def lift_points_rgb(frame: Frame, max_points: int, device="cuda"):
    """lift_points' points and the colours of the same pixels -> (fp32 [P, 3], fp32 [P, 3]) on the device: the same selection rule, the
    colours uint8 / 255 as an fp32 division (what integration adds to the volume's colour sums)."""
    import torch
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(device)   # noqa: E731
    return _lift_rgb(up(frame.depth, np.float32), up(frame.mask, np.uint8), up(frame.rgb, np.uint8), frame.cam, max_points)


def fuse_tracked(frames: Sequence[Frame], given: Sequence[Optional[np.ndarray]], opts=None, device="cuda", sequence: Optional[Sequence[int]] = None):
    """Track mode's fusion: the frames go through one at a time, in order.  given[k] is a 12-vector pose or None;
    sequence[k] names the sequence a frame belongs to (None: one sequence), and the first frame of every sequence must have a pose.
    An anchor -- the first frame of a sequence and, with track_anchor_every = N > 0, every Nth frame of it that has a pose -- is
    integrated at its given pose.  Any other frame is tracked (ops.tsdf_track) against the volume of the frames before it, from the start
    pose predict_pose gives, scored by one more evaluation at the result, and integrated at the tracked pose -- or lost: not
    integrated, and the next frame starts from the last kept pose.  More than track_max_lost lost frames in a row raise RuntimeError.
    With track_color_weight > 0 (section 31) the tracking call also takes the colours of the frame's points; the score at the result stays
    geometric, and the frame's record names the weight (its cost_in / cost_out are then the joint objective's).
    -> (volume, poses: a 12-vector or None (lost) per frame, records: one dict per frame)."""
    import torch

    from . import ops
    opts = load_opts(opts)
    if not frames:
        raise ValueError("no frame to fuse")
    if len(given) != len(frames) or (sequence is not None and len(sequence) != len(frames)):
        raise ValueError(f"{len(frames)} frames, {len(given)} given poses" + ("" if sequence is None else f", {len(sequence)} sequence ids"))
    sequence = [0] * len(frames) if sequence is None else list(sequence)
    first: Dict[Any, int] = {}
    for k, s in enumerate(sequence):
        if s not in first:
            first[s] = k
            if given[k] is None:
                raise ValueError(f"frame {k}, the first of sequence {s}, has no pose: tracking starts from one known pose per sequence")
    if opts.bounds is None:
        raise ValueError("pose_source 'track' needs opts.bounds: the poses do not exist before fusion, so the volume cannot be chosen from them; "
                         + anchor_box_hint(frames, given))
    origin, dims = choose_volume(frames, opts, device)
    vol = ops.tsdf_new_volume(origin, opts.voxel_mm, dims, device)
    tau, md = opts.trunc_mm, float(opts.track_max_dist_voxels) * float(opts.voxel_mm)
    color_weight = float(opts.track_color_weight)
    zero = torch.zeros(1, dtype=torch.int32, device=device)
    poses: List[Optional[np.ndarray]] = []
    records: List[Dict[str, Any]] = []
    history: List[Tuple[int, np.ndarray]] = []
    lost_run = 0
    for k, fr in enumerate(frames):
        if first[sequence[k]] == k:
            history = []
        idx = k - first[sequence[k]]
        depth, mask, rgb = _upload([fr], device)
        rec: Dict[str, Any] = {"frame": k, "sequence": sequence[k]}
        if idx == 0 or (opts.track_anchor_every > 0 and idx % opts.track_anchor_every == 0 and given[k] is not None):
            pose, lost_run = np.asarray(given[k], np.float64).reshape(12), 0
            rec["role"] = "anchor"
        else:
            t_start = time.perf_counter()
            T0 = predict_pose(history, idx, opts.track_motion)
            if color_weight > 0:
                pts, cols = _lift_rgb(depth[0], mask[0], rgb[0], fr.cam, opts.track_max_points)
                rec["color_weight"] = color_weight                              # cost_in / cost_out below are then the joint objective's
            else:
                pts = _lift(depth[0], mask[0], fr.cam, opts.track_max_points)
            n = int(pts.shape[0])
            end = torch.full((1,), n, dtype=torch.int32, device=device)
            if n > 0:
                run = lambda R, t, iters: ops.tsdf_track(vol, pts, zero, end, R, t, md, int(opts.track_min_count), tau, iters)   # noqa: E731
                R0, t0 = torch.from_numpy(T0[:3, :3].copy()).to(device), torch.from_numpy(T0[:3, 3].copy()).to(device)
                if color_weight > 0:
                    out = ops.tsdf_track(vol, pts, zero, end, R0, t0, md, int(opts.track_min_count), tau, int(opts.track_iters), colors=cols,
                                         color_weight=color_weight, color_max=float(opts.track_color_max))
                else:
                    out = run(R0, t0, int(opts.track_iters))
                at = run(out["R"], out["t"], 0)                                 # the inliers and the cost at the result: shape alone, either way
                o = {key: v.cpu().numpy()[0] for key, v in out.items()}
                inl, cost = int(at["num_points"].cpu()[0]), float(at["cost_out"].cpu()[0])
                share = inl / n
                rms = math.sqrt(max(cost * n - (n - inl) * md * md, 0.0) / inl) if inl else 0.0   # cost n = sum r^2 over inliers + md^2 per other point
            else:
                o = {"R": T0[:3, :3], "t": T0[:3, 3], "cost_in": 0.0, "cost_out": 0.0, "num_points": 0, "iters_used": 0, "status": 2}
                inl, share, rms = 0, 0.0, 0.0
            kept = share >= opts.track_min_inlier_share and int(o["status"]) != 2
            rec["seconds"] = time.perf_counter() - t_start                      # lifting, both calls and the read-back that waits for them
            rec.update(role="tracked" if kept else "lost", start=np.concatenate([T0[:3, :3].reshape(9), T0[:3, 3]]).tolist(), points=n, inliers_in=int(o["num_points"]), inliers_out=inl, share=share, rms=rms,
                       cost_in=float(o["cost_in"]), cost_out=float(o["cost_out"]), iters=int(o["iters_used"]), status=int(o["status"]))
            pose = np.concatenate([np.asarray(o["R"], np.float64).reshape(9), np.asarray(o["t"], np.float64).reshape(3)]) if kept else None
            if kept:
                lost_run = 0
            else:
                lost_run += 1
                if lost_run > opts.track_max_lost:
                    raise RuntimeError(f"frame {k} (sequence {sequence[k]}): tracking lost on more than track_max_lost = {opts.track_max_lost} "
                                       f"consecutive frames (inlier share {share:.2f}, status {int(o['status'])})")
            if pose is not None and given[k] is not None:
                g = np.asarray(given[k], np.float64).reshape(12)
                c = (np.trace(pose[:9].reshape(3, 3).T @ g[:9].reshape(3, 3)) - 1.0) / 2.0
                rec.update(rot_err_deg=float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), t_err_mm=float(np.linalg.norm(pose[9:] - g[9:])))
        records.append(rec)
        poses.append(pose)
        if pose is not None:
            ops.tsdf_integrate(vol, depth, mask, rgb, np.array([fr.cam], np.float64), pose[None], tau)
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = pose[:9].reshape(3, 3), pose[9:]
            history.append((idx, T))
    return vol, poses, records


def fill_volume(volume: Dict[str, Any], opts=None) -> Tuple[Dict[str, Any], Dict[str, Any]]:
    """Closes a fused volume (tests/tsdf_fill_ref.py restates it bit for bit) -> (volume', stats).  The input is
    left as it is; volume' is extracted with min_count = 1.  Elementwise torch on the device, every operation rounded on its own, around
    two runs of fp_tsdf_diffuse:
      1  f = (float)((double)sdf_sum / (double)sdf_cnt) where sdf_cnt > 0
      2  src = sdf_cnt >= min_count; g = f where sdf_cnt > 0, else -1 (unseen is inside); fixed = src
      3  fill_plane (a, b, c, d): non-src voxels whose centre has ((a X + b Y) + c Z) + d > 0 (fp64) get g = +1 and are fixed
      4  the outermost voxel layer gets g = +1 and is fixed, whatever it held
      5  fill_smooth_iters iterations of fp_tsdf_diffuse on g: FIXED where fixed, else FREE
      6  non-fixed voxels with |g| < 2^-10 become +2^-10
      7  src voxels off the outer layer keep sdf_sum and sdf_cnt; every other voxel gets sdf_sum = g, sdf_cnt = 1
      8  m = rgb_sum / (float)rgb_cnt where rgb_cnt > 0: FIXED there, UNKNOWN elsewhere; fill_color_iters iterations on the three
         channels; voxels that became FREE get rgb_sum = m, rgb_cnt = 1, the others keep what they had
    stats: filled_voxels (non-src voxels that end inside), plane_voxels (step 3), clipped_voxels (src voxels of the outer layer with
    f < 0: there the object sticks out of the bounds and gets a flat cap), snapped_voxels (step 6), uncoloured_voxels (voxels at an end
    of a sign-changing edge of the tetrahedral split that still have no colour), smooth_iters, color_iters, last_change (the largest
    |g_T - g_(T-1)| over non-fixed voxels; 0 when T = 0) and seconds."""
    import torch

    from . import ops
    opts = load_opts(opts)
    t0 = time.perf_counter()
    nx, ny, nz = (int(d) for d in volume["dims"])
    ops._tsdf_state("fill_volume", volume, (nx, ny, nz))
    if min(nx, ny, nz) < 3:
        raise ValueError(f"fill_volume: a volume of {nx} x {ny} x {nz} voxels has no interior: every dimension must be >= 3")
    dev = volume["sdf_sum"].device
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)   # noqa: E731
    cnt = volume["sdf_cnt"]
    seen, src = cnt > 0, cnt >= int(opts.min_count)
    f = (volume["sdf_sum"].double() / cnt.double()).float()
    g = torch.where(seen, f, f32(-1.0))
    fixed = src.clone()
    plane_voxels = 0
    if opts.fill_plane is not None:
        a, b, c, d = (float(v) for v in opts.fill_plane)
        centre = lambda o, n: float(o) + (torch.arange(n, dtype=torch.float64, device=dev) + 0.5) * float(volume["voxel_mm"])   # noqa: E731
        X, Y, Z = centre(volume["origin"][0], nx)[None, None, :], centre(volume["origin"][1], ny)[None, :, None], centre(volume["origin"][2], nz)[:, None, None]
        empty = ~src & ((((a * X + b * Y) + c * Z) + d) > 0)
        g = torch.where(empty, f32(1.0), g)
        fixed |= empty
        plane_voxels = int(empty.sum())
    outer = torch.zeros_like(fixed)
    outer[[0, -1]] = True
    outer[:, [0, -1]] = True
    outer[:, :, [0, -1]] = True
    clipped = int((outer & src & (f < 0)).sum())
    g = torch.where(outer, f32(1.0), g)
    fixed |= outer
    state = torch.where(fixed, 1, 2).to(torch.uint8)
    T = int(opts.fill_smooth_iters)
    free = ~fixed
    last_change = 0.0
    if T > 0:
        before = ops.tsdf_diffuse(g[None], state, T - 1)[0]
        g = ops.tsdf_diffuse(before, state, 1)[0][0]                              # T - 1 iterations and one more: the bits of T in one call
        if bool(free.any()):
            last_change = float((g - before[0]).abs()[free].max())
    snap = free & (g.abs() < FILL_SNAP)
    g = torch.where(snap, f32(FILL_SNAP), g)
    keep = src & ~outer
    out = dict(volume)
    out["sdf_sum"] = torch.where(keep, volume["sdf_sum"], g).contiguous()
    out["sdf_cnt"] = torch.where(keep, cnt, 1).to(torch.int32).contiguous()
    has = volume["rgb_cnt"] > 0
    m = (volume["rgb_sum"].double() / volume["rgb_cnt"].double()[None]).float()   # fp32 operands: the fp64 quotient rounds to the fp32 one
    m = torch.where(has[None], m, f32(0.0))
    m, cstate = ops.tsdf_diffuse(m, torch.where(has, 1, 0).to(torch.uint8), int(opts.fill_color_iters))
    got = cstate == 2
    out["rgb_sum"] = torch.where(got[None], m, volume["rgb_sum"]).contiguous()
    out["rgb_cnt"] = torch.where(got, 1, volume["rgb_cnt"]).to(torch.int32).contiguous()
    inside = torch.where(keep, f, g) < 0
    near = torch.zeros_like(inside)
    for dx, dy, dz in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)):   # the edges of the tetrahedral split
        lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        hi = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        cross = inside[lo] != inside[hi]
        near[lo] |= cross
        near[hi] |= cross
    stats = {"filled_voxels": int((~src & inside).sum()), "plane_voxels": plane_voxels, "clipped_voxels": clipped, "snapped_voxels": int(snap.sum()),
             "uncoloured_voxels": int((near & (out["rgb_cnt"] == 0)).sum()), "smooth_iters": T, "color_iters": int(opts.fill_color_iters),
             "last_change": last_change}
    torch.cuda.synchronize()
    stats["seconds"] = time.perf_counter() - t0
    return out, stats


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
                device: str = "cuda", tracked_poses_dir: Optional[str] = None) -> Dict[str, Any]:
    """Reads the sequences, fuses, extracts and writes <output_dir>/obj_%06d.ply (and the report) -> the report.  With
    opts.pose_source "track" the frames are tracked (fuse_tracked), the report gains "tracking", and tracked_poses_dir, when given,
    receives per sequence k <k:06d>_scene_gt.json with this object's entry for every frame that was kept."""
    import torch

    from . import _lib
    from .renderer import save_ply
    t0 = time.perf_counter()
    opts = load_opts(opts)
    track = opts.pose_source == "track"
    if tracked_poses_dir and not track:
        raise ValueError("tracked poses are written with pose_source 'track' only")
    out_path = os.path.join(output_dir, f"obj_{int(obj_id):06d}.ply")
    pose_paths = [os.path.join(tracked_poses_dir, f"{k:06d}_scene_gt.json") for k in range(len(sequences))] if tracked_poses_dir else []
    refuse_existing([out_path] + ([report_path] if report_path else []) + pose_paths, overwrite)
    frames: List[Frame] = []
    given: List[Optional[np.ndarray]] = []
    seq_of: List[int] = []
    images: List[int] = []
    for k, sd in enumerate(sequences):
        if track:
            got, poses_k, ims = read_sequence_tracked(sd, obj_id, opts.mask_dir)
            if not got:
                raise ValueError(f"{sd}: scene_camera.json lists no image")
            if poses_k[0] is None:
                raise ValueError(f"{sd}: its first image does not show object {obj_id} in scene_gt.json: tracking starts from one known pose per sequence")
            given += poses_k
            seq_of += [k] * len(got)
            images += ims
        else:
            got = read_sequence(sd, obj_id, opts.mask_dir)
            if not got:
                raise ValueError(f"{sd}: no frame shows object {obj_id}")
        frames += got
    if track and opts.bounds is None:
        fuse_tracked(frames, given, opts, device, seq_of)                       # raises: bounds are needed, with a hint
    t_read = time.perf_counter()
    _lib.lib()
    if not torch.cuda.is_available():
        raise _lib.FoundPoseNativeError("reconstruct runs on the MI355X only: no device is available and no CPU path exists")
    tracking = None
    if track:
        vol, poses, records = fuse_tracked(frames, given, opts, device, seq_of)
        torch.cuda.synchronize()
        for rec, im in zip(records, images):
            rec["image"] = im
        roles = [r["role"] for r in records]
        tracking = {"frames": records, "totals": {role: roles.count(role) for role in ("anchor", "tracked", "lost")},
                    "seconds": float(sum(r.get("seconds", 0.0) for r in records))}
        if opts.track_color_weight > 0:                                          # tracked on shape and colour (section 31)
            tracking["totals"]["color_weight"] = float(opts.track_color_weight)
    else:
        vol = fuse(frames, opts, device)
    observed = int((vol["sdf_cnt"] >= opts.min_count).sum())
    torch.cuda.synchronize()
    t_fuse = time.perf_counter()
    fill = None
    if opts.fill == "carve":                                                     # the same step after fuse and after fuse_tracked (section 34)
        vol, fill = fill_volume(vol, opts)
    mesh = extract_mesh(vol, opts if fill is None else opts._replace(min_count=1))
    t_mesh = time.perf_counter()
    os.makedirs(output_dir, exist_ok=True)
    save_ply(out_path, mesh)
    topo = mesh_topology(mesh.faces)
    lo = np.asarray(vol["origin"])
    if tracking is not None and tracked_poses_dir:
        os.makedirs(tracked_poses_dir, exist_ok=True)
        for k, path in enumerate(pose_paths):                                    # scene_gt.json's format; lost frames are omitted
            entries = {str(im): [{"cam_R_m2c": p[:9].tolist(), "cam_t_m2c": p[9:].tolist(), "obj_id": int(obj_id)}]
                       for im, s, p in zip(images, seq_of, poses) if s == k and p is not None}
            with open(path, "w") as f:
                json.dump(entries, f)
    used = len(frames) if tracking is None else tracking["totals"]["anchor"] + tracking["totals"]["tracked"]
    report = {"obj_id": int(obj_id), "output": out_path, "sequences": [os.path.abspath(s) for s in sequences], "frames_used": used,
              "opts": opts._asdict(), "bounds": [lo.tolist(), (lo + np.asarray(vol["dims"]) * vol["voxel_mm"]).tolist()],
              "dims": list(vol["dims"]), "observed_voxels": observed, "vertices": int(len(mesh.vertices)), "triangles": int(len(mesh.faces)),
              **topo,
              "note": None if topo["watertight"] else ("the surface is open where no frame saw it; nothing is filled" if fill is None else
                                                       "the filled surface is still open: an observed value that is exactly 0 counts as outside and puts "
                                                       "its vertices on the voxel's corner, where welding drops the collapsed triangles"),
              "seconds": {"read": t_read - t0, "fuse": t_fuse - t_read, "extract": t_mesh - t_fuse, "total": time.perf_counter() - t0}}
    if fill is not None:
        report["fill"] = fill                                                    # its seconds are part of "extract"
    if tracking is not None:
        report["tracking"] = tracking
    if report_path:
        with open(report_path, "w") as f:
            json.dump(report, f, indent=1)
    return report


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m foundpose_amd.reconstruct", description=__doc__.split("\n\n")[0])
    ap.add_argument("--sequence", action="append", required=True, help="a BOP scene directory; repeat to fuse several, in order")
    ap.add_argument("--obj-id", type=int, required=True)
    ap.add_argument("--output", required=True, help="the models directory obj_%%06d.ply is written into")
    ap.add_argument("--opts", default=None, help="JSON with ReconstructOpts fields; fill: \"carve\" closes the surface no frame saw (fill_smooth_iters, "
                    "fill_color_iters, fill_plane: [a, b, c, d] with a x + b y + c z + d > 0 known to be empty, model frame, mm)")
    ap.add_argument("--report", default=None, help="write the report to this JSON file")
    ap.add_argument("--overwrite", action="store_true", help="replace an existing output")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--tracked-poses", default=None, help="pose_source 'track': write <k:06d>_scene_gt.json per sequence k into this directory")
    a = ap.parse_args(argv)
    r = reconstruct(a.sequence, a.obj_id, a.output, a.opts, a.report, a.overwrite, a.device, a.tracked_poses)
    if "tracking" in r:
        tot = r["tracking"]["totals"]
        print(f"tracking: {tot['anchor']} anchor(s), {tot['tracked']} tracked, {tot['lost']} lost in {r['tracking']['seconds']:.2f} s"
              + (f" (on shape and colour, weight {tot['color_weight']:g} mm per unit)" if "color_weight" in tot else ""))
    if "fill" in r:
        fl = r["fill"]
        print(f"fill: {fl['filled_voxels']} voxel(s) filled, {fl['plane_voxels']} emptied by the plane, {fl['clipped_voxels']} clipped at the bounds, "
              f"{fl['uncoloured_voxels']} at the surface without colour in {fl['seconds']:.2f} s")
    print(f"{r['output']}: {r['vertices']} vertices, {r['triangles']} triangles from {r['frames_used']} frame(s) in a volume of "
          f"{r['dims'][0]} x {r['dims'][1]} x {r['dims'][2]} voxels; {r['boundary_edges']} boundary edge(s), "
          f"{'watertight' if r['watertight'] else 'open: ' + str(r['note'])}; {r['seconds']['total']:.2f} s")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
