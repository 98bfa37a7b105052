"""Object templates rendered on the MI355X (scripts/gen_templates.py): a BOP mesh in, the templates directory that
gen_repre reads out -- RGB / 16-bit depth / mask PNGs, metadata.json and config.json under
<output>/templates/<version>/<dataset>/<lid>/ -- with the reference's option names, view sampling, cameras and casts.

Per batch of views (32 by default) the chain stays on the device: render at SSAA resolution (renderer.HipRasterizer,
csrc/render.hip) -> one host synchronisation for the object boxes -> crop cameras on the host (crop_util, fp64) ->
colour / mask warps (fp_warp_crops) and depth warp (fp_warp_depth) -> SSAA downsample with the output casts
(fp_template_downsample).  PNGs are written from a thread pool; `synthesize_templates(..., return_templates=True)` also
hands the uint8 / uint16 tensors to gen_repre.generate_repre(templates=...) without a PNG round trip.

  python -m foundpose_amd.gen_templates --opts configs/gen_templates/lmo.json --datasets-path <bop root> \\
      --output-path <out> --depth-range MIN MAX

The depth range (mm) is required: the reference reads it from bop_toolkit's built-in per-dataset tables.
"""

import argparse
import json
import math
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import crop_util
from ._lib import call, ptr, stream, upload_async
from .crop_util import AlignedBox2f, PinholePlaneCameraModel
from .renderer import HipRasterizer


class GenTemplatesOpts(NamedTuple):
    """Options of scripts/gen_templates.py (same names, same defaults).  max_num_triangles, texture_size, background_type
    (always black) and light_type are accepted and ignored, as the reference's own code ignores them."""
    version: str
    object_dataset: str
    object_lids: Optional[List[int]] = None
    num_viewspheres: int = 1
    min_num_viewpoints: int = 57
    num_inplane_rotations: int = 14
    images_per_view: int = 1
    max_num_triangles: int = 20000
    back_face_culling: bool = False
    texture_size: Tuple[int, int] = (1024, 1024)
    ssaa_factor: float = 4.0
    background_type: str = "black"
    light_type: str = "multi_directional"
    crop: bool = True
    crop_rel_pad: float = 0.2
    crop_size: Tuple[int, int] = (420, 420)
    features_patch_size: int = 14
    save_templates: bool = True
    overwrite: bool = True
    debug: bool = True


def load_opts(path_or_dict) -> GenTemplatesOpts:
    d = path_or_dict
    if not isinstance(d, dict):
        with open(path_or_dict) as f:
            d = json.load(f)
    d = dict(d.get("gen_templates_opts", d))
    for k in ("texture_size", "crop_size"):
        if k in d:
            d[k] = tuple(d[k])
    return GenTemplatesOpts(**d)


# ---------------------------------------------------------------- views (utils/misc.py:47-175)
def fibonacci_points(n: int, radius: float) -> np.ndarray:
    """n (odd) points of the Fibonacci lattice on a sphere, from the south pole up."""
    assert n % 2 == 1
    half = n // 2
    golden_angle = 2.0 * math.pi * ((math.sqrt(5.0) + 1.0) / 2.0 - 1.0)
    pts = []
    for i in range(-half, half + 1):
        lat = math.asin(2 * i / float(2 * half + 1))
        lon = (golden_angle * i) % (2 * math.pi)
        r = math.cos(lat) * radius
        pts.append([math.cos(lon) * r, math.sin(lon) * r, math.tan(lat) * r])
    return np.array(pts, np.float64)


def sample_views(min_n_views: int, radius: float = 1.0) -> List[Dict[str, np.ndarray]]:
    """Fibonacci viewpoints looking at the origin with +Z up (gluLookAt), in the OpenCV camera convention:
    [{"R": 3x3 model-to-camera rotation, "t": 3x1 translation (mm)}]."""
    n = min_n_views + (1 - min_n_views % 2)
    views = []
    for p in fibonacci_points(n, radius):
        fwd = -p / np.linalg.norm(p)
        side = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        if not np.any(side):
            side = np.array([1.0, 0.0, 0.0])
        side = side / np.linalg.norm(side)
        up = np.cross(side, fwd)
        R = np.stack([side, -up, fwd])   # OpenGL rows (s, u, -f) with Y and Z flipped
        views.append({"R": R, "t": -R.dot(p.reshape(3, 1))})
    return views


def inplane_rotation(angle: float) -> np.ndarray:
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def viewsphere_radii(depth_range: Sequence[float], num_viewspheres: int) -> List[float]:
    lo, hi = float(np.min(depth_range)), float(np.max(depth_range))
    cell = (hi - lo) / float(num_viewspheres)
    return [lo + (i + 0.5) * cell for i in range(num_viewspheres)]


def template_views(opts: GenTemplatesOpts, depth_range: Sequence[float]) -> List[Dict[str, np.ndarray]]:
    """Every sphere view combined with each in-plane rotation (R_inplane @ R, R_inplane @ t), each repeated images_per_view
    times -- the order in which templates are numbered."""
    sphere = [v for r in viewsphere_radii(depth_range, opts.num_viewspheres) for v in sample_views(opts.min_num_viewpoints, r)]
    if opts.num_inplane_rotations == 1:
        views = sphere
    else:
        step = 2 * np.pi / opts.num_inplane_rotations
        views = [{"R": inplane_rotation(step * k).dot(v["R"]), "t": inplane_rotation(step * k).dot(v["t"])}
                 for v in sphere for k in range(opts.num_inplane_rotations)]
    return [v for v in views for _ in range(opts.images_per_view)]


# ---------------------------------------------------------------- cameras (gen_templates.py steps 1, 4-6)
def base_cameras(K: np.ndarray, im_size: Tuple[int, int], opts: GenTemplatesOpts) -> Tuple[PinholePlaneCameraModel, PinholePlaneCameraModel]:
    """(square template camera, its SSAA render camera) from the dataset camera K and (width, height)."""
    W, H = im_size
    side = opts.features_patch_size * int(max(W, H) / opts.features_patch_size)
    cam = PinholePlaneCameraModel(side, side, (K[0, 0], K[1, 1]), (K[0, 2] - 0.5 * (W - side), K[1, 2] - 0.5 * (H - side)))
    s = opts.ssaa_factor
    render = PinholePlaneCameraModel(int(cam.width * s), int(cam.height * s), (cam.f[0] * s, cam.f[1] * s), (cam.c[0] * s, cam.c[1] * s))
    return cam, render


def view_camera(render_cam: PinholePlaneCameraModel, view: Dict[str, np.ndarray]) -> PinholePlaneCameraModel:
    """The render camera placed at a view: T_world_from_eye = inverse of the model-to-camera view (fp64)."""
    R_c2m = view["R"].T
    T = np.eye(4)
    T[:3, :3], T[:3, 3:] = R_c2m, -R_c2m.dot(view["t"])
    return PinholePlaneCameraModel(render_cam.width, render_cam.height, render_cam.f, render_cam.c, T)


def check_fits(box: Sequence[int], width: int, height: int) -> None:
    """The reference's fit check: a box touching the viewport border (or an empty render, whose box is all zeros)."""
    if box[0] == 0 or box[1] == 0 or box[2] == width - 1 or box[3] == height - 1:
        raise ValueError("The model does not fit the viewport.")


def crop_camera(box: Sequence[int], cam_c2w: PinholePlaneCameraModel, opts: GenTemplatesOpts) -> PinholePlaneCameraModel:
    crop_box = crop_util.calc_crop_box(AlignedBox2f(box[0], box[1], box[2], box[3]), make_square=True)
    size = (int(opts.crop_size[0] * opts.ssaa_factor), int(opts.crop_size[1] * opts.ssaa_factor))
    return crop_util.construct_crop_camera(crop_box, cam_c2w, size, opts.crop_rel_pad)


def template_camera(crop_cam: PinholePlaneCameraModel, opts: GenTemplatesOpts) -> PinholePlaneCameraModel:
    """The crop camera at the output size: f and c scaled by crop_size / (crop_size * ssaa), no half-pixel correction.
    The float32 camera numbers are scaled in fp64 (numpy 1.x scalar promotion, the reference's pinned numpy)."""
    scale = opts.crop_size[0] / float(crop_cam.width)
    return PinholePlaneCameraModel(opts.crop_size[0], opts.crop_size[1], (float(crop_cam.f[0]) * scale, float(crop_cam.f[1]) * scale),
                                   (float(crop_cam.c[0]) * scale, float(crop_cam.c[1]) * scale), crop_cam.T_world_from_eye)


def camera_to_json(cam: PinholePlaneCameraModel) -> Dict[str, Any]:
    """utils/structs.py PinholePlaneCameraModel.to_json."""
    return {"ImageSizeX": cam.width, "ImageSizeY": cam.height, "T_WorldFromCamera": cam.T_world_from_eye.tolist(),
            "ModelViewMatrix": np.linalg.inv(cam.T_world_from_eye).tolist(), "fx": float(cam.f[0]), "fy": float(cam.f[1]),
            "cx": float(cam.c[0]), "cy": float(cam.c[1])}


# ---------------------------------------------------------------- device chain
def _host_box(b) -> List[int]:
    """Device box (INT_MAX when empty) -> the reference's calc_2d_box convention (zeros when empty)."""
    b = [int(x) for x in b]
    return [0, 0, 0, 0] if b[0] > b[2] else b


def render_templates(renderer: HipRasterizer, obj_id: int, views: Sequence[Dict[str, np.ndarray]], render_cam: PinholePlaneCameraModel,
                     opts: GenTemplatesOpts) -> Dict[str, Any]:
    """One batch of views through steps 3-7 -> rgb u8 [B,3,S,S], depth u16 [B,S,S], mask u8 [B,S,S] (device tensors),
    boxes (host, final mask), template cameras."""
    if not opts.crop:
        raise NotImplementedError("crop=False: the reference raises NameError there (trans_c2w undefined, gen_templates.py:369)")
    f = opts.ssaa_factor
    if f != int(f) or f < 1:
        raise NotImplementedError("ssaa_factor must be a positive integer")
    f = int(f)
    cams = [view_camera(render_cam, v) for v in views]
    r = renderer.render_views(obj_id, cams)
    boxes = r["boxes"].cpu().numpy()     # the batch's host synchronisation: boxes define the crop cameras
    crop_cams = []
    for cam, b in zip(cams, boxes):
        box = _host_box(b)
        check_fits(box, cam.width, cam.height)
        crop_cams.append(crop_camera(box, cam, opts))
    B = len(cams)
    S4w, S4h = crop_cams[0].width, crop_cams[0].height
    color, mask = crop_util.warp_crops(r["color"], r["mask"], cams, crop_cams)
    params = np.stack([crop_util.camera_pair_params(s, d) for s, d in zip(cams, crop_cams)])
    dev = r["depth"].device
    p = upload_async(torch.from_numpy(params), dev)
    recompute = upload_async(torch.tensor([0 if np.allclose(s.T_world_from_eye, d.T_world_from_eye) else 1 for s, d in zip(cams, crop_cams)],
                                          dtype=torch.int32), dev)
    depth = torch.empty(B, S4h, S4w, dtype=torch.float32, device=dev)
    call("fp_warp_depth", ptr(r["depth"]), render_cam.height, render_cam.width, ptr(p), ptr(recompute), B, S4h, S4w, 1, ptr(depth), stream())
    Sw, Sh = opts.crop_size
    if (Sw * f, Sh * f) != (S4w, S4h):
        raise ValueError("crop_size x ssaa_factor must be the crop viewport")
    rgb = torch.empty(B, 3, Sh, Sw, dtype=torch.uint8, device=dev)
    d16 = torch.empty(B, Sh, Sw, dtype=torch.uint16, device=dev)
    m8 = torch.empty(B, Sh, Sw, dtype=torch.uint8, device=dev)
    fboxes = torch.empty(B, 4, dtype=torch.int32, device=dev)
    call("fp_template_downsample", ptr(color), ptr(depth), ptr(mask), B, Sh, Sw, f, ptr(rgb), ptr(d16), ptr(m8), ptr(fboxes), stream())
    return {"rgb": rgb, "depth": d16, "mask": m8, "boxes": [_host_box(b) for b in fboxes.cpu().numpy()],
            "cameras": [template_camera(c, opts) for c in crop_cams]}


def _save_pngs(rgb: np.ndarray, depth: np.ndarray, mask: np.ndarray, paths: Tuple[str, str, str]) -> None:
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(rgb.transpose(1, 2, 0))).save(paths[0])
    Image.fromarray(depth).save(paths[1])           # 16-bit greyscale PNG (inout.save_depth)
    Image.fromarray(mask).save(paths[2])


def load_bop_camera(datasets_path: str, dataset: str) -> Tuple[np.ndarray, Tuple[int, int]]:
    with open(os.path.join(datasets_path, dataset, "camera.json")) as f:
        c = json.load(f)
    K = np.array([[c["fx"], 0.0, c["cx"]], [0.0, c["fy"], c["cy"]], [0.0, 0.0, 1.0]])
    return K, (int(c["width"]), int(c["height"]))


def synthesize_templates(opts: GenTemplatesOpts, datasets_path: str, output_path: str, depth_range: Sequence[float],
                         renderer: Optional[HipRasterizer] = None, batch_size: int = 32, return_templates: bool = False,
                         workers: int = 8) -> Optional[Dict[int, Dict[str, Any]]]:
    """scripts/gen_templates.py for every object of opts.object_lids (all of models/models_info.json when None).
    With return_templates: {lid: {"rgb" u8 [T,3,S,S], "depth" u16 [T,S,S], "mask" u8 [T,S,S] (device), "metadata"}}."""
    K, im_size = load_bop_camera(datasets_path, opts.object_dataset)
    _, render_cam = base_cameras(K, im_size, opts)
    views = template_views(opts, depth_range)
    lids = opts.object_lids
    if lids is None:
        with open(os.path.join(datasets_path, opts.object_dataset, "models", "models_info.json")) as f:
            lids = sorted(int(k) for k in json.load(f))
    renderer = renderer or HipRasterizer()
    result: Dict[int, Dict[str, Any]] = {}
    pool = ThreadPoolExecutor(max_workers=workers)
    try:
        for lid in lids:
            out_dir = os.path.join(output_path, "templates", opts.version, opts.object_dataset, str(lid))
            if os.path.exists(out_dir) and not opts.overwrite:
                raise ValueError(f"Output directory already exists: {out_dir}")
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, "config.json"), "w") as f:
                json.dump(opts._asdict(), f, indent=2)
            dirs = {k: os.path.join(out_dir, k) for k in ("rgb", "depth", "mask")}
            if opts.save_templates:
                for d in dirs.values():
                    os.makedirs(d, exist_ok=True)
            renderer.add_object_model(lid, os.path.join(datasets_path, opts.object_dataset, "models", f"obj_{lid:06d}.ply"))
            metadata, kept, pending = [], [], []
            for start in range(0, len(views), batch_size):
                t = render_templates(renderer, lid, views[start:start + batch_size], render_cam, opts)
                host = [t[k].cpu().numpy() for k in ("rgb", "depth", "mask")] if opts.save_templates else None
                for i, cam in enumerate(t["cameras"]):
                    tid = start + i
                    paths = tuple(os.path.join(dirs[k], f"template_{tid:04d}.png") for k in ("rgb", "depth", "mask"))
                    if host is not None:
                        pending.append(pool.submit(_save_pngs, host[0][i], host[1][i], host[2][i], paths))
                    metadata.append({"dataset": opts.object_dataset, "lid": lid, "template_id": tid,
                                     "pose": {"R": np.eye(3).tolist(), "t": np.zeros((3, 1)).tolist()},
                                     "boxes_amodal": [[float(x) for x in t["boxes"][i]]], "visibilities": [1.0],
                                     "cameras": camera_to_json(cam), "rgb_image_path": paths[0], "depth_map_path": paths[1],
                                     "binary_mask_path": paths[2]})
                if return_templates:
                    kept.append(t)
            for p in pending:
                p.result()
            with open(os.path.join(out_dir, "metadata.json"), "w") as f:
                json.dump(metadata, f, indent=2)
            if return_templates:
                result[lid] = {k: torch.cat([t[k] for t in kept]) for k in ("rgb", "depth", "mask")}
                result[lid]["metadata"] = metadata
    finally:
        pool.shutdown(wait=True)
    return result if return_templates else None


def main(argv: Optional[Sequence[str]] = None) -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--opts", required=True)
    ap.add_argument("--datasets-path", required=True, help="BOP root holding <dataset>/camera.json and <dataset>/models/")
    ap.add_argument("--output-path", required=True)
    ap.add_argument("--depth-range", type=float, nargs=2, required=True, metavar=("MIN", "MAX"),
                    help="camera-object distances (mm) the view spheres span (bop_toolkit's depth_range of the test split)")
    ap.add_argument("--batch-size", type=int, default=32)
    args = ap.parse_args(argv)
    synthesize_templates(load_opts(args.opts), args.datasets_path, args.output_path, args.depth_range, batch_size=args.batch_size)


if __name__ == "__main__":
    main()
