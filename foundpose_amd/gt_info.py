"""Writes `scene_gt_info.json` and the instance masks `mask/`, `mask_visib/` of a BOP split from its ground-truth poses: what
bop_toolkit's `calc_gt_info.py` and `calc_gt_masks.py` write, and what `eval_bop19`, `eval_bop24`, `eval_add`, `eval_coco` and
`infer --eval-gt` read.

    python -m foundpose_amd.gt_info --dataset-dir <datasets>/<dataset>/<split> --models-dir <datasets>/<dataset>/models
        [--dataset NAME] [--delta MM] [--scenes 1 2] [--output-dir DIR] [--no-masks] [--targets bop19|bop24] [--depth-from-gt] [--overwrite]

Per scene it reads `scene_gt.json`, `scene_camera.json` and `depth/<im>.png`; every GT instance is rendered alone by the HIP rasterizer
(renderer.HipRasterizer) into a window of 3W x 3H around the image, as the toolkit does to count the truncated part of a silhouette, and
fp_gt_visibility (csrc/gt_info.hip) turns a chunk of renders into pixel counts, boxes and masks.  The record assembly, the targets and
the file layout are host code below.  With --depth-from-gt (RGB-only splits) a frame's depth is the per-pixel nearest surface of its
own instance renders: annotated objects then occlude each other and nothing else does.  There is no CPU path.

NOTHING HERE IS PINNED AGAINST bop_toolkit: the toolkit is not installed, and its GL rasterizer's pixel coverage is not this
rasterizer's, so counts at silhouette edges can differ from BOP's published files.  A GT pose with a vertex inside the rasterizer's
100 mm near plane is refused (the toolkit clips it)."""

import argparse
import json
import os
import re
import time
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .device_timer import DeviceTimer
from .eval_bop19 import DEFAULT_VSD_DELTA, MAX_IO_WORKERS, NEAR_LIMIT_MM, VSD_DELTA

MIN_VISIB_FRACT = 0.1              # test_targets_bop19.json counts the instances at least this visible
WINDOW_SCALE = 3                   # the render window is 3W x 3H, the image in its middle
MAX_CHUNK_VIEWS = 32               # views per render_views / fp_gt_visibility call, at most
MAX_CHUNK_BYTES = 1 << 30          # ... and their render outputs (depth fp32 + mask u8 per window pixel) stay below about this
IMAGE_BLOCK = 32                   # frames whose depth images are held at once
TARGET_KINDS = ("bop19", "bop24")
NOT_PINNED = ("nothing here is pinned against bop_toolkit: its GL rasterizer's pixel coverage is not this rasterizer's, "
              "so counts at silhouette edges can differ from BOP's published files")


# ---------------------------------------------------------------------------------------------------------- host logic
def gt_record(row: Sequence[int]) -> Dict[str, Any]:
    """A row of fp_gt_visibility's `out` -> the toolkit's per-instance entry, in its key order.  Boxes are [x, y, w, h] with
    w = max x - min x (misc.calc_2d_bbox adds no 1), both -1 unless px_count_visib > 0; visib_fract is 0.0 for an empty render."""
    r = [int(v) for v in row]
    px_all, px_valid, px_visib = r[:3]
    if px_visib > 0:
        bbox_obj = [r[3], r[4], r[5] - r[3], r[6] - r[4]]
        bbox_visib = [r[7], r[8], r[9] - r[7], r[10] - r[8]]
    else:
        bbox_obj, bbox_visib = [-1, -1, -1, -1], [-1, -1, -1, -1]
    return {"bbox_obj": bbox_obj, "bbox_visib": bbox_visib, "px_count_all": px_all, "px_count_valid": px_valid,
            "px_count_visib": px_visib, "visib_fract": (px_visib / float(px_all)) if px_all > 0 else 0.0}


def count_targets(instances: Iterable[Tuple[int, int, int, float]], kind: str = "bop19") -> List[Dict[str, int]]:
    """instances: (scene_id, im_id, obj_id, visib_fract) of every GT instance.  "bop19": one {scene_id, im_id, obj_id, inst_count} per
    image and object, inst_count the instances with visib_fract >= 0.1, entries with 0 left out; "bop24": one {scene_id, im_id} per image."""
    if kind not in TARGET_KINDS:
        raise ValueError(f"targets must be one of {TARGET_KINDS}, got {kind!r}")
    if kind == "bop24":
        return [{"scene_id": s, "im_id": im} for s, im in sorted({(int(s), int(im)) for s, im, _, _ in instances})]
    count: Dict[Tuple[int, int, int], int] = defaultdict(int)
    for s, im, lid, vf in instances:
        count[(int(s), int(im), int(lid))] += int(float(vf) >= MIN_VISIB_FRACT)
    return [{"scene_id": s, "im_id": im, "obj_id": lid, "inst_count": n} for (s, im, lid), n in sorted(count.items()) if n > 0]


def refuse_existing(paths: Iterable[str], overwrite: bool) -> None:
    """Raises FileExistsError, before anything is written, when an output file exists and `overwrite` is not set."""
    if overwrite:
        return
    found = [p for p in paths if os.path.exists(p)]
    if found:
        raise FileExistsError(f"{found[0]} exists" + (f" (and {len(found) - 1} more output files)" if len(found) > 1 else "")
                              + "; pass overwrite=True / --overwrite to replace them")


def chunk_views(width: int, height: int) -> int:
    """Views per chunk: render outputs (depth + mask of the 3W x 3H window) below about 1 GiB, 32 views at most, one at least."""
    per_view = WINDOW_SCALE * WINDOW_SCALE * int(width) * int(height) * 5
    return int(max(1, min(MAX_CHUNK_VIEWS, MAX_CHUNK_BYTES // per_view)))


def scan_box(box: Sequence[int]) -> Tuple[int, int, int, int]:
    """The renderer's `boxes` row -> fp_gt_visibility's scan box (an empty render: x1 = x0 - 1)."""
    x0, y0, x1, y1 = (int(v) for v in box)
    return (0, 0, -1, -1) if x0 > x1 or y0 > y1 else (x0, y0, x1, y1)


def _read_json(path: str):
    with open(path) as f:
        return json.load(f)


def _scene_ids(split_dir: str, scenes: Optional[Sequence[int]]) -> List[int]:
    if not os.path.isdir(split_dir):
        raise FileNotFoundError(f"{split_dir}: no such split directory")
    found = sorted(int(n) for n in os.listdir(split_dir) if re.fullmatch(r"\d{6}", n) and os.path.isfile(os.path.join(split_dir, n, "scene_gt.json")))
    if scenes is None:
        if not found:
            raise FileNotFoundError(f"{split_dir}: no scene folder with a scene_gt.json")
        return found
    missing = [int(s) for s in scenes if int(s) not in found]
    if missing:
        raise FileNotFoundError(f"{split_dir}: no scene_gt.json for scene(s) {missing}")
    return [int(s) for s in scenes]


def _image_path(scene_dir: str, im: int, depth_from_gt: bool) -> str:
    subs = (("rgb", "png"), ("rgb", "jpg"), ("gray", "tif"), ("gray", "png")) if depth_from_gt else (("depth", "png"),)
    for sub, ext in subs:
        p = os.path.join(scene_dir, sub, f"{im:06d}.{ext}")
        if os.path.exists(p):
            return p
    if depth_from_gt:
        raise FileNotFoundError(f"{scene_dir}: no rgb/ or gray/ image {im:06d} to take the image size from")
    raise FileNotFoundError(f"{scene_dir}: no depth/{im:06d}.png; an RGB-only split needs depth_from_gt=True / --depth-from-gt")


def _image_size(path: str) -> Tuple[int, int]:
    from PIL import Image
    with Image.open(path) as im:
        return int(im.size[0]), int(im.size[1])


def _save_mask(path: str, mask: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(mask, np.uint8)).save(path)   # 8-bit grey


def _dump_scene_json(path: str, content: Dict[str, Any]) -> None:
    """One image per line, the way the toolkit lays its scene files out."""
    lines = [f'  "{k}": {json.dumps(v)}' for k, v in content.items()]
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n" if lines else "{}\n")


# ---------------------------------------------------------------------------------------------------------- the tool
def write_gt_info(split_dir: str, models_dir: str, dataset: Optional[str] = None, delta: Optional[float] = None,
                  scenes: Optional[Sequence[int]] = None, output_dir: Optional[str] = None, write_masks: bool = True,
                  targets: Optional[str] = None, depth_from_gt: bool = False, overwrite: bool = False, device: str = "cuda") -> Dict[str, Any]:
    """scene_gt_info.json (and mask/, mask_visib/ when write_masks) for the scenes of `split_dir` (<datasets>/<dataset>/<split>; all, or
    `scenes`), the meshes read as <models_dir>/obj_XXXXXX.ply.  dataset: its name (default the parent directory's), which picks the
    visibility tolerance, 5 mm for itodd, else 15 mm, unless `delta` is given.  output_dir: the scene folders are mirrored there instead
    of written into the split.  targets: "bop19" / "bop24" also writes <split or output dir>/../test_targets_<kind>.json.  depth_from_gt:
    the frames' depth is composed from the instance renders (RGB-only splits; the image size then comes from rgb/ or gray/).  An existing
    output file is refused before anything is written unless `overwrite`.  A GT pose the rasterizer cannot draw raises ValueError naming
    the scene, image and instance.  -> summary dict (counts, wall time, device time of renders and kernel).  Nothing here is pinned
    against bop_toolkit (see the module's doc string)."""
    import torch

    from . import _lib, ops
    from .eval_bop19 import _Camera, _m2c, load_depth, prescreen
    from .renderer import HipRasterizer, load_ply
    t_start = time.perf_counter()
    if targets is not None and targets not in TARGET_KINDS:
        raise ValueError(f"targets must be one of {TARGET_KINDS} or None, got {targets!r}")
    split_dir = os.path.abspath(split_dir)
    dataset = dataset or os.path.basename(os.path.dirname(split_dir))
    delta = float(delta) if delta is not None else VSD_DELTA.get(dataset, DEFAULT_VSD_DELTA)
    if not delta == delta:
        raise ValueError("delta is NaN")
    out_root = os.path.abspath(output_dir) if output_dir is not None else split_dir
    scene_ids = _scene_ids(split_dir, scenes)

    # ---- every input but the pixels is read, and every refusal made, before any device work and before anything is written
    plan = []          # (scene, scene dir, out dir, gts {im: entries}, cams)
    outputs: List[str] = []
    obj_ids = set()
    for s in scene_ids:
        sd, od = os.path.join(split_dir, f"{s:06d}"), os.path.join(out_root, f"{s:06d}")
        gts = {int(k): v for k, v in _read_json(os.path.join(sd, "scene_gt.json")).items()}
        cams = {int(k): v for k, v in _read_json(os.path.join(sd, "scene_camera.json")).items()}
        outputs.append(os.path.join(od, "scene_gt_info.json"))
        for im in sorted(gts):
            if im not in cams:
                raise ValueError(f"scene {s}: image {im} of scene_gt.json is missing from scene_camera.json")
            for g, e in enumerate(gts[im]):
                obj_ids.add(int(e["obj_id"]))
                if write_masks:
                    outputs += [os.path.join(od, sub, f"{im:06d}_{g:06d}.png") for sub in ("mask", "mask_visib")]
        plan.append((s, sd, od, gts, cams))
    target_path = os.path.join(os.path.dirname(out_root), f"test_targets_{targets}.json") if targets else None
    if target_path:
        outputs.append(target_path)
    refuse_existing(outputs, overwrite)

    meshes = {}
    for lid in sorted(obj_ids):
        path = os.path.join(models_dir, f"obj_{lid:06d}.ply")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path}: no model file for object {lid}")
        meshes[lid] = load_ply(path, geometry_only=True)
    sizes: Dict[Tuple[int, int], Tuple[int, int]] = {}
    paths: Dict[Tuple[int, int], str] = {}
    for s, sd, _, gts, cams in plan:
        for im in sorted(gts):
            paths[(s, im)] = _image_path(sd, im, depth_from_gt)
            W, H = sizes[(s, im)] = _image_size(paths[(s, im)])
            K = np.asarray(cams[im]["cam_K"], np.float64).reshape(3, 3)
            Kw = K.copy()
            Kw[0, 2] += W
            Kw[1, 2] += H
            for g, e in enumerate(gts[im]):
                if not prescreen(meshes[int(e["obj_id"])].vertices, np.linalg.inv(_m2c(e["cam_R_m2c"], e["cam_t_m2c"])), Kw):
                    raise ValueError(f"the GT pose of instance {g} (scene {s}, image {im}, object {int(e['obj_id'])}) puts a vertex within "
                                     f"{NEAR_LIMIT_MM} mm of the camera or beyond the rasterizer's range: it cannot be drawn")

    _lib.lib()
    if not torch.cuda.is_available():
        raise _lib.FoundPoseNativeError("gt_info runs on the MI355X only: no device is available and no CPU path exists")
    dev = torch.device(device)
    ras = HipRasterizer(device)
    for lid, m in meshes.items():
        ras.add_object_model(lid, mesh=m)
    timer = DeviceTimer()
    timed = timer.timed

    n_images = n_inst = n_low = 0
    all_inst: List[Tuple[int, int, int, float]] = []
    with ThreadPoolExecutor(max_workers=MAX_IO_WORKERS) as pool:
        for s, sd, od, gts, cams in plan:
            os.makedirs(od, exist_ok=True)
            if write_masks:
                for sub in ("mask", "mask_visib"):
                    os.makedirs(os.path.join(od, sub), exist_ok=True)
            ims = sorted(gts)
            info: Dict[int, List[Any]] = {im: [None] * len(gts[im]) for im in ims}
            pending = []
            for b0 in range(0, len(ims), IMAGE_BLOCK):
                block = ims[b0:b0 + IMAGE_BLOCK]
                if depth_from_gt:
                    depths = [None] * len(block)
                else:
                    depths = list(pool.map(lambda im: load_depth(paths[(s, im)], float(cams[im]["depth_scale"])), block))
                    for im, d in zip(block, depths):
                        if (d.shape[1], d.shape[0]) != sizes[(s, im)]:
                            raise ValueError(f"scene {s} image {im}: the depth image changed size while it was read")
                by_size = defaultdict(list)
                for im, d in zip(block, depths):
                    by_size[sizes[(s, im)]].append((im, d))
                for (W, H), group in by_size.items():
                    # ---- the group's frames and, per object, its instances with their shifted cameras
                    index = {im: n for n, (im, _) in enumerate(group)}
                    req = defaultdict(list)
                    for im, _ in group:
                        K = np.asarray(cams[im]["cam_K"], np.float64).reshape(3, 3)
                        Kw = K.copy()
                        Kw[0, 2] += W
                        Kw[1, 2] += H
                        for g, e in enumerate(gts[im]):
                            cam = _Camera(Kw, WINDOW_SCALE * W, WINDOW_SCALE * H, np.linalg.inv(_m2c(e["cam_R_m2c"], e["cam_t_m2c"])))
                            req[int(e["obj_id"])].append((im, g, K, cam))
                    step = chunk_views(W, H)
                    chunks = [(lid, rq[c0:c0 + step]) for lid, rq in sorted(req.items()) for c0 in range(0, len(rq), step)]
                    if depth_from_gt:   # a first pass of renders: the nearest surface of a frame's own instances is its depth
                        near = torch.full((len(group), H, W), float("inf"), dtype=torch.float32, device=dev)
                        for lid, chunk in chunks:
                            r = timed("render", ras.render_views, lid, [c for *_, c in chunk], with_color=False)
                            crop = r["depth"][:, H:2 * H, W:2 * W]
                            crop = torch.where(crop > 0, crop, torch.full_like(crop, float("inf")))
                            for b, (im, *_) in enumerate(chunk):   # in place, frame by frame: a chunk can hold a frame twice
                                torch.minimum(near[index[im]], crop[b], out=near[index[im]])
                            del r, crop
                        test = torch.where(torch.isinf(near), torch.zeros_like(near), near)
                        del near
                    else:
                        test = _lib.upload_async(torch.from_numpy(np.stack([d for _, d in group])), dev)
                    for lid, chunk in chunks:
                        r = timed("render", ras.render_views, lid, [c for *_, c in chunk], with_color=False)
                        boxes = r["boxes"].cpu().numpy()
                        inst = np.array([(index[im],) + scan_box(boxes[b]) + (W, H) for b, (im, *_) in enumerate(chunk)], np.int64)
                        par = np.array([(K[0, 0], K[1, 1], K[0, 2], K[1, 2], delta) for _, _, K, _ in chunk], np.float64)
                        rows, mask, mask_visib = timed("gt_visibility", ops.gt_visibility, test, r["depth"], inst, par)
                        rows = rows.cpu().numpy()
                        if write_masks:
                            mask, mask_visib = mask.cpu().numpy(), mask_visib.cpu().numpy()
                        for b, (im, g, _, _) in enumerate(chunk):
                            rec = info[im][g] = gt_record(rows[b])
                            all_inst.append((s, im, lid, rec["visib_fract"]))
                            n_low += rec["visib_fract"] < MIN_VISIB_FRACT
                            if write_masks:
                                name = f"{im:06d}_{g:06d}.png"
                                pending.append(pool.submit(_save_mask, os.path.join(od, "mask", name), mask[b]))
                                pending.append(pool.submit(_save_mask, os.path.join(od, "mask_visib", name), mask_visib[b]))
                        del r
                        if len(pending) >= 512:   # bounds the masks waiting for the encoders
                            for f in pending:
                                f.result()
                            pending = []
                    del test
            for f in pending:
                f.result()
            _dump_scene_json(os.path.join(od, "scene_gt_info.json"), {str(im): info[im] for im in ims})
            n_images += len(ims)
            n_inst += sum(len(gts[im]) for im in ims)
    if target_path:
        with open(target_path, "w") as f:
            json.dump(count_targets(all_inst, targets), f)
    dev_s = timer.seconds()
    return {"num_scenes": len(plan), "num_images": int(n_images), "num_instances": int(n_inst), "num_instances_below_min_visib": int(n_low),
            "min_visib_fract": MIN_VISIB_FRACT, "delta": delta, "dataset": dataset, "depth_from_gt": bool(depth_from_gt),
            "masks_written": bool(write_masks), "targets": target_path, "wall_seconds": time.perf_counter() - t_start,
            "device_seconds": {"render": dev_s.get("render", 0.0), "gt_visibility": dev_s.get("gt_visibility", 0.0)}}


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m foundpose_amd.gt_info", description=__doc__.split("\n\n")[0], epilog=NOT_PINNED)
    ap.add_argument("--dataset-dir", required=True, help="BOP split directory (<datasets>/<dataset>/<split>)")
    ap.add_argument("--models-dir", required=True, help="obj_XXXXXX.ply of the annotated objects")
    ap.add_argument("--dataset", default=None, help="dataset name (default: the name of <dataset-dir>'s parent)")
    ap.add_argument("--delta", type=float, default=None, help="visibility tolerance in mm (default: 5 for itodd, else 15)")
    ap.add_argument("--scenes", type=int, nargs="+", default=None, help="scene ids (default: every scene folder with a scene_gt.json)")
    ap.add_argument("--output-dir", default=None, help="mirror the scene folders here instead of writing into the split")
    ap.add_argument("--no-masks", action="store_true", help="write scene_gt_info.json only")
    ap.add_argument("--targets", default=None, choices=TARGET_KINDS, help="also write ../test_targets_<kind>.json")
    ap.add_argument("--depth-from-gt", action="store_true", help="RGB-only split: the frame depth is composed from the instance renders")
    ap.add_argument("--overwrite", action="store_true", help="replace existing output files")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    s = write_gt_info(a.dataset_dir, a.models_dir, a.dataset, a.delta, a.scenes, a.output_dir, not a.no_masks, a.targets, a.depth_from_gt,
                      a.overwrite, a.device)
    print(f"{s['num_scenes']} scene(s), {s['num_images']} image(s), {s['num_instances']} instance(s), {s['num_instances_below_min_visib']} below "
          f"visib_fract {MIN_VISIB_FRACT}; {s['wall_seconds']:.2f} s (device: renders {s['device_seconds']['render']:.3f} s, "
          f"fp_gt_visibility {s['device_seconds']['gt_visibility']:.3f} s)")
    print(NOT_PINNED)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
