"""Result pictures of the inference driver (utils/vis_util.py:179-687 vis_inference_results in its default vis_for_paper
layout, with utils/vis_base_util.py and utils/render_vis_util.py) composited on the MI355X by csrc/vis.hip: only finished
uint8 tiles cross to the host.  The pixel contract is this project's own (tests/vis_ref.py restates
it): cv2, matplotlib and pyrender are not restated, so the pictures are not pixel-equal to the reference's.

  vis_inference_results_batch(...)   one tile per detection of a frame and object: pose contours | retrieved templates | matches
  vis_frame_summary(...)             the whole image with every final pose of the frame, mutual occlusion resolved
  pca_colorize, mask_tint, contour, resize_area, draw_matches, scene_composite   the kernels, on device tensors
"""

import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import projector_util
from ._lib import VIS_MAX_MATCHES, call, ptr, require_cuda, stream, upload_async, vp
from .crop_util import PinholePlaneCameraModel

COLOUR_GT, COLOUR_COARSE, COLOUR_FINAL = (255, 0, 0), (0, 0, 255), (0, 255, 0)   # drawn in this order: later ones win
MATCH_COLOUR, MATCH_ALPHA, MATCH_LW, MATCH_RADIUS = (230, 230, 230), 1.0, 1.0, 2.5
PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180),
           (70, 240, 240), (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 128, 128), (170, 110, 40))


def palette_colour(object_id: int) -> Tuple[int, int, int]:
    """The frame summary's colour of an object: a fixed 12-entry palette indexed by object id % 12."""
    return PALETTE[int(object_id) % len(PALETTE)]


def tile_path(output_dir: str, scene_id: int, im_id: int, object_lid: int, inst_id: int, hypothesis_id: int = 0) -> str:
    """scripts/infer.py:783-786: <output_dir>/<lid>/<scene>_<im>_<lid>_<inst>_<hypothesis>.png."""
    return os.path.join(output_dir, str(object_lid), f"{scene_id}_{im_id}_{object_lid}_{inst_id}_{hypothesis_id}.png")


def summary_path(output_dir: str, scene_id: int, im_id: int) -> str:
    return os.path.join(output_dir, "vis", f"{scene_id}_{im_id}.png")


def check_opts(opts) -> None:
    """Called before any device work when pictures are requested: the labelled layout is not built."""
    if not opts.vis_for_paper:
        raise NotImplementedError("vis_for_paper=False (text labels, the matplotlib figure) is not implemented; only the paper layout is")
    if not 1 <= int(opts.vis_corresp_top_n) <= VIS_MAX_MATCHES:
        raise ValueError(f"vis_corresp_top_n must lie in [1, {VIS_MAX_MATCHES}], got {opts.vis_corresp_top_n}")


# ---------------------------------------------------------------------------------------------------- kernels
def _u8(t: torch.Tensor, shape_tail) -> torch.Tensor:
    require_cuda(t)
    if t.dtype != torch.uint8 or tuple(t.shape[-len(shape_tail):]) != tuple(shape_tail):
        raise ValueError(f"expected uint8 [..., {', '.join(map(str, shape_tail))}], got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def pca_colorize(fmap: torch.Tensor, size_hw: Tuple[int, int], dim: Tuple[int, int] = (1, 1)) -> torch.Tensor:
    """fmap fp32 [B, gh, gw, C] -> uint8 [B, H, W, 3] (fp_vis_pca_colorize); dim = (9, 10) gives (9 v) // 10."""
    require_cuda(fmap)
    if fmap.dim() != 4 or fmap.dtype != torch.float32:
        raise ValueError(f"expected an fp32 [B, gh, gw, C] map, got {fmap.dtype} {tuple(fmap.shape)}")
    fmap = fmap.contiguous()
    B, gh, gw, C = fmap.shape
    H, W = int(size_hw[0]), int(size_hw[1])
    rng = torch.empty(B, 2, dtype=torch.float32, device=fmap.device)
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=fmap.device)
    call("fp_vis_pca_colorize", ptr(fmap), B, gh, gw, C, H, W, int(dim[0]), int(dim[1]), ptr(rng), ptr(out), stream())
    return out


def mask_tint(img: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """img uint8 [B, H, W, 3], mask uint8 [B, H, W] -> (img + 255) >> 1 where the mask is set (fp_vis_mask_tint)."""
    B, H, W = mask.shape
    img, mask = _u8(img, (H, W, 3)), _u8(mask, (H, W))
    out = torch.empty_like(img)
    call("fp_vis_mask_tint", ptr(img), ptr(mask), B, H, W, ptr(out), stream())
    return out


def contour(img: torch.Tensor, mask: torch.Tensor, colour: Sequence[int], dilate_iterations: int = 1) -> torch.Tensor:
    """Paints the dilated edge of mask uint8 [B, H, W] onto img uint8 [B, H, W, 3] IN PLACE (fp_vis_contour); returns img."""
    B, H, W = mask.shape
    mask = _u8(mask, (H, W))
    if _u8(img, (H, W, 3)).data_ptr() != img.data_ptr() or img.shape[0] != B:
        raise ValueError("img must be a contiguous uint8 [B, H, W, 3] tensor (it is painted in place)")
    call("fp_vis_contour", ptr(mask), B, H, W, int(dilate_iterations), int(colour[0]), int(colour[1]), int(colour[2]), ptr(img), stream())
    return img


def resize_area(src: torch.Tensor, out_hw: Tuple[int, int]) -> torch.Tensor:
    """src uint8 [B, h, w, 3] -> [B, h', w', 3], area-averaged; downscaling only (fp_vis_resize_area)."""
    B, h, w, _ = src.shape
    src = _u8(src, (h, w, 3))
    out = torch.empty(B, int(out_hw[0]), int(out_hw[1]), 3, dtype=torch.uint8, device=src.device)
    call("fp_vis_resize_area", ptr(src), B, h, w, int(out_hw[0]), int(out_hw[1]), ptr(out), stream())
    return out


def draw_matches(tile: torch.Tensor, segments: torch.Tensor, counts: torch.Tensor, colour: Sequence[float] = MATCH_COLOUR,
                 alpha: float = MATCH_ALPHA, lw: float = MATCH_LW, radius: float = MATCH_RADIUS) -> torch.Tensor:
    """Draws counts[b] of segments fp32 [B, N, 4] (x0, y0, x1, y1) with end discs onto tile uint8 [B, H, W2, 3] IN PLACE, in
    the given order (fp_vis_draw_matches); returns tile."""
    B, H, W2, _ = tile.shape
    require_cuda(segments, counts)
    if _u8(tile, (H, W2, 3)).data_ptr() != tile.data_ptr():
        raise ValueError("tile must be contiguous (it is drawn in place)")
    if segments.dtype != torch.float32 or segments.dim() != 3 or segments.shape[0] != B or segments.shape[2] != 4 or counts.shape != (B,):
        raise ValueError("segments must be fp32 [B, N, 4] and counts [B]")
    segments, counts = segments.contiguous(), counts.to(torch.int32).contiguous()
    col = np.asarray(colour, np.float32)
    call("fp_vis_draw_matches", ptr(segments), ptr(counts), B, int(segments.shape[1]), H, W2, col.ctypes.data_as(vp), float(alpha), float(lw),
         float(radius), ptr(tile), stream())
    return tile


def scene_composite(img: torch.Tensor, depth: torch.Tensor, colours: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """img uint8 [H, W, 3], depth fp32 [K, H, W] (mm, 0 = background), colours uint8 [K, 3] -> (picture, ids int32 [H, W])."""
    K, H, W = depth.shape
    require_cuda(depth)
    if depth.dtype != torch.float32:
        raise ValueError("depth must be fp32")
    img, colours, depth = _u8(img, (H, W, 3)), _u8(colours, (K, 3)), depth.contiguous()
    out = torch.empty_like(img)
    ids = torch.empty(H, W, dtype=torch.int32, device=img.device)
    call("fp_vis_scene_composite", ptr(depth), ptr(colours), K, H, W, ptr(img), ptr(out), ptr(ids), stream())
    return out, ids


# ---------------------------------------------------------------------------------------------------- poses -> masks
def _as_T(T) -> np.ndarray:
    T = np.asarray(T, np.float64)
    return np.vstack([T, [0.0, 0.0, 0.0, 1.0]]) if T.shape == (3, 4) else T


def _render_poses(rasterizer, obj_id: int, intrinsics: Sequence[Any], poses_m2c: Sequence[np.ndarray], notes: List[str],
                  labels: Sequence[str]) -> Tuple[Optional[Dict[str, torch.Tensor]], List[int]]:
    """ONE render_views call over every pose the rasterizer accepts -> (its outputs, the view index of each pose or -1).
    A pose it refuses (not finite, not rigid, a vertex within the near plane) is skipped with a note."""
    from .renderer import NEAR_PLANE_MM
    verts = rasterizer.objects[obj_id].mesh.vertices.astype(np.float64)
    cams, index = [], []
    for cam, T, label in zip(intrinsics, poses_m2c, labels):
        T = _as_T(T)
        ok = T.shape == (4, 4) and bool(np.all(np.isfinite(T)))
        if ok and not (verts @ T[2, :3] + T[2, 3]).min() > NEAR_PLANE_MM:
            ok = False
        if ok:
            try:
                cams.append(PinholePlaneCameraModel(cam.width, cam.height, cam.f, cam.c, np.linalg.inv(T)))
            except (ValueError, np.linalg.LinAlgError):
                ok = False
        if not ok:
            notes.append(f"{label}: pose refused by the rasterizer (not rigid, or within its near plane); contour skipped")
        index.append(len(cams) - 1 if ok else -1)
    if not cams:
        return None, index
    try:
        return rasterizer.render_views(obj_id, cams, with_color=False), index
    except ValueError as e:   # (a projection beyond the fixed-point range: the whole call is refused)
        notes.append(f"rasterizer refused the batch ({e}); contours skipped")
        return None, [-1] * len(index)


def _select_masks(render: Optional[Dict[str, torch.Tensor]], index: Sequence[int], H: int, W: int, device) -> torch.Tensor:
    """uint8 [len(index), H, W]: the view's mask, zeros for a skipped pose."""
    out = torch.zeros(len(index), H, W, dtype=torch.uint8, device=device)
    if render is not None:
        have = [i for i, v in enumerate(index) if v >= 0]
        if have:
            out[torch.tensor(have, device=device)] = render["mask"][torch.tensor([index[i] for i in have], device=device)]
    return out


# ---------------------------------------------------------------------------------------------------- the per-detection tile
def _to_u8_hwc(images: torch.Tensor) -> torch.Tensor:
    """uint8 [B, H, W, 3] from uint8 HWC or float CHW in [0, 1] (the crop producer's layout): floor(255 x + 1/2)."""
    if images.dtype == torch.uint8:
        return images.contiguous()
    return (images.permute(0, 2, 3, 1) * 255.0 + 0.5).clamp_(0.0, 255.0).to(torch.uint8).contiguous()


def _same_projector(a, b) -> bool:
    if a is b:
        return True
    return (isinstance(a, projector_util.PCAProjector) and isinstance(b, projector_util.PCAProjector)
            and a.components.shape == b.components.shape and torch.equal(a.components.cpu(), b.components.cpu())
            and torch.equal(a.mean.cpu(), b.mean.cpu()))


def _nearest_resize(img: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """uint8 [B, h, w, 3] -> [B, H, W, 3], source index floor(dst * size_src / size_dst)."""
    h, w = img.shape[1:3]
    if (h, w) == (H, W):
        return img
    ys = (torch.arange(H, device=img.device) * h) // H
    xs = (torch.arange(W, device=img.device) * w) // W
    return img[:, ys][:, :, xs].contiguous()


def select_matches(conf: torch.Tensor, counts: torch.Tensor, left: torch.Tensor, right: torch.Tensor, top_n: int, W: int, H: int
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """conf [B, K], counts [B], left / right [B, K, 2] (right already in the W x H picture) -> segments fp32 [B, top_n, 4],
    kept [B]: the top_n valid correspondences by confidence (stable, descending, ties to the lower index; NaN ranks last),
    those whose right point lies in [0, W) x [0, H), least confident first, the right point shifted by (W, 0)."""
    B, K = conf.shape
    n = min(int(top_n), K)
    valid = torch.arange(K, device=conf.device)[None, :] < counts[:, None]
    key = torch.where(valid & ~torch.isnan(conf), conf, torch.full_like(conf, float("-inf")))
    order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :n].flip(1)         # least confident first
    l, r = left.gather(1, order[..., None].expand(-1, -1, 2)), right.gather(1, order[..., None].expand(-1, -1, 2))
    keep = valid.gather(1, order) & (r[..., 0] >= 0) & (r[..., 0] < W) & (r[..., 1] >= 0) & (r[..., 1] < H)
    front = torch.sort((~keep).to(torch.int8), dim=1, stable=True).indices                       # kept ones first, order preserved
    seg = torch.cat([l, r[..., :1] + float(W), r[..., 1:]], dim=2).gather(1, front[..., None].expand(-1, -1, 4))
    return seg.to(torch.float32).contiguous(), keep.sum(1).to(torch.int32)


def vis_inference_results_batch(crops: torch.Tensor, crop_masks: torch.Tensor, cameras: Sequence[Any], res, found: Sequence[bool],
                                corresp_id: Sequence[int], poses_coarse: Sequence[np.ndarray], poses_final: Sequence[np.ndarray],
                                repre, rasterizer, object_id: int, extractor=None, poses_gt: Optional[Sequence[Optional[np.ndarray]]] = None,
                                draw_coarse: bool = False, vis_corresp_top_n: int = 100, vis_feat_map: bool = True,
                                vis_for_paper: bool = True, templates: Optional[torch.Tensor] = None
                                ) -> Tuple[torch.Tensor, List[Dict[str, Any]]]:
    """The paper layout for the B detections of one frame and object, as one uint8 [B, H + h2 + H, 2W, 3] device tensor, and
    one record per detection ({"found", "template_ids", "num_matches", "notes"}).
      row 1  the crop with the modal mask tinted | the crop with the contours of the ground-truth (red), best coarse (blue,
             with draw_coarse: when the final pose is a refined one) and final (green) pose, rendered in the crop camera
      row 2  the retrieved templates side by side, area-resized to 2W wide
      row 3  (9 q) // 10 of the query's PCA picture | the best template's, with the vis_corresp_top_n most confident matches
             (vis_feat_map=False: the crop | the template image)
    crops: float [B, 3, H, W] in [0, 1] or uint8 [B, H, W, 3]; crop_masks uint8 [B, H, W]; cameras: the crop cameras; res: the
    MatchResult of infer_batch(..., keep_feature_map=True); poses: 4x4 (or 3x4) model -> crop camera, ignored where not found;
    templates: repre.templates on the device (uploaded here when absent).  A detection without a pose gets its pictures
    without contours; its slot 0 stands in for the best template."""
    if not vis_for_paper:
        raise NotImplementedError("vis_for_paper=False (text labels, the matplotlib figure) is not implemented; only the paper layout is")
    if not 1 <= int(vis_corresp_top_n) <= VIS_MAX_MATCHES:
        raise ValueError(f"vis_corresp_top_n must lie in [1, {VIS_MAX_MATCHES}]")
    res.wait()
    dev = crop_masks.device
    img = _to_u8_hwc(crops)
    B, H, W, _ = img.shape
    records = [{"found": bool(found[b]), "notes": []} for b in range(B)]

    # ---- row 1
    left1 = mask_tint(img, (crop_masks != 0).to(torch.uint8))
    right1 = img.clone()
    kinds = ([("gt", COLOUR_GT, poses_gt)] if poses_gt is not None else []) + ([("coarse", COLOUR_COARSE, poses_coarse)] if draw_coarse else []) \
        + [("final", COLOUR_FINAL, poses_final)]
    views = [(k, b) for k, (_, _, poses) in enumerate(kinds) for b in range(B) if found[b] and poses[b] is not None]
    notes: List[str] = []
    render, index = _render_poses(rasterizer, object_id, [cameras[b] for _, b in views], [kinds[k][2][b] for k, b in views], notes,
                                  [f"{kinds[k][0]} pose of detection {b}" for k, b in views])
    for note in notes:
        for b in range(B):
            if note.endswith("contours skipped") or f"detection {b}:" in note:
                records[b]["notes"].append(note)
    for k, (_, colour, _) in enumerate(kinds):
        sel = [i for i, (kk, _) in enumerate(views) if kk == k]
        if not sel:
            continue
        masks = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
        masks[torch.tensor([views[i][1] for i in sel], device=dev)] = _select_masks(render, [index[i] for i in sel], H, W, dev)
        contour(right1, masks, colour)
    row1 = torch.cat([left1, right1], dim=2)

    # ---- row 2
    tpl = templates if templates is not None else repre.templates.to(dev)              # [T, 3, Ht, Wt] uint8
    Ht, Wt = int(tpl.shape[2]), int(tpl.shape[3])
    tids = res.template_ids.to(torch.int64)                                             # [B, n]
    n = int(tids.shape[1])
    strip = tpl[tids.clamp_min(0)] * (tids >= 0)[:, :, None, None, None].to(torch.uint8)   # a missing template: black
    strip = strip.permute(0, 3, 1, 4, 2).reshape(B, Ht, n * Wt, 3)                      # side by side, HWC
    h2 = int(Ht * 2 * W / (n * Wt))
    up = max(1, -(-2 * W // (n * Wt)), -(-h2 // Ht))                                    # a strip smaller than its row: replicate pixels first,
    if up > 1:                                                                          # so that the area resize only ever shrinks
        strip = strip.repeat_interleave(up, dim=1).repeat_interleave(up, dim=2)
    row2 = resize_area(strip.contiguous(), (max(h2, 1), 2 * W))

    # ---- row 3
    cid = torch.as_tensor([int(c) if f else 0 for c, f in zip(corresp_id, found)], device=dev, dtype=torch.int64)
    ar = torch.arange(B, device=dev)
    best_tid = tids[ar, cid].clamp_min(0)
    best_tpl = tpl[best_tid]                                                            # [B, 3, Ht, Wt]
    if vis_feat_map:
        if extractor is None:
            raise ValueError("vis_feat_map=True needs the extractor (the best templates go through it in one batch)")
        vis_proj = list(repre.feat_vis_projectors)
        if not vis_proj:
            raise ValueError("the object representation has no feat_vis_projectors")
        raw = list(repre.feat_raw_projectors)
        if res.feature_map is not None and len(raw) == 1 and len(vis_proj) == 1 and _same_projector(vis_proj[0], raw[0]):
            qmap = res.feature_map                                                      # the engine's projected map: channels 0..2
        else:
            qmap = _projected_map(extractor, crops if crops.dtype != torch.uint8 else crops.permute(0, 3, 1, 2).float() / 255.0, vis_proj)
        left3 = pca_colorize(qmap, (H, W), dim=(9, 10))
        tmap = _projected_map(extractor, best_tpl.to(torch.float32) / 255.0, vis_proj)
        right3 = _nearest_resize(pca_colorize(tmap, (Ht, Wt)), H, W)
    else:
        left3, right3 = img, _nearest_resize(best_tpl.permute(0, 2, 3, 1).contiguous(), H, W)
    cam_tab = _template_camera_table(repre, dev)                                        # [T, 16]: f, c, R (model -> camera), t
    c = cam_tab[best_tid]
    X = res.coord_3d[ar, cid].to(torch.float64)                                         # [B, K, 3] = vertices[nn_vertex_ids]
    Xc = X @ c[:, 4:13].reshape(B, 3, 3).transpose(1, 2) + c[:, None, 13:16]
    uv = Xc[..., :2] / Xc[..., 2:] * c[:, None, 0:2] + c[:, None, 2:4]
    uv = torch.where(Xc[..., 2:] > 0, uv, torch.full_like(uv, -1.0)) * torch.tensor([W / Wt, H / Ht], dtype=torch.float64, device=dev)
    segs, kept = select_matches(res.conf[ar, cid], res.counts[ar, cid], res.coord_2d[ar, cid].to(torch.float64), uv, vis_corresp_top_n, W, H)
    row3 = draw_matches(torch.cat([left3, right3], dim=2), segs, kept)

    kept_host, tid_host = kept.cpu().tolist(), res.template_ids.cpu().tolist()
    for b in range(B):
        records[b]["num_matches"], records[b]["template_ids"] = kept_host[b], tid_host[b]
    return torch.cat([row1, row2, row3], dim=1), records


def _projected_map(extractor, images: torch.Tensor, projectors) -> torch.Tensor:
    """float [B, 3, H, W] -> the extractor's patch features through `projectors`, fp32 [B, gh, gw, C]."""
    fm = extractor(images.contiguous())["feature_maps"]                                 # [B, D, gh, gw], a view of [B, gh, gw, D]
    B, D, gh, gw = fm.shape
    flat = fm.permute(0, 2, 3, 1).reshape(-1, D).to(torch.float32).contiguous()
    return projector_util.project_features(flat, projectors).reshape(B, gh, gw, -1).contiguous()


def _template_camera_table(repre, device) -> torch.Tensor:
    cams = repre.template_cameras_cam_from_model
    if not len(cams):
        raise ValueError("the object representation has no template cameras: the matches cannot be drawn")
    tab = np.empty((len(cams), 16), np.float64)
    for i, cam in enumerate(cams):
        get = (lambda k: cam[k]) if isinstance(cam, dict) else (lambda k: getattr(cam, k))
        T = np.linalg.inv(np.asarray(torch.as_tensor(get("T_world_from_eye")).cpu().numpy(), np.float64))
        tab[i, 0:2], tab[i, 2:4] = np.asarray(torch.as_tensor(get("f")).cpu().numpy(), np.float64), np.asarray(torch.as_tensor(get("c")).cpu().numpy(), np.float64)
        tab[i, 4:13], tab[i, 13:16] = T[:3, :3].reshape(-1), T[:3, 3]
    return upload_async(torch.from_numpy(tab), device)


# ---------------------------------------------------------------------------------------------------- the frame summary
def vis_frame_summary(image, camera, poses: Sequence[Tuple[int, np.ndarray, Optional[Sequence[int]]]], rasterizer
                      ) -> Tuple[torch.Tensor, torch.Tensor, List[str]]:
    """The whole image with every final pose of a frame: `poses` = [(object id, T_m2c in `camera`, colour or None)]; colour
    None = palette_colour(object id).  Each pose is rendered on its own (one render_views call per object), the layers are
    merged by fp_vis_scene_composite (nearest surface wins), then every visible silhouette gets its contour in its colour.
    -> (picture uint8 [H, W, 3], ids int32 [H, W]: the index into `poses` per pixel, -1 background, notes)."""
    dev = rasterizer.device
    img = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    if img.dtype != torch.uint8:
        img = (img.to(torch.float32) * 255.0 + 0.5).clamp(0.0, 255.0).to(torch.uint8)
    img = img.to(dev).contiguous()
    H, W = int(img.shape[0]), int(img.shape[1])
    notes: List[str] = []
    K = len(poses)
    if K == 0:
        return img.clone(), torch.full((H, W), -1, dtype=torch.int32, device=dev), notes
    depth = torch.zeros(K, H, W, dtype=torch.float32, device=dev)
    for obj_id in sorted({int(p[0]) for p in poses}):
        sel = [k for k, p in enumerate(poses) if int(p[0]) == obj_id]
        render, index = _render_poses(rasterizer, obj_id, [camera] * len(sel), [poses[k][1] for k in sel], notes,
                                      [f"object {obj_id}, pose {k}" for k in sel])
        if render is not None:
            for k, v in zip(sel, index):
                if v >= 0:
                    depth[k] = render["depth"][v]
    colours = torch.tensor([list(p[2]) if p[2] is not None else list(palette_colour(p[0])) for p in poses], dtype=torch.uint8)
    out, ids = scene_composite(img, depth, upload_async(colours, dev))
    pic = out[None]
    for k in range(K):
        contour(pic, (ids == k).to(torch.uint8)[None], colours[k].tolist())
    return pic[0], ids, notes


# ---------------------------------------------------------------------------------------------------- host side
def tiles_to_host(tiles: torch.Tensor) -> np.ndarray:
    """One device -> pinned host copy for the whole batch."""
    host = torch.empty(tiles.shape, dtype=tiles.dtype, pin_memory=True)
    host.copy_(tiles, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return host.numpy()


def write_png(path: str, picture: np.ndarray) -> None:
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(np.ascontiguousarray(picture, np.uint8)).save(path)
