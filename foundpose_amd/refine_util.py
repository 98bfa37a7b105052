"""Refinement of the best coarse pose on the MI355X: featuremetric, against the frame's depth (section 14), and on
both in one objective (section 15).

The FoundPose paper's third stage, which the released reference leaves as hooks only (scripts/infer.py:619, `final_pose_type`):
Levenberg-Marquardt on the 6-DoF pose that aligns the per-point features of the template behind the best coarse pose with the
query's projected patch-feature map.  One fp_featuremetric_refine call (csrc/refine.hip) refines a whole batch; the contract is
restated in numpy fp64 by tests/featuremetric_ref.py.  The depth term is this project's own: Levenberg-Marquardt on the truncated
quadratic of (measured depth at a template point's projection) - (the point's depth), in the frame's own camera; one
fp_depth_refine call (csrc/depth_refine.hip) per batch, restated by tests/depth_refine_ref.py.  The joint objective E_f + w_d E_d puts
both terms into one normal equation: one fp_rgbd_refine call (csrc/rgbd_refine.hip) per batch, restated by tests/rgbd_refine_ref.py.
The silhouette refinement (section 38) needs no depth: Levenberg-Marquardt on the distance of the whole-model sample's projections to
the detection's mask and of the mask's contour pixels to their nearest projection, in the frame's own camera; fp_mask_distance and
fp_mask_refine (csrc/mask_refine.hip), restated by tests/mask_refine_ref.py.
"""

from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call, depth_refine_scratch_bytes, mask_refine_scratch_bytes, ptr, refine_scratch_bytes, require_cuda, rgbd_refine_scratch_bytes, stream, upload_async
from .bank import DeviceBank
from .matching import MatchResult
from .ops import _lm_inputs, _lm_outputs, mask_distance
from .pnp_util import _intrinsics

STATUS_REFINED, STATUS_NOT_IMPROVED, STATUS_SKIPPED = 0, 1, 2


def _map_shape(feature_map: torch.Tensor) -> Tuple[int, int, int, int]:
    if feature_map.dim() != 4:
        raise ValueError("feature_map must be [B, gh, gw, C]")
    B, gh, gw, C = feature_map.shape
    if gh < 2 or gw < 2:
        raise ValueError(f"the feature map is {gh} x {gw}: refinement needs at least 2 x 2 cells")
    return B, gh, gw, C


def _depth_stack(depth: torch.Tensor) -> torch.Tensor:
    if depth.dim() == 2:
        depth = depth[None]
    if depth.dim() != 3:
        raise ValueError("depth must be [N, H, W] or [H, W]")
    H, W = depth.shape[1:]
    if H < 2 or W < 2:
        raise ValueError(f"the depth image is {H} x {W}: refinement needs at least 2 x 2 pixels")
    return depth


def _tau_per_detection(tau, B: int) -> torch.Tensor:
    """tau, a number or one per detection -> [B] f64 on the host."""
    tau_h = torch.as_tensor(tau, dtype=torch.float64).reshape(-1).cpu()
    if tau_h.numel() == 1:
        tau_h = tau_h.expand(B)
    if tau_h.numel() != B:
        raise ValueError(f"{tau_h.numel()} tau values for {B} detections")
    return tau_h.contiguous()


def _upload_cameras(cameras: Sequence[Any], B: int, dev) -> torch.Tensor:
    return upload_async(torch.tensor([_intrinsics(c) for c in cameras], dtype=torch.float64).reshape(B, 4), dev)


def refine_featuremetric(feature_map: torch.Tensor, image_size: Tuple[int, int], cameras: Sequence[Any], R: torch.Tensor, t: torch.Tensor,
                         row_begin: torch.Tensor, row_end: torch.Tensor, feats: torch.Tensor, vertices: torch.Tensor, has_pose: torch.Tensor,
                         iters: int = 30, return_normal_equations: bool = False, max_points: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """feature_map [B, gh, gw, C] fp32 (any strides), image_size (W, H) of the camera the poses live in, cameras: one pinhole
    camera per detection (what pnp_util accepts), R [B, 3, 3] / t [B, 3] model -> camera (mm), row_begin / row_end [B] int:
    each detection's rows of feats [N, C] / vertices [N, 3], has_pose [B] bool.  max_points bounds row_end - row_begin (None:
    read back from the device).  -> dict of device tensors: R [B, 3, 3] f64, t [B, 3] f64, cost_in, cost_out [B] f64,
    num_points, iters_used, status [B] i32 (0 refined, 1 no step accepted, 2 skipped), + normal_eq [B, 28] f64 (H upper
    triangle row-major | g | E at the input pose) with return_normal_equations."""
    require_cuda(feature_map, R, t, row_begin, row_end, feats, vertices, has_pose)
    B, gh, gw, C = _map_shape(feature_map)
    if int(iters) < 0:
        raise ValueError("iters must be >= 0")
    if feats.dim() != 2 or feats.shape[1] != C or vertices.shape != (feats.shape[0], 3):
        raise ValueError(f"feats {tuple(feats.shape)} / vertices {tuple(vertices.shape)} do not match a C = {C} map")
    if len(cameras) != B:
        raise ValueError(f"{len(cameras)} cameras for {B} detections")
    dev = feature_map.device
    fmap = feature_map if feature_map.dtype == torch.float32 else feature_map.float()
    W, H = int(image_size[0]), int(image_size[1])
    cam = _upload_cameras(cameras, B, dev)
    Rin, tin, rb, re, hp, f32, v32, max_points = _lm_inputs(B, R, t, row_begin, row_end, has_pose, feats, vertices, max_points)
    scratch = torch.empty(refine_scratch_bytes(B, max_points), dtype=torch.uint8, device=dev)
    out, outs = _lm_outputs(B, dev, 28 if return_normal_equations else 0)
    sb, sy, sx, sc = fmap.stride()
    call("fp_featuremetric_refine", ptr(fmap), sb, sy, sx, sc, gh, gw, C, W, H, ptr(cam), ptr(Rin), ptr(tin), ptr(rb), ptr(re), ptr(f32), ptr(v32),
         int(f32.shape[0]), ptr(hp), B, max_points, int(iters), ptr(scratch), scratch.numel(), *outs, stream())
    return out


def best_template_rows(res: MatchResult, best: Dict[str, torch.Tensor], bank: DeviceBank, det_obj: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The bank rows of the template behind each detection's best coarse pose, on the device: global template
    g = tpl_base[object] + template_ids[b, corresp_id[b]] -> rows [tpl_off[g], tpl_off[g + 1]).  -> (row_begin, row_end,
    has_pose): has_pose is false where no coarse pose was found or the slot holds no template (id -1)."""
    dev = res.template_ids.device
    B = res.template_ids.shape[0]
    base = upload_async(torch.tensor([bank.objects[o].tpl_base for o in det_obj], dtype=torch.int64), dev)
    cid = best["corresp_id"].to(torch.int64).reshape(B, 1)
    tid = res.template_ids.gather(1, cid)[:, 0].to(torch.int64)
    ok = best["found"].bool() & (tid >= 0)
    g = torch.where(ok, base + tid, torch.zeros_like(tid))
    off = bank.tpl_off.to(torch.int64)
    return off[g].to(torch.int32), off[g + 1].to(torch.int32), ok


def refine_best_coarse(res: MatchResult, best: Dict[str, torch.Tensor], bank: DeviceBank, det_obj: Optional[Sequence[int]], cameras: Sequence[Any],
                       image_size: Tuple[int, int], iters: int = 30, return_normal_equations: bool = False) -> Dict[str, torch.Tensor]:
    """Refines pnp_util.select_best_coarse's pose of every detection of an infer_batch(..., keep_feature_map=True) result
    against that result's projected feature map.  cameras / image_size: the cameras PnP solved in (the crop cameras) and
    their image size (the crop size).  -> refine_featuremetric's dict."""
    if res.feature_map is None:
        raise ValueError("the MatchResult carries no feature map: run infer_batch(..., keep_feature_map=True)")
    res.wait()
    B = res.template_ids.shape[0]
    det_obj = [0] * B if det_obj is None else list(det_obj)
    rb, re, ok = best_template_rows(res, best, bank, det_obj)
    return refine_featuremetric(res.feature_map, image_size, cameras, best["R"], best["t"], rb, re, bank.feats, bank.vertices, ok, iters,
                                return_normal_equations, max_points=bank.p_max)


def refine_depth(depth: torch.Tensor, image_index: torch.Tensor, cameras: Sequence[Any], R: torch.Tensor, t: torch.Tensor, row_begin: torch.Tensor,
                 row_end: torch.Tensor, vertices: torch.Tensor, has_pose: torch.Tensor, tau, iters: int = 30, return_normal_equations: bool = False,
                 max_points: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """depth [N, H, W] (or [H, W]) fp32 mm, 0 = no measurement: the frames' full depth images; image_index [B] int: the image of each
    detection; cameras: the FRAME's pinhole camera per detection (what pnp_util accepts); R [B, 3, 3] / t [B, 3] model -> that camera
    (mm); row_begin / row_end [B] int: each detection's rows of vertices [N, 3]; has_pose [B] bool; tau: the truncation distance in mm,
    a number or one per detection.  max_points bounds row_end - row_begin (None: read back from the device).
    -> refine_featuremetric's dict; num_points counts the inliers at the input pose, cost = sum min(r^2, tau^2) / points."""
    require_cuda(depth, image_index, R, t, row_begin, row_end, vertices, has_pose)
    depth = _depth_stack(depth)
    N, H, W = depth.shape
    if int(iters) < 0:
        raise ValueError("iters must be >= 0")
    B = int(R.shape[0])
    if len(cameras) != B:
        raise ValueError(f"{len(cameras)} cameras for {B} detections")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices {tuple(vertices.shape)} are not [N, 3]")
    dev = depth.device
    tau_h = _tau_per_detection(tau, B)
    d32 = depth.float().contiguous()
    cam = _upload_cameras(cameras, B, dev)
    tau_d = upload_async(tau_h, dev)
    ii = image_index.to(torch.int32).contiguous()
    Rin, tin, rb, re, hp, _, v32, max_points = _lm_inputs(B, R, t, row_begin, row_end, has_pose, None, vertices, max_points)
    scratch = torch.empty(depth_refine_scratch_bytes(B, max_points), dtype=torch.uint8, device=dev)
    out, outs = _lm_outputs(B, dev, 28 if return_normal_equations else 0)
    call("fp_depth_refine", ptr(d32), N, H, W, ptr(ii), ptr(cam), ptr(Rin), ptr(tin), ptr(rb), ptr(re), ptr(v32), int(v32.shape[0]), ptr(hp), ptr(tau_d),
         B, max_points, int(iters), ptr(scratch), scratch.numel(), *outs, stream())
    return out


def _pose_matrices(R, t) -> np.ndarray:
    R = R.detach().cpu().numpy() if isinstance(R, torch.Tensor) else np.asarray(R)
    t = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    T = np.tile(np.eye(4), (len(R), 1, 1))
    T[:, :3, :3], T[:, :3, 3] = R.astype(np.float64).reshape(-1, 3, 3), t.astype(np.float64).reshape(-1, 3)
    return T


def _into_frame_cameras(pose: Dict[str, torch.Tensor], frame_cameras: Sequence[Any], solve_cameras: Sequence[Any], dev):
    """Moves pose["R"] / pose["t"] from solve_cameras into frame_cameras: inv(frame.T_world_from_eye) @ solve.T_world_from_eye @ T_m2c in
    fp64.  -> (R, t, back): back [B, 4, 4] is the inverse move, None where both cameras are the same object and nothing is converted."""
    if all(f is s for f, s in zip(frame_cameras, solve_cameras)):
        return pose["R"], pose["t"], None
    rel = np.stack([np.linalg.inv(np.asarray(f.T_world_from_eye, np.float64)) @ np.asarray(s.T_world_from_eye, np.float64)
                    for f, s in zip(frame_cameras, solve_cameras)])
    T = rel @ _pose_matrices(pose["R"], pose["t"])
    R, t = upload_async(torch.from_numpy(T[:, :3, :3].copy()), dev), upload_async(torch.from_numpy(T[:, :3, 3].copy()), dev)
    return R, t, np.linalg.inv(rel)


def _back_to_solve_cameras(out: Dict[str, torch.Tensor], pose: Dict[str, torch.Tensor], back: Optional[np.ndarray], dev) -> Dict[str, torch.Tensor]:
    """Moves a refiner's out["R"] / out["t"] back with _into_frame_cameras's `back`; poses whose status is not STATUS_REFINED did not move
    and keep the bits they came with in `pose`."""
    if back is not None:
        moved = (out["status"] == STATUS_REFINED).cpu().numpy()
        T = back @ _pose_matrices(out["R"], out["t"])
        T0 = _pose_matrices(pose["R"], pose["t"])
        T[~moved] = T0[~moved]
        out["R"], out["t"] = torch.from_numpy(T[:, :3, :3].copy()).to(dev), torch.from_numpy(T[:, :3, 3].copy()).to(dev)
    return out


def refine_best_coarse_depth(res: MatchResult, pose: Dict[str, torch.Tensor], bank: DeviceBank, det_obj: Optional[Sequence[int]],
                             frame_cameras: Sequence[Any], solve_cameras: Sequence[Any], depth: torch.Tensor, image_index, tau,
                             iters: int = 30) -> Dict[str, torch.Tensor]:
    """Refines a pose of every detection (pose: select_best_coarse's dict, its "R" / "t" possibly replaced by a featuremetric
    refinement's) against the frames' depth.  The poses live in solve_cameras (the cameras PnP solved in: the crop cameras); they are
    moved into frame_cameras (the frames' own), inv(frame.T_world_from_eye) @ solve.T_world_from_eye @ T_m2c in fp64, refined there
    on the unwarped depth [N, H, W] (image_index: the image of each detection), and moved back.  Where both cameras are the same
    object (crop=False) nothing is converted.  -> refine_depth's dict, R / t in the solve cameras."""
    res.wait()
    B = res.template_ids.shape[0]
    det_obj = [0] * B if det_obj is None else list(det_obj)
    rb, re, ok = best_template_rows(res, pose, bank, det_obj)
    dev = res.template_ids.device
    R, t, back = _into_frame_cameras(pose, frame_cameras, solve_cameras, dev)
    ii = image_index if isinstance(image_index, torch.Tensor) else upload_async(torch.tensor(list(image_index), dtype=torch.int32), dev)
    out = refine_depth(depth, ii, frame_cameras, R, t, rb, re, bank.vertices, ok, tau, iters, max_points=bank.p_max)
    return _back_to_solve_cameras(out, pose, back, dev)


def refine_rgbd(feature_map: torch.Tensor, image_size: Tuple[int, int], feature_cameras: Sequence[Any], A: torch.Tensor, a: torch.Tensor,
                depth: torch.Tensor, image_index: torch.Tensor, frame_cameras: Sequence[Any], R: torch.Tensor, t: torch.Tensor,
                row_begin: torch.Tensor, row_end: torch.Tensor, feats: torch.Tensor, vertices: torch.Tensor, has_pose: torch.Tensor, tau,
                depth_weight: float = 1.0, iters: int = 30, return_normal_equations: bool = False,
                max_points: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Features and depth in one Levenberg-Marquardt objective E_f + depth_weight E_d.  feature_map [B, gh, gw, C],
    image_size (W, H) and feature_cameras: refine_featuremetric's map arguments (the crop cameras); A [B, 3, 3] / a [B, 3] fp64: the rigid
    transform frame camera -> feature camera, X_f = A X_c + a; depth [N, Hd, Wd], image_index, frame_cameras, tau: refine_depth's;
    R [B, 3, 3] / t [B, 3]: model -> FRAME camera (mm); rows, feats, vertices, has_pose as in the two calls above.
    -> refine_depth's dict (num_points: the valid points of the feature term) + num_depth_inliers [B] i32, the depth inliers at the input
    pose; with return_normal_equations normal_eq [B, 57] f64: H_f | g_f | E_f, H_d | g_d | E_d, E at the input pose."""
    require_cuda(feature_map, A, a, depth, image_index, R, t, row_begin, row_end, feats, vertices, has_pose)
    B, gh, gw, C = _map_shape(feature_map)
    depth = _depth_stack(depth)
    N, Hd, Wd = depth.shape
    if int(iters) < 0:
        raise ValueError("iters must be >= 0")
    if not (float(depth_weight) >= 0.0 and float(depth_weight) < float("inf")):
        raise ValueError(f"depth_weight must be a finite number >= 0, got {depth_weight!r}")
    if feats.dim() != 2 or feats.shape[1] != C or vertices.shape != (feats.shape[0], 3):
        raise ValueError(f"feats {tuple(feats.shape)} / vertices {tuple(vertices.shape)} do not match a C = {C} map")
    if len(feature_cameras) != B or len(frame_cameras) != B:
        raise ValueError(f"{len(feature_cameras)} feature cameras and {len(frame_cameras)} frame cameras for {B} detections")
    if tuple(A.shape) != (B, 3, 3) or tuple(a.shape) != (B, 3):
        raise ValueError(f"A {tuple(A.shape)} / a {tuple(a.shape)} are not [{B}, 3, 3] / [{B}, 3]")
    dev = feature_map.device
    tau_h = _tau_per_detection(tau, B)
    fmap = feature_map if feature_map.dtype == torch.float32 else feature_map.float()
    W, H = int(image_size[0]), int(image_size[1])
    fcam = _upload_cameras(feature_cameras, B, dev)
    cam = _upload_cameras(frame_cameras, B, dev)
    tau_d = upload_async(tau_h, dev)
    Ain = A.to(torch.float64).reshape(B, 9).contiguous()
    ain = a.to(torch.float64).reshape(B, 3).contiguous()
    d32 = depth.float().contiguous()
    ii = image_index.to(torch.int32).contiguous()
    Rin, tin, rb, re, hp, f32, v32, max_points = _lm_inputs(B, R, t, row_begin, row_end, has_pose, feats, vertices, max_points)
    scratch = torch.empty(rgbd_refine_scratch_bytes(B, max_points), dtype=torch.uint8, device=dev)
    out, outs = _lm_outputs(B, dev, 57 if return_normal_equations else 0, depth_inliers=True)
    sb, sy, sx, sc = fmap.stride()
    call("fp_rgbd_refine", ptr(fmap), sb, sy, sx, sc, gh, gw, C, W, H, ptr(fcam), ptr(Ain), ptr(ain), ptr(d32), N, Hd, Wd, ptr(ii), ptr(cam), ptr(Rin),
         ptr(tin), ptr(rb), ptr(re), ptr(f32), ptr(v32), int(f32.shape[0]), ptr(hp), ptr(tau_d), float(depth_weight), B, max_points, int(iters),
         ptr(scratch), scratch.numel(), *outs, stream())
    return out


def refine_best_coarse_rgbd(res: MatchResult, best: Dict[str, torch.Tensor], bank: DeviceBank, det_obj: Optional[Sequence[int]],
                            frame_cameras: Sequence[Any], solve_cameras: Sequence[Any], image_size: Tuple[int, int], depth: torch.Tensor,
                            image_index, tau, depth_weight: float = 1.0, iters: int = 30) -> Dict[str, torch.Tensor]:
    """Refines select_best_coarse's pose of every detection of an infer_batch(..., keep_feature_map=True) result on that result's
    projected feature map and the frames' depth in one objective.  The poses live in solve_cameras (the crop cameras, image_size
    their size); they are moved into frame_cameras as in refine_best_coarse_depth, refined there -- the feature term reaches its crop
    camera through (A, a) = the inverse of that move -- and moved back.  Where both cameras are the same object (crop=False) nothing is
    converted and (A, a) is the identity.  -> refine_rgbd's dict, R / t in the solve cameras."""
    if res.feature_map is None:
        raise ValueError("the MatchResult carries no feature map: run infer_batch(..., keep_feature_map=True)")
    res.wait()
    B = res.template_ids.shape[0]
    det_obj = [0] * B if det_obj is None else list(det_obj)
    rb, re, ok = best_template_rows(res, best, bank, det_obj)
    dev = res.template_ids.device
    R, t, back = _into_frame_cameras(best, frame_cameras, solve_cameras, dev)
    Aa = np.tile(np.eye(4), (B, 1, 1)) if back is None else back   # frame camera -> feature camera: the inverse of that move
    A, a = upload_async(torch.from_numpy(Aa[:, :3, :3].copy()), dev), upload_async(torch.from_numpy(Aa[:, :3, 3].copy()), dev)
    ii = image_index if isinstance(image_index, torch.Tensor) else upload_async(torch.tensor(list(image_index), dtype=torch.int32), dev)
    out = refine_rgbd(res.feature_map, image_size, solve_cameras, A, a, depth, ii, frame_cameras, R, t, rb, re, bank.feats, bank.vertices, ok, tau,
                      depth_weight, iters, max_points=bank.p_max)
    return _back_to_solve_cameras(out, best, back, dev)


# ---------------------------------------------------------------------------------------------------- against the detection's mask (section 38)
def _check_masks(masks, who: str) -> None:
    if not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or masks.dim() != 3 or not masks.is_cuda:
        raise ValueError(f"{who}: masks must be a uint8 tensor [B, H, W] on the device, got "
                         f"{(masks.dtype, list(masks.shape), str(masks.device)) if isinstance(masks, torch.Tensor) else type(masks).__name__}")


def _check_count(name: str, v, lo: int, hi: Optional[int] = None) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{name} must be an integer {'>= ' + str(lo) if hi is None else 'in [' + str(lo) + ', ' + str(hi) + ']'}, got {v!r}")
    return v


def _check_huber(v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (np.isfinite(v) and v > 0):
        raise ValueError(f"huber_px must be a finite number > 0, got {v!r}")
    return float(v)


def mask_contours(masks: torch.Tensor, max_contour: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The contour pixels of masks uint8 [B, H, W] (non-zero = set): the set pixels with at least one of their four neighbours INSIDE the
    image unset -- a mask cut off by the image border has no contour there -- per mask in row-major order.  A mask with K > max_contour of
    them keeps the entries floor(j K / max_contour), j = 0 .. max_contour - 1.
    -> (rows int32 [sum K', 2] = (x, y), begin int32 [B], end int32 [B]) on the device.  Torch on the device, no per-mask loop.  The rule
    is evaluated per pixel -- a contour pixel's index l within its mask by a cumulative sum over the frame, kept iff K <= max_contour or
    l = floor(j K / max_contour) for the one j that can give it, j = ceil(l max_contour / K) -- so that the one nonzero() yields the kept
    rows already and is the only synchronisation; the price is a few int64 temporaries of the masks' size."""
    _check_masks(masks, "mask_contours")
    cap = _check_count("max_contour", max_contour, 1)
    m = masks != 0
    inner = torch.ones_like(m)   # "every neighbour inside the image is set"
    inner[:, 1:, :] &= m[:, :-1, :]
    inner[:, :-1, :] &= m[:, 1:, :]
    inner[:, :, 1:] &= m[:, :, :-1]
    inner[:, :, :-1] &= m[:, :, 1:]
    contour = (m & ~inner).flatten(1)                                 # [B, H W], row-major
    l = torch.cumsum(contour, 1, dtype=torch.int64) - 1               # on a contour pixel: its index among its mask's contour pixels
    K = l[:, -1:] + 1                                                 # [B, 1]
    j = (l * cap + (K - 1)) // torch.clamp(K, min=1)                  # 64-bit integers
    keep = contour & ((K <= cap) | ((j < cap) & ((j * K) // cap == l)))
    kept = keep.sum(1)
    end = torch.cumsum(kept, 0)
    begin = end - kept
    nz = torch.nonzero(keep.view_as(m))                               # [sum K', 3] = (b, y, x), sorted: row-major within a mask
    rows = nz[:, [2, 1]].to(torch.int32).contiguous()
    return rows, begin.to(torch.int32), end.to(torch.int32)


def refine_mask(d2: torch.Tensor, contour: torch.Tensor, contour_begin: torch.Tensor, contour_end: torch.Tensor, cameras: Sequence[Any],
                R: torch.Tensor, t: torch.Tensor, row_begin: torch.Tensor, row_end: torch.Tensor, vertices: torch.Tensor, has_pose: torch.Tensor,
                huber_px: float = 8.0, iters: int = 30, return_normal_equations: bool = False, max_points: Optional[int] = None,
                max_contour: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The raw call of the silhouette refinement (fp_mask_refine).  d2 int32 [B, H, W]: ops.mask_distance of each
    detection's mask in its FRAME camera's image; contour int32 [K_total, 2] with contour_begin / contour_end int [B]: mask_contours' rows;
    cameras: the frame's pinhole camera per detection; R [B, 3, 3] / t [B, 3] model -> that camera (mm); row_begin / row_end [B] int:
    each detection's rows of vertices [N, 3]; has_pose [B] bool; huber_px: the Huber delta in pixels.  max_points / max_contour bound
    row_end - row_begin / contour_end - contour_begin (None: read back from the device).
    -> refine_featuremetric's dict; num_points counts the measurable forward rows at the input pose."""
    require_cuda(d2, contour, contour_begin, contour_end, R, t, row_begin, row_end, vertices, has_pose)
    if d2.dtype != torch.int32 or d2.dim() != 3:
        raise ValueError(f"d2 must be int32 [B, H, W], got {d2.dtype} {tuple(d2.shape)}")
    B, H, W = (int(n) for n in d2.shape)
    delta = _check_huber(huber_px)
    _check_count("iters", iters, 0, 1000)
    if int(R.shape[0]) != B or len(cameras) != B or int(contour_begin.numel()) != B or int(contour_end.numel()) != B:
        raise ValueError(f"{int(R.shape[0])} poses, {len(cameras)} cameras and {int(contour_begin.numel())} contour ranges for {B} distance maps")
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices {tuple(vertices.shape)} are not [N, 3]")
    if contour.dim() != 2 or contour.shape[1] != 2:
        raise ValueError(f"contour {tuple(contour.shape)} is not [K, 2]")
    dev = d2.device
    cam = _upload_cameras(cameras, B, dev)
    d2c = d2.contiguous()
    rows = contour.to(torch.int32).contiguous()
    if rows.shape[0] == 0:
        rows = torch.zeros(1, 2, dtype=torch.int32, device=dev)   # a pointer the entry can take; no range reaches it
    cb, ce = contour_begin.to(torch.int32).contiguous(), contour_end.to(torch.int32).contiguous()
    if max_contour is None:
        max_contour = int((ce - cb).max().item())
    max_contour = max(1, int(max_contour))
    Rin, tin, rb, re, hp, _, v32, max_points = _lm_inputs(B, R, t, row_begin, row_end, has_pose, None, vertices, max_points)
    scratch = torch.empty(mask_refine_scratch_bytes(B, max_points, max_contour), dtype=torch.uint8, device=dev)
    out, outs = _lm_outputs(B, dev, 28 if return_normal_equations else 0)
    call("fp_mask_refine", ptr(d2c), H, W, ptr(rows), int(contour.shape[0]), ptr(cb), ptr(ce), ptr(cam), ptr(Rin), ptr(tin), ptr(rb), ptr(re), ptr(v32),
         int(v32.shape[0]), ptr(hp), delta, B, max_points, max_contour, int(iters), ptr(scratch), scratch.numel(), *outs, stream())
    return out


def refine_best_coarse_mask(pose: Dict[str, torch.Tensor], bank: DeviceBank, det_obj: Optional[Sequence[int]], frame_cameras: Sequence[Any],
                            solve_cameras: Sequence[Any], masks: torch.Tensor, huber_px: float = 8.0, iters: int = 30, max_points: int = 4096,
                            max_contour: int = 1024) -> Dict[str, torch.Tensor]:
    """Refines a pose of every detection (pose: select_best_coarse's dict, its "R" / "t" possibly replaced by a featuremetric
    refinement's) against the detection's own mask: masks uint8 [B, H, W] on the device, in the frame cameras' images.  The poses live
    in solve_cameras; they are moved into frame_cameras as in refine_best_coarse_depth, refined there on the whole-model sample
    bank.verify_points(max_points) against the mask's distance field and its contour (at most max_contour rows), and moved back; a pose
    that was not refined comes back bit for bit.  Masks of another type or shape, lengths that do not match and bad options raise
    ValueError before anything is launched; B = 0 returns empty tensors without a launch.  -> refine_mask's dict, R / t in the solve
    cameras."""
    _check_masks(masks, "refine_best_coarse_mask")
    delta = _check_huber(huber_px)
    _check_count("iters", iters, 0, 1000)
    _check_count("max_points", max_points, 1)
    _check_count("max_contour", max_contour, 1)
    B = int(masks.shape[0])
    det_obj = [0] * B if det_obj is None else list(det_obj)
    if len(det_obj) != B or len(frame_cameras) != B or len(solve_cameras) != B or int(pose["R"].shape[0]) != B or int(pose["found"].shape[0]) != B:
        raise ValueError(f"{len(det_obj)} objects, {len(frame_cameras)} frame cameras, {len(solve_cameras)} solve cameras and {int(pose['R'].shape[0])} poses "
                         f"for {B} masks")
    if any(isinstance(o, bool) or not 0 <= int(o) < len(bank.objects) for o in det_obj):
        raise ValueError(f"an object index outside [0, {len(bank.objects)})")
    H, W = int(masks.shape[1]), int(masks.shape[2])
    if B and not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise ValueError(f"masks of {W} x {H}: sides in [1, 16384]")
    dev = masks.device
    if B == 0:
        return _lm_outputs(0, dev, 0)[0]
    vp = bank.verify_points(max_points)
    rng = torch.tensor([vp.ranges[int(o)] for o in det_obj], dtype=torch.int32).reshape(B, 2)
    cap = max(1, int((rng[:, 1] - rng[:, 0]).max()))
    rng = upload_async(rng, dev)
    R, t, back = _into_frame_cameras(pose, frame_cameras, solve_cameras, dev)
    rows, cb, ce = mask_contours(masks, max_contour)
    out = refine_mask(mask_distance(masks), rows, cb, ce, frame_cameras, R, t, rng[:, 0], rng[:, 1], vp.points, pose["found"].bool(), delta, iters,
                      max_points=cap, max_contour=max_contour)
    return _back_to_solve_cameras(out, pose, back, dev)
