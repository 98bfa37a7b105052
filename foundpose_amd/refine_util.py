"""Refinement of the best coarse pose on the MI355X: featuremetric, against the frame's depth (section 14), and on
both in one objective (section 15).

The FoundPose paper's third stage, which the released reference leaves as hooks only (scripts/infer.py:619, `final_pose_type`):
Levenberg-Marquardt on the 6-DoF pose that aligns the per-point features of the template behind the best coarse pose with the
query's projected patch-feature map.  One fp_featuremetric_refine call (csrc/refine.hip) refines a whole batch; the contract is
restated in numpy fp64 by tests/featuremetric_ref.py.  The depth term is this project's own: Levenberg-Marquardt on the truncated
quadratic of (measured depth at a template point's projection) - (the point's depth), in the frame's own camera; one
fp_depth_refine call (csrc/depth_refine.hip) per batch, restated by tests/depth_refine_ref.py.  The joint objective E_f + w_d E_d puts
both terms into one normal equation: one fp_rgbd_refine call (csrc/rgbd_refine.hip) per batch, restated by tests/rgbd_refine_ref.py.
"""

from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call, depth_refine_scratch_bytes, ptr, refine_scratch_bytes, require_cuda, rgbd_refine_scratch_bytes, stream, upload_async
from .bank import DeviceBank
from .matching import MatchResult
from .ops import _lm_inputs, _lm_outputs
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
