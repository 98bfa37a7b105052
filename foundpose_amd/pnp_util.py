"""Pose from 2D-3D correspondences with the reference's interface (/root/reference/utils/pnp_util.py:20-84: cv2.solvePnPRansac +
optional cv2.solvePnPRefineLM), run on the MI355X for a whole batch of (detection, template) pairs at once, and the
best-coarse-pose selection of /root/reference/scripts/infer.py:552-602.

cv2 is not a dependency of this path (and is absent from the image): the scheme is OpenCV's -- RANSAC over minimal
samples, inlier = reprojection error <= threshold, best = first model with the most inliers within the adaptively
shortened budget, Levenberg-Marquardt on the inliers -- with a P3P minimal solver and a counter-based sampler
(csrc/pnp.hip).  cv2's random stream is not reproduced, so individual hypotheses differ; the estimate agrees wherever the
inlier set is unambiguous (parity of cv2's own arithmetic: unpinned).
"""

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call, ptr, stream, require_cuda, upload_async
from .matching import MatchResult

MIN_CORRESP = 6  # scripts/infer.py:555-559


def _intrinsics(camera) -> Tuple[float, float, float, float]:
    """(fx, fy, cx, cy) of a pinhole camera: an object or dict with f / c (the reference's PinholePlaneCameraModel), a 3x3 K,
    or the four numbers themselves."""
    if isinstance(camera, dict):
        f, c = camera["f"], camera["c"]
    elif hasattr(camera, "f") and hasattr(camera, "c"):
        f, c = camera.f, camera.c
    else:
        K = np.asarray(camera, np.float64)
        if K.shape == (4,):
            return float(K[0]), float(K[1]), float(K[2]), float(K[3])
        return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    f, c = np.asarray(f, np.float64).reshape(-1), np.asarray(c, np.float64).reshape(-1)
    return float(f[0]), float(f[1]), float(c[0]), float(c[1])


def solve_pnp_ransac_batch(coord_2d: torch.Tensor, coord_3d: torch.Tensor, counts: torch.Tensor, cameras: Sequence[Any],
                           pnp_ransac_iter: int = 1000, pnp_inlier_thresh: float = 3.0, pnp_required_ransac_conf: float = 0.99,
                           pnp_refine_lm: bool = True, seed: int = 0, return_ransac_pose: bool = False,
                           min_corresp: int = 6, pair_keys=None) -> Dict[str, torch.Tensor]:
    """coord_2d [B, n, K, 2], coord_3d [B, n, K, 3], counts [B, n] (MatchResult's padded layout); cameras: one per detection.
    -> dict of device tensors: success [B, n] bool, R [B, n, 3, 3] f64, t [B, n, 3] f64, quality [B, n] (RANSAC inliers),
    inliers [B, n, K] bool (+ ransac_pose [B, n, 12]).  min_corresp: sets with fewer correspondences fail without being tried --
    6 in the driver's loop (scripts/infer.py:555-559), 4 for a bare estimate_pose call (what cv2.solvePnPRansac needs).
    pair_keys: [B, n] int64 tensor or nested sequence, the sampler key of every pair (fp_pnp_ransac_keyed): a pair's hypotheses then depend on
    (seed, its key) and not on where it sits in this batch.  None: the pair's index b * n + j (fp_pnp_ransac)."""
    require_cuda(coord_2d, coord_3d, counts)
    B, n, K = coord_2d.shape[:3]
    dev = coord_2d.device
    if len(cameras) != B:
        raise ValueError(f"{len(cameras)} cameras for {B} detections")
    cam = upload_async(torch.tensor([_intrinsics(c) for c in cameras], dtype=torch.float64).reshape(B, 4), dev)   # (a pageable upload would block until the batch has drained)
    c2, c3 = coord_2d.float().contiguous(), coord_3d.float().contiguous()
    cnt = counts.to(torch.int32).contiguous()
    P = B * n
    success = torch.zeros(P, dtype=torch.int32, device=dev)
    R = torch.zeros(P, 9, dtype=torch.float64, device=dev)
    t = torch.zeros(P, 3, dtype=torch.float64, device=dev)
    ninl = torch.zeros(P, dtype=torch.int32, device=dev)
    mask = torch.zeros(P, K, dtype=torch.uint8, device=dev)
    rp = torch.zeros(P, 12, dtype=torch.float64, device=dev) if return_ransac_pose else None
    lm_iters = 20 + (20 if pnp_refine_lm else 0)
    keys = _pair_keys_tensor(pair_keys, B, n, dev)
    entry, key_arg = ("fp_pnp_ransac", ()) if keys is None else ("fp_pnp_ransac_keyed", (ptr(keys),))
    call(entry, ptr(c2), ptr(c3), ptr(cnt), ptr(cam), *key_arg, P, n, K, int(pnp_ransac_iter), float(pnp_inlier_thresh),
         float(pnp_required_ransac_conf), lm_iters, int(min_corresp), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(success), ptr(R), ptr(t), ptr(ninl), ptr(mask), ptr(rp), stream())
    out = {"success": success.reshape(B, n).bool(), "R": R.reshape(B, n, 3, 3), "t": t.reshape(B, n, 3),
           "quality": ninl.reshape(B, n).to(torch.float64), "inliers": mask.reshape(B, n, K).bool()}
    if rp is not None:
        out["ransac_pose"] = rp.reshape(B, n, 12)
    return out


PNP_TYPES = ("opencv", "kabsch_depth")


def _pair_keys_tensor(pair_keys, B: int, n: int, dev):
    if pair_keys is None:
        return None
    if isinstance(pair_keys, torch.Tensor):
        if pair_keys.dtype != torch.int64:
            raise ValueError(f"pair_keys must be int64, got {pair_keys.dtype}")
    else:
        pair_keys = torch.tensor(pair_keys, dtype=torch.int64)
    if tuple(pair_keys.shape) != (B, n):
        raise ValueError(f"pair_keys must have shape [{B}, {n}], got {list(pair_keys.shape)}")
    return pair_keys.contiguous() if pair_keys.is_cuda else upload_async(pair_keys, dev)   # (the int64 bits are the uint64 keys)


def solve_to_frame_rotations(solve_cameras: Sequence[Any], frame_cameras: Sequence[Any], what: str = "kabsch_depth") -> np.ndarray:
    """A [B, 3, 3] fp64: the rotation solve camera -> frame camera of every detection, from rel = inv(frame.T_world_from_eye) @
    solve.T_world_from_eye.  The crop camera looks at its box from the frame camera's own position, so rel has no translation; one whose
    translation exceeds 1e-6 (1 + |eye position|) is refused (a depth pixel then could not be found from a ray alone).  The same camera
    object on both sides (crop=False) gives the identity.  what: the stage the refusal names."""
    A = np.empty((len(solve_cameras), 3, 3), np.float64)
    for i, (s, f) in enumerate(zip(solve_cameras, frame_cameras)):
        if s is f:
            A[i] = np.eye(3)
            continue
        Tf, Ts = np.asarray(f.T_world_from_eye, np.float64), np.asarray(s.T_world_from_eye, np.float64)
        rel = np.linalg.inv(Tf) @ Ts
        off, bound = float(np.linalg.norm(rel[:3, 3])), 1e-6 * (1.0 + float(np.linalg.norm(Tf[:3, 3])))
        if not off <= bound:
            raise ValueError(f"detection {i}: the solve camera's centre is {off:.3g} away from the frame camera's (more than {bound:.3g}): "
                             f"{what} needs cameras that share their centre")
        A[i] = rel[:3, :3]
    return A


def solve_kabsch_ransac_batch(coord_2d: torch.Tensor, coord_3d: torch.Tensor, counts: torch.Tensor, solve_cameras: Sequence[Any],
                              frame_cameras: Sequence[Any], depth: torch.Tensor, image_index, inlier_thresh_mm, ransac_iter: int = 1000,
                              required_conf: float = 0.99, refit: bool = True, seed: int = 0, return_ransac_pose: bool = False,
                              min_corresp: int = 6, pair_keys=None) -> Dict[str, torch.Tensor]:
    """Coarse poses from depth-lifted correspondences: 3D-3D RANSAC + Horn's closed-form refit (csrc/kabsch.hip).
    coord_2d / coord_3d / counts / pair_keys / min_corresp: as in solve_pnp_ransac_batch, the pixels in solve_cameras (one per detection);
    frame_cameras: the frames' own cameras (the same objects with crop=False); depth [N, H, W] fp32 mm on the device, 0 = no measurement;
    image_index: B host integers, the image of each detection; inlier_thresh_mm: one number or one per detection (> 0).
    -> solve_pnp_ransac_batch's dict (poses model -> solve camera, quality = 3D inliers) + num_valid [B, n], the correspondences that
    found a depth measurement.  A bad image index, threshold or camera pair raises ValueError before anything is launched."""
    require_cuda(coord_2d, coord_3d, counts, depth)
    B, n, K = coord_2d.shape[:3]
    dev = coord_2d.device
    if len(solve_cameras) != B or len(frame_cameras) != B:
        raise ValueError(f"{len(solve_cameras)} solve cameras and {len(frame_cameras)} frame cameras for {B} detections")
    if depth.dim() != 3 or depth.dtype != torch.float32:
        raise ValueError(f"depth must be a float32 stack [N, H, W], got {depth.dtype} {list(depth.shape)}")
    N, H, W = (int(s) for s in depth.shape)
    if isinstance(image_index, torch.Tensor):
        image_index = image_index.cpu().tolist()
    ii = [int(i) for i in image_index]
    if len(ii) != B:
        raise ValueError(f"{len(ii)} image indices for {B} detections")
    for b, i in enumerate(ii):
        if not 0 <= i < N:
            raise ValueError(f"detection {b}: image index {i} outside [0, {N})")
    tau = np.broadcast_to(np.asarray(inlier_thresh_mm, np.float64), (B,)) if np.ndim(inlier_thresh_mm) == 0 else np.asarray(inlier_thresh_mm, np.float64).reshape(-1)
    if tau.shape != (B,) or not np.all(tau > 0) or not np.all(np.isfinite(tau)):
        raise ValueError(f"inlier_thresh_mm must be one finite number > 0 or {B} of them, got {inlier_thresh_mm!r}")
    A = solve_to_frame_rotations(solve_cameras, frame_cameras)
    table = torch.cat([torch.tensor([_intrinsics(c) for c in solve_cameras], dtype=torch.float64).reshape(B, 4),
                       torch.tensor([_intrinsics(c) for c in frame_cameras], dtype=torch.float64).reshape(B, 4),
                       torch.from_numpy(A.reshape(B, 9)), torch.from_numpy(np.ascontiguousarray(tau)).reshape(B, 1)], dim=1)   # [B, 18]: one upload
    table = upload_async(table, dev)
    cam, fcam, Ad, taud = table[:, :4].contiguous(), table[:, 4:8].contiguous(), table[:, 8:17].contiguous(), table[:, 17].contiguous()
    iid = upload_async(torch.tensor(ii, dtype=torch.int32), dev)
    keys = _pair_keys_tensor(pair_keys, B, n, dev)
    c2, c3 = coord_2d.float().contiguous(), coord_3d.float().contiguous()
    cnt = counts.to(torch.int32).contiguous()
    dimg = depth.contiguous()
    P = B * n
    success = torch.zeros(P, dtype=torch.int32, device=dev)
    R = torch.zeros(P, 9, dtype=torch.float64, device=dev)
    t = torch.zeros(P, 3, dtype=torch.float64, device=dev)
    ninl = torch.zeros(P, dtype=torch.int32, device=dev)
    nval = torch.zeros(P, dtype=torch.int32, device=dev)
    mask = torch.zeros(P, K, dtype=torch.uint8, device=dev)
    rp = torch.zeros(P, 12, dtype=torch.float64, device=dev) if return_ransac_pose else None
    call("fp_kabsch_ransac", ptr(c2), ptr(c3), ptr(cnt), ptr(cam), ptr(fcam), ptr(Ad), ptr(iid), ptr(taud), ptr(dimg), N, H, W, ptr(keys), P, n, K,
         int(ransac_iter), float(required_conf), int(bool(refit)), int(min_corresp), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(success), ptr(R), ptr(t),
         ptr(ninl), ptr(nval), ptr(mask), ptr(rp), stream())
    out = {"success": (success.reshape(B, n) > 0), "R": R.reshape(B, n, 3, 3), "t": t.reshape(B, n, 3),
           "quality": ninl.reshape(B, n).to(torch.float64), "inliers": mask.reshape(B, n, K).bool(), "num_valid": nval.reshape(B, n)}
    if rp is not None:
        out["ransac_pose"] = rp.reshape(B, n, 12)
    return out


def estimate_poses(res: MatchResult, cameras: Sequence[Any], pnp_type: str = "opencv", pnp_ransac_iter: int = 1000,
                   pnp_inlier_thresh: float = 3.0, pnp_required_ransac_conf: float = 0.99, pnp_refine_lm: bool = True, seed: int = 0, pair_keys=None,
                   *, frame_cameras: Optional[Sequence[Any]] = None, depth: Optional[torch.Tensor] = None, image_index=None,
                   depth_inlier_thresh_mm=None):
    """All coarse poses of a batch (the loop of infer.py:552-580 for every detection at once).  pair_keys: see solve_pnp_ransac_batch.
    pnp_type "kabsch_depth": 3D-3D RANSAC on depth-lifted correspondences (solve_kabsch_ransac_batch) -- needs the four keyword
    arguments (the frames' cameras, the depth stack, each detection's image in it, the inlier threshold in mm); pnp_inlier_thresh
    (pixels) is not used by it."""
    if pnp_type not in PNP_TYPES:
        raise ValueError("Unsupported PnP type")
    counts = torch.where(res.template_ids >= 0, res.counts, torch.zeros_like(res.counts))
    if pnp_type == "kabsch_depth":
        missing = [k for k, v in (("frame_cameras", frame_cameras), ("depth", depth), ("image_index", image_index),
                                  ("depth_inlier_thresh_mm", depth_inlier_thresh_mm)) if v is None]
        if missing:
            raise ValueError(f"pnp_type 'kabsch_depth' needs {', '.join(missing)}")
        return solve_kabsch_ransac_batch(res.coord_2d, res.coord_3d, counts, cameras, frame_cameras, depth, image_index, depth_inlier_thresh_mm,
                                         pnp_ransac_iter, pnp_required_ransac_conf, pnp_refine_lm, seed, pair_keys=pair_keys)
    return solve_pnp_ransac_batch(res.coord_2d, res.coord_3d, counts, cameras, pnp_ransac_iter, pnp_inlier_thresh,
                                  pnp_required_ransac_conf, pnp_refine_lm, seed, pair_keys=pair_keys)


def _selection(poses: Dict[str, torch.Tensor], found: torch.Tensor, first: torch.Tensor, quality: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The selectors' result: the pose of slot first[b] of every detection b."""
    idx = first[:, None, None]
    return {"found": found, "corresp_id": first,
            "R": poses["R"].gather(1, idx[..., None].expand(-1, 1, 3, 3))[:, 0], "t": poses["t"].gather(1, idx.expand(-1, 1, 3))[:, 0],
            "quality": quality}


def select_best_coarse(poses: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """infer.py:582-602: among a detection's successful coarse poses the one of the highest quality, the first on ties.
    -> found [B] bool, corresp_id [B], R [B, 3, 3], t [B, 3], quality [B]."""
    q = torch.where(poses["success"], poses["quality"], torch.full_like(poses["quality"], -1.0))
    best_q, _ = q.max(dim=1)
    n = q.shape[1]
    first = torch.where(q == best_q[:, None], torch.arange(n, device=q.device)[None, :], torch.full_like(q, n, dtype=torch.int64)).min(dim=1).values
    return _selection(poses, best_q >= 0, first.clamp_max(n - 1), best_q)


VERIFY_MIN_GRID, VERIFY_MAX_GRID = 8, 128   # the z-buffer's side in cells (csrc/verify.hip: G * G words of LDS)


def _check_verify_grid(grid) -> None:
    if isinstance(grid, bool) or not isinstance(grid, int) or not VERIFY_MIN_GRID <= grid <= VERIFY_MAX_GRID:
        raise ValueError(f"grid must be an integer in [{VERIFY_MIN_GRID}, {VERIFY_MAX_GRID}], got {grid!r}")


def _verify_sample(bank, max_points: int, det_obj: Sequence[int], solve_cameras: Sequence[Any], frame_cameras: Sequence[Any], what: str):
    """What both verifiers place at a pose: -> (bank.verify_points(max_points), the detections' object indices checked against it, the
    rotations solve camera -> frame camera [B, 3, 3])."""
    vp = bank.verify_points(max_points)
    objs = [int(o) for o in det_obj]
    for b, o in enumerate(objs):
        if not 0 <= o < len(vp.ranges):
            raise ValueError(f"detection {b}: object {o} outside the bank's [0, {len(vp.ranges)})")
    return vp, objs, solve_to_frame_rotations(solve_cameras, frame_cameras, what)


def _verify_results(B: int, n: int, num_counts: int, dev):
    """-> (the kernels' zeroed outputs counts [P, num_counts], score [P], status [P], the verifiers' dict of them as [B, n, ...] views)."""
    counts = torch.zeros(B * n, num_counts, dtype=torch.int32, device=dev)
    score = torch.zeros(B * n, dtype=torch.float64, device=dev)
    status = torch.zeros(B * n, dtype=torch.int32, device=dev)
    return counts, score, status, {"counts": counts.reshape(B, n, num_counts), "score": score.reshape(B, n), "status": status.reshape(B, n)}


def _verify_inputs(poses: Dict[str, torch.Tensor], frame_cameras: Sequence[Any], A: np.ndarray, vp, objs: List[int], more_reals: Sequence[torch.Tensor],
                   ints: torch.Tensor):
    """The verifiers' device inputs.  One byte buffer, one upload: the fp64 table [B, 17 + ...] = (the frame cameras' intrinsics 4, A 9, the
    objects' sphere centres 3 and radii 1, then more_reals) followed by the int32 table `ints` [B, c], each read back as its own type.
    -> (success int32, R f64, t f64, intrinsics, A, centres, radii -- contiguous --, the table's further columns, ints on the device)."""
    B, dev = len(objs), poses["success"].device
    reals = torch.cat([torch.tensor([_intrinsics(c) for c in frame_cameras], dtype=torch.float64).reshape(B, 4), torch.from_numpy(A.reshape(B, 9)),
                       torch.from_numpy(vp.centers[objs].reshape(B, 3)), torch.from_numpy(vp.radii[objs].reshape(B, 1)), *more_reals], dim=1).contiguous()
    raw = upload_async(torch.cat([reals.view(torch.uint8).reshape(-1), ints.view(torch.uint8).reshape(-1)]), dev)
    split = reals.numel() * 8   # (the int32 part starts at a multiple of 8 bytes)
    table, idev = raw[:split].view(torch.float64).reshape(reals.shape), raw[split:].view(torch.int32).reshape(ints.shape)
    return (poses["success"].to(torch.int32).contiguous(), poses["R"].to(torch.float64).contiguous(), poses["t"].to(torch.float64).contiguous(),
            table[:, :4].contiguous(), table[:, 4:13].contiguous(), table[:, 13:16].contiguous(), table[:, 16].contiguous(), table[:, 17:], idev)


def verify_poses_depth(poses: Dict[str, torch.Tensor], bank, det_obj: Sequence[int], solve_cameras: Sequence[Any], frame_cameras: Sequence[Any],
                       depth: torch.Tensor, image_index, thresh_mm, max_points: int = 16384, grid: int = 64,
                       min_visible: int = 16) -> Dict[str, torch.Tensor]:
    """Every coarse pose of a batch checked against the frame's depth (csrc/verify.hip): the point sample of the
    whole model (bank.verify_points(max_points)) placed at the pose, its self-occlusion decided by a grid x grid z-buffer, each visible point
    counted as confirmed by the depth image, occluded, in free space, on a hole or outside the image.
    poses: estimate_poses' dict (success [B, n], R [B, n, 3, 3], t [B, n, 3], model -> solve camera); det_obj: the object of each detection
    in `bank`; solve_cameras / frame_cameras / depth [N, H, W] fp32 mm / image_index: as in solve_kabsch_ransac_batch; thresh_mm: one
    number or one per detection (> 0).
    -> counts [B, n, 6] int32 = (n_vis, n_in, n_occ, n_free, n_hole, n_out), score [B, n] f64 = n_in / n_vis (0 below min_visible visible
    points), status [B, n] int32 (0 scored, 1 too few visible points, 2 skipped: no pose, no points, or the model's sphere reaches the
    camera).  B = 0 or n = 0 returns empty tensors without a launch.  A bad image index, threshold, camera pair or grid raises ValueError before anything is launched."""
    success, R, t = poses["success"], poses["R"], poses["t"]
    require_cuda(success, R, t, depth)
    B, n = (int(s) for s in success.shape)
    dev = success.device
    if len(solve_cameras) != B or len(frame_cameras) != B or len(det_obj) != B:
        raise ValueError(f"{len(solve_cameras)} solve cameras, {len(frame_cameras)} frame cameras and {len(det_obj)} objects for {B} detections")
    if depth.dim() != 3 or depth.dtype != torch.float32:
        raise ValueError(f"depth must be a float32 stack [N, H, W], got {depth.dtype} {list(depth.shape)}")
    _check_verify_grid(grid)
    if isinstance(min_visible, bool) or not isinstance(min_visible, int) or min_visible < 1:
        raise ValueError(f"min_visible must be an integer >= 1, got {min_visible!r}")
    N, H, W = (int(s) for s in depth.shape)
    if isinstance(image_index, torch.Tensor):
        image_index = image_index.cpu().tolist()
    ii = [int(i) for i in image_index]
    if len(ii) != B:
        raise ValueError(f"{len(ii)} image indices for {B} detections")
    for b, i in enumerate(ii):
        if not 0 <= i < N:
            raise ValueError(f"detection {b}: image index {i} outside [0, {N})")
    tau = np.full(B, thresh_mm, np.float64) if np.ndim(thresh_mm) == 0 else np.array(thresh_mm, np.float64).reshape(-1)
    if tau.shape != (B,) or not np.all(tau > 0) or not np.all(np.isfinite(tau)):
        raise ValueError(f"thresh_mm must be one finite number > 0 or {B} of them, got {thresh_mm!r}")
    vp, objs, A = _verify_sample(bank, max_points, det_obj, solve_cameras, frame_cameras, "depth verification")
    counts, score, status, out = _verify_results(B, n, 6, dev)
    if B * n == 0:   # nothing to launch
        return out
    # the table's extra column: tau; the int32 table [B, 3]: (image, begin, end)
    ok, Rd, td, cam, Ad, cen, rad, more, idev = _verify_inputs(poses, frame_cameras, A, vp, objs, [torch.from_numpy(tau).reshape(B, 1)],
                                                               torch.tensor([[i, *vp.ranges[o]] for i, o in zip(ii, objs)], dtype=torch.int32).reshape(B, 3))
    taud, iid, rng = more[:, 0].contiguous(), idev[:, 0].contiguous(), idev[:, 1:3].contiguous()
    dimg = depth.contiguous()
    call("fp_pose_verify_depth", ptr(ok), ptr(Rd), ptr(td), ptr(cam), ptr(Ad), ptr(iid), ptr(taud), ptr(rng), ptr(cen), ptr(rad), ptr(vp.points),
         int(vp.points.shape[0]), ptr(dimg), N, H, W, B * n, n, grid, min_visible, ptr(counts), ptr(score), ptr(status), stream())
    return out


def verify_poses_mask(poses: Dict[str, torch.Tensor], bank, det_obj: Sequence[int], solve_cameras: Sequence[Any], frame_cameras: Sequence[Any],
                      masks: torch.Tensor, max_points: int = 16384, grid: int = 64, min_pixels: int = 16) -> Dict[str, torch.Tensor]:
    """Every coarse pose of a batch checked against its detection's mask (csrc/mask_verify.hip): the point sample of
    the whole model (bank.verify_points(max_points)) placed at the pose, the cells of a grid x grid square its points project into taken as
    the model's silhouette, and the silhouette's pixels compared with the mask's.
    poses / bank / det_obj / solve_cameras / frame_cameras: as in verify_poses_depth; masks: uint8 [B, H, W] on the device, each detection's
    own mask in its frame camera's image (non-zero = set).
    -> counts [B, n, 4] int32 = (n_both, n_model_only, n_mask_only, n_cells), score [B, n] f64 = n_both / (n_both + n_model_only +
    n_mask_only) (0 below min_pixels model pixels), status [B, n] int32 (0 scored, 1 too few model pixels, 2 skipped: no pose, no points,
    or the model's sphere reaches the camera).  B = 0 or n = 0 returns empty tensors without a launch.  Masks of another type or shape,
    lengths that do not match, a bad object index, grid, min_pixels or camera pair raise ValueError before anything is launched."""
    success, R, t = poses["success"], poses["R"], poses["t"]
    _check_verify_grid(grid)
    if isinstance(min_pixels, bool) or not isinstance(min_pixels, int) or min_pixels < 1:
        raise ValueError(f"min_pixels must be an integer >= 1, got {min_pixels!r}")
    if not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or masks.dim() != 3:
        raise ValueError(f"masks must be a uint8 tensor [B, H, W] on the device, got "
                         f"{(masks.dtype, list(masks.shape)) if isinstance(masks, torch.Tensor) else type(masks).__name__}")
    B, n = (int(s) for s in success.shape)
    if len(solve_cameras) != B or len(frame_cameras) != B or len(det_obj) != B or int(masks.shape[0]) != B:
        raise ValueError(f"{len(solve_cameras)} solve cameras, {len(frame_cameras)} frame cameras, {len(det_obj)} objects and {int(masks.shape[0])} masks "
                         f"for {B} detections")
    H, W = int(masks.shape[1]), int(masks.shape[2])
    if B and not 1 <= H * W <= 1 << 30:
        raise ValueError(f"masks of {W} x {H}: between 1 and 2^30 pixels")
    if not masks.is_cuda:
        raise ValueError(f"masks must be a uint8 tensor [B, H, W] on the device, got one on {masks.device}")
    require_cuda(success, R, t)
    dev = success.device
    vp, objs, A = _verify_sample(bank, max_points, det_obj, solve_cameras, frame_cameras, "mask verification")
    counts, score, status, out = _verify_results(B, n, 4, dev)
    if B * n == 0:   # nothing to launch
        return out
    # no extra column; the int32 table [B, 2]: (begin, end)
    ok, Rd, td, cam, Ad, cen, rad, _, rng = _verify_inputs(poses, frame_cameras, A, vp, objs, [],
                                                           torch.tensor([vp.ranges[o] for o in objs], dtype=torch.int32).reshape(B, 2))
    mk = masks.contiguous()
    area = mk.ne(0).flatten(1).sum(1, dtype=torch.int32)   # plumbing on the device, no synchronisation: the set pixels of each mask
    call("fp_pose_verify_mask", ptr(ok), ptr(Rd), ptr(td), ptr(cam), ptr(Ad), ptr(rng), ptr(cen), ptr(rad), ptr(vp.points), int(vp.points.shape[0]),
         ptr(mk), ptr(area), H, W, B * n, n, grid, min_pixels, ptr(counts), ptr(score), ptr(status), stream())
    return out


def select_best_verified(poses: Dict[str, torch.Tensor], verify: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """select_best_coarse with the hypotheses ranked by verify_poses_depth's result: among a detection's successful coarse poses the scored
    ones (status 0) before the others, then the higher score, then the higher coarse quality, then the first slot.
    -> select_best_coarse's dict (quality: the chosen hypothesis's coarse quality, -1 where nothing was found) + verify_score [B]."""
    ok, quality = poses["success"], poses["quality"]
    n = ok.shape[1]
    scored = ok & (verify["status"] == 0)
    cand = torch.where(scored.any(dim=1, keepdim=True), scored, ok)
    neg = torch.full_like(quality, -float("inf"))
    for key in (torch.where(scored, verify["score"].to(quality.dtype), torch.zeros_like(quality)), quality):
        k = torch.where(cand, key, neg)
        cand = cand & (k == k.max(dim=1, keepdim=True).values)
    first = torch.where(cand, torch.arange(n, device=ok.device)[None, :], torch.full_like(cand, n, dtype=torch.int64)).min(dim=1).values
    found = first < n
    first = first.clamp_max(n - 1)
    pick = lambda v: v.gather(1, first[:, None])[:, 0]
    return dict(_selection(poses, found, first, torch.where(found, pick(quality), torch.full_like(pick(quality), -1.0))),
                verify_score=torch.where(found, pick(verify["score"]), torch.zeros_like(pick(verify["score"]))))


def estimate_pose(corresp: Dict[str, Any], camera_c2w: Any, pnp_type: str, pnp_ransac_iter: int, pnp_inlier_thresh: float,
                  pnp_required_ransac_conf: float, pnp_refine_lm: bool, seed: int = 0) -> Tuple[bool, Optional[np.ndarray], Optional[np.ndarray], Optional[np.ndarray], Optional[float]]:
    """The reference's per-correspondence-set call (utils/pnp_util.py:20-84): -> (success, R_m2c [3,3], t_m2c [3,1], inlier ids
    [num_inliers, 1], quality); (False, None, None, None, None) where cv2 would have raised or failed."""
    if pnp_type != "opencv":
        raise ValueError("Unsupported PnP type")
    c2 = torch.as_tensor(corresp["coord_2d"]).to("cuda", torch.float32)
    c3 = torch.as_tensor(corresp["coord_3d"]).to("cuda", torch.float32)
    k = int(c2.shape[0])
    if k < 4:
        return False, None, None, None, None
    out = solve_pnp_ransac_batch(c2.reshape(1, 1, k, 2), c3.reshape(1, 1, k, 3), torch.tensor([[k]], dtype=torch.int32, device="cuda"),
                                 [camera_c2w], pnp_ransac_iter, pnp_inlier_thresh, pnp_required_ransac_conf, pnp_refine_lm, seed, min_corresp=4)
    if not bool(out["success"][0, 0]):
        return False, None, None, None, None
    inl = torch.nonzero(out["inliers"][0, 0]).to(torch.int32).cpu().numpy()
    return True, out["R"][0, 0].cpu().numpy(), out["t"][0, 0].cpu().numpy().reshape(3, 1), inl, float(out["quality"][0, 0])
