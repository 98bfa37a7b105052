"""Result collection, pose evaluation and the output formats of the driver (/root/reference/utils/eval_util.py:26-516,
utils/eval_errors.py and /root/reference/scripts/prepare_bop_submission.py:30-99): `estimated-poses.json` per object, the
BOP19 csv built from them, and -- when the frames carry ground-truth poses -- the BOP errors MSSD / MSPD (one
fp_pose_errors launch per batch of hypotheses) with the reference's other per-detection errors and its metrics table."""

import json
import math
import os
from collections import defaultdict
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import numpy as np


def _jsonable(x):
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, (np.floating, np.integer)):
        return x.item()
    if isinstance(x, dict):
        return {k: _jsonable(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_jsonable(v) for v in x]
    return x


# ---------------------------------------------------------------------------------------------------- symmetries, errors
def _rotation_matrix(angle: float, direction) -> np.ndarray:
    """transformations.rotation_matrix(angle, direction)[:3, :3] (the toolkit's bop_toolkit_lib.transform)."""
    sina, cosa = math.sin(angle), math.cos(angle)
    d = np.array(direction[:3], dtype=np.float64)
    d /= math.sqrt(np.dot(d, d))
    R = np.diag([cosa, cosa, cosa])
    R += np.outer(d, d) * (1.0 - cosa)
    d *= sina
    R += np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return R


def get_symmetry_transformations(model_info: Dict[str, Any], max_sym_disc_step: float) -> List[Dict[str, np.ndarray]]:
    """bop_toolkit_lib.misc.get_symmetry_transformations, restated from its published behaviour (the toolkit is not part of
    the reference checkout, so this is not pinned against its code): the identity and every `symmetries_discrete` entry
    (4x4, row-major); each `symmetries_continuous` {axis, offset} discretised into n = ceil(pi / step) rotations
    i * 2 pi / n, i = 1 .. n-1, about the axis through the offset (t = -R offset + offset); with continuous symmetries every
    discrete one composed with every continuous one (R = R_c R_d, t = R_c t_d + t_c) -- so the identity itself is then NOT
    in the list, as in the toolkit.  -> [{"R": 3x3, "t": 3x1}]."""
    trans_disc = [{"R": np.eye(3), "t": np.array([[0, 0, 0]]).T}]
    for sym in model_info.get("symmetries_discrete", []):
        m = np.reshape(np.asarray(sym, np.float64), (4, 4))
        trans_disc.append({"R": m[:3, :3], "t": m[:3, 3].reshape((3, 1))})
    trans_cont = []
    for sym in model_info.get("symmetries_continuous", []):
        axis = np.array(sym["axis"], np.float64)
        offset = np.array(sym["offset"], np.float64).reshape((3, 1))
        n = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / n
        for i in range(1, n):
            R = _rotation_matrix(i * step, axis)
            trans_cont.append({"R": R, "t": -R.dot(offset) + offset})
    trans = []
    for td in trans_disc:
        if len(trans_cont):
            for tc in trans_cont:
                trans.append({"R": tc["R"].dot(td["R"]), "t": tc["R"].dot(td["t"]) + tc["t"]})
        else:
            trans.append(td)
    return trans


@dataclass
class EvalModel:
    """What evaluating one object needs (scripts/infer.py:727-734): the full model's vertices (fp64, mm), its symmetry
    transformations and its diameter."""
    pts: np.ndarray
    syms: List[Dict[str, np.ndarray]]
    diameter: float


def load_eval_model(models_dir: str, lid: int, max_sym_disc_step: float = 0.01, models_info: Optional[Dict[str, Any]] = None) -> EvalModel:
    """<models_dir>/obj_<lid:06d>.ply + models_info.json -> EvalModel."""
    from .renderer import load_ply
    if models_info is None:
        with open(os.path.join(models_dir, "models_info.json")) as f:
            models_info = json.load(f)
    info = models_info[str(lid)] if str(lid) in models_info else models_info[lid]
    pts = load_ply(os.path.join(models_dir, f"obj_{lid:06d}.ply"), geometry_only=True).vertices.astype(np.float64)  # textured models too
    return EvalModel(pts, get_symmetry_transformations(info, max_sym_disc_step), float(info["diameter"]))


def rotation_error_deg(R_est: np.ndarray, R_gt: np.ndarray) -> float:
    """eval_errors.compute_rotation_error: the angle of R_est R_gt^T in degrees, as scipy's
    Rotation.from_matrix(R).magnitude() gives it (Markley's quaternion extraction, normalised, 2 atan2(|v|, |w|))."""
    m = np.asarray(R_est, np.float64).dot(np.asarray(R_gt, np.float64).T)
    dec = np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2]])
    c = int(np.argmax(dec))
    q = np.empty(4)
    if c != 3:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[i] = 1 - dec[3] + 2 * m[i, i]
        q[j] = m[j, i] + m[i, j]
        q[k] = m[k, i] + m[i, k]
        q[3] = m[k, j] - m[j, k]
    else:
        q[0] = m[2, 1] - m[1, 2]
        q[1] = m[0, 2] - m[2, 0]
        q[2] = m[1, 0] - m[0, 1]
        q[3] = 1 + dec[3]
    q /= np.linalg.norm(q)
    return float(np.rad2deg(2 * np.arctan2(np.linalg.norm(q[:3]), abs(q[3]))))


def template_orientation_error(R_m2c_gt: np.ndarray, template_R: np.ndarray, sym_R: np.ndarray) -> float:
    """min over retrieved templates x symmetries of eval_errors.re(R_tpl, R_m2c_gt S_R) (eval_util.py:179-187), vectorised:
    the inverses depend on the symmetry only, the traces of all pairs come from one batched product."""
    R_gs = np.matmul(R_m2c_gt, sym_R)                                    # [S, 3, 3]
    inv = np.linalg.inv(R_gs)
    prod = np.matmul(np.asarray(template_R, np.float64)[:, None], inv[None])   # [T, S, 3, 3]
    cos = 0.5 * (np.trace(prod, axis1=-2, axis2=-1) - 1.0)
    err = 180.0 * np.arccos(np.clip(cos, -1.0, 1.0)) / np.pi
    return float(err.min())


def _rigid(pose) -> np.ndarray:
    """misc.get_rigid_matrix of an ObjectPose-like (.R, .t), an (R, t) pair or a 4x4 matrix."""
    if hasattr(pose, "R"):
        R, t = pose.R, pose.t
    elif isinstance(pose, (tuple, list)) and len(pose) == 2:
        R, t = pose
    else:
        return np.array(pose, np.float64).reshape(4, 4)
    m = np.eye(4)
    m[:3, :3] = np.asarray(R, np.float64)
    m[:3, 3:] = np.asarray(t, np.float64).reshape(3, 1)
    return m


def _intrinsics(cam) -> np.ndarray:
    return np.array([[cam.f[0], 0.0, cam.c[0]], [0.0, cam.f[1], cam.c[1]], [0.0, 0.0, 1.0]])


def _eye_to_window(cam, v: np.ndarray) -> np.ndarray:
    """structs.PinholePlaneCameraModel.eye_to_window: (v.xy / v.z) * f + c."""
    return v[..., :2] / v[..., 2, None] * np.asarray(cam.f, np.float64) + np.asarray(cam.c, np.float64)


def _transform(trans: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """geometry.transform_3d_points_numpy."""
    return trans.dot(np.hstack((pts, np.ones((pts.shape[0], 1)))).T)[:3, :].T


def _template_rotation(cam) -> np.ndarray:
    T = cam["T_world_from_eye"] if isinstance(cam, dict) else cam.T_world_from_eye
    T = T.cpu().numpy() if hasattr(T, "cpu") else T
    return np.asarray(T, np.float64)[:3, :3]


def _inlier_ratio(corr_dist: np.ndarray, ids: np.ndarray, radius: float):
    """The share of query patches (coord_2d_ids, first-appearance order) with at least one match within `radius`; the
    reference's loop leaves the int 0 when there are no matches."""
    if len(ids) == 0:
        return 0
    uniq, inv = np.unique(ids, return_inverse=True)
    hit = np.zeros(len(uniq), dtype=float)
    np.maximum.at(hit, inv, (corr_dist <= radius).astype(float))
    return np.mean(hit)


def pose_errors_batch(items: Sequence[Dict[str, Any]], device: str = "cuda"):
    """pose_errors_device read back: -> (err [H, 2] numpy = (mssd, mspd), idx [H, 4] numpy int = (mssd vertex, mssd sym, mspd vertex, mspd
    sym))."""
    err, idx = pose_errors_device(items, device)
    return err.cpu().numpy(), idx.cpu().numpy().astype(np.int64)


def pose_errors_device(items: Sequence[Dict[str, Any]], device: str = "cuda"):
    """MSSD / MSPD of several hypotheses in ONE fp_pose_errors launch.  Each item: R_est, t_est, R_gt, t_gt (model ->
    original camera), K (3x3), pts (the mesh vertices, numpy fp64 or a device tensor), syms (list of {"R", "t"}).
    Objects shared by several items are uploaded once.  The symmetry stack of each item is composed on the host,
    vectorised: R_gt_sym = R_gt S_R, t_gt_sym = R_gt S_t + t_gt (eval_errors.py:22-23), P = K [R | t] (project_pts).
    -> (err [H, 2] fp64 = (mssd, mspd), idx [H, 4] int32 = (mssd vertex, mssd sym, mspd vertex, mspd sym)), both left on the device."""
    import torch
    from . import ops
    pts_keys, pts_list, pts_off = {}, [], 0
    sym_keys, sym_stacks = {}, {}
    ranges, est, p_est, gt_rows, pgt_rows, sym_off = [], [], [], [], [], 0
    for it in items:
        pk = id(it["pts"])
        if pk not in pts_keys:
            p = it["pts"]
            n = int(p.shape[0])
            pts_keys[pk] = (pts_off, n)
            pts_list.append(p)
            pts_off += n
        sk = id(it["syms"])
        if sk not in sym_stacks:
            sym_stacks[sk] = (np.stack([np.asarray(s_["R"], np.float64) for s_ in it["syms"]]),
                              np.stack([np.asarray(s_["t"], np.float64).reshape(3, 1) for s_ in it["syms"]]))
        SR, St = sym_stacks[sk]
        R_gt, t_gt = np.asarray(it["R_gt"], np.float64), np.asarray(it["t_gt"], np.float64).reshape(3, 1)
        R_est, t_est = np.asarray(it["R_est"], np.float64), np.asarray(it["t_est"], np.float64).reshape(3, 1)
        K = np.asarray(it["K"], np.float64)
        R_gs = np.matmul(R_gt, SR)                       # [S, 3, 3]
        t_gs = np.matmul(R_gt, St) + t_gt                # [S, 3, 1]
        Rt_gs = np.concatenate([R_gs, t_gs], axis=2)     # [S, 3, 4]
        gt_rows.append(np.concatenate([R_gs.reshape(-1, 9), t_gs.reshape(-1, 3)], axis=1))
        pgt_rows.append(np.matmul(K, Rt_gs).reshape(-1, 12))
        est.append(np.concatenate([R_est.reshape(9), t_est.reshape(3)]))
        p_est.append(K.dot(np.hstack((R_est, t_est))).reshape(12))
        ranges.append((pts_keys[pk][0], pts_keys[pk][1], sym_off, len(SR)))
        sym_off += len(SR)

    def dev(a):
        return a.to(device, torch.float64) if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(device)
    pts_d = torch.cat([dev(p).reshape(-1, 3) for p in pts_list])
    err, idx = ops.pose_errors(pts_d, dev(np.stack(est)), dev(np.stack(p_est)), dev(np.concatenate(gt_rows)), dev(np.concatenate(pgt_rows)),
                               np.array(ranges, np.int64))
    return err, idx


class PoseEvaluator:
    """The reference's EvaluatorPose: pose estimates in the ORIGINAL camera frame, the many-to-many aware inlier ratio as
    the score, per-stage run times, CNOS detection times -- and, for hypotheses with a ground-truth pose (`update`,
    `update_batch`), the BOP errors and the reference's other per-detection errors."""

    def __init__(self, obj_lids: Optional[Sequence[int]] = None) -> None:
        self.obj_lids = list(obj_lids) if obj_lids is not None else None
        self.result_ids: List[tuple] = []
        self.obj_ids: List[int] = []
        self.R: List[np.ndarray] = []
        self.t: List[np.ndarray] = []
        self.score: List[float] = []
        self.time: List[Dict[str, float]] = []
        self.inliers_est_err: List[Dict[str, float]] = []
        self.detection_times: Dict[tuple, float] = {}
        # filled by update / update_batch only (empty: estimated-poses.json keeps the annotation-free entry)
        self.mssd: List[float] = []
        self.mspd: List[float] = []
        self.mssd_n: List[float] = []
        self.inliers_gt_err: List[Dict[str, float]] = []
        self.inliers_gt: List[np.ndarray] = []
        self.inliers_est: List[np.ndarray] = []
        self.corr_dist_gt: List[np.ndarray] = []
        self.corr_dist_est: List[np.ndarray] = []
        self.point_errors: List[np.ndarray] = []
        self.rotation_errors: List[np.ndarray] = []
        self.translation_errors: List[np.ndarray] = []
        self.template_ori_err: List[float] = []
        self.mask_iou: List[float] = []

    def update(self, scene_id: int, im_id: int, inst_id: int, hypothesis_id: int, base_image, object_repre_vertices: np.ndarray, obj_lid: int,
               object_pose_m2w, object_pose_m2w_gt, orig_camera_c2w, camera_c2w, pred_mask: np.ndarray, gt_mask: np.ndarray,
               corresp: Dict[str, np.ndarray], retrieved_templates_camera_m2c: Sequence[Any], time_per_inst: Dict[str, float],
               object_mesh_vertices, object_syms: Sequence[Dict[str, np.ndarray]], object_diameter: float,
               inlier_radius: float = 10) -> Dict[str, Any]:
        """utils/eval_util.py:74-229 (`base_image` is accepted and unused: it only fed the visualisation).  MSSD / MSPD come
        from fp_pose_errors; everything else is the reference's numpy.  Returns the reference's dict plus the other errors
        this call records (point / rotation / translation errors, mask IoU, template orientation error, chosen symmetries)."""
        return self.update_batch([dict(scene_id=scene_id, im_id=im_id, inst_id=inst_id, hypothesis_id=hypothesis_id, base_image=base_image,
                                       object_repre_vertices=object_repre_vertices, obj_lid=obj_lid, object_pose_m2w=object_pose_m2w,
                                       object_pose_m2w_gt=object_pose_m2w_gt, orig_camera_c2w=orig_camera_c2w, camera_c2w=camera_c2w,
                                       pred_mask=pred_mask, gt_mask=gt_mask, corresp=corresp,
                                       retrieved_templates_camera_m2c=retrieved_templates_camera_m2c, time_per_inst=time_per_inst,
                                       object_mesh_vertices=object_mesh_vertices, object_syms=object_syms, object_diameter=object_diameter,
                                       inlier_radius=inlier_radius)])[0]

    def update_batch(self, items: Sequence[Dict[str, Any]]) -> List[Dict[str, Any]]:
        """`update` of several hypotheses (each item: update's keyword arguments), in order, with ONE fp_pose_errors launch
        for all of them.  The values are those of calling `update` once per item."""
        pre = []
        for it in items:
            # Transformations to the crop camera and to the original camera (eval_util.py:98-106).
            trans_w2c = np.linalg.inv(it["camera_c2w"].T_world_from_eye)
            trans_m2c_gt = trans_w2c.dot(_rigid(it["object_pose_m2w_gt"]))
            trans_m2c = trans_w2c.dot(_rigid(it["object_pose_m2w"]))
            trans_w2oc = np.linalg.inv(it["orig_camera_c2w"].T_world_from_eye)
            trans_m2oc_gt = trans_w2oc.dot(_rigid(it["object_pose_m2w_gt"]))
            trans_m2oc = trans_w2oc.dot(_rigid(it["object_pose_m2w"]))
            # Quirk kept from the reference (eval_util.py:150-152): MSPD projects with the CROP camera's intrinsics a pose
            # expressed in the ORIGINAL camera frame.
            pre.append(dict(trans_m2c_gt=trans_m2c_gt, trans_m2c=trans_m2c, R_est=trans_m2oc[:3, :3], t_est=trans_m2oc[:3, 3:],
                            R_gt=trans_m2oc_gt[:3, :3], t_gt=trans_m2oc_gt[:3, 3:], K=_intrinsics(it["camera_c2w"])))
        err, idx = pose_errors_batch([dict(R_est=p_["R_est"], t_est=p_["t_est"], R_gt=p_["R_gt"], t_gt=p_["t_gt"], K=p_["K"],
                                           pts=it["object_mesh_vertices"], syms=it["object_syms"]) for it, p_ in zip(items, pre)])
        out = []
        for h, (it, p_) in enumerate(zip(items, pre)):
            out.append(self._record(it, p_, float(err[h, 0]), float(err[h, 1]), idx[h]))
        return out

    def _record(self, it: Dict[str, Any], p_: Dict[str, Any], mssd_e: float, mspd_e: float, idx: np.ndarray) -> Dict[str, Any]:
        radius = it.get("inlier_radius", 10)
        key = str(int(radius))
        cam = it["camera_c2w"]
        corresp = it["corresp"]
        verts = np.asarray(it["object_repre_vertices"], np.float64)
        vertex_ids = np.asarray(corresp["nn_vertex_ids"], np.int64)
        coord_2d = np.asarray(corresp["coord_2d"], np.float64)
        ids = np.asarray(corresp["coord_2d_ids"], np.int64)
        # Inliers / outliers under the GT and the estimated pose (eval_util.py:108-127), in the crop camera.
        vertices_in_c_gt = _transform(p_["trans_m2c_gt"], verts)
        corr_dist_gt = np.linalg.norm(coord_2d - _eye_to_window(cam, vertices_in_c_gt)[vertex_ids], axis=1)
        inliers_gt = np.where(corr_dist_gt <= radius)[0]
        vertices_in_c = _transform(p_["trans_m2c"], verts)
        corr_dist_est = np.linalg.norm(coord_2d - _eye_to_window(cam, vertices_in_c)[vertex_ids], axis=1)
        inliers_est = np.where(corr_dist_est <= radius)[0]
        inliers_gt_err = {key: _inlier_ratio(corr_dist_gt, ids, radius)}
        inliers_est_err = {key: _inlier_ratio(corr_dist_est, ids, radius)}
        score = inliers_est_err[key]
        normalized_mssd = mssd_e / it["object_diameter"]
        point_errors = np.sqrt(np.sum((vertices_in_c_gt - vertices_in_c) ** 2, axis=-1))
        rotation_errors = rotation_error_deg(p_["R_est"], p_["R_gt"])
        translation_errors = np.linalg.norm(np.linalg.norm(np.abs(p_["t_est"] - p_["t_gt"]), axis=-1), axis=-1)
        mask_iou = _mask_iou(it["pred_mask"], it["gt_mask"])
        tpl_R = [_template_rotation(c) for c in it["retrieved_templates_camera_m2c"]]
        sym_R = np.stack([np.asarray(s_["R"], np.float64) for s_ in it["object_syms"]])
        template_ori_err = template_orientation_error(p_["trans_m2c_gt"][:3, :3], np.stack(tpl_R), sym_R) if tpl_R else float("nan")

        self.template_ori_err.append(template_ori_err)
        self.mask_iou.append(mask_iou)
        self.mspd.append(mspd_e)
        self.mssd.append(mssd_e)
        self.mssd_n.append(normalized_mssd)
        self.inliers_gt_err.append(inliers_gt_err)
        self.inliers_est_err.append(inliers_est_err)
        self.inliers_gt.append(inliers_gt)
        self.inliers_est.append(inliers_est)
        self.corr_dist_gt.append(corr_dist_gt)
        self.corr_dist_est.append(corr_dist_est)
        self.score.append(score)
        self.R.append(p_["R_est"])
        self.t.append(p_["t_est"])
        self.time.append(it["time_per_inst"])
        self.result_ids.append((it["scene_id"], it["im_id"], it["obj_lid"], it["inst_id"], it["hypothesis_id"]))
        self.obj_ids.append(it["obj_lid"])
        self.point_errors.append(np.array(point_errors))
        self.rotation_errors.append(np.array(rotation_errors))
        self.translation_errors.append(np.array(translation_errors))
        return {"inliers_gt": inliers_gt, "inliers_est": inliers_est, "mspd": mspd_e, "mssd": mssd_e, "mspd_id": int(idx[2]),
                "mssd_id": int(idx[0]), "normalized_mssd": normalized_mssd, "inliers_gt_err": inliers_gt_err,
                "inliers_est_err": inliers_est_err, "corr_dist_gt": corr_dist_gt, "corr_dist_est": corr_dist_est,
                # not in the reference's return value (it only appends them):
                "mssd_sym": int(idx[1]), "mspd_sym": int(idx[3]), "point_errors": point_errors, "rotation_errors": rotation_errors,
                "translation_errors": translation_errors, "mask_iou": mask_iou, "template_ori_err": template_ori_err}

    def update_without_anno(self, scene_id: int, im_id: int, inst_id: int, hypothesis_id: int, object_repre_vertices: np.ndarray, obj_lid: int,
                            R_m2w: np.ndarray, t_m2w: np.ndarray, orig_camera_c2w, camera_c2w, time_per_inst: Dict[str, float],
                            corresp: Dict[str, np.ndarray], inlier_radius: float = 10) -> Dict[str, Any]:
        T_m2w = np.eye(4)
        T_m2w[:3, :3], T_m2w[:3, 3] = np.asarray(R_m2w, np.float64), np.asarray(t_m2w, np.float64).reshape(3)
        T_m2c = np.linalg.inv(camera_c2w.T_world_from_eye) @ T_m2w
        T_m2oc = np.linalg.inv(orig_camera_c2w.T_world_from_eye) @ T_m2w
        v = np.asarray(object_repre_vertices, np.float64)[np.asarray(corresp["nn_vertex_ids"], np.int64)]
        vc = v @ T_m2c[:3, :3].T + T_m2c[:3, 3]
        proj = np.stack([camera_c2w.f[0] * vc[:, 0] / vc[:, 2] + camera_c2w.c[0], camera_c2w.f[1] * vc[:, 1] / vc[:, 2] + camera_c2w.c[1]], 1)
        corr_dist_est = np.linalg.norm(np.asarray(corresp["coord_2d"], np.float64) - proj, axis=1)
        inliers_est = np.where(corr_dist_est <= inlier_radius)[0]
        ids = np.asarray(corresp["coord_2d_ids"], np.int64)
        unique_2d_ids = list(dict.fromkeys(ids.tolist()))
        est_err = np.zeros(len(unique_2d_ids), dtype=float)
        for i, q in enumerate(unique_2d_ids):  # a query patch counts once, however many of its matches are inliers
            if np.sum(corr_dist_est[ids == q] <= inlier_radius) > 0:
                est_err[i] = 1
        inliers_est_err = {str(int(inlier_radius)): float(np.mean(est_err)) if len(est_err) else 0.0}
        self.R.append(T_m2oc[:3, :3])
        self.t.append(T_m2oc[:3, 3:])
        self.time.append(dict(time_per_inst))
        self.score.append(inliers_est_err[str(int(inlier_radius))])
        self.result_ids.append((scene_id, im_id, obj_lid, inst_id, hypothesis_id))
        self.obj_ids.append(obj_lid)
        self.inliers_est_err.append(inliers_est_err)
        return {"inliers_est": inliers_est, "inliers_est_err": inliers_est_err, "corr_dist_est": corr_dist_est}

    def save_results_json(self, path: str) -> None:
        """estimated-poses.json: ids and score as strings, R [3][3], t [3][1], the run-time dict, the detector's time; when
        the run was evaluated (mssd non-empty) also the errors and inlier counts of eval_util.py:331-353."""
        out = []
        for i, (scene_id, img_id, obj_id, inst_id, hypothesis_id) in enumerate(self.result_ids):
            e = {"scene_id": str(scene_id), "img_id": str(img_id), "obj_id": str(obj_id), "inst_id": str(inst_id),
                 "hypothesis_id": str(hypothesis_id), "score": str(self.score[i]), "R": _jsonable(self.R[i]), "t": _jsonable(self.t[i]),
                 "time": _jsonable(self.time[i]), "cnos_time": self.detection_times[(scene_id, img_id)]}
            if len(self.mssd) != 0:
                e.update({"mspd": _jsonable(self.mspd[i]), "mssd": _jsonable(self.mssd[i]), "mssd_n": _jsonable(self.mssd_n[i]),
                          "inliers_gt": len(self.inliers_gt[i]), "inliers_est": len(self.inliers_est[i]),
                          "inliers_gt_err": _jsonable(self.inliers_gt_err[i]), "inliers_est_err": _jsonable(self.inliers_est_err[i])})
            out.append(e)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=2)

    def save_metrics(self, path: str, inlier_thresh: float) -> None:
        """The reference's metrics table (eval_util.py:400-516): tabulate(tsv, floatfmt .2f, no alignment), per object and
        overall.  The reference opens the file with os.open(path, "wb"), which raises TypeError, so it never writes this
        table; it is written with open() here."""
        from tabulate import tabulate
        key = str(int(inlier_thresh))
        lids = self.obj_lids if self.obj_lids is not None else sorted(set(self.obj_ids))
        obj_ids = np.array(self.obj_ids)
        per = defaultdict(list)
        for lid in lids:
            sel = np.where(obj_ids == lid)[0]
            per["mssd"].append(np.nanmean(np.array(self.mssd)[sel]))
            per["mssd_n"].append(np.nanmean(np.array(self.mssd_n)[sel]))
            per["mspd"].append(np.nanmean(np.array(self.mspd)[sel]))
            per["num"].append(len(sel))
            per["inl_gt"].append(np.nanmean([self.inliers_gt_err[i][key] for i in sel]))
            per["inl_est"].append(np.nanmean([self.inliers_est_err[i][key] for i in sel]))
            pe = np.concatenate([self.point_errors[i] for i in sel]) if len(sel) else np.array([np.nan])
            per["pt50"].append(np.nanpercentile(pe, 50))
            per["pt95"].append(np.nanpercentile(pe, 95))
            rot = np.array(self.rotation_errors)[sel] if len(sel) else np.array([np.nan])
            per["rot50"].append(np.nanpercentile(rot, 50))
            per["rot95"].append(np.nanpercentile(rot, 95))
            tr = np.array(self.translation_errors)[sel] if len(sel) else np.array([np.nan])
            per["tr50"].append(np.nanpercentile(tr, 50))
            per["tr95"].append(np.nanpercentile(tr, 95))
            per["tpl"].append(np.nanmean(np.array(self.template_ori_err)[sel]))
        pts_all = np.concatenate(self.point_errors, axis=0)
        header = ["", "overall", "pmean", "sym", "nonsym"] + [str(lid) for lid in lids]
        table = [
            ["mssd", np.nanmean(self.mssd), np.nanmean(per["mssd"]), 0, 0] + per["mssd"],
            ["mssd_n", np.nanmean(self.mssd_n), np.nanmean(per["mssd_n"]), 0, 0] + per["mssd_n"],
            ["mspd", np.nanmean(self.mspd), np.nanmean(per["mspd"]), 0, 0] + per["mspd"],
            ["inliers_gt", np.nanmean([e[key] for e in self.inliers_gt_err]), np.nanmean(per["inl_gt"]), 0, 0] + per["inl_gt"],
            ["inliers_est", np.nanmean([e[key] for e in self.inliers_est_err]), np.nanmean(per["inl_est"]), 0, 0] + per["inl_est"],
            ["Point_p50", np.percentile(pts_all, 50), 0, 0, 0] + per["pt50"],
            ["Point_p95", np.percentile(pts_all, 95), 0, 0, 0] + per["pt95"],
            ["Rot_p50", np.percentile(self.rotation_errors, 50), 0, 0, 0] + per["rot50"],
            ["Rot_p95", np.percentile(self.rotation_errors, 95), 0, 0, 0] + per["rot95"],
            ["Trans_p50", np.percentile(self.translation_errors, 50), 0, 0, 0] + per["tr50"],
            ["Trans_p95", np.percentile(self.translation_errors, 95), 0, 0, 0] + per["tr95"],
            ["Tpl_ori_err", np.mean(self.template_ori_err), 0, 0, 0] + per["tpl"],
            ["num_obj", np.sum(per["num"]), np.mean(per["num"]), 0, 0] + per["num"],
        ]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "wb") as f:
            f.write(tabulate(table, headers=header, tablefmt="tsv", floatfmt=".2f", numalign=None, stralign=None).encode("utf-8"))


def _mask_iou(mask1: np.ndarray, mask2: np.ndarray) -> float:
    """eval_errors.mask_iou."""
    inter = np.logical_and(mask1, mask2)
    union = np.logical_or(mask1, mask2)
    union_count = float(union.sum())
    return inter.sum() / union_count if union_count > 0 else 0.0


def prepare_bop_submission(output_dir: str, object_dataset: str, object_lids: Sequence[int]) -> str:
    """<output_dir>/<lid>/estimated-poses.json of every object -> coarse_<dataset>-estimated-poses.csv (BOP19 format).
    `time` of a row = run time of the whole image: the instances' stage times summed over all objects + the detector's."""
    per_image, det_time = defaultdict(float), {}
    loaded = {}
    for lid in object_lids:
        with open(os.path.join(output_dir, str(lid), "estimated-poses.json")) as f:
            loaded[lid] = json.load(f)
        for e in loaded[lid]:
            key = (e["scene_id"], e["img_id"])
            det_time[key] = e["cnos_time"]
            per_image[key] += sum(e["time"].values())
    lines = ["scene_id,im_id,obj_id,score,R,t,time"]
    for lid in object_lids:
        for e in loaded[lid]:
            key = (e["scene_id"], e["img_id"])
            lines.append("{},{},{},{},{},{},{}".format(
                e["scene_id"], e["img_id"], e["obj_id"], e["score"], " ".join(map(str, np.array(e["R"]).flatten().tolist())),
                " ".join(map(str, np.array(e["t"]).flatten().tolist())), per_image[key] + det_time[key]))
    path = os.path.join(output_dir, f"coarse_{object_dataset}-estimated-poses.csv")
    with open(path, "wb") as f:
        f.write("\n".join(lines).encode("utf-8"))
    return path
