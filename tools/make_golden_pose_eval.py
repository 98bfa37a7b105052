"""Freezes the reference's pose evaluation into tests/golden/pose_eval.npz and tests/golden/pose_eval_estimated-poses.json
(BUILD CONTAINER ONLY: it imports the reference checkout).

Seeded synthetic inputs -- three objects (asymmetric; a 2-fold discrete symmetry; a continuous symmetry about z combined
with a 2-fold discrete one, 628 transforms), 2000 vertices each, crop cameras that differ from the original camera --
go through the reference's own utils/eval_util.py EvaluatorPose.update (and so utils/eval_errors.py mssd / mspd / re /
compute_rotation_error with the real scipy) and save_results_json.  bop_toolkit_lib is not part of the reference
checkout: a stand-in is registered here with misc.transform_pts_Rt / project_pts restated from the toolkit's published
code and an empty inout; the symmetry transforms come from foundpose_amd.eval_util.get_symmetry_transformations (the
toolkit's expansion is unpinned).  The npz holds the inputs as well, so the tests need nothing else.

    python tools/make_golden_pose_eval.py
"""
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from foundpose_amd.eval_util import get_symmetry_transformations  # noqa: E402
from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
N_PTS, N_REPRE, N_CORR, IMG = 2000, 300, 120, 96
MODEL_INFOS = {
    1: {"diameter": 180.0},
    2: {"diameter": 150.0, "symmetries_discrete": [[-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]]},
    3: {"diameter": 120.0, "symmetries_discrete": [[1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 4.0, 0, 0, 0, 1]],
        "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 2.0]}]},
}


def _rot(rng, deg=180.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(rng.uniform(-deg, deg))
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def _rigid(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, np.asarray(t).reshape(3)
    return T


def make_inputs(seed=2024):
    """Every input array of the fixture, deterministic in `seed`."""
    rng = np.random.default_rng(seed)
    cases = []
    for lid in (1, 2, 3):
        pts = rng.normal(0, 40.0, (N_PTS, 3)) * np.array([1.0, 0.8, 1.2])
        repre = rng.normal(0, 35.0, (N_REPRE, 3))
        for h in range(2):
            T_oc = _rigid(_rot(rng, 20), rng.normal(0, 30, 3))                 # original camera (c2w)
            T_cc = _rigid(_rot(rng, 8) @ T_oc[:3, :3], T_oc[:3, 3])             # crop camera: same centre, turned
            R_gt_c = _rot(rng)
            t_gt_c = np.array([rng.normal(0, 40), rng.normal(0, 40), rng.uniform(600, 900)])
            T_gt = T_oc @ _rigid(R_gt_c, t_gt_c)                                # model -> world
            dR = _rot(rng, 6 if h == 0 else 25)
            T_est = T_gt @ _rigid(dR, rng.normal(0, 5 if h == 0 else 20, 3))
            if lid >= 2 and h == 1:                                              # an estimate that is a symmetric copy of the GT
                T_est = T_gt @ _rigid(np.diag([-1.0, -1.0, 1.0]), [0, 0, 0]) @ _rigid(_rot(rng, 2), rng.normal(0, 1, 3))
            f = rng.uniform(500, 700, 2)
            c = np.array([IMG / 2, IMG / 2]) + rng.normal(0, 3, 2)
            vid = rng.integers(0, N_REPRE, N_CORR)
            vc = (np.linalg.inv(T_cc) @ T_est @ np.hstack([repre[vid], np.ones((N_CORR, 1))]).T).T[:, :3]
            uv = vc[:, :2] / vc[:, 2:] * f + c + rng.normal(0, 6.0, (N_CORR, 2))
            qid = np.sort(rng.integers(0, N_CORR // 2, N_CORR))
            pred = np.zeros((IMG, IMG), np.uint8)
            gt = np.zeros((IMG, IMG), np.uint8)
            x0, y0 = rng.integers(5, 30, 2)
            pred[y0:y0 + 50, x0:x0 + 45] = 1
            gt[y0 + 4:y0 + 52, x0 - 3:x0 + 40] = 1
            tpl = np.stack([_rigid(_rot(rng), [0, 0, 500.0]) for _ in range(5)])
            cases.append(dict(lid=lid, h=h, pts=pts, repre=repre, T_oc=T_oc, T_cc=T_cc, T_gt=T_gt, T_est=T_est, f=f, c=c, vid=vid, uv=uv,
                              qid=qid, pred=pred, gt=gt, tpl=tpl, times={"prep": 0.01 * (h + 1), "pose_coarse": 0.02}))
    return cases


def _install_bop_standin():
    bop = types.ModuleType("bop_toolkit_lib")
    for sub in ("inout", "misc"):
        m = types.ModuleType(f"bop_toolkit_lib.{sub}")
        setattr(bop, sub, m)
        sys.modules[f"bop_toolkit_lib.{sub}"] = m
    sys.modules["bop_toolkit_lib"] = bop

    def transform_pts_Rt(pts, R, t):
        assert pts.shape[1] == 3
        return (R.dot(pts.T) + t.reshape((3, 1))).T

    def project_pts(pts, K, R, t):
        assert pts.shape[1] == 3
        P = K.dot(np.hstack((R, t)))
        pts_h = np.hstack((pts, np.ones((pts.shape[0], 1))))
        pts_im = P.dot(pts_h.T)
        pts_im /= pts_im[2, :]
        return pts_im[:2, :].T
    bop.misc.transform_pts_Rt, bop.misc.project_pts = transform_pts_Rt, project_pts
    for name, attrs in (("skimage", ()), ("skimage.color", ("label2rgb",)), ("skimage.feature", ("canny",)), ("skimage.morphology", ("binary_dilation",)),
                        ("imageio", ()), ("trimesh", ()), ("pyrender", ()), ("distinctipy", ())):   # visualisation-only imports
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except Exception:
                m = types.ModuleType(name)
                for a_ in attrs:
                    setattr(m, a_, None)
                sys.modules[name] = m


def main():
    if not ref_shim.reference_available():
        sys.exit("reference not present; fixtures can only be generated in the build container")
    ref_shim.import_reference()          # the reference on sys.path, with the stand-ins of its native dependencies
    _install_bop_standin()
    eu = importlib.import_module("utils.eval_util")
    structs = importlib.import_module("utils.structs")
    cases = make_inputs()
    ev = eu.EvaluatorPose([1, 2, 3])
    out = {k: [] for k in ("mssd", "mspd", "mssd_n", "mssd_id", "mspd_id", "rotation_errors", "translation_errors", "template_ori_err",
                           "mask_iou", "inliers_gt_err", "inliers_est_err", "n_inliers_gt", "n_inliers_est")}
    flat = {k: [] for k in ("point_errors", "inliers_gt", "inliers_est", "corr_dist_gt", "corr_dist_est")}
    for i, d in enumerate(cases):
        syms = get_symmetry_transformations(MODEL_INFOS[d["lid"]], 0.01)
        mk = lambda T: structs.PinholePlaneCameraModel(width=IMG, height=IMG, f=d["f"], c=d["c"], T_world_from_eye=T)
        tpl = [structs.PinholePlaneCameraModel(width=IMG, height=IMG, f=d["f"], c=d["c"], T_world_from_eye=T) for T in d["tpl"]]
        ev.detection_times[(7, 10 + i)] = 0.5
        r = ev.update(scene_id=7, im_id=10 + i, inst_id=d["h"], hypothesis_id=0, base_image=None, object_repre_vertices=d["repre"], obj_lid=d["lid"],
                      object_pose_m2w=structs.ObjectPose(R=d["T_est"][:3, :3], t=d["T_est"][:3, 3:]),
                      object_pose_m2w_gt=structs.ObjectPose(R=d["T_gt"][:3, :3], t=d["T_gt"][:3, 3:]),
                      orig_camera_c2w=mk(d["T_oc"]), camera_c2w=mk(d["T_cc"]), pred_mask=d["pred"], gt_mask=d["gt"],
                      corresp={"nn_vertex_ids": d["vid"], "coord_2d": d["uv"], "coord_2d_ids": d["qid"]}, retrieved_templates_camera_m2c=tpl,
                      time_per_inst=d["times"], object_mesh_vertices=d["pts"], object_syms=syms, object_diameter=MODEL_INFOS[d["lid"]]["diameter"],
                      inlier_radius=10.0)
        out["mssd"].append(r["mssd"]), out["mspd"].append(r["mspd"]), out["mssd_n"].append(r["normalized_mssd"])
        out["mssd_id"].append(r["mssd_id"]), out["mspd_id"].append(r["mspd_id"])
        out["rotation_errors"].append(float(ev.rotation_errors[-1])), out["translation_errors"].append(float(ev.translation_errors[-1]))
        out["template_ori_err"].append(ev.template_ori_err[-1]), out["mask_iou"].append(ev.mask_iou[-1])
        out["inliers_gt_err"].append(r["inliers_gt_err"]["10"]), out["inliers_est_err"].append(r["inliers_est_err"]["10"])
        out["n_inliers_gt"].append(len(r["inliers_gt"])), out["n_inliers_est"].append(len(r["inliers_est"]))
        flat["point_errors"].append(ev.point_errors[-1])
        for k in ("inliers_gt", "inliers_est", "corr_dist_gt", "corr_dist_est"):
            flat[k].append(r[k])
    tmp = tempfile.mkdtemp()
    ev.save_results_json(os.path.join(tmp, "est.json"))
    with open(os.path.join(tmp, "est.json")) as f:
        est_json = json.load(f)
    arrays = {"in_" + k: np.stack([d[k] for d in cases]) for k in ("T_oc", "T_cc", "T_gt", "T_est", "f", "c", "vid", "uv", "qid", "pred", "gt", "tpl")}
    arrays["in_lid"] = np.array([d["lid"] for d in cases])
    arrays["in_h"] = np.array([d["h"] for d in cases])
    arrays["in_pts"] = np.stack([cases[i]["pts"] for i in (0, 2, 4)])
    arrays["in_repre"] = np.stack([cases[i]["repre"] for i in (0, 2, 4)])
    arrays["model_infos"] = np.array(json.dumps(MODEL_INFOS))
    for k, v in out.items():
        arrays[k] = np.array(v)
    for k, v in flat.items():
        arrays[k] = np.concatenate(v)
        arrays[k + "_len"] = np.array([len(x) for x in v])
    np.savez_compressed(os.path.join(OUT, "pose_eval.npz"), **arrays)
    with open(os.path.join(OUT, "pose_eval_estimated-poses.json"), "w") as f:
        json.dump(est_json, f, indent=2)
    print("pose_eval.npz:", {k: np.round(np.asarray(out[k]), 4).tolist() for k in ("mssd", "mspd", "rotation_errors")})


if __name__ == "__main__":
    main()
