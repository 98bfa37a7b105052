"""GPU: fp_pose_errors (MSSD / MSPD, csrc/pose_eval.hip) against a numpy restatement of utils/eval_errors.py, its exact-input,
tie, NaN, shape and argument edges; PoseEvaluator.update / update_batch against the reference's own evaluation
(tests/golden/pose_eval.npz); the driver's opt-in evaluation end to end and through the CLI."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, eval_util, infer, infer_pose_util, ops, repre_util, synthetic
from foundpose_amd.crop_util import PinholePlaneCameraModel
from tests import pose_eval_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rot(rng, deg=180.0):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.deg2rad(rng.uniform(-deg, deg))
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def _syms(rng, n):
    """n symmetry transforms: the identity and n-1 random rigid ones (small offsets)."""
    out = [{"R": np.eye(3), "t": np.zeros((3, 1))}]
    for _ in range(n - 1):
        out.append({"R": _rot(rng), "t": rng.normal(0, 2.0, (3, 1))})
    return out


def _hyp(rng, pts, syms):
    R_gt, t_gt = _rot(rng), np.array([rng.normal(0, 30), rng.normal(0, 30), rng.uniform(500, 900)])
    R_est, t_est = R_gt @ _rot(rng, 10), t_gt + rng.normal(0, 8, 3)
    K = np.array([[rng.uniform(500, 700), 0, rng.uniform(200, 400)], [0, rng.uniform(500, 700), rng.uniform(150, 300)], [0, 0, 1.0]])
    return dict(R_est=R_est, t_est=t_est, R_gt=R_gt, t_gt=t_gt, K=K, pts=pts, syms=syms)


def _run(hyps):
    """One fp_pose_errors call over `hyps` (each: R_est, t_est, R_gt, t_gt, K, pts, syms); objects shared by identity."""
    pts_off, pts_list, sym_off, ranges, est, pe, gt, pg = {}, [], 0, [], [], [], [], []
    n_pts = 0
    for h in hyps:
        if id(h["pts"]) not in pts_off:
            pts_off[id(h["pts"])] = n_pts
            pts_list.append(h["pts"])
            n_pts += len(h["pts"])
        e, p, g, q = ref.rows(h["R_est"], h["t_est"], h["R_gt"], h["t_gt"], h["K"], h["syms"])
        est.append(e), pe.append(p), gt.append(g), pg.append(q)
        ranges.append((pts_off[id(h["pts"])], len(h["pts"]), sym_off, len(h["syms"])))
        sym_off += len(h["syms"])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
    err, idx = ops.pose_errors(d(np.concatenate(pts_list)), d(np.stack(est)), d(np.stack(pe)), d(np.concatenate(gt)), d(np.concatenate(pg)), np.array(ranges))
    return err.cpu().numpy(), idx.cpu().numpy()


def _check(hyps, err, idx, rtol=1e-12):
    for h, hy in enumerate(hyps):
        want = ref.errors(hy["R_est"], hy["t_est"], hy["R_gt"], hy["t_gt"], hy["K"], hy["pts"], hy["syms"])
        for m in range(2):
            val, vtx, sym = want[3 * m:3 * m + 3]
            assert abs(err[h, m] - val) <= rtol * abs(val), (h, m, err[h, m], val)
            assert (idx[h, 2 * m], idx[h, 2 * m + 1]) == (vtx, sym), (h, m)


def test_random_ragged_batch_matches_numpy():
    rng = np.random.default_rng(0)
    objs = [(rng.normal(0, 40, (n, 3)), _syms(rng, s)) for n, s in ((1500, 1), (700, 2), (3333, 17), (64, 5), (513, 40))]
    hyps = [_hyp(rng, *objs[i % len(objs)]) for i in range(12)]
    err, idx = _run(hyps)
    _check(hyps, err, idx)   # (random fp64 inputs: ties or runner-ups within 1e-12 do not occur at these sizes)


def _exact_case(rng, n, nsym, tie=False):
    """Integer vertices, 90-degree rotations, integer translations and an integer K: every transformed coordinate is an exact
    integer, so the kernel and the numpy restatement must agree bit for bit, ties included."""
    perms = []
    for p in ([0, 1, 2], [1, 2, 0], [2, 0, 1]):
        for sgn in ([1, 1, 1], [-1, -1, 1], [-1, 1, -1], [1, -1, -1]):
            R = np.zeros((3, 3))
            R[np.arange(3), p] = sgn
            perms.append(R * np.linalg.det(R))
    pts = rng.integers(-20, 21, (n, 3)).astype(np.float64)
    syms = [{"R": perms[rng.integers(len(perms))], "t": rng.integers(-3, 4, (3, 1)).astype(np.float64)} for _ in range(nsym)]
    if tie:
        pts[n // 3] = pts[n // 2] = pts[-1] = [20, 20, 20]   # the same extreme vertex three times
        syms = syms[:2] + [syms[1]] + syms[2:]                # a duplicated symmetry: the lower one must win
        syms[0] = {"R": np.eye(3), "t": np.zeros((3, 1))}
    K = np.array([[600.0, 0, 320], [0, 600, 240], [0, 0, 1]])
    R_gt = perms[rng.integers(len(perms))]
    t_gt = np.array([3.0, -5.0, 400.0])
    return dict(R_est=perms[rng.integers(len(perms))], t_est=np.array([1.0, 2.0, 410.0]), R_gt=R_gt, t_gt=t_gt, K=K, pts=pts, syms=syms)


def test_exact_inputs_are_bit_equal_including_ties():
    rng = np.random.default_rng(1)
    hyps = [_exact_case(rng, 1000, 6), _exact_case(rng, 5000, 24, tie=True), _exact_case(rng, 77, 3, tie=True)]
    # planted ties in the symmetry choice: the estimate IS the ground truth under symmetries 1 and 2 (a duplicate)
    h = _exact_case(rng, 900, 5, tie=True)
    h["R_est"], h["t_est"] = h["R_gt"] @ h["syms"][1]["R"], h["R_gt"] @ h["syms"][1]["t"].ravel() + h["t_gt"]
    hyps.append(h)
    err, idx = _run(hyps)
    _check(hyps, err, idx, rtol=0.0)
    assert err[3, 0] == 0.0 and idx[3, 1] == 1 and idx[3, 0] == 0   # the first of the zero-error symmetries, vertex 0 of an all-zero row


def test_shapes_edges_and_production_worst_case():
    rng = np.random.default_rng(2)
    one = _hyp(rng, rng.normal(0, 40, (1, 3)), _syms(rng, 1))
    err, idx = _run([one])
    _check([one], err, idx)
    assert idx[0].tolist() == [0, 0, 0, 0]
    big = _hyp(rng, rng.normal(0, 40, (100_000, 3)), _syms(rng, 630))   # N = 1e5 vertices, S = 630 symmetries
    err, idx = _run([big])
    _check([big], err, idx)
    objs = [(rng.normal(0, 40, (int(n), 3)), _syms(rng, int(s))) for n, s in zip(rng.integers(1, 3000, 8), rng.integers(1, 50, 8))]
    mixed = [_hyp(rng, *objs[rng.integers(len(objs))]) for _ in range(64)]
    err, idx = _run(mixed)
    _check(mixed, err, idx)


def test_batch_independence_and_determinism():
    rng = np.random.default_rng(3)
    objs = [(rng.normal(0, 40, (n, 3)), _syms(rng, s)) for n, s in ((2500, 9), (600, 1), (9000, 33))]
    hyps = [_hyp(rng, *objs[i % 3]) for i in range(9)]
    err, idx = _run(hyps)
    err2, idx2 = _run(hyps)
    assert np.array_equal(err.view(np.int64), err2.view(np.int64)) and np.array_equal(idx, idx2)
    for h, hy in enumerate(hyps):
        e1, i1 = _run([hy])
        assert np.array_equal(e1[0].view(np.int64), err[h].view(np.int64)) and np.array_equal(i1[0], idx[h])


def test_vertex_at_camera_centre_follows_numpys_nan_rules():
    rng = np.random.default_rng(4)
    K = np.array([[600.0, 0, 320], [0, 610, 240], [0, 0, 1]])
    pts = rng.normal(0, 30, (800, 3))
    h = _hyp(rng, pts, _syms(rng, 4))
    # vertex 300 maps exactly onto the camera centre under the estimate: 0/0 in its projection, NaN under every symmetry's MSPD
    h["R_est"], h["t_est"], h["K"] = np.eye(3), np.array([3.0, -4.0, 700.0]), K
    pts[300] = -h["t_est"]
    err, idx = _run([h])
    want = ref.errors(h["R_est"], h["t_est"], h["R_gt"], h["t_gt"], h["K"], pts, h["syms"])
    assert np.isnan(want[3]) and np.isnan(err[0, 1]) and (idx[0, 2], idx[0, 3]) == (want[4], want[5]) == (300, 0)
    assert abs(err[0, 0] - want[0]) <= 1e-12 * want[0] and (idx[0, 0], idx[0, 1]) == (want[1], want[2])
    # a NaN under symmetry 2 only (its ground truth puts vertex 5 exactly on the camera centre): Python's min() skips it, np.argmin picks it
    h2 = _hyp(rng, rng.normal(0, 30, (500, 3)), _syms(rng, 4))
    h2["R_gt"], h2["t_gt"], h2["K"] = np.eye(3), np.array([1.0, 2.0, 650.0]), K
    h2["syms"][2] = {"R": np.eye(3), "t": np.array([[4.0], [-2.0], [9.0]])}
    h2["pts"][5] = -(h2["t_gt"] + h2["syms"][2]["t"].ravel())
    err, idx = _run([h2])
    want = ref.errors(h2["R_est"], h2["t_est"], h2["R_gt"], h2["t_gt"], h2["K"], h2["pts"], h2["syms"])
    assert not np.isnan(want[3]) and (want[4], want[5]) == (5, 2)
    assert abs(err[0, 1] - want[3]) <= 1e-12 * want[3] and (idx[0, 2], idx[0, 3]) == (5, 2)


def test_invalid_arguments_write_nothing():
    lib = _lib.lib()
    d = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")
    pts, est, pe, gt, pg = d(10, 3), d(2, 12), d(2, 12), d(4, 12), d(4, 12)
    err = torch.full((2, 2), -7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((2, 4), -7, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    good = np.array([[0, 10, 0, 2], [3, 5, 2, 2]], np.int32)

    def call(ranges=good, num_hyp=2, total_pts=10, total_syms=4, nbytes=1 << 16, null=None):
        p = [_lib.ptr(t) for t in (pts, est, pe, gt, pg)]
        if null is not None:
            p[null] = _lib.vp(0)
        r = np.ascontiguousarray(ranges, np.int32)
        return lib.fp_pose_errors(p[0], total_pts, p[1], p[2], p[3], p[4], total_syms, r.ctypes.data_as(_lib.vp), num_hyp, _lib.ptr(scratch), nbytes,
                                  _lib.ptr(err), _lib.ptr(idx), _lib.stream())
    bad = []
    for r in ([[0, 0, 0, 2], [3, 5, 2, 2]], [[0, 10, 0, 0], [3, 5, 2, 2]], [[0, 11, 0, 2], [3, 5, 2, 2]], [[-1, 5, 0, 2], [3, 5, 2, 2]],
              [[0, 10, 0, 2], [3, 5, 3, 2]], [[0, 10, -1, 2], [3, 5, 2, 2]]):
        bad.append(call(ranges=np.array(r)))
    bad += [call(num_hyp=0), call(nbytes=100)] + [call(null=k) for k in range(5)]
    r0 = np.ascontiguousarray(good)
    bad.append(lib.fp_pose_errors(_lib.ptr(pts), 10, _lib.ptr(est), _lib.ptr(pe), _lib.ptr(gt), _lib.ptr(pg), 4, _lib.vp(0), 2, _lib.ptr(scratch), 1 << 16,
                                  _lib.ptr(err), _lib.ptr(idx), _lib.stream()))
    bad.append(lib.fp_pose_errors(_lib.ptr(pts), 10, _lib.ptr(est), _lib.ptr(pe), _lib.ptr(gt), _lib.ptr(pg), 4, r0.ctypes.data_as(_lib.vp), 2, _lib.ptr(scratch), 1 << 16,
                                  _lib.vp(0), _lib.ptr(idx), _lib.stream()))
    torch.cuda.synchronize()
    assert bad == [1] * len(bad)   # FP_ERR_INVALID
    assert (err == -7.0).all() and (idx == -7).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (idx[:, 1] >= 0).all() and (idx[:, 1] < 2).all()


def test_cpu_tensors_raise():
    z = torch.zeros(4, 12, dtype=torch.float64)
    with pytest.raises(_lib.FoundPoseNativeError, match="CPU tensor"):
        ops.pose_errors(torch.zeros(5, 3, dtype=torch.float64), z[:1], z[:1], z, z, [[0, 5, 0, 4]])


# ------------------------------------------------------------------------------------------------ the reference's evaluator
def _golden_items():
    g = dict(np.load(os.path.join(GOLDEN, "pose_eval.npz")))
    infos = {int(k): v for k, v in json.loads(str(g["model_infos"])).items()}
    syms = {lid: eval_util.get_symmetry_transformations(infos[lid], 0.01) for lid in infos}
    items = []
    for i in range(len(g["in_lid"])):
        lid = int(g["in_lid"][i])
        f, c = g["in_f"][i], g["in_c"][i]
        mk = lambda T: PinholePlaneCameraModel(96, 96, f, c, T)
        items.append(dict(scene_id=7, im_id=10 + i, inst_id=int(g["in_h"][i]), hypothesis_id=0, base_image=None, object_repre_vertices=g["in_repre"][lid - 1],
                          obj_lid=lid, object_pose_m2w=(g["in_T_est"][i][:3, :3], g["in_T_est"][i][:3, 3:]),
                          object_pose_m2w_gt=(g["in_T_gt"][i][:3, :3], g["in_T_gt"][i][:3, 3:]), orig_camera_c2w=mk(g["in_T_oc"][i]),
                          camera_c2w=mk(g["in_T_cc"][i]), pred_mask=g["in_pred"][i], gt_mask=g["in_gt"][i],
                          corresp={"nn_vertex_ids": g["in_vid"][i], "coord_2d": g["in_uv"][i], "coord_2d_ids": g["in_qid"][i]},
                          retrieved_templates_camera_m2c=[{"T_world_from_eye": T} for T in g["in_tpl"][i]], time_per_inst={"prep": 0.01 * (int(g["in_h"][i]) + 1), "pose_coarse": 0.02},
                          object_mesh_vertices=g["in_pts"][lid - 1], object_syms=syms[lid], object_diameter=infos[lid]["diameter"], inlier_radius=10.0))
    return g, items


def _split(g, k):
    return np.split(g[k], np.cumsum(g[k + "_len"])[:-1])


def test_update_matches_the_reference_fixture():
    g, items = _golden_items()
    ev = eval_util.PoseEvaluator()
    got = [ev.update(**it) for it in items]
    rel = lambda a, b, tol: abs(a - b) <= tol * abs(b)
    for i, r in enumerate(got):
        assert rel(r["mssd"], g["mssd"][i], 1e-9) and rel(r["mspd"], g["mspd"][i], 1e-9) and rel(r["normalized_mssd"], g["mssd_n"][i], 1e-9), i
        assert (r["mssd_id"], r["mspd_id"]) == (g["mssd_id"][i], g["mspd_id"][i]), i
        assert abs(r["rotation_errors"] - g["rotation_errors"][i]) <= 1e-6 and abs(r["template_ori_err"] - g["template_ori_err"][i]) <= 1e-6, i
        assert rel(r["translation_errors"], g["translation_errors"][i], 1e-9) and r["mask_iou"] == g["mask_iou"][i]
        assert np.array_equal(r["inliers_gt"], _split(g, "inliers_gt")[i]) and np.array_equal(r["inliers_est"], _split(g, "inliers_est")[i])
        assert r["inliers_gt_err"]["10"] == g["inliers_gt_err"][i] and r["inliers_est_err"]["10"] == g["inliers_est_err"][i]
        np.testing.assert_allclose(r["point_errors"], _split(g, "point_errors")[i], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(r["corr_dist_gt"], _split(g, "corr_dist_gt")[i], rtol=1e-9, atol=1e-9)
    ev.detection_times = {(7, 10 + i): 0.5 for i in range(len(items))}
    # estimated-poses.json: the reference's extended entries
    want = json.load(open(os.path.join(GOLDEN, "pose_eval_estimated-poses.json")))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        ev.save_results_json(os.path.join(d, "e.json"))
        mine = json.load(open(os.path.join(d, "e.json")))
    assert [set(e) for e in mine] == [set(e) for e in want]
    for a, b in zip(mine, want):
        for k in ("scene_id", "img_id", "obj_id", "inst_id", "hypothesis_id", "inliers_gt", "inliers_est", "inliers_gt_err", "inliers_est_err", "time", "cnos_time", "score"):
            assert a[k] == b[k], k
        for k in ("mssd", "mspd", "mssd_n"):
            assert rel(a[k], b[k], 1e-9), k
        np.testing.assert_allclose(np.array(a["R"]), np.array(b["R"]), rtol=0, atol=1e-12)


def test_update_batch_equals_update():
    _, items = _golden_items()
    ev1, ev2 = eval_util.PoseEvaluator(), eval_util.PoseEvaluator()
    one = [ev1.update(**it) for it in items]
    many = ev2.update_batch(items[::-1])[::-1]
    for a, b in zip(one, many):
        for k in ("mssd", "mspd", "normalized_mssd", "mssd_id", "mspd_id", "mssd_sym", "mspd_sym", "rotation_errors", "template_ori_err"):
            assert a[k] == b[k], k


# ------------------------------------------------------------------------------------------------ the driver
def _eval_model(syms=None):
    mesh = synthetic.make_blob_mesh(50, 50, radius=55.0, seed=7)
    return eval_util.EvalModel(mesh.vertices.astype(np.float64), syms or [{"R": np.eye(3), "t": np.zeros((3, 1))}], 120.0)


def test_driver_evaluates_annotated_frames(tmp_path):
    from foundpose_amd import feature_util
    from tests.test_gpu_infer_driver import NAME, _scene
    ex = feature_util.make_feature_extractor(NAME, random_init_seed=1234, precision="fp32").to("cuda")
    sc = _scene(tmp_path, ex)
    o1 = sc["opts"]._replace(num_preds_factor=1.0)
    dets = infer_pose_util.load_detections_in_bop_format(str(sc["det_path"]))
    rep = {1: repre_util.load_object_repre(sc["rdir"])}
    planted = []
    for b in range(2):
        T_m2c = np.eye(4)
        T_m2c[:3, :3], T_m2c[:3, 3] = sc["R"][b].numpy(), sc["t"][b].numpy()
        planted.append(sc["cams"][b].T_world_from_eye @ T_m2c)   # model -> world (the original camera is the world)
    flip = np.diag([-1.0, -1.0, 1.0, 1.0])                         # a 2-fold symmetry about the model's z axis

    class Anno:
        def __init__(self, b, pose_T=None):
            self.lid, self.visibilities, self.masks_modal = 1, 0.9, sc["masks"][b]
            self.boxes_amodal = np.array(sc["boxes_xyxy"][b], np.float32)
            self.pose = None if pose_T is None else infer.GtPose(pose_T[:3, :3], pose_T[:3, 3:])

    def run(tag, annos, models=None):
        d = str(tmp_path / tag)
        fr = lambda lid: iter([{"scene_id": 1, "im_id": 3, "image": sc["image"], "camera": sc["cam"], "gt_annos": annos}])
        infer.infer(o1, fr, dets, rep, d, extractor=ex, eval_models=models)
        return json.load(open(os.path.join(d, "1", "estimated-poses.json")))

    plain = run("plain", [Anno(0), Anno(1)])
    posed_no_eval = run("posed", [Anno(0, planted[0]), Anno(1, planted[1])])
    ev = run("eval", [Anno(0, planted[0]), Anno(1, planted[1])], {1: _eval_model()})
    base = lambda es: [(e["scene_id"], e["img_id"], e["obj_id"], e["inst_id"], e["hypothesis_id"], e["score"], e["R"], e["t"], sorted(e)) for e in es]
    assert len(plain) == 2 and base(posed_no_eval) == base(plain)
    assert set(plain[0]) == {"scene_id", "img_id", "obj_id", "inst_id", "hypothesis_id", "score", "R", "t", "time", "cnos_time"}
    assert [(e["inst_id"], e["R"], e["t"]) for e in ev] == [(e["inst_id"], e["R"], e["t"]) for e in plain]
    bound = (2.0 + 55.0 * np.deg2rad(1.0) * 1.2) / 120.0     # the onboarding test's 1 degree / 2 mm on this 55 mm blob
    for e in ev:
        assert {"mssd", "mspd", "mssd_n", "inliers_gt", "inliers_est", "inliers_gt_err", "inliers_est_err"} <= set(e)
        assert e["mssd_n"] < bound and e["mssd"] == pytest.approx(e["mssd_n"] * 120.0)
    # the ground truth is the estimate composed with the symmetry: ~0 with the symmetry declared, large without it
    sym = [{"R": np.eye(3), "t": np.zeros((3, 1))}, {"R": flip[:3, :3], "t": np.zeros((3, 1))}]
    flipped = [Anno(0, planted[0] @ flip), Anno(1, planted[1] @ flip)]
    with_sym = run("sym", flipped, {1: _eval_model(sym)})
    no_sym = run("nosym", flipped, {1: _eval_model()})
    for a, b in zip(with_sym, no_sym):
        assert a["mssd_n"] < bound and b["mssd"] > 50.0


def test_cli_eval_gt_on_a_bop_tree(tmp_path):
    from PIL import Image
    from foundpose_amd import feature_util
    from foundpose_amd.renderer import save_ply
    from foundpose_amd.vit_config import ARCHS
    from tests.test_gpu_infer_driver import NAME, _scene
    sd = synthetic.make_vit_state_dict(ARCHS["vits14-reg"], seed=77)
    ck = tmp_path / "ckpt"
    ck.mkdir()
    torch.save(sd, ck / "dinov2_vits14_reg4_pretrain.pth")
    ex = feature_util.make_feature_extractor(NAME, state_dict=sd, precision="fp32").to("cuda")
    sc = _scene(tmp_path, ex)
    root = tmp_path / "synth"
    sdir = root / "test" / "000001"
    (sdir / "rgb").mkdir(parents=True)
    (sdir / "mask_visib").mkdir()
    Image.fromarray(sc["image"]).save(sdir / "rgb" / "000003.png")
    cam = sc["cam"]
    (sdir / "scene_camera.json").write_text(json.dumps({"3": {"cam_K": [cam.f[0], 0, cam.c[0], 0, cam.f[1], cam.c[1], 0, 0, 1], "depth_scale": 1.0}}))
    gts, infos = [], []
    for b in range(2):
        T_m2c = np.eye(4)
        T_m2c[:3, :3], T_m2c[:3, 3] = sc["R"][b].numpy(), sc["t"][b].numpy()
        T = sc["cams"][b].T_world_from_eye @ T_m2c
        gts.append({"cam_R_m2c": T[:3, :3].ravel().tolist(), "cam_t_m2c": T[:3, 3].tolist(), "obj_id": 1})
        x1, y1, x2, y2 = sc["boxes_xyxy"][b]
        infos.append({"bbox_obj": [x1, y1, x2 - x1, y2 - y1], "visib_fract": 0.9})
        Image.fromarray((sc["masks"][b] * 255).astype(np.uint8)).save(sdir / "mask_visib" / f"000003_{b:06d}.png")
    (sdir / "scene_gt.json").write_text(json.dumps({"3": gts}))
    (sdir / "scene_gt_info.json").write_text(json.dumps({"3": infos}))
    (root / "test_targets_bop19.json").write_text(json.dumps([{"scene_id": 1, "im_id": 3, "obj_id": 1, "inst_count": 2}]))
    (root / "models").mkdir()
    save_ply(str(root / "models" / "obj_000001.ply"), synthetic.make_blob_mesh(50, 50, radius=55.0, seed=7))
    (root / "models" / "models_info.json").write_text(json.dumps({"1": {"diameter": 120.0, "symmetries_discrete": [np.diag([-1.0, -1, 1, 1]).ravel().tolist()]}}))
    argv = ["--opts", str(sc["opts_path"]), "--dataset-dir", str(root / "test"), "--detections", str(sc["det_path"]), "--repre-dir", str(tmp_path / "object_repre"),
            "--precision", "fp32", "--weights", str(ck)]
    infer.main(argv + ["--output-dir", str(tmp_path / "plain")])
    infer.main(argv + ["--output-dir", str(tmp_path / "eval"), "--eval-gt"])
    plain = json.load(open(tmp_path / "plain" / "1" / "estimated-poses.json"))
    ev = json.load(open(tmp_path / "eval" / "1" / "estimated-poses.json"))
    assert len(plain) == len(ev) == 2 and all("mssd" not in e for e in plain)
    for a, b in zip(plain, ev):
        assert (a["inst_id"], a["R"], a["t"]) == (b["inst_id"], b["R"], b["t"])
        assert b["mssd"] < 5.0 and b["mspd"] < 5.0 and b["inliers_gt"] > 0
