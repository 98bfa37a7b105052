"""GPU: featuremetric refinement of the best coarse pose (csrc/refine.hip, refine_util, engine keep_feature_map, the driver's
final_pose_type="featuremetric") against the numpy restatement tests/featuremetric_ref.py."""
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, refine_util, synthetic
from tests import featuremetric_ref as fr

pytestmark = pytest.mark.gpu
W = H = 518
CAM = (600.0, 605.0, 259.0, 257.0)


def _pose(rng, z=600.0):
    return fr.rot_exp(rng.normal(size=3) * 0.5), np.array([rng.uniform(-20, 20), rng.uniform(-20, 20), z])


def _blob_points(n, seed):
    v = synthetic.make_blob_mesh(30, 30, radius=50.0, seed=seed).vertices.astype(np.float32)
    return v[np.random.default_rng(seed).choice(len(v), n, replace=False)]


def _run(maps, dets, iters=30, normal_eq=False, max_points=None):
    """maps: list of [gh, gw, C] fp32 arrays (one per detection); dets: list of dict(X, f, R, t, has_pose=True) -> refine dict (cpu numpy)."""
    B = len(dets)
    X = np.concatenate([d["X"] for d in dets]).astype(np.float32)
    f = np.concatenate([d["f"] for d in dets]).astype(np.float32)
    n = np.array([len(d["X"]) for d in dets])
    rb = np.concatenate([[0], np.cumsum(n)[:-1]])
    cuda = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    out = refine_util.refine_featuremetric(
        cuda(np.stack(maps)), (W, H), [CAM] * B, cuda(np.stack([d["R"] for d in dets]), torch.float64), cuda(np.stack([d["t"] for d in dets]), torch.float64),
        cuda(rb, torch.int32), cuda(rb + n, torch.int32), cuda(f), cuda(X), cuda(np.array([d.get("has_pose", True) for d in dets])),
        iters=iters, return_normal_equations=normal_eq, max_points=max_points)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _planted(seed, C=64, n=300, rot_deg=3.0, trans_mm=10.0):
    rng = np.random.default_rng(seed)
    M = fr.smooth_field(37, 37, C, seed)
    X = _blob_points(n, seed)
    R, t = _pose(rng)
    f = fr.sample_at(M, R, t, X, CAM, W, H)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    dt = rng.normal(size=3)
    dt *= trans_mm / np.linalg.norm(dt)
    R0 = fr.rot_exp(ax * np.radians(rot_deg)) @ R
    return M, dict(X=X, f=f, R=R0, t=t + dt), (R, t)


@pytest.mark.parametrize("C", [64, 256])
def test_normal_equations_match_restatement(C):
    rng = np.random.default_rng(C)
    maps, dets = [], []
    for k in range(4):
        M = fr.smooth_field(37, 37, C, 10 * C + k, terms=2)
        R, t = _pose(rng)
        n = int(rng.integers(150, 400))
        uv = rng.uniform(10, 508, size=(n, 2))
        z = rng.uniform(550, 650, size=n)
        Xc = np.stack([(uv[:, 0] - CAM[2]) / CAM[0] * z, (uv[:, 1] - CAM[3]) / CAM[1] * z, z], 1)
        X = ((Xc - t) @ R).astype(np.float32)       # R^T (Xc - t)
        f = rng.normal(size=(n, C)).astype(np.float32) * 0.5
        maps.append(M)
        dets.append(dict(X=X, f=f, R=R, t=t))
    out = _run(maps, dets, iters=0, normal_eq=True)
    for b, d in enumerate(dets):
        want = fr.normal_equations(d["R"], d["t"], d["X"].astype(np.float64), d["f"], CAM, W, H, maps[b])
        got = out["normal_eq"][b]
        for lo, hi in ((0, 21), (21, 27), (27, 28)):
            scale = np.abs(want[lo:hi]).max()
            assert np.abs(got[lo:hi] - want[lo:hi]).max() <= 1e-4 * scale, (b, lo, got[lo:hi], want[lo:hi])
        assert out["status"][b] == 1 and out["iters_used"][b] == 0
        assert out["num_points"][b] == int(fr.valid_set(d["R"], d["t"], d["X"], CAM, W, H, maps[b]).sum())
        assert out["cost_in"][b] == out["cost_out"][b] == got[27]


def _reproj_rms(R, t, R_gt, t_gt, X):
    def uv(R_, t_):
        Xc = X.astype(np.float64) @ R_.T + t_
        return np.stack([CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2], CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]], 1)
    return float(np.sqrt(np.mean(np.sum((uv(R, t) - uv(R_gt, t_gt)) ** 2, 1))))


def test_planted_field_converges_to_ground_truth():
    for seed in (1, 2, 3):
        M, det, (R_gt, t_gt) = _planted(seed)
        out = _run([M], [det])
        R, t = out["R"][0], out["t"][0]
        coarse = _reproj_rms(det["R"], det["t"], R_gt, t_gt, det["X"])
        fine = _reproj_rms(R, t, R_gt, t_gt, det["X"])
        print(f"seed {seed}: reprojection RMS {coarse:.3f} px (start) -> {fine:.5f} px (refined), rotation "
              f"{fr.rot_angle_deg(det['R'], R_gt):.3f} -> {fr.rot_angle_deg(R, R_gt):.5f} deg, {out['iters_used'][0]} iterations")
        assert out["status"][0] == 0 and out["cost_out"][0] < out["cost_in"][0]
        assert fine < 0.02, fine
        ref = fr.refine(det["R"], det["t"], det["X"].astype(np.float64), det["f"], CAM, W, H, M)
        assert np.radians(fr.rot_angle_deg(R, ref["R"])) < 1e-6 and np.linalg.norm(t - ref["t"]) < 1e-3


def test_batch_invariance_and_determinism():
    probe = [_planted(s) for s in (5, 6)]
    alone = [_run([M], [d]) for M, d, _ in probe]
    maps, dets = [], []
    for k in range(32):
        if k in (3, 20):
            M, d, _ = probe[0 if k == 3 else 1]
        else:
            M, d, _ = _planted(100 + k, n=int(50 + 17 * k))
        maps.append(M)
        dets.append(d)
    batch = _run(maps, dets, max_points=600)
    again = _run(maps, dets, max_points=600)
    for key in batch:
        assert np.array_equal(batch[key], again[key]), key
    for j, k in enumerate((3, 20)):
        for key in alone[j]:
            assert np.array_equal(alone[j][key][0], batch[key][k]), (key, k)


def test_degenerate_inputs():
    M, det, (R_gt, t_gt) = _planted(9)
    few = dict(det, X=det["X"][:5], f=det["f"][:5])
    behind = dict(det, t=np.array([0.0, 0.0, -600.0]))
    outside = dict(det, t=np.array([4000.0, 0.0, 600.0]))      # every point projects far outside the map
    nopose = dict(det, has_pose=False)
    at_opt = dict(det, R=R_gt, t=t_gt)
    dets = [few, behind, outside, nopose, at_opt]
    out = _run([M] * len(dets), dets)
    for b in range(4):
        assert out["status"][b] == 2, b
        assert np.array_equal(out["R"][b].reshape(3, 3), dets[b]["R"]) and np.array_equal(out["t"][b], dets[b]["t"]), b
    assert out["num_points"][0] == 5 and out["num_points"][1] == 0 and out["num_points"][2] == 0
    s = out["status"][4]
    assert s in (0, 1)
    if s == 1:
        assert np.array_equal(out["R"][4], R_gt) and np.array_equal(out["t"][4], t_gt)
    else:
        assert fr.rot_angle_deg(out["R"][4], R_gt) < 1e-4 and np.linalg.norm(out["t"][4] - t_gt) < 1e-3
    assert out["cost_out"][4] <= out["cost_in"][4]
    from foundpose_amd.bank import DeviceBank
    from foundpose_amd.matching import MatchResult
    # maps smaller than 2 x 2 are refused
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    with pytest.raises(ValueError):
        refine_util.refine_featuremetric(z(1, 1, 1, 8), (14, 14), [CAM], z(1, 3, 3), z(1, 3), z(1, dt=torch.int32), z(1, dt=torch.int32),
                                         z(10, 8), z(10, 3), z(1, dt=torch.bool))
    # a bank row range outside the bank is reported, not read
    with pytest.raises(_lib.FoundPoseNativeError, match="bank rows"):
        refine_util.refine_featuremetric(z(1, 4, 4, 8), (56, 56), [CAM], z(1, 3, 3), z(1, 3), z(1, dt=torch.int32),
                                         torch.full((1,), 11, dtype=torch.int32, device="cuda"), z(10, 8), z(10, 3),
                                         torch.ones(1, dtype=torch.bool, device="cuda"), max_points=64)
    # template id -1 / no coarse pose in a MatchResult -> has_pose false
    rs = _tiny_repre()
    bank = DeviceBank([rs])
    ids = torch.tensor([[2, -1], [-1, 1], [0, 1]], dtype=torch.int32, device="cuda")
    res = MatchResult(template_ids=ids, template_scores=z(3, 2), counts=z(3, 2, dt=torch.int32), q_ids=z(3, 2, 1, dt=torch.int32),
                      feat_ids=z(3, 2, 1, dt=torch.int32), dists=z(3, 2, 1), conf=z(3, 2, 1), coord_2d=z(3, 2, 1, 2), coord_3d=z(3, 2, 1, 3))
    best = {"found": torch.tensor([True, True, False], device="cuda"), "corresp_id": torch.tensor([0, 0, 1], device="cuda")}
    rb, re, ok = refine_util.best_template_rows(res, best, bank, [0, 0, 0])
    off = bank.tpl_off.cpu().tolist()
    assert ok.cpu().tolist() == [True, False, False]
    assert (int(rb[0]), int(re[0])) == (off[2], off[3])


def _tiny_repre():
    from foundpose_amd import repre_util
    g = torch.Generator().manual_seed(0)
    f2t = torch.tensor([0] * 7 + [1] * 9 + [2] * 8)
    n = len(f2t)
    return repre_util.FeatureBasedObjectRepre(
        vertices=torch.randn(n, 3, generator=g), feat_vectors=torch.randn(n, 16, generator=g), feat_to_template_ids=f2t,
        feat_cluster_centroids=torch.randn(4, 16, generator=g), feat_cluster_idfs=torch.ones(4), template_descs=torch.rand(3, 4, generator=g),
        template_desc_opts=repre_util.TemplateDescOpts())


# ---------------------------------------------------------------------------------------------------- engine + driver
NAME = "dinov2_version=vits14-reg_stride=14_facet=token_layer=9_logbin=0_norm=1"


def _engine_inputs(tmp_path, precision):
    from foundpose_amd import crop_util, feature_util, repre_util
    from tests.test_gpu_infer_driver import _scene
    ex = feature_util.make_feature_extractor(NAME, random_init_seed=1234, precision=precision).to("cuda")
    sc = _scene(tmp_path, ex)
    img = torch.from_numpy(sc["image"]).cuda().float() / 255.0
    crops, cmasks, cams = crop_util.crop_detections(img, torch.from_numpy(sc["masks"]).cuda(), sc["boxes_xyxy"], sc["cam"], (224, 224), 0.2)
    return ex, sc, repre_util.load_object_repre(sc["rdir"]), crops, cmasks, cams


@pytest.mark.parametrize("overlap", [False, True])
def test_engine_keeps_the_projected_map_without_changing_matches(tmp_path, overlap):
    from foundpose_amd import engine as fe
    from foundpose_amd.bank import DeviceBank
    from foundpose_amd.projector_util import project_features
    ex, sc, repre, crops, cmasks, cams = _engine_inputs(tmp_path, "bf16")
    assert ex.supports_token_selection
    for det_obj, repres in (([0, 0], [repre]), ([0, 1], [repre, repre])):
        eng = fe.FoundPoseEngine(ex, DeviceBank(repres), 14.0, 5, 300, tie_order="torch", overlap_matching=overlap)
        a = eng.infer_batch(crops, cmasks, det_obj).wait()
        b = eng.infer_batch(crops, cmasks, det_obj, keep_feature_map=True).wait()
        assert a.feature_map is None and b.feature_map is not None
        for k in ("template_ids", "template_scores", "counts", "q_ids", "feat_ids", "dists", "conf", "coord_2d", "coord_3d"):
            assert torch.equal(getattr(a, k).view(torch.int32), getattr(b, k).view(torch.int32)), k   # bits (conf holds NaN: 0 / 0)
        torch.cuda.synchronize()
        fm = ex(crops)["feature_maps"]                         # [B, D, gh, gw]
        B, D, gh, gw = fm.shape
        assert b.feature_map.shape == (B, gh, gw, eng.bank.feat_dim)
        for i, o in enumerate(det_obj):
            want = project_features(fm[i].permute(1, 2, 0).reshape(-1, D).contiguous(), eng.bank.objects[o].projectors).reshape(gh, gw, -1)
            err = float((b.feature_map[i] - want).abs().max() / want.abs().max())
            assert err < 1e-5, err


def test_refine_best_coarse_on_rendered_features(tmp_path):
    """tests/test_gpu_onboarding.py's setup: a template is the query; its pose perturbed by 2 deg / 5 mm is refined on real features."""
    from PIL import Image
    from foundpose_amd import engine as fe, feature_util, gen_repre, gen_templates, repre_util
    from foundpose_amd.bank import DeviceBank
    from foundpose_amd.crop_util import PinholePlaneCameraModel
    from tests.test_gpu_onboarding import _bop_root
    root = str(tmp_path)
    _bop_root(root)
    opts = gen_templates.load_opts({"gen_templates_opts": {"version": "v1", "object_dataset": "synth", "object_lids": None,
                                                           "min_num_viewpoints": 9, "num_inplane_rotations": 2, "crop_size": [224, 224]}})
    gen_templates.synthesize_templates(opts, root, root, (450.0, 550.0))
    meta = json.load(open(os.path.join(root, "templates", "v1", "synth", "1", "metadata.json")))
    ro = gen_repre.load_opts({"gen_repre_opts": {"version": "v1", "templates_version": "v1", "object_dataset": "synth", "object_lids": [1],
                                                 "extractor_name": NAME, "pca_components": 64, "cluster_num": 32,
                                                 "template_desc_opts": {"desc_type": "tfidf"}}})
    ex = feature_util.make_feature_extractor(NAME, random_init_seed=1234, precision="fp32").to("cuda")
    repre = repre_util.load_object_repre(gen_repre.generate_repre(ro, "synth", 1, root, extractor=ex))
    bank = DeviceBank([repre])
    eng = fe.FoundPoseEngine(ex, bank, 14.0, 5, 300, tie_order="torch")
    rng = np.random.default_rng(0)
    for k in (5, 12):
        crop = repre.templates[k:k + 1].cuda().float() / 255.0
        mask = torch.from_numpy(np.asarray(Image.open(meta[k]["binary_mask_path"]))[None].copy()).cuda()
        res = eng.infer_batch(crop, mask, keep_feature_map=True)
        assert int(res.template_ids[0, 0]) == k
        c = meta[k]["cameras"]
        cam = PinholePlaneCameraModel(c["ImageSizeX"], c["ImageSizeY"], (c["fx"], c["fy"]), (c["cx"], c["cy"]), np.array(c["T_WorldFromCamera"]))
        T_cw = np.linalg.inv(cam.T_world_from_eye)
        ax = rng.normal(size=3)
        ax /= np.linalg.norm(ax)
        dt = rng.normal(size=3)
        R0 = fr.rot_exp(ax * np.radians(2.0)) @ T_cw[:3, :3]
        t0 = T_cw[:3, 3] + dt * 5.0 / np.linalg.norm(dt)
        best = {"found": torch.tensor([True], device="cuda"), "corresp_id": torch.tensor([0], device="cuda"),
                "R": torch.from_numpy(R0)[None].cuda(), "t": torch.from_numpy(t0)[None].cuda()}
        out = refine_util.refine_best_coarse(res, best, bank, [0], [cam], (224, 224))
        R = out["R"][0].cpu().numpy()
        e0, e1 = fr.rot_angle_deg(R0, T_cw[:3, :3]), fr.rot_angle_deg(R, T_cw[:3, :3])
        tr0, tr1 = np.linalg.norm(t0 - T_cw[:3, 3]), np.linalg.norm(out["t"][0].cpu().numpy() - T_cw[:3, 3])
        print(f"template {k}: rotation error {e0:.3f} -> {e1:.3f} deg, translation {tr0:.2f} -> {tr1:.2f} mm, "
              f"cost {float(out['cost_in'][0]):.4g} -> {float(out['cost_out'][0]):.4g}, {int(out['num_points'][0])} points")
        assert int(out["status"][0]) == 0 and float(out["cost_out"][0]) < float(out["cost_in"][0])
        assert e1 <= 0.5 * e0


def test_driver_featuremetric_final_pose(tmp_path):
    from foundpose_amd import engine as fe, infer, infer_pose_util, pnp_util
    from foundpose_amd.bank import DeviceBank
    ex, sc, repre, crops, cmasks, cams = _engine_inputs(tmp_path, "fp32")
    frames = lambda lid: iter([{"scene_id": 1, "im_id": 3, "image": sc["image"], "camera": sc["cam"]}])
    dets = infer_pose_util.load_detections_in_bop_format(str(sc["det_path"]))
    outs = {}
    for kind in ("best_coarse", "featuremetric"):
        d = str(tmp_path / kind)
        paths = infer.infer(sc["opts"]._replace(final_pose_type=kind), frames, dets, {1: repre}, d, extractor=ex, num_target_insts={1: {(1, 3): 1}})
        outs[kind] = (json.load(open(os.path.join(d, "1", "estimated-poses.json"))), open(paths[-1]).read().splitlines())
    (ec, csv_c), (er, csv_r) = outs["best_coarse"], outs["featuremetric"]
    assert len(ec) == len(er) == 2 and csv_c[0] == csv_r[0] and len(csv_c) == len(csv_r)
    for a, b in zip(ec, er):
        assert set(b) == set(a)
        assert set(b["time"]) == set(a["time"]) | {"pose_refine"} and b["time"]["pose_refine"] > 0
    # the same chain by hand: coarse poses equal the best_coarse run's, written poses equal refine_best_coarse's
    o = sc["opts"]
    eng = fe.FoundPoseEngine(ex, DeviceBank([repre]), o.grid_cell_size, o.match_top_n_templates, o.match_top_k_buddies, tie_order="torch")
    res = eng.infer_batch(crops, cmasks, [0, 0], keep_feature_map=True)
    poses = pnp_util.estimate_poses(res, cams, o.pnp_type, o.pnp_ransac_iter, o.pnp_inlier_thresh, o.pnp_required_ransac_conf, o.pnp_refine_lm)
    best = pnp_util.select_best_coarse(poses)
    ref = refine_util.refine_best_coarse(res, best, eng.bank, [0, 0], cams, (224, 224), o.refine_iters)
    to_cam = lambda b, R, t: np.linalg.inv(sc["cam"].T_world_from_eye) @ cams[b].T_world_from_eye @ np.block([[R, t.reshape(3, 1)], [0, 0, 0, 1]])
    verts = repre.vertices.cpu().numpy().astype(np.float64)
    for e_c, e_r in zip(ec, er):
        b = int(e_r["inst_id"])
        Tc = to_cam(b, best["R"][b].cpu().numpy(), best["t"][b].cpu().numpy())
        Tr = to_cam(b, ref["R"][b].cpu().numpy(), ref["t"][b].cpu().numpy())
        assert np.abs(np.array(e_c["R"]) - Tc[:3, :3]).max() < 1e-9 and np.abs(np.array(e_c["t"]).ravel() - Tc[:3, 3]).max() < 1e-6
        assert np.abs(np.array(e_r["R"]) - Tr[:3, :3]).max() < 1e-9 and np.abs(np.array(e_r["t"]).ravel() - Tr[:3, 3]).max() < 1e-6
        # against the planted pose: MSSD (no symmetries) and MSPD of the coarse and the refined estimate
        Tg = to_cam(b, sc["R"][b].numpy(), sc["t"][b].numpy())
        K = np.array([[sc["cam"].f[0], 0, sc["cam"].c[0]], [0, sc["cam"].f[1], sc["cam"].c[1]], [0, 0, 1]])
        tr = lambda T: verts @ T[:3, :3].T + T[:3, 3]
        pr = lambda T: (lambda p: p[:, :2] / p[:, 2:])(tr(T) @ K.T)
        mssd = lambda T: float(np.linalg.norm(tr(T) - tr(Tg), axis=1).max())
        mspd = lambda T: float(np.linalg.norm(pr(T) - pr(Tg), axis=1).max())
        print(f"instance {b}: status {int(ref['status'][b])}, MSSD coarse {mssd(Tc):.4f} mm -> refined {mssd(Tr):.4f} mm, "
              f"MSPD coarse {mspd(Tc):.4f} px -> refined {mspd(Tr):.4f} px")
        assert float(ref["cost_out"][b]) <= float(ref["cost_in"][b])
