"""CPU: the depth refinement's numpy restatement (tests/depth_refine_ref.py), the driver's options and the split reader's depth."""

import json
import os
import re

import numpy as np
import pytest

from tests import depth_refine_ref as dr

CAM = (180.0, 185.0, 47.3, 39.6)
H, W = 80, 96
BASE = dict(version="v", repre_version="r", object_dataset="lmo")


def _planted(seed, n=120):
    """Points on the bilinear surface of an analytic depth image, in a model frame with a random ground-truth pose."""
    rng = np.random.default_rng(seed)
    D, _ = dr.analytic_depth(H, W, CAM)
    uv = np.stack([rng.uniform(4, W - 5, n), rng.uniform(4, H - 5, n)], 1)
    Xc = dr.backproject(D, CAM, uv)
    R = dr.rot_exp(rng.normal(size=3) * 0.4)
    t = np.array([3.0, -4.0, 600.0])
    X = (Xc - t) @ R          # R^T (Xc - t)
    return D, X, R, t


def test_jacobian_matches_central_differences():
    D, X, R, t = _planted(1)
    R0, t0 = dr.update(R, t, np.array([0.01, -0.008, 0.012, 1.5, -1.0, 2.0]))
    p = dr.point_terms(R0, t0, X, CAM, D)
    Xc = p["Xc"]
    u, v = CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2], CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3]
    # away from the pixel borders, where the bilinear surface is smooth
    inner = p["measurable"] & (np.abs(u - np.round(u)) > 0.05) & (np.abs(v - np.round(v)) > 0.05)
    assert inner.sum() > 50
    X = X[inner]
    J = dr.point_terms(R0, t0, X, CAM, D)["J"]
    eps = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = eps
        rp, _ = dr.residual(*dr.update(R0, t0, d), X, CAM, D)
        rm, _ = dr.residual(*dr.update(R0, t0, -d), X, CAM, D)
        fd = (rp - rm) / (2 * eps)
        np.testing.assert_allclose(J[:, k], fd, rtol=1e-5, atol=1e-6 * np.abs(J[:, k]).max())


def test_planted_depth_converges_to_ground_truth():
    for seed in (2, 3):
        D, X, R, t = _planted(seed)
        rng = np.random.default_rng(seed + 100)
        ax, dt = rng.normal(size=3), rng.normal(size=3)
        R0 = dr.rot_exp(ax / np.linalg.norm(ax) * np.radians(3.0)) @ R
        t0 = t + dt * 10.0 / np.linalg.norm(dt)
        out = dr.refine(R0, t0, X, CAM, D, tau=30.0, iters=50)
        assert out["status"] == 0 and out["cost_out"] < 1e-6 * out["cost_in"]
        assert dr.rot_angle_deg(out["R"], R) < 1e-3, dr.rot_angle_deg(out["R"], R)
        assert np.linalg.norm(out["t"] - t) < 1e-2, np.linalg.norm(out["t"] - t)


def test_truncation_holes_and_occluder_add_tau_squared_and_no_gradient():
    D, X, R, t = _planted(4)
    tau = 15.0
    p = dr.point_terms(R, t, X, CAM, D)
    u = CAM[0] * p["Xc"][:, 0] / p["Xc"][:, 2] + CAM[2]
    v = CAM[1] * p["Xc"][:, 1] / p["Xc"][:, 2] + CAM[3]
    hole = (u > 20) & (u < 40) & (v > 10) & (v < 30)
    occl = (u > 60) & (u < 80) & (v > 40) & (v < 60)
    assert hole.sum() >= 3 and occl.sum() >= 3
    Dm = D.copy()
    Dm[8:33, 18:43] = 0.0                       # a hole around the first group (a point next to it loses a tap as well)
    Dm[38:63, 58:83] -= 40.0                    # an occluder 40 mm in front of the second group
    E, Hm, g, inl = dr.system(R, t, X, CAM, Dm, tau)
    rest = ~(hole | occl)
    assert not inl[hole].any() and not inl[occl].any()
    pm = dr.point_terms(R, t, X, CAM, Dm)
    assert not pm["measurable"][hole].any() and pm["measurable"][occl].all()
    # the truncated points add exactly tau^2 each; the gradient is the remaining inliers' alone
    keep = inl
    E2, H2, g2, inl2 = dr.system(R, t, X[keep], CAM, Dm, tau)
    assert inl2.all()
    assert E * len(X) == pytest.approx(E2 * keep.sum() + (~keep).sum() * tau * tau, rel=1e-12)
    np.testing.assert_allclose(Hm, H2, rtol=1e-12)
    np.testing.assert_allclose(g, g2, rtol=1e-12, atol=1e-12 * np.abs(g).max())
    assert keep[rest].sum() > 0.8 * rest.sum()
    # a point whose +1 tap would lie outside the image is not measurable, and an empty image leaves nothing
    edge = np.array([[(W - 1 + 0.5 - CAM[2]) / CAM[0] * 600.0, 0.0, 600.0], [0.0, (H - 1 + 0.25 - CAM[3]) / CAM[1] * 600.0, 600.0]])
    assert not dr.point_terms(np.eye(3), np.zeros(3), edge, CAM, D)["measurable"].any()
    out = dr.refine(R, t, X, CAM, np.zeros_like(D), tau)
    assert out["status"] == 2 and out["num_points"] == 0 and out["cost_in"] == tau * tau and np.array_equal(out["R"], R)


def test_reference_errors_of_the_gpu_tests_are_the_restatements_own():
    """tests/test_gpu_depth_refine.py holds the GPU to twice REF_ERROR: the constants are recomputed here from their generator (the
    rasterizer's numpy restatement), and the scenes that count as recoveries end below the start's error in rotation and translation."""
    from tests import test_gpu_depth_refine as g
    cases = g.blob_cases(g.render_ref_depth)
    assert {c[0] for c in cases} == set(g.REF_ERROR) and set(g.RECOVERED) < set(g.REF_ERROR)
    for name, depth, det, gt in cases:
        assert g.pose_error(det["R"], det["t"], gt) == pytest.approx(g.START_ERROR, rel=1e-9)
        ref = g._ref(depth[None], det)
        err = g.pose_error(ref["R"], ref["t"], gt)
        assert err == pytest.approx(g.REF_ERROR[name], rel=2e-4), (name, err)
        if name in g.RECOVERED:
            assert ref["status"] == 0 and err[0] < g.START_ERROR[0] and err[1] < g.START_ERROR[1], (name, err)
    assert "occluded" not in g.RECOVERED and g.REF_ERROR["occluded"][0] > g.START_ERROR[0]


def test_skips_and_zero_iterations():
    D, X, R, t = _planted(5)
    assert dr.refine(R, t, X, CAM, D, 10.0, has_pose=False)["status"] == 2
    assert dr.refine(R, t, X[:5], CAM, D, 10.0)["status"] == 2
    out = dr.refine(R, t, X, CAM, D, 10.0, iters=0)
    assert out["status"] == 1 and out["iters_used"] == 0 and np.array_equal(out["R"], R) and out["cost_in"] == out["cost_out"]


def test_load_opts_accepts_depth_pose_types_and_options():
    from foundpose_amd import infer
    for kind in ("depth", "featuremetric_depth"):
        o = infer.load_opts({"infer_opts": dict(BASE, final_pose_type=kind, depth_refine_iters=12, depth_refine_max_dist=25.0)})
        assert o.final_pose_type == kind and o.depth_refine_iters == 12 and o.depth_refine_max_dist == 25.0
    d = infer.InferOpts(**BASE)
    assert d.depth_refine_iters == 30 and d.depth_refine_max_dist == 0.0 and d.final_pose_type == "best_coarse"
    assert set(infer.FINAL_POSE_TYPES) == {"best_coarse", "featuremetric", "depth", "featuremetric_depth"}


@pytest.mark.parametrize("bad", [dict(depth_refine_max_dist=-1.0), dict(final_pose_type="depth", depth_refine_max_dist=-0.5),
                                 dict(final_pose_type="depth", depth_refine_iters=-1), dict(final_pose_type="refined"),
                                 dict(final_pose_type="depth_featuremetric")])
def test_driver_refuses_bad_depth_options_before_gpu_work(bad):
    from foundpose_amd import infer
    with pytest.raises(ValueError):
        infer._check_driver_opts(infer.InferOpts(**BASE, **bad))
    with pytest.raises(ValueError):
        infer.infer_object(infer.InferOpts(**BASE, **bad), 1, None, [], {})


@pytest.mark.parametrize("kind", ["depth", "featuremetric_depth"])
def test_depth_pose_types_are_no_longer_refused(kind):
    """Past the option checks the call goes on to the extractor (no checkpoint here: some other error, or none)."""
    from foundpose_amd import infer
    opts = infer.InferOpts(**BASE, final_pose_type=kind)
    refine, _ = infer._check_driver_opts(opts)
    assert refine == (kind == "featuremetric_depth")
    try:
        infer.infer_object(opts, 1, None, [], {})
    except ValueError as e:
        pytest.fail(f"final_pose_type={kind!r} is refused: {e}")
    except Exception:
        pass


def test_default_tau_is_a_tenth_of_the_bounding_box_diagonal():
    import torch
    from foundpose_amd import infer

    class Repre:
        vertices = torch.tensor([[-10.0, 0.0, 5.0], [20.0, 40.0, 5.0], [0.0, -20.0, 25.0]])
    assert infer.depth_refine_tau(infer.InferOpts(**BASE), Repre()) == pytest.approx(0.1 * np.sqrt(30.0 ** 2 + 60.0 ** 2 + 20.0 ** 2))
    assert infer.depth_refine_tau(infer.InferOpts(**BASE, depth_refine_max_dist=12.5), Repre()) == 12.5


def test_frames_without_depth_or_of_another_size_are_named():
    from foundpose_amd import crop_util, infer
    cam = crop_util.PinholePlaneCameraModel(W, H, CAM[:2], CAM[2:], np.eye(4))
    frame = {"scene_id": 7, "im_id": 21, "image": np.zeros((H, W, 3), np.uint8), "camera": cam}
    with pytest.raises(ValueError, match="scene 7 image 21"):
        infer._check_frame_depth(frame)
    with pytest.raises(ValueError, match="scene 7 image 21"):
        infer._check_frame_depth(dict(frame, depth=np.zeros((W, H), np.float32)))
    infer._check_frame_depth(dict(frame, depth=np.zeros((H, W), np.float32)))


def _write_rgb(split_dir, im_ids, width, height):
    from PIL import Image
    os.makedirs(os.path.join(split_dir, "000001", "rgb"), exist_ok=True)
    for im in im_ids:
        Image.fromarray(np.full((height, width, 3), 10 * im % 255, np.uint8)).save(os.path.join(split_dir, "000001", "rgb", f"{im:06d}.png"))


def _check_reader_depth(split_dir, targets, scales):
    from foundpose_amd import eval_bop19, infer
    frames = list(infer.load_bop_frames_all(split_dir, targets, with_depth=True))
    assert len(frames) == len({(t["scene_id"], t["im_id"]) for t in targets})
    for f in frames:
        want = eval_bop19.load_depth(os.path.join(split_dir, "000001", "depth", f"{f['im_id']:06d}.png"), scales[f["im_id"]])
        assert f["depth"].dtype == np.float32 and f["depth"].shape == (f["camera"].height, f["camera"].width)
        assert np.array_equal(f["depth"], want) and want.max() > 0
    per_object = list(infer.load_bop_frames(split_dir, targets, targets[0]["obj_id"], with_depth=True))
    assert per_object and all(np.array_equal(f["depth"], next(g["depth"] for g in frames if g["im_id"] == f["im_id"])) for f in per_object)
    assert all("depth" not in f for f in infer.load_bop_frames_all(split_dir, targets))


def test_split_reader_loads_depth_like_the_evaluation(tmp_path):
    """A split in synthetic.make_bop_eval_scene's layout written by hand (that generator renders on the GPU): uint16 depth PNGs in
    depth_scale units beside the images."""
    from PIL import Image
    split = str(tmp_path / "synth" / "test")
    os.makedirs(os.path.join(split, "000001", "depth"))
    rng = np.random.default_rng(0)
    scales, cams = {0: 0.1, 1: 1.0, 2: 0.5}, {}
    for im, sc in scales.items():
        Image.fromarray(rng.integers(0, 20000, size=(H, W)).astype(np.uint16)).save(os.path.join(split, "000001", "depth", f"{im:06d}.png"))
        cams[str(im)] = {"cam_K": [CAM[0], 0, CAM[2], 0, CAM[1], CAM[3], 0, 0, 1], "depth_scale": sc}
    with open(os.path.join(split, "000001", "scene_camera.json"), "w") as f:
        json.dump(cams, f)
    _write_rgb(split, scales, W, H)
    targets = [{"scene_id": 1, "im_id": im, "obj_id": 1 + im % 2, "inst_count": 1} for im in scales] + [{"scene_id": 1, "im_id": 0, "obj_id": 2, "inst_count": 1}]
    _check_reader_depth(split, targets, scales)


@pytest.mark.gpu
def test_split_reader_depth_on_a_generated_eval_scene(tmp_path):
    from foundpose_amd import synthetic
    sc = synthetic.make_bop_eval_scene(str(tmp_path), num_images=2, num_objects=2, width=W, height=H, mesh_res=12)
    _write_rgb(sc["split_dir"], [im for im, _ in sc["images"]], W, H)
    _check_reader_depth(sc["split_dir"], sc["targets"], {im: 0.1 for im, _ in sc["images"]})


def test_depth_refine_symbol_declared_and_prototyped():
    from foundpose_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "foundpose_amd.h")).read()
    assert re.search(r"\bfp_depth_refine\s*\(", header)
    assert "fp_depth_refine" in _lib.exported_symbols() and _lib.ABI_VERSION == 20
    assert _lib.depth_refine_scratch_bytes(32, 300) == 512 * 32 + 256 * 32 * 10 + 8


def test_refine_depth_rejects_cpu_tensors():
    import torch
    from foundpose_amd import _lib, refine_util
    z = torch.zeros
    with pytest.raises(_lib.FoundPoseNativeError):
        refine_util.refine_depth(z(1, 8, 8), z(1, dtype=torch.int32), [CAM], z(1, 3, 3), z(1, 3), z(1, dtype=torch.int32), z(1, dtype=torch.int32),
                                 z(10, 3), z(1, dtype=torch.bool), 10.0)
