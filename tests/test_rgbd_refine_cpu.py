"""CPU: the joint feature + depth refinement's numpy restatement (tests/rgbd_refine_ref.py) against the two restatements it is made of,
the reason for the feature (complementarity), the tap-consistency test, and the plumbing: C ABI entry, driver options."""

import os
import re

import numpy as np
import pytest

from tests import depth_refine_ref as dr
from tests import featuremetric_ref as fr
from tests import rgbd_refine_ref as rg
from tests.test_featuremetric_cpu import CAM, H, W, _scene

BASE = dict(version="v", repre_version="r", object_dataset="lmo")
EYE, ZERO = np.eye(3), np.zeros(3)


def _feature_problem(A=EYE, a=ZERO, seed=3):
    """test_featuremetric_cpu.py's planted smooth field; the depth image is never an inlier (all zero) and depth_weight is 0."""
    M, X, R, t = _scene(seed, C=32)
    f = fr.sample_at(M, R, t, X, CAM, W, H)
    R0, t0 = fr.update(R, t, np.array([np.radians(2.0), 0.0, 0.0, 5.0, 0.0, 0.0]))
    pr = rg.Problem(X, f, M, CAM, W, H, A, a, np.zeros((8, 8), np.float32), CAM, 10.0, depth_weight=0.0)
    return pr, (R, t), (R0, t0)


def test_feature_term_alone_reaches_the_featuremetric_restatements_pose():
    pr, (R, t), (R0, t0) = _feature_problem()
    out = rg.refine(R0, t0, pr, iters=30)
    ref = fr.refine(R0, t0, pr.X, pr.f, CAM, W, H, pr.M, iters=30)
    assert out["status"] == 0 and ref["status"] == 0 and out["num_points"] == ref["num_points"] and out["num_depth_inliers"] == 0
    assert out["cost_out"] <= out["cost_in"]
    # the tolerance of test_featuremetric_cpu.py::test_planted_field_converges for a final pose, here between the two restatements
    assert fr.rot_angle_deg(out["R"], ref["R"]) < 0.01 and np.linalg.norm(out["t"] - ref["t"]) < 0.1
    assert fr.rot_angle_deg(out["R"], R) < 0.01 and np.linalg.norm(out["t"] - t) < 0.1


def test_another_frame_camera_gives_the_same_pose():
    """The same computation in another frame: the feature camera reached through a non-identity (A, a) from a frame camera in which the
    pose is expressed; mapped back, the result equals the identity-transform run's within 1e-9 rad / 1e-6 mm."""
    pr, _, (R0, t0) = _feature_problem()
    same = rg.refine(R0, t0, pr, iters=30)
    A = fr.rot_exp(np.array([0.11, -0.23, 0.07]))
    a = np.array([31.0, -17.0, 12.0])
    pr2, _, _ = _feature_problem(A, a)
    Rc0, tc0 = A.T @ R0, A.T @ (t0 - a)                     # the start in the frame camera: X_f = A X_c + a
    other = rg.refine(Rc0, tc0, pr2, iters=30)
    Rf, tf = rg.to_feature_camera(other["R"], other["t"], A, a)
    print(f"identity vs other frame: {rg.rot_angle_rad(Rf, same['R']):.3e} rad, {np.linalg.norm(tf - same['t']):.3e} mm")
    assert other["status"] == same["status"] == 0 and other["num_points"] == same["num_points"]
    assert rg.rot_angle_rad(Rf, same["R"]) < 1e-9 and np.linalg.norm(tf - same["t"]) < 1e-6


def test_jacobian_of_the_feature_term_through_A_matches_central_differences():
    A = fr.rot_exp(np.array([0.2, 0.1, -0.15]))
    a = np.array([20.0, 10.0, -30.0])
    M, X, R, t = _scene(1, C=8)
    M = M.astype(np.float64)
    f = np.random.default_rng(2).normal(size=(len(X), 8))
    Rc, tc = A.T @ R, A.T @ (t - a)
    _, _, xm, ym = fr.map_coords(R, t, X, CAM, W, H, M.shape[1], M.shape[0])
    inner = fr.valid_set(R, t, X, CAM, W, H, M) & (np.abs(xm - np.round(xm)) > 0.05) & (np.abs(ym - np.round(ym)) > 0.05)
    X, f = X[inner], f[inner]

    def res(Rp, tp):
        Rf, tf = rg.to_feature_camera(Rp, tp, A, a)
        return fr.jacobian(Rf, tf, X, f, CAM, W, H, M)[1]
    p = rg.feature_terms(Rc, tc, X, f.astype(np.float32), A, a, CAM, W, H, M.astype(np.float32))
    J = p["gx"].astype(np.float64)[:, :, None] * p["ax"][:, None, :] + p["gy"].astype(np.float64)[:, :, None] * p["ay"][:, None, :]
    eps = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = eps
        fd = (res(*fr.update(Rc, tc, d)) - res(*fr.update(Rc, tc, -d))) / (2 * eps)
        np.testing.assert_allclose(J[:, :, k], fd, rtol=1e-3, atol=2e-5 * np.abs(J[:, :, k]).max())   # J's map part is fp32


MEASURED_RAD, MEASURED_MM = 2.0e-9, 3.3e-7   # the joint restatement's final error on plane_scene(7) from _plane_start, 30 iterations


def _plane_start(gt):
    """3 degrees / 10 mm off, 6 mm of the 10 in the plane."""
    R, t = gt
    ax = np.array([0.5, -0.6, 0.62])
    return fr.rot_exp(ax / np.linalg.norm(ax) * np.radians(3.0)) @ R, t + np.array([6.0, 0.0, 8.0])


def test_depth_alone_slides_in_the_plane_and_the_joint_objective_does_not():
    """DESIGN.md section 14, limit (1), and the reason for section 15: on a fronto-parallel plane the depth term does not see in-plane
    translation; the joint objective ends at the planted pose."""
    M, D, X, f, gt, cam, w, h = rg.plane_scene(7)
    R0, t0 = _plane_start(gt)
    inplane = lambda tt: float(np.linalg.norm((tt - gt[1])[:2]))
    alone = dr.refine(R0, t0, X, cam, D, 25.0, iters=30)
    print(f"depth alone: in-plane translation error {inplane(t0):.3f} -> {inplane(alone['t']):.3f} mm, status {alone['status']}")
    assert inplane(alone["t"]) > 0.5 * inplane(t0)
    pr = rg.Problem(X, f, M, cam, w, h, EYE, ZERO, D, cam, 25.0, depth_weight=1.0)
    out = rg.refine(R0, t0, pr, iters=30)
    er, et = rg.rot_angle_rad(out["R"], gt[0]), float(np.linalg.norm(out["t"] - gt[1]))
    print(f"joint: {er:.3e} rad, {et:.3e} mm, {out['num_depth_inliers']} depth inliers, {out['iters_used']} iterations, "
          f"cost {out['cost_in']:.4g} -> {out['cost_out']:.4g}")
    assert out["status"] == 0 and out["num_depth_inliers"] >= 6 and out["cost_out"] <= out["cost_in"]
    # 10 x the restatement's own final error here, MEASURED_RAD / MEASURED_MM: a smooth exact planted problem converges to
    # rounding level, the margin covers the platform's libm
    assert er < 10 * MEASURED_RAD and et < 10 * MEASURED_MM


def _taps(z00, z10, z01, z11):
    """A 4 x 4 depth image at 1000 mm whose four taps around (1.5, 1.5) are given, and the one model point that projects there at 1000 mm."""
    D = np.full((4, 4), 1000.0, np.float32)
    D[1, 1], D[1, 2], D[2, 1], D[2, 2] = z00, z10, z01, z11
    cam = (100.0, 100.0, 0.0, 0.0)
    X = np.array([[1.5 / 100.0 * 1000.0, 1.5 / 100.0 * 1000.0, 1000.0]])
    return D, cam, X


def test_tap_consistency_by_hand():
    """tau = 25.  Taps 1000, 960, 1000, 960 straddle a 40 mm step: bilinear depth at the centre is 980, |r| = 20 < tau, so section 14 counts
    an inlier with a 40 mm / px gradient; here the spread 40 > tau makes the point not measurable and it adds exactly 1 / N to E_d.
    Taps 1000, 980, 1000, 980 (spread 20 <= tau): d = 990, r = -10, an inlier adding 100 / 625 / N."""
    tau = 25.0
    D, cam, X = _taps(1000.0, 960.0, 1000.0, 960.0)
    old = dr.point_terms(EYE, ZERO, X, cam, D)
    assert old["measurable"][0] and old["r"][0] == -20.0                      # section 14 alone: an inlier
    p = rg.depth_terms(EYE, ZERO, X, cam, D, tau)
    assert p["spread"][0] == 40.0 and not p["measurable"][0] and not p["J"].any()
    pad = np.repeat(X, 3, axis=0)                                             # N = 3 equal rows
    Ed, Hd, gd, inl = rg.depth_system(EYE, ZERO, pad, cam, D, tau)
    assert Ed == 1.0 and not inl.any() and not Hd.any() and not gd.any()      # each row adds exactly 1 / N
    D, cam, X = _taps(1000.0, 980.0, 1000.0, 980.0)
    p = rg.depth_terms(EYE, ZERO, X, cam, D, tau)
    assert p["spread"][0] == 20.0 and p["measurable"][0] and p["r"][0] == -10.0
    Ed, Hd, gd, inl = rg.depth_system(EYE, ZERO, X, cam, D, tau)
    assert inl.all() and Ed == 100.0 / 625.0 and Hd[5, 5] > 0 and gd.any()
    # a spread of exactly tau is still measurable
    D, cam, X = _taps(1000.0, 975.0, 1000.0, 975.0)
    assert rg.depth_terms(EYE, ZERO, X, cam, D, tau)["measurable"][0]


def test_skips_feature_only_runs_and_zero_iterations():
    M, D, X, f, gt, cam, w, h = rg.plane_scene(8, n=60)
    R0, t0 = _plane_start(gt)
    mk = lambda **k: rg.Problem(k.get("X", X), k.get("f", f), M, cam, w, h, EYE, ZERO, k.get("D", D), cam, k.get("tau", 25.0), k.get("wd", 1.0))
    assert rg.refine(R0, t0, mk(), has_pose=False)["status"] == 2
    few = rg.refine(R0, t0, mk(X=X[:5], f=f[:5]))
    assert few["status"] == 2 and few["num_points"] == 5 and np.array_equal(few["R"], R0)
    z = rg.refine(R0, t0, mk(), iters=0)
    assert z["status"] == 1 and z["iters_used"] == 0 and np.array_equal(z["R"], R0) and z["cost_in"] == z["cost_out"]
    for kw in (dict(tau=float("nan")), dict(D=np.zeros_like(D)), dict(wd=0.0)):
        out = rg.refine(R0, t0, mk(**kw))
        assert out["status"] == 0 and np.isfinite(out["cost_out"]) and out["cost_out"] <= out["cost_in"], kw
        assert (out["num_depth_inliers"] >= 6) == ("wd" in kw) and (out["num_depth_inliers"] == 0) == ("wd" not in kw), kw   # counted, not used


# ---------------------------------------------------------------------------------------------------- plumbing
def test_symbol_declared_prototyped_and_abi_unchanged():
    from foundpose_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "foundpose_amd.h")).read()
    assert re.search(r"\bfp_rgbd_refine\s*\(", header) and "FP_RGBD_REFINE_SCRATCH_BYTES" in header
    assert "fp_rgbd_refine" in _lib.exported_symbols()
    assert int(re.search(r"#define\s+FP_ABI_VERSION\s+(\d+)", header).group(1)) == 20
    # state + one 64-double record per chunk + the valid flags + the error word
    assert _lib.rgbd_refine_scratch_bytes(32, 449) == 512 * 32 + 8 * 64 * 32 * 15 + ((32 * 449 + 7) // 8) * 8 + 8


def test_load_opts_accepts_the_joint_pose_type_and_its_weight():
    from foundpose_amd import infer
    o = infer.load_opts({"infer_opts": dict(BASE, final_pose_type="featuremetric_depth_joint", depth_refine_weight=0.25, refine_iters=12,
                                            depth_refine_max_dist=25.0)})
    assert o.final_pose_type == "featuremetric_depth_joint" and o.depth_refine_weight == 0.25 and o.refine_iters == 12
    assert infer.InferOpts(**BASE).depth_refine_weight == 1.0
    assert "featuremetric_depth_joint" in infer.DEPTH_POSE_TYPES
    refine, _ = infer._check_driver_opts(o)
    assert refine                                            # the engine keeps the feature map
    try:
        infer.infer_object(o, 1, None, [], {})
    except ValueError as e:
        pytest.fail(f"final_pose_type='featuremetric_depth_joint' is refused: {e}")
    except Exception:
        pass                                                 # past the option checks: no checkpoint here


@pytest.mark.parametrize("bad", [dict(final_pose_type="featuremetric_depth_joint", depth_refine_weight=-1.0),
                                 dict(final_pose_type="featuremetric_depth_joint", depth_refine_weight=float("nan")),
                                 dict(depth_refine_weight=-0.5), dict(depth_refine_weight="1"),
                                 dict(final_pose_type="featuremetric_depth_joint", refine_iters=-1),
                                 dict(final_pose_type="featuremetric_depth_joint", refine_iters=2.5),
                                 dict(final_pose_type="refined"), dict(final_pose_type="joint")])
def test_driver_refuses_bad_options_before_gpu_work(bad):
    from foundpose_amd import infer
    with pytest.raises(ValueError):
        infer._check_driver_opts(infer.InferOpts(**BASE, **bad))
    with pytest.raises(ValueError):
        infer.infer_object(infer.InferOpts(**BASE, **bad), 1, None, [], {})
    with pytest.raises(ValueError):
        infer.infer_batched(infer.InferOpts(**BASE, **bad), iter([]), {}, {}, "unused")


def test_refine_rgbd_rejects_cpu_tensors_and_bad_weights():
    import torch
    from foundpose_amd import _lib, refine_util
    z = torch.zeros
    args = lambda: (z(1, 4, 4, 8), (56, 56), [CAM], z(1, 3, 3), z(1, 3), z(1, 8, 8), z(1, dtype=torch.int32), [CAM], z(1, 3, 3), z(1, 3),
                    z(1, dtype=torch.int32), z(1, dtype=torch.int32), z(10, 8), z(10, 3), z(1, dtype=torch.bool), 10.0)
    with pytest.raises(_lib.FoundPoseNativeError):
        refine_util.refine_rgbd(*args())
