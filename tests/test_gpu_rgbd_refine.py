"""GPU: refinement of the final pose on features and depth in one objective (csrc/rgbd_refine.hip, refine_util.refine_rgbd, the drivers'
final_pose_type="featuremetric_depth_joint") against the numpy restatement tests/rgbd_refine_ref.py.  The kernel tests use a batch of
four detections with 5, 6, 33 and 449 points (skipped, minimal, one past a chunk, the headline bank's mean), a 37 x 37 map of 64 or 192
channels (one and three per lane), stacks of two depth images of 64 x 48 or 161 x 97 pixels read in a non-monotone order, and a
non-identity transform between the frame's camera and the feature camera."""
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, refine_util
from tests import depth_refine_ref as dr
from tests import featuremetric_ref as fr
from tests import rgbd_refine_ref as rg
from tests import test_gpu_depth_refine as gd
from tests.test_gpu_depth_refine import driver_split  # noqa: F401  (the planted split of the depth drivers' tests)

pytestmark = pytest.mark.gpu
W = H = 518            # the feature camera's image
COUNTS = (5, 6, 33, 449)
A_REL = fr.rot_exp(np.array([0.04, -0.06, 0.05]))


def _frame_cam(Wd, Hd):
    return (1.9 * Wd, 1.95 * Wd, 0.49 * Wd, 0.52 * Hd)


def _feature_view(Xc, cam_d, Wd):
    """A feature camera that sees the frame-camera points Xc in the middle 3/4 of its W x H image, turned by A_REL against the frame's
    camera: -> (fcam, A, a)."""
    c = Xc.mean(0)
    a = np.array([0.0, 0.0, c[2]]) - A_REL @ c
    ff = 0.75 * W * cam_d[0] / Wd
    return (ff, 1.02 * ff, 259.0, 257.0), A_REL, a


def _planted_features(M, X, gt, fcam, A, a):
    Rf, tf = rg.to_feature_camera(gt[0], gt[1], A, a)
    return fr.sample_at(M, Rf, tf, X.astype(np.float64), fcam, W, H)


def _scene(seed, n, C, Hd, Wd, tau=25.0, rot_deg=1.0, trans_mm=4.0):
    """n points on the bilinear surface of an analytic depth image (exact planted depth) with planted smooth features, under a pose a
    little off the planted one.  -> dict(M, D, cam, fcam, A, a, X, f, R, t, tau, gt)."""
    rng = np.random.default_rng(seed)
    cam = _frame_cam(Wd, Hd)
    D, _ = dr.analytic_depth(Hd, Wd, cam)
    uv = np.stack([rng.uniform(3, Wd - 4, n), rng.uniform(3, Hd - 4, n)], 1)
    Xc = dr.backproject(D, cam, uv)
    R = dr.rot_exp(rng.normal(size=3) * 0.4)
    t = np.array([3.0, -4.0, 600.0])
    X = ((Xc - t) @ R).astype(np.float32)
    fcam, A, a = _feature_view(Xc, cam, Wd)
    M = fr.smooth_field(37, 37, C, seed)
    R0, t0 = gd._perturb(rng, R, t, rot_deg, trans_mm)
    return dict(M=M, D=D, cam=cam, fcam=fcam, A=A, a=a, X=X, f=_planted_features(M, X, (R, t), fcam, A, a), R=R0, t=t0, tau=tau, gt=(R, t))


def _run(dets, depth=None, image_index=None, iters=30, wd=1.0, normal_eq=False, max_points=None):
    """dets: list of _scene dicts (+ has_pose); depth [N, Hd, Wd] (default: each detection's own image) -> refine_rgbd's dict (cpu numpy)."""
    B = len(dets)
    if depth is None:
        depth, image_index = np.stack([d["D"] for d in dets]), np.arange(B)
    n = np.array([len(d["X"]) for d in dets])
    rb = np.concatenate([[0], np.cumsum(n)[:-1]])
    cuda = lambda v, dt=None: torch.as_tensor(np.ascontiguousarray(v), dtype=dt).cuda()
    out = refine_util.refine_rgbd(
        cuda(np.stack([d["M"] for d in dets])), (W, H), [d["fcam"] for d in dets], cuda(np.stack([d["A"] for d in dets]), torch.float64),
        cuda(np.stack([d["a"] for d in dets]), torch.float64), cuda(depth, torch.float32), cuda(np.asarray(image_index), torch.int32),
        [d["cam"] for d in dets], cuda(np.stack([d["R"] for d in dets]), torch.float64), cuda(np.stack([d["t"] for d in dets]), torch.float64),
        cuda(rb, torch.int32), cuda(rb + n, torch.int32), cuda(np.concatenate([d["f"] for d in dets]).astype(np.float32)),
        cuda(np.concatenate([d["X"] for d in dets]).astype(np.float32)), cuda(np.array([d.get("has_pose", True) for d in dets])),
        [d["tau"] for d in dets], depth_weight=wd, iters=iters, return_normal_equations=normal_eq, max_points=max_points)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _problem(d, D=None, wd=1.0):
    return rg.Problem(d["X"].astype(np.float64), d["f"], d["M"], d["fcam"], W, H, d["A"], d["a"], d["D"] if D is None else D, d["cam"], d["tau"], wd)


def _ref(d, D=None, wd=1.0, iters=30):
    return rg.refine(d["R"], d["t"], _problem(d, D, wd), iters, d.get("has_pose", True))


def _ragged(C, Hd, Wd, seed=0):
    """The batch of four: detections b read image (1, 0, 1, 0)[b] of a stack of two."""
    dets = [_scene(100 * seed + 10 * C + k, n, C, Hd, Wd) for k, n in enumerate(COUNTS)]
    index = [1, 0, 1, 0]
    base = dets[0]["D"]
    stack = np.stack([base * np.float32(1.002), base])        # image 0: the surface 1.2 mm further away
    return dets, stack, index


@pytest.mark.parametrize("C,Hd,Wd", [(64, 48, 64), (192, 97, 161)])
def test_normal_equations_and_cost_match_restatement(C, Hd, Wd):
    """All 57 values at the input pose.  Feature half and E: fp32 dot products, 1e-4 of the largest entry per block (tests/test_gpu_featuremetric.py);
    depth half: fp64 from the same fp32 taps, 1e-9 (tests/test_gpu_depth_refine.py)."""
    dets, stack, index = _ragged(C, Hd, Wd)
    out = _run(dets, stack, index, iters=0, normal_eq=True)
    for b, d in enumerate(dets):
        pr = _problem(d, stack[index[b]])
        ref = rg.refine(d["R"], d["t"], pr, iters=0)
        assert out["num_points"][b] == ref["num_points"] and out["num_depth_inliers"][b] == ref["num_depth_inliers"], b
        assert out["status"][b] == ref["status"] == (2 if COUNTS[b] < 6 else 1) and out["iters_used"][b] == 0
        assert np.array_equal(out["R"][b], d["R"]) and np.array_equal(out["t"][b], d["t"])
        got = out["normal_eq"][b]
        if COUNTS[b] < 6:
            assert not got.any() and out["cost_in"][b] == out["cost_out"][b] == 0.0
            continue
        want = rg.normal_equations(d["R"], d["t"], pr)
        assert ref["num_points"] >= 6 and ref["num_depth_inliers"] >= 6
        for lo, hi, tol in ((0, 21, 1e-4), (21, 27, 1e-4), (27, 28, 1e-4), (28, 49, 1e-9), (49, 55, 1e-9), (55, 56, 1e-9), (56, 57, 1e-4)):
            scale = np.abs(want[lo:hi]).max()
            print(f"C {C}, {COUNTS[b]} points, block {lo}: max error {np.abs(got[lo:hi] - want[lo:hi]).max():.3e} of {scale:.3e}")
            assert np.abs(got[lo:hi] - want[lo:hi]).max() <= tol * scale, (b, lo, got[lo:hi], want[lo:hi])
        assert out["cost_in"][b] == out["cost_out"][b] == got[56]


def _check_against_restatement(out, b, ref, name):
    er, et = rg.rot_angle_rad(out["R"][b], ref["R"]), float(np.linalg.norm(out["t"][b] - ref["t"]))
    print(f"{name}: GPU vs restatement {er:.3e} rad / {et:.3e} mm, status {out['status'][b]} / {ref['status']}, iterations {out['iters_used'][b]} / "
          f"{ref['iters_used']}, cost {out['cost_in'][b]:.6g} -> {out['cost_out'][b]:.6g} (restatement {ref['cost_in']:.6g} -> {ref['cost_out']:.6g}), "
          f"{out['num_points'][b]} valid, {out['num_depth_inliers'][b]} depth inliers")
    assert out["status"][b] == ref["status"]
    assert out["num_points"][b] == ref["num_points"] and out["num_depth_inliers"][b] == ref["num_depth_inliers"]
    assert out["cost_out"][b] <= out["cost_in"][b]
    assert er < 1e-6 and et < 1e-3


def _plane_det(seed=7):
    """tests/test_rgbd_refine_cpu.py's complementarity scene (one camera, A = I), its points as the fp32 a bank stores."""
    from tests.test_rgbd_refine_cpu import _plane_start
    M, D, X, f, gt, cam, w, h = rg.plane_scene(seed)
    assert (w, h) == (W, H)
    X = X.astype(np.float32)
    R0, t0 = _plane_start(gt)
    return dict(M=M, D=D, cam=cam, fcam=cam, A=np.eye(3), a=np.zeros(3), X=X, f=fr.sample_at(M, gt[0], gt[1], X.astype(np.float64), cam, W, H), R=R0, t=t0,
                tau=25.0, gt=gt)


def _blob_det(name, C=64):
    """One of tests/test_gpu_depth_refine.py's rendered blob cases, given a feature camera and planted smooth features at the ground truth."""
    _, depth, det, gt = next(c for c in gd.blob_cases(gd.hip_depth) if c[0] == name)
    Xc = det["X"].astype(np.float64) @ gt[0].T + gt[1]
    fcam, A, a = _feature_view(Xc, gd.CAM, gd.W)
    M = fr.smooth_field(37, 37, C, 5)
    return dict(M=M, D=depth, cam=gd.CAM, fcam=fcam, A=A, a=a, X=det["X"], f=_planted_features(M, det["X"], gt, fcam, A, a), R=det["R"], t=det["t"],
                tau=det["tau"], gt=gt)


def test_plane_scene_converges_like_the_restatement():
    d = _plane_det()
    out = _run([d])
    ref = _ref(d)
    _check_against_restatement(out, 0, ref, "plane")
    assert out["status"][0] == 0 and abs(int(out["iters_used"][0]) - ref["iters_used"]) <= 1
    e = gd.pose_error(out["R"][0], out["t"][0], d["gt"])
    print(f"plane: GPU ends {e[0]:.3e} rad / {e[1]:.3e} mm from the planted pose")
    assert e[0] < 1e-5 and e[1] < 1e-2          # fp32 points are up to 3e-5 mm off the plane: not the CPU test's rounding level


def test_rendered_blob_converges_like_the_restatement():
    d = _blob_det("clean0")
    out = _run([d])
    ref = _ref(d)
    _check_against_restatement(out, 0, ref, "clean0")
    e0, e1 = gd.pose_error(d["R"], d["t"], d["gt"]), gd.pose_error(out["R"][0], out["t"][0], d["gt"])
    print(f"clean0: start {e0[0]:.4e} rad / {e0[1]:.4f} mm -> GPU {e1[0]:.4e} rad / {e1[1]:.4f} mm from the ground truth")
    assert out["status"][0] == 0 and abs(int(out["iters_used"][0]) - ref["iters_used"]) <= 1
    assert e1[0] < gd.START_ERROR[0] and e1[1] < gd.START_ERROR[1]


def test_occluder_strip_follows_the_restatement():
    """The case of tests/test_gpu_depth_refine.py::test_occluder_strip_shows_the_limit_of_bilinear_taps, with planted features.  The GPU
    follows the restatement; the restatement's final error is printed beside that of the sequential pair of restatements (section 11,
    then section 14).  Which is smaller is not asserted."""
    d = _blob_det("occluded")
    out = _run([d])
    ref = _ref(d)
    _check_against_restatement(out, 0, ref, "occluded")
    Rf, tf = rg.to_feature_camera(d["R"], d["t"], d["A"], d["a"])
    X64 = d["X"].astype(np.float64)
    s1 = fr.refine(Rf, tf, X64, d["f"], d["fcam"], W, H, d["M"], iters=30)
    Rc, tc = d["A"].T @ s1["R"], d["A"].T @ (s1["t"] - d["a"])
    s2 = dr.refine(Rc, tc, X64, d["cam"], d["D"], d["tau"], iters=30)
    ej, es, e1 = gd.pose_error(ref["R"], ref["t"], d["gt"]), gd.pose_error(s2["R"], s2["t"], d["gt"]), gd.pose_error(Rc, tc, d["gt"])
    print(f"occluder strip, error against the ground truth: joint restatement {ej[0]:.4e} rad / {ej[1]:.4f} mm; sequential restatements "
          f"{es[0]:.4e} rad / {es[1]:.4f} mm (after the feature stage alone {e1[0]:.4e} rad / {e1[1]:.4f} mm); start {gd.START_ERROR[0]:.4e} rad / 10 mm")


def test_batch_invariance_and_determinism():
    dets, stack, index = _ragged(64, 48, 64, seed=1)
    batch = _run(dets, stack, index, normal_eq=True, max_points=480)
    again = _run(dets, stack, index, normal_eq=True, max_points=480)
    rev = _run(dets[::-1], stack, index[::-1], normal_eq=True, max_points=480)
    assert batch["status"].tolist() == [2, 0, 0, 0] and batch["iters_used"][3] > 2
    for key in batch:
        assert np.array_equal(batch[key], again[key]), key
        assert np.array_equal(batch[key], rev[key][::-1]), key
    for b, d in enumerate(dets):
        alone = _run([d], stack[index[b]][None], [0], normal_eq=True)
        for key in alone:
            assert np.array_equal(alone[key][0], batch[key][b]), (key, b)


def test_degenerate_inputs():
    d = _scene(40, 50, 64, 48, 64)
    nan_tau = dict(d, tau=float("nan"))
    out = _run([dict(d, has_pose=False), dict(d, X=d["X"][:5], f=d["f"][:5]), d, nan_tau, d], np.stack([d["D"], np.zeros_like(d["D"])]), [0, 0, 0, 0, 1])
    assert out["status"].tolist() == [2, 2, 0, 0, 0] and out["num_points"][1] == 5
    for b in (0, 1):
        assert np.array_equal(out["R"][b], d["R"]) and np.array_equal(out["t"][b], d["t"]) and out["iters_used"][b] == 0
    assert out["num_depth_inliers"].tolist()[2] >= 6 and out["num_depth_inliers"].tolist()[3:] == [0, 0]
    assert np.isfinite(out["cost_out"]).all() and (out["cost_out"] <= out["cost_in"]).all()
    # tau = NaN and a depth image that is all zero: the feature term alone, the same poses as depth_weight = 0 gives
    feat = _run([d], wd=0.0)
    for b in (3, 4):
        assert np.array_equal(out["R"][b], feat["R"][0]) and np.array_equal(out["t"][b], feat["t"][0])
    assert feat["status"][0] == 0 and feat["num_depth_inliers"][0] >= 6       # counted, not used
    _check_against_restatement(feat, 0, _ref(d, wd=0.0), "depth_weight 0")
    # an empty range is skipped; iters = 0 accepts no step
    out = _run([dict(d, X=d["X"][:0], f=d["f"][:0]), d], np.stack([d["D"]]), [0, 0], iters=0)
    assert out["status"].tolist() == [2, 1] and out["iters_used"].tolist() == [0, 0] and out["cost_in"][1] == out["cost_out"][1] > 0
    for b in range(2):
        assert np.array_equal(out["R"][b], d["R"]) and np.array_equal(out["t"][b], d["t"])
    # a bank row range outside the bank and an image index outside the stack are reported, not read
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    one = torch.ones(2, dtype=torch.bool, device="cuda")
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    call = lambda re, ii, **k: refine_util.refine_rgbd(z(2, 4, 4, 8), (56, 56), [gd.CAM] * 2, z(2, 3, 3), z(2, 3), z(1, 48, 64), ii, [gd.CAM] * 2, z(2, 3, 3),
                                                        z(2, 3), i32(0, 0), re, z(10, 8), z(10, 3), one, 10.0, max_points=64, **k)
    with pytest.raises(_lib.FoundPoseNativeError, match="detection 1: bank rows"):
        call(i32(10, 11), i32(0, 0))
    for bad in (1, -1):
        with pytest.raises(_lib.FoundPoseNativeError, match="detection 0: image index"):
            call(i32(10, 10), i32(bad, 0))
    with pytest.raises(ValueError):
        call(i32(10, 10), i32(0, 0), depth_weight=-1.0)
    with pytest.raises(ValueError):
        call(i32(10, 10), i32(0, 0), depth_weight=float("nan"))
    with pytest.raises(_lib.FoundPoseNativeError):          # a CPU tensor is refused
        call(i32(10, 10), torch.zeros(2, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------- the drivers
def test_driver_joint_pose_is_the_same_in_both_drivers(tmp_path, driver_split, monkeypatch):
    ex, split, opts, depths = driver_split
    costs = []
    real = refine_util.refine_rgbd

    def spy(*a, **k):
        out = real(*a, **k)
        costs.append((out["status"].cpu().numpy(), out["cost_in"].cpu().numpy(), out["cost_out"].cpu().numpy(), out["num_depth_inliers"].cpu().numpy()))
        return out
    monkeypatch.setattr(refine_util, "refine_rgbd", spy)
    jopts = opts._replace(final_pose_type="featuremetric_depth_joint", refine_iters=10, depth_refine_max_dist=15.0, depth_refine_weight=1.0)
    per_object, full = gd._drive(tmp_path, "joint", ex, split, jopts, depths)
    n_calls = len(costs)
    batched, full_b = gd._drive(tmp_path, "joint_b4", ex, split, jopts, depths, batch=4)
    assert per_object == batched and [len(per_object[lid]) for lid in (1, 2)] == [4, 2]      # estimated-poses.json up to its times
    assert n_calls >= 3 and len(costs) > n_calls
    for st, cin, cout, ninl in costs:
        assert (cout <= cin).all()
    assert any((st == 0).any() for st, *_ in costs) and any((ninl >= 6).any() for *_, ninl in costs)
    for entries in (*full.values(), *full_b.values()):
        assert all(e["time"]["pose_refine"] > 0 for e in entries)
    coarse, _ = gd._drive(tmp_path, "coarse", ex, split, opts, depths)
    assert coarse != per_object                                # the final pose is the refined one
    with pytest.raises(ValueError, match="scene 1 image 3"):
        gd._drive(tmp_path, "nodepth", ex, split, jopts, None)
    with pytest.raises(ValueError, match="scene 1 image 3"):
        gd._drive(tmp_path, "nodepth_b", ex, split, jopts, None, batch=4)
