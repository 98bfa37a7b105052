"""GPU: refinement of the final pose against the frame's depth (csrc/depth_refine.hip, refine_util.refine_depth, the drivers'
final_pose_type="depth" / "featuremetric_depth") against the numpy restatement tests/depth_refine_ref.py.  Every kernel test uses a
96 x 80 depth image: not square, so that a swap of W and H shows."""
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, refine_util, synthetic
from tests import depth_refine_ref as dr

pytestmark = pytest.mark.gpu
H, W = 80, 96
CAM = (180.0, 185.0, 47.3, 39.6)


def _run(depth, dets, iters=30, normal_eq=False, max_points=None):
    """depth [N, H, W] fp32; dets: list of dict(X, R, t, tau, image=0, has_pose=True) -> refine_depth's dict (cpu numpy)."""
    X = np.concatenate([d["X"] for d in dets]).astype(np.float32)
    n = np.array([len(d["X"]) for d in dets])
    rb = np.concatenate([[0], np.cumsum(n)[:-1]])
    cuda = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    out = refine_util.refine_depth(
        cuda(depth, torch.float32), cuda(np.array([d.get("image", 0) for d in dets]), torch.int32), [CAM] * len(dets),
        cuda(np.stack([d["R"] for d in dets]), torch.float64), cuda(np.stack([d["t"] for d in dets]), torch.float64), cuda(rb, torch.int32),
        cuda(rb + n, torch.int32), cuda(X), cuda(np.array([d.get("has_pose", True) for d in dets])), [d["tau"] for d in dets], iters=iters,
        return_normal_equations=normal_eq, max_points=max_points)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ref(depth, d, iters=100):
    return dr.refine(d["R"], d["t"], d["X"].astype(np.float32).astype(np.float64), CAM, depth[d.get("image", 0)], d["tau"], iters, d.get("has_pose", True))


def _perturb(rng, R, t, rot_deg=3.0, trans_mm=10.0):
    ax, dt = rng.normal(size=3), rng.normal(size=3)
    return dr.rot_exp(ax / np.linalg.norm(ax) * np.radians(rot_deg)) @ R, t + dt * trans_mm / np.linalg.norm(dt)


def _analytic(seed, n, tau=25.0, rot_deg=1.0, trans_mm=4.0):
    """n points on the bilinear surface of an analytic depth image, under a pose a little off the planted one."""
    rng = np.random.default_rng(seed)
    D, _ = dr.analytic_depth(H, W, CAM)
    uv = np.stack([rng.uniform(4, W - 5, n), rng.uniform(4, H - 5, n)], 1)
    R = dr.rot_exp(rng.normal(size=3) * 0.4)
    t = np.array([3.0, -4.0, 600.0])
    X = ((dr.backproject(D, CAM, uv) - t) @ R).astype(np.float32)
    R0, t0 = _perturb(rng, R, t, rot_deg, trans_mm)
    return D, dict(X=X, R=R0, t=t0, tau=tau), (R, t)


# ---------------------------------------------------------------------------------------------------- the planted blob
def render_ref_depth(mesh, T_m2c):
    """The rasterizer's depth by its numpy restatement (bit-identical to HipRasterizer's; tests/test_gpu_render.py).  No GPU test calls
    it: blob_cases(render_ref_depth) is the generator of REF_ERROR below, and tests/test_depth_refine_cpu.py recomputes the constants
    from it so that they cannot drift."""
    from tests import render_ref
    Tc = np.linalg.inv(T_m2c)
    cam = np.concatenate([[CAM[0], CAM[1], CAM[2] + 0.5, CAM[3] + 0.5], Tc[:3, :3].reshape(-1), Tc[:3, 3]])
    return render_ref.rasterize(mesh.vertices, mesh.faces, cam, W, H)[0]


def hip_depth(mesh, T_m2c):
    from foundpose_amd.crop_util import PinholePlaneCameraModel
    from foundpose_amd.renderer import HipRasterizer
    ras = HipRasterizer("cuda")
    ras.add_object_model(1, mesh=mesh)
    # the rasterizer samples at pixel centres x + 1/2; the refinement's camera has them at integers: shift the principal point
    cam = PinholePlaneCameraModel(W, H, CAM[:2], (CAM[2] + 0.5, CAM[3] + 0.5), np.linalg.inv(T_m2c))
    return ras.render_views(1, [cam], with_color=False)["depth"][0].cpu().numpy()


def blob_scene(render, seed=0, step=2):
    """Depth rendered from synthetic.make_blob_mesh at a ground-truth pose; the points are every step-th pixel of a render 10 degrees
    away, back-projected and moved into the model frame.  -> (depth [H, W], X [P, 3] fp32, (R_gt, t_gt))."""
    rng = np.random.default_rng(seed)
    mesh = synthetic.make_blob_mesh(20, 20, radius=50.0, seed=seed)
    to_T = lambda R, t: np.block([[R, np.reshape(t, (3, 1))], [np.zeros((1, 3)), np.ones((1, 1))]])
    R = dr.rot_exp(rng.normal(size=3) * 0.5)
    t = np.array([4.0, -3.0, 600.0])
    ax = rng.normal(size=3)
    R2 = dr.rot_exp(ax / np.linalg.norm(ax) * np.radians(10.0)) @ R
    depth, other = render(mesh, to_T(R, t)), render(mesh, to_T(R2, t))
    ys, xs = np.nonzero(other > 0)
    ys, xs = ys[::step], xs[::step]
    z = other[ys, xs].astype(np.float64)
    Xc = np.stack([(xs - CAM[2]) / CAM[0] * z, (ys - CAM[3]) / CAM[1] * z, z], 1)
    return depth, ((Xc - t) @ R2).astype(np.float32), (R, t)


def blob_cases(render):
    """The detections of the planted-blob tests: [(name, depth, det, (R_gt, t_gt))] -- two clean starts, holes, holes and an occluder strip
    (the scene that shows limit (2) of DESIGN.md section 14), and two scenes with holes and an occluder 40 mm in front of the object's
    whole left part, from which the pose is recovered."""
    cases = []
    for seed in (0, 1):
        depth, X, gt = blob_scene(render, seed)
        R0, t0 = _perturb(np.random.default_rng(50 + seed), *gt)
        cases.append((f"clean{seed}", depth, dict(X=X, R=R0, t=t0, tau=20.0), gt))
    depth, X, gt = blob_scene(render, 0)
    ys, xs = np.nonzero(depth > 0)
    cy, cx = int(np.median(ys)), int(np.median(xs))
    bad = depth.copy()
    bad[cy - 14:cy - 6, cx - 4:cx + 6] = 0.0                                                         # a hole
    bad[0:6, 0:8] = 0.0
    R0, t0 = _perturb(np.random.default_rng(60), *gt)
    cases.append(("holes", bad.copy(), dict(X=X, R=R0, t=t0, tau=10.0), gt))
    bad[cy + 3:cy + 11, :cx] = np.where(depth[cy + 3:cy + 11, :cx] > 0, depth[cy + 3:cy + 11, :cx] - 40.0, 0.0)   # an occluder 40 mm in front
    cases.append(("occluded", bad, dict(X=X, R=R0, t=t0, tau=10.0), gt))
    for seed in (1, 2):   # every pixel of the other render as a point: the occluder's one edge across the object weighs less
        depth, X, gt = blob_scene(render, seed, step=1)
        ys, xs = np.nonzero(depth > 0)
        cy, cx = int(np.median(ys)), int(np.median(xs))
        bad = depth.copy()
        bad[cy - 14:cy - 6, cx - 4:cx + 6] = 0.0
        bad[:, :cx - 8] = np.where(depth[:, :cx - 8] > 0, depth[:, :cx - 8] - 40.0, 0.0)
        R0, t0 = _perturb(np.random.default_rng(60), *gt)
        cases.append((f"occluded_left{seed}", bad, dict(X=X, R=R0, t=t0, tau=10.0), gt))
    return cases


def pose_error(R, t, gt):
    return np.radians(dr.rot_angle_deg(R, gt[0])), float(np.linalg.norm(np.asarray(t) - gt[1]))


START_ERROR = (np.radians(3.0), 10.0)   # every start is 3 degrees / 10 mm off (rad, mm)
# The restatement's own final error against the ground truth on blob_cases (render_ref_depth, numpy, on the CPU;
# tests/test_depth_refine_cpu.py recomputes it): bilinear depth is not the true surface and the points come from another render (a fifth
# of them hidden in this one), so the minimum is not exactly the ground truth.  (rad, mm).  "occluded" is NOT a recovery: with the occluder
# strip the restatement itself ends 6.9 degrees off -- bilinear taps that straddle the 40 mm step read depths between the two surfaces,
# those points are inliers with a 40 mm / pixel gradient, and the strip's two long edges across this smooth blob outweigh the rest
# (limit (2)); only the translation improves, from 10 to 3.8 mm.  The two "occluded_left" scenes are recoveries.
REF_ERROR = {"clean0": (1.2051e-02, 0.3167), "clean1": (4.1374e-02, 0.6311), "holes": (1.1633e-02, 0.2825), "occluded": (1.2089e-01, 3.8387),
             "occluded_left1": (2.3888e-02, 0.6079), "occluded_left2": (4.6644e-03, 0.1914)}
RECOVERED = ("clean0", "clean1", "holes", "occluded_left1", "occluded_left2")   # the restatement's error is below the start's in rotation and in translation


# ---------------------------------------------------------------------------------------------------- kernel tests
def test_normal_equations_and_cost_match_restatement():
    """Both sides compute in fp64 from the same fp32 taps and differ in summation order only: 1e-9 of the largest entry per block."""
    counts = (5, 6, 32, 33, 70)
    scenes = [_analytic(10 + n, n) for n in counts]
    depth = np.stack([s[0] for s in scenes])
    dets = [dict(s[1], image=i) for i, s in enumerate(scenes)]
    out = _run(depth, dets, iters=0, normal_eq=True)
    for b, d in enumerate(dets):
        X64 = d["X"].astype(np.float64)
        want = dr.normal_equations(d["R"], d["t"], X64, CAM, depth[b], d["tau"])
        got = out["normal_eq"][b]
        inl = int(dr.system(d["R"], d["t"], X64, CAM, depth[b], d["tau"])[3].sum())
        print(f"{counts[b]} points, {inl} inliers: max |dH| {np.abs(got[:21] - want[:21]).max():.3e} of {np.abs(want[:21]).max():.3e}, "
              f"|dg| {np.abs(got[21:27] - want[21:27]).max():.3e} of {np.abs(want[21:27]).max():.3e}, cost {got[27]!r} vs {want[27]!r}")
        assert inl == counts[b]                       # every point of these scenes is an inlier at the start
        for lo, hi in ((0, 21), (21, 27), (27, 28)):
            assert np.abs(got[lo:hi] - want[lo:hi]).max() <= 1e-9 * np.abs(want[lo:hi]).max(), (b, lo)
        assert out["num_points"][b] == inl and out["iters_used"][b] == 0
        assert out["status"][b] == (2 if counts[b] < 6 else 1)
        assert out["cost_in"][b] == out["cost_out"][b] == got[27]
        assert np.array_equal(out["R"][b], d["R"]) and np.array_equal(out["t"][b], d["t"])


def test_planted_blob_converges_like_the_restatement():
    for name, depth, det, gt in blob_cases(hip_depth)[:2]:
        assert name in RECOVERED
        out = _run(depth[None], [det], iters=100)
        ref = _ref(depth[None], det)
        R, t = out["R"][0], out["t"][0]
        e0, e1, er = pose_error(det["R"], det["t"], gt), pose_error(R, t, gt), pose_error(ref["R"], ref["t"], gt)
        print(f"{name}: {len(det['X'])} points, {out['num_points'][0]} inliers, start {e0[0]:.4e} rad / {e0[1]:.4f} mm -> GPU {e1[0]:.4e} rad / {e1[1]:.4f} mm, "
              f"restatement {er[0]:.4e} rad / {er[1]:.4f} mm, cost {out['cost_in'][0]:.4f} -> {out['cost_out'][0]:.4f}, {out['iters_used'][0]} iterations")
        assert out["status"][0] == 0 and out["cost_out"][0] < out["cost_in"][0]
        assert np.radians(dr.rot_angle_deg(R, ref["R"])) < 1e-6 and np.linalg.norm(t - ref["t"]) < 1e-3
        assert e1[0] < START_ERROR[0] and e1[1] < START_ERROR[1]
        assert e1[0] <= 2 * REF_ERROR[name][0] and e1[1] <= 2 * REF_ERROR[name][1]


def _against_restatement(cases, extra=()):
    """Runs the cases (and `extra` detections on images stacked behind theirs) as one batch; every case: the cost falls, the inliers at
    the start are the restatement's, the final pose is the restatement's within 1e-6 rad / 1e-3 mm.  -> (out, [(GPU error, restatement error)])."""
    out = _run(np.stack([c[1] for c in cases] + [e[0] for e in extra]),
               [dict(c[2], image=i) for i, c in enumerate(cases)] + [dict(e[1], image=len(cases) + i) for i, e in enumerate(extra)], iters=100)
    errs = []
    for b, (name, depth, det, gt) in enumerate(cases):
        ref = _ref(depth[None], det)
        e1, er = pose_error(out["R"][b], out["t"][b], gt), pose_error(ref["R"], ref["t"], gt)
        print(f"{name}: {out['num_points'][b]} of {len(det['X'])} points are inliers at the start, GPU {e1[0]:.4e} rad / {e1[1]:.4f} mm, "
              f"restatement {er[0]:.4e} rad / {er[1]:.4f} mm, cost {out['cost_in'][b]:.4f} -> {out['cost_out'][b]:.4f}, {out['iters_used'][b]} iterations")
        assert out["cost_out"][b] <= out["cost_in"][b] and out["status"][b] == 0
        assert out["num_points"][b] == ref["num_points"] < len(det["X"])
        assert np.radians(dr.rot_angle_deg(out["R"][b], ref["R"])) < 1e-6 and np.linalg.norm(out["t"][b] - ref["t"]) < 1e-3
        errs.append((e1, er))
    return out, errs


def test_holes_and_an_occluder():
    """Holes alone, and holes with an occluder 40 mm in front of the object's left part (two blobs): the pose is still recovered -- rotation
    and translation errors both below the start's and within twice the restatement's own.  A depth image that is all zeros is skipped."""
    cases = [c for c in blob_cases(hip_depth) if c[0] in ("holes", "occluded_left1", "occluded_left2")]
    det = cases[0][2]
    out, errs = _against_restatement(cases, extra=[(np.zeros((H, W), np.float32), det)])
    for (name, *_), (e1, _) in zip(cases, errs):
        assert e1[0] < START_ERROR[0] and e1[1] < START_ERROR[1], (name, e1)
        assert e1[0] <= 2 * REF_ERROR[name][0] and e1[1] <= 2 * REF_ERROR[name][1], (name, e1)
    z = len(cases)
    assert out["status"][z] == 2 and out["num_points"][z] == 0 and out["cost_in"][z] == out["cost_out"][z] == det["tau"] ** 2
    assert np.array_equal(out["R"][z], det["R"]) and np.array_equal(out["t"][z], det["t"])


def test_occluder_strip_shows_the_limit_of_bilinear_taps():
    """NOT a recovery test: DESIGN.md section 14, limit (2).  With a 40 mm occluder STRIP across the blob the restatement itself turns away
    from the ground truth (see REF_ERROR); what holds is that the GPU follows the restatement, the cost falls and the translation improves."""
    cases = [c for c in blob_cases(hip_depth) if c[0] == "occluded"]
    _, errs = _against_restatement(cases)
    assert errs[0][0][1] < START_ERROR[1]


def test_batch_invariance_and_determinism():
    D, probe, _ = _analytic(30, 70, rot_deg=3.0, trans_mm=10.0)
    D2, a, _ = _analytic(31, 33, tau=12.0)
    _, b, _ = _analytic(32, 140, tau=40.0)
    alone = _run(D[None], [probe], normal_eq=True)
    stack = np.stack([D2, D * 1.01, D])                      # the probe reads image 2 of 3
    dets = [dict(a, image=0), dict(b, image=1), dict(probe, image=2)]
    batch = _run(stack, dets, normal_eq=True, max_points=200)
    again = _run(stack, dets, normal_eq=True, max_points=200)
    assert alone["status"][0] == 0 and alone["iters_used"][0] > 2 and "normal_eq" in batch and np.abs(alone["normal_eq"][0]).max() > 0
    for key in batch:
        assert np.array_equal(batch[key], again[key]), key
        assert np.array_equal(alone[key][0], batch[key][2]), key


def test_degenerate_inputs():
    D, det, _ = _analytic(40, 50)
    out = _run(D[None], [dict(det, has_pose=False), det], iters=0)
    assert out["status"].tolist() == [2, 1] and out["iters_used"].tolist() == [0, 0]
    for b in range(2):
        assert np.array_equal(out["R"][b], det["R"]) and np.array_equal(out["t"][b], det["t"])
    assert out["cost_in"][0] == out["cost_out"][0] == 0.0 and out["num_points"][0] == 0
    want = dr.normal_equations(det["R"], det["t"], det["X"].astype(np.float64), CAM, D, det["tau"])[27]
    assert out["cost_in"][1] == out["cost_out"][1] and abs(out["cost_in"][1] - want) <= 1e-9 * want
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    one = torch.ones(1, dtype=torch.bool, device="cuda")
    # a bank row range outside the bank and an image index out of range are reported, not read
    with pytest.raises(_lib.FoundPoseNativeError, match="bank rows"):
        refine_util.refine_depth(z(1, H, W), z(1, dt=torch.int32), [CAM], z(1, 3, 3), z(1, 3), z(1, dt=torch.int32),
                                 torch.full((1,), 11, dtype=torch.int32, device="cuda"), z(10, 3), one, 10.0, max_points=64)
    for bad in (1, -1):
        with pytest.raises(_lib.FoundPoseNativeError, match="image index"):
            refine_util.refine_depth(z(1, H, W), torch.full((1,), bad, dtype=torch.int32, device="cuda"), [CAM], z(1, 3, 3), z(1, 3), z(1, dt=torch.int32),
                                     torch.full((1,), 10, dtype=torch.int32, device="cuda"), z(10, 3), one, 10.0, max_points=64)
    with pytest.raises(ValueError):
        refine_util.refine_depth(z(1, 1, W), z(1, dt=torch.int32), [CAM], z(1, 3, 3), z(1, 3), z(1, dt=torch.int32), z(1, dt=torch.int32), z(10, 3), one, 10.0)
    # the +1 tap of a point at x0 = W - 1 (y0 = H - 1) is never read: the restatement marks such a point not measurable, so it adds tau^2
    # (read from the next row, or past the image, it would add the flat surface's 2^2 like the points inside)
    zc = 600.0
    at = lambda u, v: [(u - CAM[2]) / CAM[0] * zc, (v - CAM[3]) / CAM[1] * zc, zc]
    edge = np.array([at(W - 1 + 0.5, 30.0), at(W - 1 + 0.01, 31.0), at(20.0, H - 1 + 0.25), at(W - 1 + 0.75, H - 1 + 0.5)]
                    + [at(10.0 + 7 * k, 12.0 + 5 * k) for k in range(8)], np.float32)
    flat = np.full((H, W), zc + 2.0, np.float32)
    d = dict(X=edge, R=np.eye(3), t=np.zeros(3), tau=10.0)
    assert not dr.point_terms(d["R"], d["t"], edge.astype(np.float64), CAM, flat)["measurable"][:4].any()
    got = _run(flat[None], [d], iters=0, normal_eq=True)
    want = dr.normal_equations(d["R"], d["t"], edge.astype(np.float64), CAM, flat, 10.0)
    assert got["num_points"][0] == 8 and np.isfinite(got["normal_eq"]).all()
    assert abs(got["normal_eq"][0][27] - want[27]) <= 1e-9 * want[27]
    assert got["normal_eq"][0][27] == pytest.approx((4 * 100.0 + 8 * 4.0) / 12, rel=1e-6)


def test_template_id_minus_one_has_no_pose():
    from foundpose_amd.bank import DeviceBank
    from foundpose_amd.matching import MatchResult
    from tests.test_gpu_featuremetric import _tiny_repre
    bank = DeviceBank([_tiny_repre()])
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    ids = torch.tensor([[2, -1], [-1, 1]], dtype=torch.int32, device="cuda")
    res = MatchResult(template_ids=ids, template_scores=z(2, 2), counts=z(2, 2, dt=torch.int32), q_ids=z(2, 2, 1, dt=torch.int32),
                      feat_ids=z(2, 2, 1, dt=torch.int32), dists=z(2, 2, 1), conf=z(2, 2, 1), coord_2d=z(2, 2, 1, 2), coord_3d=z(2, 2, 1, 3))
    R = torch.eye(3, dtype=torch.float64, device="cuda")[None].repeat(2, 1, 1)
    t = torch.tensor([[0.0, 0.0, 600.0], [1.0, 2.0, 500.0]], dtype=torch.float64, device="cuda")
    best = {"found": torch.tensor([True, True], device="cuda"), "corresp_id": torch.tensor([0, 0], device="cuda"), "R": R, "t": t}
    out = refine_util.refine_best_coarse_depth(res, best, bank, [0, 0], [CAM, CAM], [CAM, CAM], torch.full((1, H, W), 600.0, device="cuda"), [0, 0], 10.0)
    assert out["status"].cpu().tolist()[1] == 2
    assert torch.equal(out["R"][1], R[1]) and torch.equal(out["t"][1], t[1])


# ---------------------------------------------------------------------------------------------------- the drivers
def _split_depth(split, opts):
    """make_bop_eval_scene-style depth for tests/test_gpu_infer_batched.py's split: every instance's planted surface (workload.planted_vertices'
    depth in its crop camera, sampled twice per crop pixel and splatted into the frame) over a background plane at 1500 mm, an occluder
    40 mm in front of a strip of each frame's first instance and a hole; quantised to depth_scale 0.1 like a stored PNG."""
    from foundpose_amd import crop_util
    from tests.test_gpu_infer_batched import INSTANCES
    depths = [np.full((c.height, c.width), 1500.0, np.float32) for c in split.cams]
    seen, first = {}, {}
    for f, lid, (x, y, w, h) in INSTANCES:
        i = seen.get((f, lid), 0)
        seen[(f, lid)] = i + 1
        cam = split.cams[f]
        box = crop_util.calc_crop_box(crop_util.AlignedBox2f(x, y, x + w, y + h), make_square=True)
        cc = crop_util.construct_crop_camera(box, cam, tuple(opts.crop_size), opts.crop_rel_pad)
        pose = split.annos[(f, lid)][i].pose
        T_m2c = np.linalg.inv(cc.T_world_from_eye) @ np.block([[pose.R, pose.t.reshape(3, 1)], [np.zeros((1, 3)), np.ones((1, 1))]])
        u, v = np.meshgrid(np.arange(0, cc.width, 0.5), np.arange(0, cc.height, 0.5))
        u, v = u.ravel(), v.ravel()
        S = 2.0 * cc.c[0]
        z = T_m2c[2, 3] + 40.0 * np.sin(u * (2.0 * np.pi / S)) * np.cos(v * (2.0 * np.pi / S)) + 15.0 * np.cos(u * (5.0 / S) + v * (3.0 / S))
        xc = np.stack([(u - cc.c[0]) / cc.f[0] * z, (v - cc.c[1]) / cc.f[1] * z, z, np.ones_like(z)], 0)
        xf = (np.linalg.inv(cam.T_world_from_eye) @ cc.T_world_from_eye @ xc)[:3]
        px = np.rint(cam.f[0] * xf[0] / xf[2] + cam.c[0]).astype(np.int64)
        py = np.rint(cam.f[1] * xf[1] / xf[2] + cam.c[1]).astype(np.int64)
        ok = (px >= 0) & (px < cam.width) & (py >= 0) & (py < cam.height)
        depths[f][py[ok], px[ok]] = xf[2][ok].astype(np.float32)
        if f not in first:
            first[f] = True
            depths[f][y + h // 2:y + h // 2 + 12, x:x + w // 2] -= 40.0
            depths[f][y + 20:y + 40, x + w - 50:x + w - 30] = 0.0
    return [np.clip(np.rint(d / 0.1), 0, 65535).astype(np.uint16).astype(np.float32) * np.float32(0.1) for d in depths]


@pytest.fixture(scope="module")
def driver_split():
    from foundpose_amd import feature_util, infer
    from tests.test_gpu_infer_batched import SEED_STATE, Split, _opts
    from tests.test_gpu_infer_driver import NAME
    ex = feature_util.make_feature_extractor(NAME, random_init_seed=SEED_STATE, precision="fp32").to("cuda")
    split = Split(ex)
    opts = infer.load_opts({"infer_opts": _opts(object_lids=[1, 2])})
    return ex, split, opts, _split_depth(split, opts)


def _drive(tmp, tag, ex, split, opts, depths, batch=0):
    from foundpose_amd import infer
    from tests.test_gpu_infer_batched import TARGETS, _entries
    targets = {lid: TARGETS[lid] for lid in (1, 2)}
    frame = lambda f, lids: dict(split.frame(f, lids), **({} if depths is None else {"depth": depths[f]}))
    d = str(tmp / tag)
    if batch:
        infer.infer_batched(opts, iter([frame(f, None) for f in range(3)]), split.dets, split.repres, d, batch_detections=batch, extractor=ex,
                            num_target_insts=targets)
    else:
        infer.infer(opts, lambda lid: iter([frame(f, [lid]) for f in range(3)]), split.dets, split.repres, d, extractor=ex, num_target_insts=targets)
    full = {lid: json.load(open(os.path.join(d, str(lid), "estimated-poses.json"))) for lid in (1, 2)}
    return {lid: _entries(d, lid) for lid in (1, 2)}, full


def test_driver_depth_pose_is_the_same_in_both_drivers(tmp_path, driver_split, monkeypatch):
    ex, split, opts, depths = driver_split
    costs = []
    real = refine_util.refine_depth

    def spy(*a, **k):
        out = real(*a, **k)
        costs.append((out["status"].cpu().numpy(), out["cost_in"].cpu().numpy(), out["cost_out"].cpu().numpy()))
        return out
    monkeypatch.setattr(refine_util, "refine_depth", spy)
    coarse, _ = _drive(tmp_path, "coarse", ex, split, opts, depths)
    coarse_no_depth, _ = _drive(tmp_path, "coarse_nd", ex, split, opts, None)
    assert coarse == coarse_no_depth and not costs          # best_coarse never looks at the depth
    dopts = opts._replace(final_pose_type="depth", depth_refine_iters=20)
    per_object, full = _drive(tmp_path, "depth", ex, split, dopts, depths)
    n_calls = len(costs)
    batched, full_b = _drive(tmp_path, "depth_b3", ex, split, dopts, depths, batch=3)
    assert per_object == batched and [len(per_object[lid]) for lid in (1, 2)] == [4, 2]
    for st, cin, cout in costs:
        assert (cout <= cin).all()
    assert n_calls >= 3 and any((st == 0).any() for st, _, _ in costs)
    for entries in (*full.values(), *full_b.values()):
        assert all(e["time"]["pose_refine"] > 0 for e in entries)
    # MSSD (no symmetries) of the coarse and the depth-refined pose against the planted one, over the object's bank vertices
    by_frame = {3: 0, 4: 1, 5: 2}
    errs = {"coarse": [], "depth": []}
    for lid in (1, 2):
        V = split.repres[lid].vertices.cpu().numpy().astype(np.float64)
        for kind, est in (("coarse", coarse[lid]), ("depth", per_object[lid])):
            for e in est:
                gt = split.annos[(by_frame[int(e["img_id"])], lid)][int(e["inst_id"])].pose
                a = V @ np.array(e["R"]).T + np.array(e["t"]).reshape(1, 3)
                b = V @ gt.R.T + gt.t.reshape(1, 3)
                errs[kind].append(float(np.linalg.norm(a - b, axis=1).max()))
    print(f"MSSD against the planted poses, mean over {len(errs['coarse'])} detections: coarse {np.mean(errs['coarse']):.4f} mm, "
          f"depth-refined {np.mean(errs['depth']):.4f} mm; per detection {np.round(errs['coarse'], 3).tolist()} -> {np.round(errs['depth'], 3).tolist()}")
    with pytest.raises(ValueError, match="scene 1 image 3"):
        _drive(tmp_path, "nodepth", ex, split, dopts, None)
    with pytest.raises(ValueError, match="scene 1 image 3"):
        _drive(tmp_path, "nodepth_b", ex, split, dopts, None, batch=3)


def test_driver_featuremetric_then_depth_runs(tmp_path, driver_split):
    ex, split, opts, depths = driver_split
    fopts = opts._replace(final_pose_type="featuremetric_depth", refine_iters=5, depth_refine_iters=10, depth_refine_max_dist=15.0)
    per_object, full = _drive(tmp_path, "fd", ex, split, fopts, depths)
    batched, _ = _drive(tmp_path, "fd_b3", ex, split, fopts, depths, batch=3)
    assert per_object == batched and [len(per_object[lid]) for lid in (1, 2)] == [4, 2]
    assert all(e["time"]["pose_refine"] > 0 for es in full.values() for e in es)
