"""CPU: the featuremetric refinement's numpy restatement (tests/featuremetric_ref.py), the driver's option checks and the C ABI entry."""

import os
import re

import numpy as np
import pytest

from tests import featuremetric_ref as fr

CAM = (300.0, 310.0, 259.0, 255.0)
W = H = 518


def _scene(seed, n=200, C=16, grid=37):
    rng = np.random.default_rng(seed)
    M = fr.smooth_field(grid, grid, C, seed)
    from foundpose_amd import synthetic
    v = synthetic.make_blob_mesh(20, 20, radius=50.0, seed=seed).vertices.astype(np.float64)
    X = v[rng.choice(len(v), n, replace=False)]
    R = fr.rot_exp(rng.normal(size=3) * 0.3)
    t = np.array([5.0, -8.0, 600.0])
    return M, X, R, t


def test_jacobian_matches_central_differences():
    M, X, R, t = _scene(1, C=8)
    M = M.astype(np.float64)
    rng = np.random.default_rng(2)
    f = rng.normal(size=(len(X), M.shape[2]))
    valid = fr.valid_set(R, t, X, CAM, W, H, M)
    _, _, xm, ym = fr.map_coords(R, t, X, CAM, W, H, M.shape[1], M.shape[0])
    # away from the cell borders, where the bilinear field is smooth
    inner = valid & (np.abs(xm - np.round(xm)) > 0.05) & (np.abs(ym - np.round(ym)) > 0.05)
    X, f = X[inner], f[inner]
    assert len(X) > 50
    J, _ = fr.jacobian(R, t, X, f, CAM, W, H, M)
    eps = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = eps
        Rp, tp = fr.update(R, t, d)
        Rm, tm = fr.update(R, t, -d)
        _, rp = fr.jacobian(Rp, tp, X, f, CAM, W, H, M)
        _, rm = fr.jacobian(Rm, tm, X, f, CAM, W, H, M)
        fd = (rp - rm) / (2 * eps)
        np.testing.assert_allclose(J[:, :, k], fd, rtol=1e-4, atol=1e-6 * np.abs(J[:, :, k]).max())


def test_planted_field_converges():
    M, X, R, t = _scene(3, C=32)
    f = fr.sample_at(M, R, t, X, CAM, W, H)
    R0, t0 = fr.update(R, t, np.array([np.radians(2.0), 0.0, 0.0, 5.0, 0.0, 0.0]))
    out = fr.refine(R0, t0, X, f, CAM, W, H, M, iters=30)
    assert out["status"] == 0 and out["cost_out"] < out["cost_in"]
    assert fr.rot_angle_deg(out["R"], R) < 0.01
    assert np.linalg.norm(out["t"] - t) < 0.1


def test_skips_and_zero_iterations():
    M, X, R, t = _scene(4)
    f = fr.sample_at(M, R, t, X, CAM, W, H)
    assert fr.refine(R, t, X, f, CAM, W, H, M, has_pose=False)["status"] == 2
    assert fr.refine(R, t, X[:5], f[:5], CAM, W, H, M)["status"] == 2
    out = fr.refine(R, t, X, f, CAM, W, H, M, iters=0)
    assert out["status"] == 1 and out["iters_used"] == 0 and np.array_equal(out["R"], R)


def test_load_opts_accepts_refinement_options():
    from foundpose_amd import infer
    o = infer.load_opts({"infer_opts": dict(version="v", repre_version="r", object_dataset="lmo", final_pose_type="featuremetric", refine_iters=12)})
    assert o.final_pose_type == "featuremetric" and o.refine_iters == 12
    assert infer.InferOpts(version="v", repre_version="r", object_dataset="lmo").refine_iters == 30


@pytest.mark.parametrize("bad", [dict(final_pose_type="refined"), dict(final_pose_type="best_refined"),
                                 dict(final_pose_type="featuremetric", refine_iters=-1)])
def test_driver_refuses_unknown_final_pose_types_before_gpu_work(bad):
    from foundpose_amd import infer
    with pytest.raises(ValueError):
        infer.infer_object(infer.InferOpts(version="v", repre_version="r", object_dataset="lmo", **bad), 1, None, [], {})


def test_refine_symbol_declared_and_prototyped():
    from foundpose_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "foundpose_amd.h")).read()
    assert re.search(r"\bfp_featuremetric_refine\s*\(", header)
    assert "fp_featuremetric_refine" in _lib.exported_symbols()
    assert _lib.refine_scratch_bytes(32, 300) >= 512 * 32 + 256 * 32 * 10 + 32 * 300


def test_refine_rejects_cpu_tensors():
    import torch
    from foundpose_amd import _lib, refine_util
    z = torch.zeros
    with pytest.raises(_lib.FoundPoseNativeError):
        refine_util.refine_featuremetric(z(1, 4, 4, 8), (56, 56), [CAM], z(1, 3, 3), z(1, 3), z(1, dtype=torch.int32), z(1, dtype=torch.int32),
                                         z(10, 8), z(10, 3), z(1, dtype=torch.bool))
