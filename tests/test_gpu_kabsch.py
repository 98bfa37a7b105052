"""fp_kabsch_ransac (pnp_util.solve_kabsch_ransac_batch) against its numpy restatement (tests/kabsch_ref.py) on the smallest batch that
reaches every path: 2 x 3 pairs, K = 40, 300 hypotheses (the loop strides, unevenly), 48 x 64 depth; counts 0, 5, K and 57 (clamped), a
pair with no depth under it, a detection whose pixels leave the frame image, A = I and a rotated A.  The fixture is far from every
decision boundary (min_margin, asserted), so success, num_valid, quality, the inlier masks and the winning hypothesis must be EQUAL;
the refit pose must agree within the project's bar for GPU against numpy fp64, 1e-6 rad / 1e-3 mm."""

import numpy as np
import pytest
import torch

from tests import kabsch_ref as kr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return kr.gpu_fixture()


@pytest.fixture(scope="module")
def ref(fix):
    out = kr.run_ref_on(fix)
    assert out["min_margin"] > 1e-6
    return out


def _run(fix, rows=None, refit=True, pair_keys=None, image_index=None, solve=None, tau=None):
    """The fixture's detections `rows` (default: both) through the GPU path -> dict of numpy arrays, pairs flattened."""
    from foundpose_amd import pnp_util
    rows = list(range(2)) if rows is None else rows
    n, K = fix["n_slots"], fix["K"]
    sel = [r * n + j for r in rows for j in range(n)]
    dev = "cuda"
    out = pnp_util.solve_kabsch_ransac_batch(
        torch.from_numpy(fix["coord_2d"][sel]).reshape(len(rows), n, K, 2).to(dev), torch.from_numpy(fix["coord_3d"][sel]).reshape(len(rows), n, K, 3).to(dev),
        torch.from_numpy(fix["counts"][sel]).reshape(len(rows), n).to(dev), [fix["solve"][r] for r in rows] if solve is None else solve,
        [fix["frames"][r] for r in rows], torch.from_numpy(fix["depth"]).to(dev), [fix["image_index"][r] for r in rows] if image_index is None else image_index,
        [fix["tau"][r] for r in rows] if tau is None else tau, fix["iters"], 0.99, refit, fix["seed"], return_ransac_pose=True, pair_keys=pair_keys)
    torch.cuda.synchronize()
    return {k: v.reshape(len(sel), *v.shape[2:]).cpu().numpy() for k, v in out.items()}


def test_matches_the_restatement(fix, ref):
    out = _run(fix)
    assert np.array_equal(out["success"], ref["success"])
    assert np.array_equal(out["num_valid"], ref["num_valid"])
    assert np.array_equal(out["quality"], ref["quality"].astype(np.float64))
    assert np.array_equal(out["inliers"], ref["inliers"])
    worst = {"hyp_rad": 0.0, "hyp_mm": 0.0, "rad": 0.0, "mm": 0.0}
    for p in range(6):
        rp = out["ransac_pose"][p]
        if not ref["success"][p]:   # fp_pnp_ransac's failure record
            assert np.array_equal(out["R"][p], np.eye(3)) and not out["t"][p].any() and not rp.any() and not out["inliers"][p].any()
            continue
        # the winning hypothesis: the same three correspondences give the same closed-form pose up to fp64 rounding -- any other hypothesis
        # is a different triangle, whole millimetres / milliradians away
        worst["hyp_rad"] = max(worst["hyp_rad"], kr.rotation_angle(rp[:9].reshape(3, 3), ref["ransac_R"][p]))
        worst["hyp_mm"] = max(worst["hyp_mm"], float(np.abs(rp[9:] - ref["ransac_t"][p]).max()))
        worst["rad"] = max(worst["rad"], kr.rotation_angle(out["R"][p], ref["R"][p]))
        worst["mm"] = max(worst["mm"], float(np.abs(out["t"][p] - ref["t"][p]).max()))
        assert abs(np.linalg.det(out["R"][p]) - 1.0) < 1e-12 and np.abs(out["R"][p] @ out["R"][p].T - np.eye(3)).max() < 1e-12
    print(f"GPU against the restatement, maximum over the pairs: winning hypothesis {worst['hyp_rad']:.3e} rad / {worst['hyp_mm']:.3e} mm, "
          f"refit pose {worst['rad']:.3e} rad / {worst['mm']:.3e} mm")
    assert worst["hyp_rad"] < 1e-9 and worst["hyp_mm"] < 1e-6
    assert worst["rad"] < 1e-6 and worst["mm"] < 1e-3


def test_without_refit_the_output_is_the_winning_hypothesis(fix, ref):
    out = _run(fix, refit=False)
    for p in np.nonzero(ref["success"])[0]:
        assert np.array_equal(out["R"][p].reshape(9), out["ransac_pose"][p][:9]) and np.array_equal(out["t"][p], out["ransac_pose"][p][9:])
    assert np.array_equal(out["inliers"], ref["inliers"])


def test_batch_invariance_and_null_keys(fix):
    n = fix["n_slots"]
    keys = [[100 + r * n + j for j in range(n)] for r in range(2)]
    both = _run(fix, pair_keys=keys)
    rev = _run(fix, rows=[1, 0], pair_keys=[keys[1], keys[0]])
    for k, v in both.items():
        assert np.array_equal(v, np.concatenate([rev[k][n:], rev[k][:n]])), k
    for r in range(2):
        alone = _run(fix, rows=[r], pair_keys=[keys[r]])
        for k, v in alone.items():
            assert np.array_equal(v, both[k][r * n:(r + 1) * n]), (r, k)
    plain = _run(fix)
    ident = _run(fix, pair_keys=torch.arange(2 * n, dtype=torch.int64).reshape(2, n))
    for k, v in plain.items():
        assert np.array_equal(v, ident[k]), k
    assert not np.array_equal(plain["ransac_pose"], both["ransac_pose"])   # other keys, other hypotheses


def test_bad_arguments_raise_before_anything_is_written(fix):
    from foundpose_amd import _lib, crop_util
    for bad in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="image index"):
            _run(fix, image_index=bad)
    with pytest.raises(ValueError, match="inlier_thresh_mm"):
        _run(fix, tau=[4.0, 0.0])
    crop = fix["solve"][1]
    Ts = crop.T_world_from_eye.copy()
    Ts[:3, 3] += (0.5, 0.0, 0.0)
    moved = crop_util.PinholePlaneCameraModel(crop.width, crop.height, crop.f, crop.c, Ts)
    with pytest.raises(ValueError, match="share their centre"):
        _run(fix, solve=[fix["solve"][0], moved])
    # the C entry itself: a detection whose image index is outside the stack is reported as success -1 and fails; the other is untouched
    from foundpose_amd._lib import call, ptr, stream
    n, K, dev = fix["n_slots"], fix["K"], "cuda"
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    c2, c3, cnt = t(fix["coord_2d"], torch.float32), t(fix["coord_3d"], torch.float32), t(fix["counts"], torch.int32)
    cam = t([kr.camera_tuple(c) for c in fix["solve"]], torch.float64)
    fcam = t([kr.camera_tuple(c) for c in fix["frames"]], torch.float64)
    A, tau, depth = t(fix["A"].reshape(2, 9), torch.float64), t(fix["tau"], torch.float64), t(fix["depth"], torch.float32)
    iid = t([0, 7], torch.int32)
    success = torch.full((6,), 9, dtype=torch.int32, device=dev)
    R, tt = torch.zeros(6, 9, dtype=torch.float64, device=dev), torch.zeros(6, 3, dtype=torch.float64, device=dev)
    ninl, nval = torch.zeros(6, dtype=torch.int32, device=dev), torch.zeros(6, dtype=torch.int32, device=dev)
    mask = torch.ones(6, K, dtype=torch.uint8, device=dev)
    call("fp_kabsch_ransac", ptr(c2), ptr(c3), ptr(cnt), ptr(cam), ptr(fcam), ptr(A), ptr(iid), ptr(tau), ptr(depth), 2, 48, 64, ptr(None), 6, n, K,
         fix["iters"], 0.99, 1, 6, fix["seed"], ptr(success), ptr(R), ptr(tt), ptr(ninl), ptr(nval), ptr(mask), ptr(None), stream())
    torch.cuda.synchronize()
    assert success.cpu().tolist() == [1, 0, 0, -1, -1, -1] and not mask[3:].any() and nval[3:].cpu().tolist() == [0, 0, 0]
    for args, msg in (((6, n, 5000, 300), "k_max"), ((6, n, K, 5000), "iterations"), ((5, n, K, 300), "multiple of n_slots")):
        with pytest.raises(_lib.FoundPoseNativeError, match=msg):
            call("fp_kabsch_ransac", ptr(c2), ptr(c3), ptr(cnt), ptr(cam), ptr(fcam), ptr(A), ptr(iid), ptr(tau), ptr(depth), 2, 48, 64, ptr(None),
                 args[0], args[1], args[2], args[3], 0.99, 1, 6, 0, ptr(success), ptr(R), ptr(tt), ptr(ninl), ptr(nval), ptr(mask), ptr(None), stream())
