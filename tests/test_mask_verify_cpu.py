"""coarse_select_type "mask_verify" without a GPU: the numpy restatement (tests/mask_verify_ref.py) on a case small enough to count by hand,
the GPU tests' fixtures (far from every decision boundary, the planted pose scores highest), the C ABI's declaration, the drivers' option
checks and the argument checks of pnp_util.verify_poses_mask that come before any device work."""

import os
import re

import numpy as np
import pytest
import torch

from tests import mask_verify_ref as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hand_case(cx):
    """G = 8, a 12 x 16 mask.  R = A = I, t = (0, 0, 8), c = 0, rho = 4, f = 4: C = (0, 0, 8) and C.z = 8 > rho + 1; r_px = 4 * 4 / (8 - 4)
    = 4, h = 2 * 4 / 8 = 1: one cell per pixel, u0 = cx - 4, v0 = cy - 4 = 1.  A point (x, y, 0) has z = 8, u = x / 2 + cx, v = y / 2 + 5."""
    X = np.array([[1, 1, 0],        # u = cx + 0.5, v = 5.5: cell (ix, iy) = (4, 4)
                  [1.5, 1.5, 0],    # u = cx + 0.75, v = 5.75: (4, 4) again
                  [-1, 1, 0],       # (3, 4)
                  [1, -1, 0],       # (4, 3)
                  [3, 1, 0],        # (5, 4)
                  [-20, 0, 0],      # u = cx - 10: (u - u0) / h = -6, clamped to ix = 0; v = 5: (0, 4)
                  [0, 0, -7.5]],    # z = 0.5 <= 1: ignored
                 np.float32)
    mask = np.zeros((12, 16), np.uint8)
    mask[4:7, 5:7] = 1   # the 6 pixels (px, py) with px in {5, 6}, py in {4, 5, 6}
    return dict(R=np.eye(3), t=np.array([0.0, 0.0, 8.0]), A=np.eye(3), cam=(4.0, 4.0, cx, 5.0), X=X, c=np.zeros(3), rho=4.0, G=8), mask


def test_the_restatement_on_a_case_counted_by_hand():
    # cx = 6: u0 = 2, v0 = 1, cell (ix, iy) is pixel (ix + 2, iy + 1).  Occupied cells (4,4) (3,4) (4,3) (5,4) (0,4) = pixels (6,5) (5,5)
    # (6,4) (7,5) (2,5): the first three are in the mask, the last two are not; 6 - 3 mask pixels are no model pixels.
    case, mask = _hand_case(6.0)
    counts, score, status, model = mv.verify_pair(mask=mask, min_pixels=5, **case)
    assert counts.tolist() == [3, 2, 3, 5] and status == 0 and score == 3.0 / 8.0
    assert sorted(zip(*np.nonzero(model)[::-1])) == [(2, 5), (5, 5), (6, 4), (6, 5), (7, 5)]
    counts, score, status, _ = mv.verify_pair(mask=mask, min_pixels=6, **case)        # 5 model pixels < 6: counts reported, not scored
    assert counts.tolist() == [3, 2, 3, 5] and status == 1 and score == 0.0
    # an empty mask and a full one
    counts, score, status, _ = mv.verify_pair(mask=np.zeros_like(mask), min_pixels=5, **case)
    assert counts.tolist() == [0, 5, 0, 5] and status == 0 and score == 0.0
    counts, score, status, _ = mv.verify_pair(mask=np.ones_like(mask), min_pixels=5, **case)
    assert counts.tolist() == [5, 0, 12 * 16 - 5, 5] and score == 5.0 / 192.0
    # cx = 0: u0 = -4, cell ix is pixel ix - 4: of the five cells only (4,4) (4,3) (5,4) = pixels (0,5) (0,4) (1,5) are in the image; what
    # leaves the image is ignored on both sides
    case, _ = _hand_case(0.0)
    counts, score, status, model = mv.verify_pair(mask=np.ones_like(mask), min_pixels=3, **case)
    assert counts.tolist() == [3, 0, 189, 5] and status == 0 and score == 3.0 / 192.0
    assert sorted(zip(*np.nonzero(model)[::-1])) == [(0, 4), (0, 5), (1, 5)]
    # the sphere reaches the camera: C.z = 5 <= rho + 1
    counts, score, status, _ = mv.verify_pair(mask=mask, **dict(case, t=np.array([0.0, 0.0, 5.0])))
    assert counts.tolist() == [0, 0, 0, 0] and status == 2 and score == 0.0


@pytest.fixture(scope="module")
def fix():
    return mv.gpu_fixture()


@pytest.fixture(scope="module")
def ref(fix):
    return mv.run_ref_on(fix)


def test_the_fixtures_are_far_from_every_boundary(fix, ref):
    assert ref["min_margin"] > 1e-6, ref["min_margin"]
    big = mv.run_ref_on(mv.gpu_fixture(seed=7, grid=128))   # the second fixture of tests/test_gpu_mask_verify.py
    assert big["min_margin"] > 1e-6, big["min_margin"]
    assert ref["status"].tolist() == [0, 0, 0, 2, 0, 2] == big["status"].tolist()
    c = ref["counts"]
    assert not c[3].any() and not c[5].any() and ref["score"][3] == 0 and ref["score"][5] == 0
    assert np.array_equal(fix["A"][0], np.eye(3)) and not np.allclose(fix["A"][1], np.eye(3))
    area = fix["masks"].reshape(2, -1).sum(1)
    for p in np.nonzero(ref["status"] == 0)[0]:
        assert c[p, 0] + c[p, 2] == area[p // 3] and ref["score"][p] == c[p, 0] / (c[p, 0] + c[p, 1] + c[p, 2])
    # detection 1's planted blob leaves the image: its mask touches the right border
    assert fix["masks"][1][:, -1].any() and not fix["masks"][0][:, -1].any()


def test_the_planted_pose_scores_highest(ref):
    print("planted / shifted / scaled / planted partly outside:", ref["score"][[0, 1, 2, 4]].tolist())
    assert ref["score"][0] > ref["score"][1] and ref["score"][0] > ref["score"][2]


def test_header_and_binding_declare_the_entry():
    from foundpose_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    assert int(re.search(r"#define\s+FP_ABI_VERSION\s+(\d+)", header).group(1)) == 20 == _lib.ABI_VERSION
    m = re.search(r"int fp_pose_verify_mask\(([^;]*)\);", header)
    assert m, "fp_pose_verify_mask is not declared in the header"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    proto = _lib._PROTOS["fp_pose_verify_mask"]
    assert len(args) == len(proto) == 22
    for a, ty in zip(args, proto):
        want = _lib.vp if ("*" in a or a.startswith("fp_stream_t")) else {"int": _lib.i32, "double": _lib.f64}[a.split()[0]]
        assert ty is want, a
    api = open(os.path.join(ROOT, "foundpose_amd", "csrc", "api.cpp")).read()
    assert "int fp_pose_verify_mask(" in api and "mask_verify.hip" in build.SOURCES and "verify_grid.hpp" in build.HEADERS
    assert "fp_pose_verify_mask" in _lib.exported_symbols()


def test_driver_options_are_validated_without_a_gpu():
    from foundpose_amd import infer
    base = infer.load_opts({"infer_opts": dict(version="v", repre_version="r", object_dataset="d")})
    assert base.coarse_select_type == "inliers" and base.mask_verify_grid == 64 and base.mask_verify_max_points == 16384
    assert "mask_verify" in infer.COARSE_SELECT_TYPES and "mask_verify" not in infer.DEPTH_SELECT_TYPES
    for pnp in ("opencv", "kabsch_depth"):
        for final in infer.FINAL_POSE_TYPES + infer.JOINT_POSE_TYPES:
            infer._check_driver_opts(base._replace(coarse_select_type="mask_verify", pnp_type=pnp, final_pose_type=final))
    for good in (8, 16, 128):
        infer._check_driver_opts(base._replace(coarse_select_type="mask_verify", mask_verify_grid=good))
    for bad in (7, 129, 0, -16, 64.0, "64", True):
        with pytest.raises(ValueError, match="mask_verify_grid"):
            infer._check_driver_opts(base._replace(mask_verify_grid=bad))
    for bad in (0, -3, 2.5, "9", True):
        with pytest.raises(ValueError, match="mask_verify_max_points"):
            infer._check_driver_opts(base._replace(mask_verify_max_points=bad))
    # no depth is asked for: the reason a frame without depth is refused with names nothing of this option
    alone = base._replace(coarse_select_type="mask_verify")
    assert infer._depth_reason(alone) == infer._depth_reason(base) == "the final pose type refines against depth"
    assert "mask_verify" not in infer._depth_reason(alone._replace(pnp_type="kabsch_depth"))


def test_argument_checks_that_come_before_any_device_work(monkeypatch):
    from foundpose_amd import pnp_util
    launched = []
    monkeypatch.setattr(pnp_util, "call", lambda *a: launched.append(a[0]))

    class NoBank:
        def verify_points(self, max_points):
            raise AssertionError("the bank is asked only after the arguments are checked")

    B, n = 2, 3
    poses = {"success": torch.ones(B, n, dtype=torch.bool), "R": torch.eye(3, dtype=torch.float64).expand(B, n, 3, 3).contiguous(),
             "t": torch.zeros(B, n, 3, dtype=torch.float64)}
    cams = [(100.0, 100.0, 31.5, 23.5)] * B
    masks = torch.ones(B, 48, 64, dtype=torch.uint8)
    run = lambda **kw: pnp_util.verify_poses_mask(poses, NoBank(), kw.pop("det_obj", [0, 1]), kw.pop("solve", cams), kw.pop("frames", cams),
                                                  kw.pop("masks", masks), **kw)
    for bad in (7, 129, 16.0, True):
        with pytest.raises(ValueError, match="grid"):
            run(grid=bad)
    for bad in (0, -1, 16.0, True):
        with pytest.raises(ValueError, match="min_pixels"):
            run(min_pixels=bad)
    for bad in (masks.bool(), masks.float(), masks.to(torch.int32), masks[0], masks[None], masks.numpy()):
        with pytest.raises(ValueError, match=r"masks must be a uint8 tensor \[B, H, W\]"):
            run(masks=bad)
    for kw in (dict(masks=masks[:1]), dict(det_obj=[0]), dict(solve=cams[:1]), dict(frames=cams * 2)):
        with pytest.raises(ValueError, match="for 2 detections"):
            run(**kw)
    with pytest.raises(ValueError, match="on the device"):   # everything else in order: a host tensor is refused, not copied
        run()
    assert launched == []
