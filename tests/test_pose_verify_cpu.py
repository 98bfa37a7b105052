"""coarse_select_type "depth_verify" without a GPU: the numpy restatement (tests/pose_verify_ref.py) on the GPU tests' fixture -- the counts
add up, the fixture is far from every decision boundary, the planted pose scores highest, a pose behind / in front of the surface is
occluded / in free space, the z-buffer hides the far side --, select_best_verified's ranking on hand-made tensors, the bank's point sample,
the C ABI's declaration and the drivers' option checks."""

import os
import re

import numpy as np
import pytest
import torch

from tests import pose_verify_ref as pv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fix():
    return pv.gpu_fixture()


@pytest.fixture(scope="module")
def ref(fix):
    return pv.run_ref_on(fix)


def test_counts_add_up_and_the_fixture_is_far_from_every_boundary(fix, ref):
    c = ref["counts"]
    assert np.array_equal(c[:, 0], c[:, 1:].sum(1))
    assert ref["min_margin"] > 1e-6, ref["min_margin"]
    assert ref["status"].tolist() == [0, 0, 0, 2, 0, 2]
    assert not c[3].any() and not c[5].any() and ref["score"][3] == 0 and ref["score"][5] == 0
    assert c[0, 2] > 0                      # the occluder strip lies over the planted blob
    assert c[4, 4] > 0 and c[4, 5] > 0      # detection 1's planted pose: holes, and points that leave the image
    assert np.array_equal(fix["A"][0], np.eye(3)) and not np.allclose(fix["A"][1], np.eye(3))
    for p in np.nonzero(ref["status"] == 0)[0]:
        assert ref["score"][p] == c[p, 1] / c[p, 0]


def test_the_planted_pose_scores_highest(fix, ref):
    n = fix["n_slots"]
    for p in fix["planted"]:
        det = p // n
        others = [q for q in range(det * n, (det + 1) * n) if q != p]
        assert all(ref["score"][p] > ref["score"][q] for q in others), ref["score"]
    assert ref["score"][0] > 0.5


def test_behind_the_surface_is_occluded_and_in_front_of_it_is_free(fix, ref):
    names = ["n_in", "n_occ", "n_free", "n_hole", "n_out"]
    pushed = ref["counts"][1]
    assert names[int(np.argmax(pushed[1:]))] == "n_occ" and pushed[2] > pushed[0] // 2, pushed
    t = fix["t"].copy()
    t[1] = pv.along_ray(fix["t"][0], -3.0 * fix["tau"][0])
    pulled = pv.run_ref_on(fix, t=t)["counts"][1]
    assert names[int(np.argmax(pulled[1:]))] == "n_free" and pulled[3] > pulled[0] // 2, pulled


def test_the_far_side_is_not_visible(fix, ref):
    """The blob is closed: at least the half of its points that faces away from the camera lies behind another part of it, more than tau
    = 3 mm behind except in a rim.  So n_vis is below 0.6 of the count without the z-buffer (every point in front of the camera)."""
    every = pv.run_ref_on(fix, zbuffer=False)["counts"]
    for p in fix["planted"]:
        assert every[p, 0] in (600, 602)
        assert ref["counts"][p, 0] < 0.6 * every[p, 0], (ref["counts"][p, 0], every[p, 0])


def test_too_few_visible_points_is_status_1(fix, ref):
    out = pv.run_ref_on(fix, min_visible=1000)
    assert out["status"].tolist() == [1, 1, 1, 2, 1, 2] and not out["score"].any()
    assert np.array_equal(out["counts"], ref["counts"])


def _poses(success, quality):
    success, quality = torch.tensor(success), torch.tensor(quality, dtype=torch.float64)
    B, n = success.shape
    R = torch.arange(B * n, dtype=torch.float64).reshape(B, n, 1, 1).expand(B, n, 3, 3).contiguous()
    return {"success": success, "quality": quality, "R": R, "t": R[..., 0].contiguous()}


def test_select_best_verified_ranking():
    from foundpose_amd import pnp_util
    poses = _poses(
        [[True, True, True, True],      # 0: a scored pair beats an unscored one of higher score-less quality
         [True, True, True, True],      # 1: among the scored, the higher score
         [True, True, True, True],      # 2: equal scores: the higher coarse quality
         [True, True, True, True],      # 3: equal scores and qualities: the first slot
         [False, False, False, False],  # 4: no success: not found
         [False, True, True, False],    # 5: the best score belongs to a failed pair: not eligible
         [True, True, True, False]],    # 6: nothing scored: the coarse quality, then the first slot
        [[90.0, 10.0, 50.0, 60.0], [10.0, 20.0, 99.0, 5.0], [10.0, 30.0, 20.0, 99.0], [7.0, 40.0, 40.0, 40.0], [5.0, 6.0, 7.0, 8.0],
         [99.0, 10.0, 20.0, 99.0], [10.0, 30.0, 30.0, 99.0]])
    verify = {"status": torch.tensor([[1, 0, 2, 1], [0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 2, 1, 0]], dtype=torch.int32),
              "score": torch.tensor([[0.0, 0.1, 0.0, 0.0], [0.5, 0.7, 0.0, 0.6], [0.4, 0.6, 0.6, 0.0], [0.2, 0.8, 0.8, 0.8], [0.9, 0.9, 0.9, 0.9],
                                     [0.9, 0.3, 0.4, 0.95], [0.0, 0.0, 0.0, 0.9]], dtype=torch.float64)}
    best = pnp_util.select_best_verified(poses, verify)
    assert best["found"].tolist() == [True, True, True, True, False, True, True]
    found = best["found"]
    assert best["corresp_id"][found].tolist() == [1, 1, 1, 1, 2, 1]
    assert best["quality"].tolist() == [10.0, 20.0, 30.0, 40.0, -1.0, 20.0, 30.0]
    assert best["verify_score"].tolist() == [0.1, 0.7, 0.6, 0.8, 0.0, 0.4, 0.0]
    for b, cid in enumerate(best["corresp_id"].tolist()):
        assert torch.equal(best["R"][b], poses["R"][b, cid]) and torch.equal(best["t"][b], poses["t"][b, cid])
    coarse = pnp_util.select_best_coarse(poses)
    assert set(coarse) | {"verify_score"} == set(best) and coarse["found"].tolist() == best["found"].tolist()
    assert coarse["corresp_id"].tolist()[:4] == [0, 2, 3, 1]   # what the inlier count alone picks


def test_bank_sample_is_every_sth_row(fix):
    from foundpose_amd import bank
    V = torch.from_numpy(np.concatenate(fix["verts"]))
    pts, ranges = bank.sample_verify_points(V, [(0, 600), (600, 1803)], 700)
    assert ranges == [(0, 600), (600, 1202)]
    assert torch.equal(pts[:600], V[:600]) and torch.equal(pts[600:], V[600:1803:2])
    pts3, ranges3 = bank.sample_verify_points(V, [(0, 600), (600, 1803), (1803, 1803)], 400)   # s = 2 and s = 4 (ceil), an empty range
    assert ranges3 == [(0, 300), (300, 601), (601, 601)] and torch.equal(pts3[300:], V[600:1803:4])
    centers, radii = bank.sample_spheres(pts, ranges)
    for (b, e), c, r in zip(ranges, centers, radii):
        P = pts[b:e].numpy().astype(np.float64)
        assert np.array_equal(c, (P.min(0) + P.max(0)) / 2) and r == np.linalg.norm(P - c, axis=1).max() and 40.0 < r < 60.0


def test_header_and_binding_declare_the_entry():
    from foundpose_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    assert int(re.search(r"#define\s+FP_ABI_VERSION\s+(\d+)", header).group(1)) == 20 == _lib.ABI_VERSION
    m = re.search(r"int fp_pose_verify_depth\(([^;]*)\);", header)
    assert m, "fp_pose_verify_depth is not declared in the header"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    proto = _lib._PROTOS["fp_pose_verify_depth"]
    assert len(args) == len(proto) == 24
    for a, ty in zip(args, proto):
        want = _lib.vp if ("*" in a or a.startswith("fp_stream_t")) else {"int": _lib.i32, "double": _lib.f64}[a.split()[0]]
        assert ty is want, a
    api = open(os.path.join(ROOT, "foundpose_amd", "csrc", "api.cpp")).read()
    assert "int fp_pose_verify_depth(" in api and "verify.hip" in build.SOURCES   # (the built library's exports: tests/test_cabi_symbols.py)
    assert "fp_pose_verify_depth" in _lib.exported_symbols()


def test_driver_options_are_validated_without_a_gpu():
    from foundpose_amd import infer
    base = infer.load_opts({"infer_opts": dict(version="v", repre_version="r", object_dataset="d")})
    assert base.coarse_select_type == "inliers" and base.depth_verify_thresh == 0.0 and base.depth_verify_max_points == 16384
    for pnp in ("opencv", "kabsch_depth"):
        for final in infer.FINAL_POSE_TYPES + infer.JOINT_POSE_TYPES:
            infer._check_driver_opts(base._replace(coarse_select_type="depth_verify", pnp_type=pnp, final_pose_type=final))
    with pytest.raises(ValueError, match="Unknown coarse select type 'votes'"):
        infer._check_driver_opts(base._replace(coarse_select_type="votes"))
    with pytest.raises(ValueError, match="Unknown coarse select type 'votes'"):   # before any GPU work: no extractor, no bank
        infer.infer_object(base._replace(coarse_select_type="votes"), 1, None, [], {})
    with pytest.raises(ValueError, match="Unknown coarse select type 'votes'"):
        infer.infer_batched(base._replace(coarse_select_type="votes"), [], {}, {}, "unused")
    for bad in (-1.0, float("nan"), float("inf"), "5", True):
        with pytest.raises(ValueError, match="depth_verify_thresh"):
            infer._check_driver_opts(base._replace(depth_verify_thresh=bad))
    for bad in (0, -3, 2.5, "9", True):
        with pytest.raises(ValueError, match="depth_verify_max_points"):
            infer._check_driver_opts(base._replace(depth_verify_max_points=bad))

    class Repre:
        vertices = torch.tensor([[0.0, 0.0, 0.0], [30.0, 40.0, 0.0], [10.0, 10.0, 0.0]])
    assert infer.depth_verify_tau(base, Repre) == pytest.approx(0.02 * 50.0)
    assert infer.depth_verify_tau(base._replace(depth_verify_thresh=3.0), Repre) == 3.0
    frame = {"scene_id": 1, "im_id": 3, "camera": None}
    with pytest.raises(ValueError, match="scene 1 image 3: coarse_select_type 'depth_verify'"):
        infer._check_frame_depth(frame, infer._depth_reason(base._replace(coarse_select_type="depth_verify")))
    # a depth PnP type keeps its own message; the default options name the final pose type as before
    assert "pnp_type 'kabsch_depth'" in infer._depth_reason(base._replace(coarse_select_type="depth_verify", pnp_type="kabsch_depth"))
    assert infer._depth_reason(base) == "the final pose type refines against depth"
