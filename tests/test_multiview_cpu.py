"""Multi-view pose consensus without a GPU: the restatement's term (tests/multiview_ref.py) against finite
differences and hand-computed Huber values, the planted scenes through the restatement's `fuse`, the host parts of
foundpose_amd/multiview.py (options, camera checks, the greedy rule, the pass-through of a scene without camera poses), the fixtures of
tests/test_gpu_multiview.py (their pinned prefix), the header's declaration."""

import os
import re

import numpy as np
import pytest

from foundpose_amd import infer, multiview, pose_nms
from tests import lm_ref, lm_steps
from tests import multiview_ref as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csv_bytes(tmp_path, name, rows):
    p = tmp_path / name
    pose_nms.write_results_csv(str(p), rows)
    return p.read_bytes()


def _world_t_err(rows, cams, Wt):
    return [float(np.linalg.norm((np.linalg.inv(mv.w2c(cams[str(r["im_id"])])) @ mv.mat(r["R"], r["t"]))[:3, 3] - Wt[:3, 3])) for r in rows]


# ---------------------------------------------------------------------------------------------------------- the term
def test_jacobian_matches_central_differences():
    fx = mv.kernel_fixture("five_views")
    args = fx.args()
    R, t = fx.det["R"], fx.det["t"]
    p = mv.row_terms(R, t, *args)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        ep = mv.row_terms(*lm_ref.update(R, t, d), *args)["e"]
        em = mv.row_terms(*lm_ref.update(R, t, -d), *args)["e"]
        num = (ep - em) / (2 * h)
        scale = max(np.abs(p["Jx"][:, k]).max(), np.abs(p["Jy"][:, k]).max())
        assert np.abs(num[:, 0] - p["Jx"][:, k]).max() < 1e-6 * scale and np.abs(num[:, 1] - p["Jy"][:, k]).max() < 1e-6 * scale, k


def test_huber_on_both_sides_of_delta_and_the_z_rule():
    cam = np.array([[600.0, 600.0, 160.0, 120.0]])
    T = np.array([[1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]])
    Y = np.array([[0.0, 0.0, 600.0]] * 4 + [[0.0, 0.0, 1.0], [0.0, 0.0, 1.0 + 1e-9], [0.0, 0.0, -5.0]])
    uv = np.array([[160.0 + 6.0, 120.0 + 8.0], [160.0 + 18.0, 120.0 + 24.0], [160.0 + 10.0, 120.0], [160.0, 120.0 - 10.0 - 1e-9],
                   [160.0, 120.0], [160.0, 120.0], [160.0, 120.0]])
    p = mv.row_terms(np.eye(3), np.zeros(3), Y, uv, np.zeros(7, int), cam, T, 10.0)
    assert p["inlier"].tolist() == [True, False, True, False, False, True, False]           # |e| = 10, 30, 10 (the bound is inclusive), 10 + 1e-9
    assert p["measurable"].tolist() == [True] * 4 + [False, True, False]                       # z = 1 is not measurable, z = 1 + 1e-9 is
    np.testing.assert_allclose(p["rho"][:3], [100.0, 2 * 10.0 * 30.0 - 100.0, 100.0], rtol=1e-12)
    np.testing.assert_allclose(p["w"][:3], [1.0, 1.0 / 3.0, 1.0], rtol=1e-12)
    assert p["rho"][4] == 100.0 and p["rho"][6] == 100.0 and not p["Jx"][[4, 6]].any() and not p["Jy"][[4, 6]].any() and p["w"][4] == 0.0
    E, H, g, inl = mv.system(np.eye(3), np.zeros(3), Y, uv, np.zeros(7, int), cam, T, 10.0)
    assert inl.sum() == 3 and np.isclose(E, p["rho"].sum() / 7)
    # rows that are not measurable add nothing to the system
    E2, H2, g2, _ = mv.system(np.eye(3), np.zeros(3), Y[[0, 1, 2, 3, 5]], uv[[0, 1, 2, 3, 5]], np.zeros(5, int), cam, T, 10.0)
    np.testing.assert_allclose(H, H2, rtol=1e-14)
    np.testing.assert_allclose(g, g2, rtol=1e-14)


# ---------------------------------------------------------------------------------------------------------- the planted scenes
@pytest.mark.parametrize("seed", range(5))
def test_planted_ring_fused_translation_beats_half_the_best_single_view(seed):
    rows, sc, models, Wt = mv.scene_ring(seed)
    out, rep = mv.fuse(rows, sc, models)
    single, fused = _world_t_err(rows, sc[1], Wt), _world_t_err(out, sc[1], Wt)
    print(f"seed {seed}: single views {min(single):.1f} .. {max(single):.1f} mm, fused {max(fused):.2f} mm")
    assert len(rep["clusters"]) == 1 and rep["clusters"][0]["status"] == 0 and all(r["fused"] for r in rep["rows"])
    assert max(fused) < 0.5 * min(single)
    assert [r["score"] for r in out] == [r["score"] for r in rows] and len(out) == len(rows)


def test_a_view_a_quarter_turn_off_stays_a_singleton_and_keeps_its_bytes(tmp_path):
    """match_thresh 0.5: a quarter turn about the centroid moves no point further than sqrt(2) x its distance from the axis, which for
    this point cloud is below one diameter -- at the default 1.0 the view joins and the Huber weight has to deal with it."""
    rows, sc, models, Wt = mv.SCENES["outlier"]()
    out, rep = mv.fuse(rows, sc, models, **mv.SCENE_OPTS["outlier"])
    off = next(i for i, r in enumerate(rows) if r["im_id"] == 2)
    assert len(rep["clusters"]) == 2 and rep["rows"][off]["views"] == 1 and not rep["rows"][off]["fused"] and rep["rows"][off]["reason"] == "singleton"
    assert out[off]["R"] is rows[off]["R"] and out[off]["t"] is rows[off]["t"]
    assert _csv_bytes(tmp_path, "a.csv", [out[off]]) == _csv_bytes(tmp_path, "b.csv", [rows[off]])
    assert sum(r["fused"] for r in rep["rows"]) == 5
    d1, _ = mv.sym_distance(mv.lift(rows[off], sc[1]["2"]), mv.lift(rows[0], sc[1]["0"]), models[1].syms, mv.sample(models[1].pts, 64))
    assert 0.5 * models[1].diameter < d1 < models[1].diameter       # what the docstring says


def test_two_instances_seen_together_give_two_clusters():
    rows, sc, models, (Wa, Wb) = mv.SCENES["two_instances"]()
    out, rep = mv.fuse(rows, sc, models)
    assert len(rep["clusters"]) == 2 and all(len(c["members"]) == 6 and c["status"] == 0 for c in rep["clusters"])
    for c in rep["clusters"]:
        assert len({rows[m]["im_id"] for m in c["members"]}) == 6      # one candidate per image
        W = mv.mat(c["R"], c["t"])
        assert min(np.linalg.norm(W[:3, 3] - Wa[:3, 3]), np.linalg.norm(W[:3, 3] - Wb[:3, 3])) < 5.0


def test_four_fold_symmetry_gives_one_cluster_and_each_pose_stays_near_its_estimate():
    rows, sc, models, Wt = mv.SCENES["fourfold"]()
    out, rep = mv.fuse(rows, sc, models)
    assert len(rep["clusters"]) == 1 and len(rep["clusters"][0]["members"]) == 6 and rep["clusters"][0]["status"] == 0
    assert len({r["sym"] for r in rep["rows"]}) > 2                     # the views really are turned differently
    for a, b in zip(out, rows):
        assert mv.rotation_deg(a["R"], b["R"]) < 45.0


def test_a_scene_lacking_a_camera_pose_passes_through_byte_for_byte(tmp_path):
    rows, sc, models, _ = mv.SCENES["missing_pose"]()
    out, rep = mv.fuse(rows, sc, models)
    assert list(rep["unfused_scenes"]) == [2] and "image 3" in rep["unfused_scenes"][2]
    second = [i for i, r in enumerate(rows) if r["scene_id"] == 2]
    assert _csv_bytes(tmp_path, "a.csv", [out[i] for i in second]) == _csv_bytes(tmp_path, "b.csv", [rows[i] for i in second])
    assert all(rep["rows"][i]["fused"] == (rows[i]["scene_id"] == 1) for i in range(len(rows)))
    # the product on the unfused scene alone: no device work is reached
    only = [rows[i] for i in second]
    out2, rep2 = multiview.fuse_results(only, sc, models)
    assert rep2["unfused_scenes"] == [{"scene_id": 2, "reason": "image 3 has no cam_K / cam_R_w2c / cam_t_w2c"}] and not rep2["clusters"]
    assert all(a["R"] is b["R"] and a["t"] is b["t"] for a, b in zip(out2, only)) and all("scene not fused" in r["reason"] for r in rep2["rows"])
    assert _csv_bytes(tmp_path, "c.csv", out2) == _csv_bytes(tmp_path, "d.csv", only)


# ---------------------------------------------------------------------------------------------------------- host parts of the product
def test_greedy_rule_and_sample_equal_the_restatements():
    for name in ("outlier", "two_instances", "fourfold"):
        rows, sc, models, _ = mv.SCENES[name]()
        X = mv.sample(models[1].pts, 64)
        assert np.array_equal(multiview.model_sample(models[1].pts, 64), X)
        W = {i: mv.lift(r, sc[1][str(r["im_id"])]) for i, r in enumerate(rows)}
        image, score = {i: r["im_id"] for i, r in enumerate(rows)}, {i: r["score"] for i, r in enumerate(rows)}
        bar = mv.SCENE_OPTS.get(name, {}).get("match_thresh", 1.0) * models[1].diameter
        dist = {(i, j): mv.sym_distance(W[i], W[j], models[1].syms, X) for i in W for j in W if i != j}
        assert multiview.greedy_clusters(list(W), image, score, dist, bar) == mv.greedy_clusters(list(W), W, image, score, models[1].syms, X, bar)
    V = np.arange(300 * 3, dtype=np.float64).reshape(300, 3)
    assert np.array_equal(multiview.model_sample(V, 64), V[::5]) and np.array_equal(mv.sample(V, 64), V[::5])


def test_bad_camera_poses_are_refused_by_name():
    e = mv.ring_cameras()["0"]
    T, cam = multiview.camera_pose(e, 1, 0)
    assert np.allclose(T, mv.w2c(e)) and cam.tolist() == [600.0, 600.0, 160.0, 120.0]
    bad = dict(e, cam_R_w2c=(1.01 * np.asarray(e["cam_R_w2c"])).tolist())
    with pytest.raises(ValueError, match="scene 7 image 4: cam_R_w2c"):
        multiview.camera_pose(bad, 7, 4)
    with pytest.raises(ValueError, match="scene 7 image 4: cam_R_w2c"):
        multiview.camera_pose(dict(e, cam_R_w2c=[float("nan")] * 9), 7, 4)
    with pytest.raises(ValueError, match="scene 7 image 4: cam_R_w2c"):
        multiview.camera_pose(dict(e, cam_R_w2c=(np.asarray(e["cam_R_w2c"]).reshape(3, 3) * [[1], [1], [-1]]).reshape(9).tolist()), 7, 4)   # a reflection
    with pytest.raises(ValueError, match="scene 7 image 4: cam_t_w2c"):
        multiview.camera_pose(dict(e, cam_t_w2c=[0.0, float("inf"), 0.0]), 7, 4)
    rows, sc, models, _ = mv.scene_ring(0)
    sc = {1: dict(sc[1], **{"2": bad})}
    with pytest.raises(ValueError, match="scene 1 image 2: cam_R_w2c"):
        multiview.fuse_results(rows, sc, models)


@pytest.mark.parametrize("bad", [dict(match_thresh=0.0), dict(match_thresh=float("nan")), dict(match_thresh=True), dict(huber_px=-1.0),
                                 dict(huber_px=float("inf")), dict(points=0), dict(points=2.5), dict(points=5000), dict(min_views=1),
                                 dict(min_views=True), dict(iters=-1), dict(iters=1001), dict(iters=2.0)])
def test_options_are_validated(bad):
    multiview.check_opts(multiview.FuseOpts())
    with pytest.raises(ValueError, match=next(iter(bad))):
        multiview.check_opts(multiview.FuseOpts()._replace(**bad))
    with pytest.raises(ValueError, match=next(iter(bad))):
        multiview.fuse_results([], {}, {}, **bad)
    opts = infer.load_opts({"version": "v", "repre_version": "v", "object_dataset": "d"})
    infer._check_driver_opts(opts)
    with pytest.raises(ValueError, match="scene_fuse_" + next(iter(bad))):
        infer._check_driver_opts(opts._replace(**{"scene_fuse_" + k: v for k, v in bad.items()}))


def test_driver_option_defaults_and_names():
    opts = infer.load_opts({"version": "v", "repre_version": "v", "object_dataset": "d"})
    assert opts.scene_select_type == "none" and infer.SCENE_SELECT_TYPES == ("none", "multiview")
    assert infer._scene_fuse_opts(opts) == multiview.FuseOpts() == multiview.FuseOpts(1.0, 10.0, 64, 2, 20)
    assert mv.DEFAULTS == multiview.FuseOpts()._asdict()
    with pytest.raises(ValueError, match="scene select type"):
        infer._check_driver_opts(opts._replace(scene_select_type="fuse"))
    infer._check_driver_opts(opts._replace(scene_select_type="multiview", frame_select_type="pose_nms"))


def test_a_missing_models_info_raises_and_names_the_file(tmp_path):
    with pytest.raises(FileNotFoundError, match="models_info.json"):
        multiview.load_models(str(tmp_path), [1])


def test_header_declares_the_entry_and_the_abi_version_stays():
    """The entry is declared in a header of its own beside the main one (whose list of entry points tests/test_cabi_symbols.py pins),
    the binding derives from that header with the main header's parser, and the main header and its version are as they were."""
    import ctypes as C
    from foundpose_amd import _lib
    from foundpose_amd._lib import f64, i32, i64, vp
    main = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    assert re.search(r"^#define\s+FP_ABI_VERSION\s+20\s*$", main, re.M) and _lib.ABI_VERSION == 20 and "multiview" not in main
    assert _lib.EXTENSION_HEADERS == ("foundpose_amd_multiview.h",) and "fp_multiview_refine" not in _lib._PROTOS
    text = open(os.path.join(ROOT, "include", "foundpose_amd_multiview.h")).read()
    assert '#include "foundpose_amd.h"' in text and re.search(r"^#if FP_ABI_VERSION != 20\s*\n#error", text, re.M)
    assert re.search(r"Added without a change of FP_ABI_VERSION[^;]*?int fp_multiview_refine\(", text, re.S)
    protos = _lib._EXT_PROTOS["foundpose_amd_multiview.h"]
    assert list(protos) == ["fp_multiview_refine"]
    params = re.search(r"\bfp_multiview_refine\s*\(([^()]*)\)\s*;", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)).group(1)
    args = protos["fp_multiview_refine"]
    assert len(args) == params.count(",") + 1 == 27
    assert args == [vp, vp, vp, i64, vp, vp, i32, vp, vp, vp, vp, vp, f64, i32, i32, i32, vp, C.c_size_t] + [vp] * 9
    assert _lib.multiview_scratch_bytes(7, 70) == _lib.depth_refine_scratch_bytes(7, 70)
    if os.path.exists(_lib.LIB_PATH):   # the library exports what the header declares, bound with these types
        import torch  # noqa: F401  (loads the HIP runtime the library links against)
        assert _lib.lib().fp_multiview_refine.argtypes == args


# ---------------------------------------------------------------------------------------------------------- the GPU test's fixtures
@pytest.mark.parametrize("name", list(mv.KERNEL_SPECS))
def test_kernel_fixtures_decide_on_a_margin(name):
    """What tests/test_gpu_multiview.py relies on: K iterations inside the pinned prefix (every decision on a margin above
    lm_steps.MARGIN["depth"], the same decisions with the rows reversed, no per-row branch within 1e-9 of flipping), rows on both sides of
    delta, and for "behind" a row behind its camera."""
    fx = mv.kernel_fixture(name)
    n, a, spread = lm_steps.pinned_prefix(fx, 40)
    print(name, "prefix", n, lm_ref.decisions(a["trace"]), "margins", [f"{r['margin']:.1e}" for r in a["trace"][:fx.K]])
    assert n >= fx.K and all(r["margin"] >= lm_steps.MARGIN["depth"] for r in a["trace"][:fx.K])
    assert fx.gaps(fx.det["R"], fx.det["t"]) >= lm_steps.BRANCH
    p = mv.row_terms(fx.det["R"], fx.det["t"], *fx.args())
    assert len(fx.det["Y"]) == lm_steps.NPTS == mv.NROWS
    assert (p["measurable"] & ~p["inlier"]).sum() >= 3 and p["inlier"].sum() >= 6
    assert ((~p["measurable"]).sum() >= 1) == (name == "behind")
    if name == "behind":
        assert "r" in lm_ref.decisions(a["trace"][:fx.K])          # steps are rejected inside the sweep
