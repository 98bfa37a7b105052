"""The silhouette refinement without a GPU: the restatement tests/mask_refine_ref.py against definitions and scipy,
its Jacobians against central differences, the margins of every GPU fixture of tests/mask_refine_steps.py, the recovery of the four
planted starts on the restatement, the driver options and the binding of include/foundpose_amd_mask_refine.h."""

import os
import re
import types

import numpy as np
import pytest

from tests import lm_ref, lm_steps
from tests import mask_refine_ref as mr
from tests import mask_refine_steps as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _masks():
    rng = np.random.default_rng(11)
    H, W = 37, 131
    single, corner = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    single[20, 77] = 1
    corner[H - 1, 0] = 255
    yy, xx = np.mgrid[:H, :W]
    return {"random": (rng.random((H, W)) < 0.02).astype(np.uint8) * 255, "single": single, "full": np.ones((H, W), np.uint8),
            "checkerboard": ((yy + xx) % 2).astype(np.uint8), "corner": corner}


@pytest.mark.parametrize("name", ["random", "single", "full", "checkerboard", "corner"])
def test_the_restated_transform_is_the_definition_and_scipys(name):
    from scipy import ndimage
    m = _masks()[name]
    d2 = mr.mask_distance(m)
    assert d2.dtype == np.int64 and np.array_equal(d2, mr.mask_distance_brute(m))
    assert np.array_equal(d2, np.rint(ndimage.distance_transform_edt(m == 0) ** 2).astype(np.int64))
    assert (d2[m != 0] == 0).all() and (d2[m == 0] > 0).all() and d2.max() < 5.4e8


def test_an_empty_mask_gives_the_sentinel():
    assert (mr.mask_distance(np.zeros((5, 9), np.uint8)) == 1 << 30).all() and (mr.mask_distance_brute(np.zeros((5, 9), np.uint8)) == 1 << 30).all()


def test_the_contour_rule_on_hand_made_masks():
    border = np.zeros((5, 6), np.uint8)
    border[0:3, 0:3] = 1                      # touches the top and the left border: no contour there
    assert mr.contour_pixels(border).tolist() == [[2, 0], [2, 1], [0, 2], [1, 2], [2, 2]]
    one = np.zeros((4, 4), np.uint8)
    one[2, 1] = 7
    assert mr.contour_pixels(one).tolist() == [[1, 2]]
    hole = np.ones((5, 5), np.uint8)
    hole[2, 2] = 0                            # a full image with a one-pixel hole: the hole's four neighbours
    assert mr.contour_pixels(hole).tolist() == [[2, 1], [1, 2], [3, 2], [2, 3]]
    assert len(mr.contour_pixels(np.ones((3, 3), np.uint8))) == 0 and mr.contour_pixels(np.ones((1, 1), np.uint8)).shape == (0, 2)


def test_the_subsample_indices():
    cap = 16
    assert mr.subsample_indices(cap, cap) == list(range(cap))
    assert mr.subsample_indices(cap + 1, cap) == [(j * 17) // 16 for j in range(16)] == list(range(16))
    got = mr.subsample_indices(3 * cap - 1, cap)
    assert got == [(j * 47) // 16 for j in range(16)] and got[0] == 0 and got[-1] == 44 and len(set(got)) == cap
    assert mr.subsample_indices(3, cap) == [0, 1, 2]


def _twist_pose(R, t, d):
    return lm_ref.update(np.asarray(R, np.float64), np.asarray(t, np.float64), d)


@pytest.mark.parametrize("name", ms.IDS)
def test_both_jacobians_against_central_differences(name):
    fx = ms.fixture(name)
    d = fx.det
    X = np.asarray(d["X"], np.float32).astype(np.float64)
    f = mr.forward_terms(d["R"], d["t"], X, d["cam"], fx.d2, d["delta"])
    b = mr.backward_terms(d["R"], d["t"], X, d["cam"], fx.q, d["delta"])
    assert f["measurable"].sum() >= 6 and (f["r"] > 0).sum() >= 6
    eps = 1e-6
    for k in range(6):
        tw = np.zeros(6)
        tw[k] = eps
        (Rp, tp), (Rm, tm) = _twist_pose(d["R"], d["t"], tw), _twist_pose(d["R"], d["t"], -tw)
        fp, fm = mr.forward_terms(Rp, tp, X, d["cam"], fx.d2, d["delta"]), mr.forward_terms(Rm, tm, X, d["cam"], fx.d2, d["delta"])
        same = f["measurable"] & fp["measurable"] & fm["measurable"] & (np.floor(fp["u"]) == np.floor(fm["u"])) & (np.floor(fp["v"]) == np.floor(fm["v"]))
        assert same.sum() >= f["measurable"].sum() - 2          # a point within 1e-6 of a cell edge is left out, not more
        num = (fp["r"] - fm["r"]) / (2 * eps)
        scale = np.abs(f["J"]).max()
        assert np.abs(num[same] - f["J"][same, k]).max() < 1e-5 * scale
        _, up, vp, _ = mr.project(Rp, tp, X, d["cam"])
        _, um, vm, _ = mr.project(Rm, tm, X, d["cam"])
        j = b["j"]
        assert np.abs((up[j] - um[j]) / (2 * eps) - b["Ju"][:, k]).max() < 1e-5 * np.abs(b["Ju"]).max()
        assert np.abs((vp[j] - vm[j]) / (2 * eps) - b["Jv"][:, k]).max() < 1e-5 * np.abs(b["Jv"]).max()


def test_the_system_is_the_weighted_sum_of_both_terms():
    fx = ms.fixture("n70_k33")
    d = fx.det
    X = np.asarray(d["X"], np.float32).astype(np.float64)
    E, Hm, g, ok = mr.system(d["R"], d["t"], X, d["cam"], fx.d2, fx.q, d["delta"])
    f, b = mr.forward_terms(d["R"], d["t"], X, d["cam"], fx.d2, d["delta"]), mr.backward_terms(d["R"], d["t"], X, d["cam"], fx.q, d["delta"])
    assert E == pytest.approx(0.5 * f["rho"].sum() / 70 + 0.5 * b["rho"].sum() / 33, rel=1e-14) and ok.sum() == f["measurable"].sum()
    Hs = sum(w * np.outer(J, J) for w, J in zip(f["w"], f["J"])) / 70 * 0.5 + sum(w * (np.outer(a, a) + np.outer(c, c)) for w, a, c in zip(b["w"], b["Ju"], b["Jv"])) / 33 * 0.5
    assert np.allclose(Hm, Hs, rtol=1e-12, atol=1e-12 * np.abs(Hs).max()) and np.allclose(Hm, Hm.T)
    far = mr.huber(np.array([3.0, 4.0, 9.0]), 4.0)
    assert far[0].tolist() == [9.0, 16.0, 2 * 4.0 * 9.0 - 16.0] and far[1].tolist() == [1.0, 1.0, 4.0 / 9.0]
    # a pose with every point behind the camera costs +inf
    Eb, _, _, _ = mr.system(d["R"], -np.asarray(d["t"]), X, d["cam"], fx.d2, fx.q, d["delta"])
    assert Eb == np.inf


@pytest.mark.parametrize("name", ms.IDS)
def test_margins_of_the_gpu_fixtures(name):
    """What tests/test_gpu_mask_refine.py compares decision by decision has to be decided clearly by the restatement alone: over the
    pinned prefix (tests/lm_steps.pinned_prefix, margin 1e-6) no accept / reject decision, floor, z > 1, Huber branch or nearest-point
    choice lies within reach of a change of summation order."""
    fx = ms.fixture(name)
    n, ref, spread = ms.prefix(fx)
    K = min(n, lm_steps.K_MAX)
    assert K >= 10, (name, n)
    assert lm_steps.MARGIN[fx.entry] == 1e-6
    assert fx.gaps(fx.det["R"], fx.det["t"]) > lm_steps.BRANCH
    for rec in ref["trace"][:K]:
        assert rec["margin"] > 1e-6 and rec["kind"] in ("acc", "rej")
        assert fx.gaps(*rec["trial"]) > lm_steps.BRANCH
    assert spread[0] < lm_steps.SPREAD_R and spread[1] < lm_steps.SPREAD_T
    assert len(fx.q) == fx.det["K_max"] and ref["status"] == 0 and ref["cost_out"] < ref["cost_in"]


def test_some_fixture_rejects_steps_inside_its_prefix():
    kinds = ""
    for name in ms.IDS:
        n, ref, _ = ms.prefix(ms.fixture(name))
        kinds += lm_ref.decisions(ref["trace"][:min(n, lm_steps.K_MAX)])
    assert "r" in kinds and "ar" in kinds and "ra" in kinds


def test_skips_of_the_restatement():
    fx = ms.fixture("n70_k6")
    d = fx.det
    X = np.asarray(d["X"], np.float32).astype(np.float64)
    for kw in (dict(has_pose=False), dict(K_max=5)):
        out = mr.refine(d["R"], d["t"], X, d["cam"], d["mask"], d["delta"], 10, **{"K_max": 6, **kw})
        assert out["status"] == 2 and np.array_equal(out["R"], d["R"]) and np.array_equal(out["t"], d["t"]) and out["iters_used"] == 0
    out = mr.refine(d["R"], d["t"], X, d["cam"], np.zeros_like(d["mask"]), d["delta"], 10)
    assert out["status"] == 2
    out = mr.refine(d["R"], d["t"], X, d["cam"], d["mask"], d["delta"], 0, 6)
    assert out["status"] == 1 and out["cost_in"] == out["cost_out"] > 0


@pytest.mark.parametrize("start", [s[0] for s in ms.recovery_starts()])
def test_recovery_on_the_restatement(start):
    """The 144 x 192 blob fixture from the four starts: the cost falls, the silhouette IoU of the refined pose exceeds the start's, and the
    lateral error falls for the starts that have one.  The figures are printed (pytest -s) for DESIGN.md; they are no thresholds."""
    r = ms.recovery_run(start)
    lateral = next(s[3] for s in ms.recovery_starts() if s[0] == start)
    print(f"{start}: cost {r['cost_in']:.4f} -> {r['cost_out']:.4f}, IoU {r['iou_in']:.3f} -> {r['iou_out']:.3f}, lateral {r['lat_in']:.2f} -> {r['lat_out']:.2f} mm, "
          f"along the ray {r['along_in']:.2f} -> {r['along_out']:.2f} mm, rotation off {r['rot_out']:.2f} deg, {r['iters_used']} iterations, status {r['status']}")
    assert r["status"] == 0 and r["cost_out"] < r["cost_in"]
    assert r["iou_out"] > r["iou_in"]
    if lateral:
        assert r["lat_out"] < r["lat_in"]


# ---------------------------------------------------------------------------------------------------------------- options
def test_the_driver_options():
    from foundpose_amd import infer
    assert infer.MASK_POSE_TYPES == ("mask", "featuremetric_mask")
    assert set(infer.FINAL_POSE_TYPES) == {"best_coarse", "featuremetric", "depth", "featuremetric_depth"}
    assert not set(infer.MASK_POSE_TYPES) & set(infer.DEPTH_POSE_TYPES)
    base = infer.InferOpts(version="v", repre_version="r", object_dataset="d", object_lids=[1])
    assert (base.mask_refine_iters, base.mask_refine_huber_px, base.mask_refine_max_points, base.mask_refine_max_contour) == (30, 8.0, 4096, 1024)
    for tp in infer.MASK_POSE_TYPES:
        for pnp in infer.pnp_util.PNP_TYPES:
            for sel in infer.COARSE_SELECT_TYPES:
                refine, _ = infer._check_driver_opts(base._replace(final_pose_type=tp, pnp_type=pnp, coarse_select_type=sel))
                assert refine == (tp == "featuremetric_mask")        # the engine keeps the feature map only where section 11 runs first
    with pytest.raises(ValueError, match="Unknown final pose type"):
        infer._check_driver_opts(base._replace(final_pose_type="masks"))
    bad = {"mask_refine_iters": (-1, 1001, 2.0, True, None), "mask_refine_huber_px": (0, -1.0, float("nan"), float("inf"), True, "8"),
           "mask_refine_max_points": (0, -5, 1.5, True), "mask_refine_max_contour": (0, -1, 2.5, False)}
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=key):
                infer._check_driver_opts(base._replace(**{key: v}))
    infer._check_driver_opts(base._replace(mask_refine_iters=0, mask_refine_huber_px=1, mask_refine_max_points=1, mask_refine_max_contour=1))


def test_a_mask_pose_type_needs_no_depth():
    from foundpose_amd import infer
    base = infer.InferOpts(version="v", repre_version="r", object_dataset="d", object_lids=[1])
    frame = {"image": np.zeros((4, 4, 3), np.uint8)}      # no "depth"
    for tp in infer.MASK_POSE_TYPES:
        opts = base._replace(final_pose_type=tp)
        pipe = types.SimpleNamespace(opts=opts, use_depth=opts.final_pose_type in infer.DEPTH_POSE_TYPES, depth_pnp=False, verify=False)
        infer._check_frame_work(pipe, frame)
    pipe = types.SimpleNamespace(opts=base._replace(final_pose_type="depth"), use_depth=True, depth_pnp=False, verify=False)
    with pytest.raises(Exception):
        infer._check_frame_work(pipe, frame)


def test_refine_best_coarse_mask_refuses_before_any_launch():
    import torch
    from foundpose_amd import refine_util
    pose = {"R": torch.zeros(2, 3, 3), "t": torch.zeros(2, 3), "found": torch.ones(2, dtype=torch.bool)}
    for masks in (torch.zeros(2, 4, 4, dtype=torch.uint8), torch.zeros(2, 4, 4), np.zeros((2, 4, 4), np.uint8)):   # not on the device / not uint8 / no tensor
        with pytest.raises(ValueError, match="masks must be a uint8 tensor"):
            refine_util.refine_best_coarse_mask(pose, None, [0, 0], [None] * 2, [None] * 2, masks)
    with pytest.raises(ValueError, match="masks must be a uint8 tensor"):
        refine_util.mask_contours(torch.zeros(4, 4, dtype=torch.uint8), 16)


# ---------------------------------------------------------------------------------------------------------------- binding
def test_the_header_binds_through_the_main_parser():
    from foundpose_amd import _lib
    from foundpose_amd._lib import f64, i32, i64, vp
    main = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    assert "mask_refine" not in main and "fp_mask_distance" not in main
    path = os.path.join(ROOT, "include", "foundpose_amd_mask_refine.h")
    text = open(path).read()
    assert '#include "foundpose_amd.h"' in text and re.search(r"^#if FP_ABI_VERSION != 20\s*\n#error", text, re.M)
    protos, names, version = _lib._parse_header(path, versioned=False)
    assert version is None and set(protos) == {"fp_mask_distance", "fp_mask_refine"}
    assert "foundpose_amd_mask_refine.h" in _lib.FEATURE_HEADERS and _lib._FEATURE_PROTOS["foundpose_amd_mask_refine.h"] == protos
    assert not set(protos) & set(_lib._PROTOS) and not any(set(protos) & set(p) for p in _lib._EXT_PROTOS.values())
    assert not set(protos) & set(_lib.exported_symbols())
    bare = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for fn, count in (("fp_mask_distance", 6), ("fp_mask_refine", 31)):
        params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % fn, bare).group(1)
        assert len(params.split(",")) == count == len(protos[fn])
    assert protos["fp_mask_distance"] == [vp, i32, i32, i32, vp, vp]
    a = protos["fp_mask_refine"]
    assert a[:7] == [vp, i32, i32, vp, i64, vp, vp] and a[13] is i64 and a[15] is f64 and a[16:20] == [i32] * 4 and a[21] is _lib.C.c_size_t and a[22:] == [vp] * 9
    chunks = lambda n: (n + 31) // 32
    assert _lib.mask_refine_scratch_bytes(3, 70, 33) == 512 * 3 + 8 * 32 * 3 * (chunks(70) + chunks(33)) + 8 + 16 * 3 * 70 + ((3 * 70 + 1) // 2) * 8
    macro = re.search(r"#define FP_MASK_REFINE_TILE (\d+)", text)
    assert int(macro.group(1)) == ms.TILE
    if os.path.exists(_lib.LIB_PATH):
        handle = _lib.lib()
        for fn in protos:
            assert list(getattr(handle, fn).argtypes) == protos[fn] and getattr(handle, fn).restype is i32
