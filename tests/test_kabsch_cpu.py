"""pnp_type "kabsch_depth" without a GPU: the numpy restatement (tests/kabsch_ref.py) recovers planted poses, its congruence gate never
rejects an all-inlier sample, the GPU tests' fixture is far from every decision boundary, the C ABI declares fp_kabsch_ransac, and the
drivers' options are validated before device work; and the fixtures of tests/test_gpu_kabsch_restatement.py are built and their conditions
asserted from the restatement alone (margins, the sweeps' class counts, the replay's witnesses, best_h, eig_gap, the lift's hand list)."""

import os
import re

import numpy as np
import pytest

from tests import kabsch_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _planted_scene(outlier_frac, holes, rotated, seed):
    """One pair: 30 correspondences in a 96 x 128 frame image, depth noise <= 0.2 tau along the ray, outliers 5.5 .. 12 tau off."""
    rng = np.random.default_rng(seed)
    K, tau = 30, 5.0
    frame_cam = (300.0, 300.0, 63.5, 47.5)
    if rotated:   # a crop camera turned 6 degrees about y and 4 about x, at the frame camera's centre
        A = kr.rot_xyz(np.deg2rad(4.0), np.deg2rad(6.0), 0.0)
        solve_cam = (700.0, 700.0, 60.0, 60.0)
    else:
        A, solve_cam = np.eye(3), frame_cam
    depth = np.zeros((96, 128), np.float32)
    R = kr.rot_xyz(*rng.uniform(-np.pi, np.pi, 3))
    t = np.array([rng.uniform(-10, 10), rng.uniform(-10, 10), rng.uniform(580, 620)])
    c2, c3, good = kr.plant_pair(rng, K, K, outlier_frac, solve_cam, frame_cam, A, depth, tau, R, t, extent=50.0, holes=holes)
    ref = kr.kabsch_ransac_ref(c2[None], c3[None], [K], [solve_cam], [frame_cam], A[None], [0], [tau], depth[None], 1, 200, seed=seed)
    return ref, c3, good, R, t, tau


@pytest.mark.parametrize("outlier_frac, holes, rotated, seed", [(0.0, 0, False, 1), (0.0, 4, True, 2), (0.3, 3, False, 3), (0.3, 0, True, 4),
                                                                (0.6, 0, False, 5), (0.6, 0, True, 6)])
def test_restatement_recovers_planted_poses(outlier_frac, holes, rotated, seed):
    ref, X, good, R, t, tau = _planted_scene(outlier_frac, holes, rotated, seed)
    nv, n_in = int(ref["num_valid"][0]), int(good.sum())
    assert nv == len(good) - holes                           # a hole takes a correspondence out, nothing else does
    assert nv >= 12 and n_in >= 0.4 * nv                     # the condition under which recovery is required: every case here meets it
    assert ref["success"][0]
    inl = ref["inliers"][0]
    assert not (inl & ~good).any()                           # an outlier (>= 5 tau off) is never an inlier of the recovered pose
    assert ref["quality"][0] == inl.sum() >= max(3, n_in // 2)
    # within the noise: both the least-squares pose and the planted one leave <= 0.2 tau (rms) at the inliers, so they differ by <= 0.4 tau there
    Xi = X[inl].astype(np.float64)
    moved = (Xi @ ref["R"][0].T + ref["t"][0]) - (Xi @ R.T + t)
    rms = float(np.sqrt((moved ** 2).sum(1).mean()))
    print(f"outliers {outlier_frac:.0%} holes {holes} rotated {rotated}: {inl.sum()} / {n_in} inliers, rms displacement {rms:.3f} mm "
          f"(bound {0.4 * tau} mm), rotation off by {kr.rotation_angle(ref['R'][0], R):.2e} rad")
    assert rms <= 0.4 * tau


def test_gate_never_rejects_an_all_inlier_sample():
    """Three correspondences that are inliers of ONE pose (each measurement within tau of its transformed model point) pass the gate:
    | |X_i - X_j| - |Y_i - Y_j| | <= |e_i| + |e_j| <= 2 tau by the triangle inequality.  Random poses, scales and errors ON the sphere
    of radius tau (the worst case), including opposed errors along an edge."""
    rng = np.random.default_rng(7)
    for trial in range(2000):
        tau = float(10.0 ** rng.uniform(-1, 2))
        R = kr.rot_xyz(*rng.uniform(-np.pi, np.pi, 3))
        t = rng.uniform(-500, 500, 3)
        X = rng.uniform(-1, 1, (3, 3)) * 10.0 ** rng.uniform(0, 3)
        e = rng.normal(size=(3, 3))
        e *= (tau * (1.0 - 1e-12)) / np.linalg.norm(e, axis=1, keepdims=True)
        if trial % 2:   # errors that stretch the first edge by the full 2 tau
            d = R @ (X[1] - X[0])
            d /= np.linalg.norm(d)
            e[0], e[1] = -d * tau * (1.0 - 1e-12), d * tau * (1.0 - 1e-12)
        Y = X @ R.T + t + e
        assert kr.gate(X, Y, tau), trial


def test_gate_rejects_a_stretched_triangle():
    X = np.array([[0.0, 0, 0], [100, 0, 0], [0, 100, 0]])
    Y = X.copy()
    Y[1, 0] += 2.0 * 5.0 + 1e-6
    assert not kr.gate(X, Y, 5.0) and kr.gate(X, X + 1.0, 5.0)


def test_sampler_is_splitmix64():
    # the first outputs of splitmix64 seeded with 0 (the published test vector): mix64(z) advances by the golden gamma and finalises
    assert kr.mix64(0) == 0xE220A8397B1DCDAF
    assert kr.mix64(kr.GOLDEN) == 0x6E789E6AA1B965F4
    ids = kr.sample3(123, 7, np.array([1, 0, 1, 1, 0, 0, 1], bool))
    assert len(set(ids)) == 3 and all(i in (0, 2, 3, 6) for i in ids)
    assert kr.sample3(123, 5, np.array([1, 1, 0, 0, 0], bool)) is None   # two valid indices cannot give three distinct ones


def test_horn_fit_is_exact_on_clean_points():
    rng = np.random.default_rng(0)
    X = rng.uniform(-50, 50, (9, 3))
    R, t = kr.rot_xyz(0.4, -1.1, 2.5), np.array([5.0, -3.0, 600.0])
    Rh, th = kr.horn(X, X @ R.T + t)
    assert np.abs(Rh - R).max() < 1e-12 and np.abs(th - t).max() < 1e-9 and np.linalg.det(Rh) > 0


@pytest.fixture(scope="module")
def fixture_ref():
    fix = kr.gpu_fixture()
    return fix, kr.run_ref_on(fix)


def test_gpu_fixture_is_far_from_every_decision_boundary(fixture_ref):
    fix, ref = fixture_ref
    print("min_margin of the GPU fixture:", ref["min_margin"])
    assert ref["min_margin"] > 1e-6
    assert ref["success"].tolist() == [True, False, False, True, False, True]
    nv = ref["num_valid"].tolist()
    assert nv[1] == 0 and nv[2] == 5 and nv[4] == 0 and nv[3] == fix["K"] and 6 <= nv[5] < fix["K"]   # holes and pixels outside the image
    assert not np.allclose(fix["A"][1], np.eye(3)) and np.array_equal(fix["A"][0], np.eye(3))
    for p in (0, 3, 5):
        assert not (ref["inliers"][p] & ~fix["good"][p]).any()
        assert kr.rotation_angle(ref["R"][p], fix["poses"][p][0]) < 0.02


def test_header_and_binding_declare_the_entry():
    from foundpose_amd import _lib
    header = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    assert int(re.search(r"#define\s+FP_ABI_VERSION\s+(\d+)", header).group(1)) == 20 == _lib.ABI_VERSION
    m = re.search(r"int fp_kabsch_ransac\(([^;]*)\);", header)
    assert m, "fp_kabsch_ransac is not declared in the header"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    proto = _lib._PROTOS["fp_kabsch_ransac"]
    assert len(args) == len(proto) == 29
    for a, ty in zip(args, proto):
        want = _lib.vp if ("*" in a or a.startswith("fp_stream_t")) else {"int": _lib.i32, "double": _lib.f64, "uint64_t": _lib.u64}[a.split()[0]]
        assert ty is want, a
    assert "fp_kabsch_ransac" in _lib.exported_symbols()
    api = open(os.path.join(ROOT, "foundpose_amd", "csrc", "api.cpp")).read()
    assert "int fp_kabsch_ransac(" in api
    from foundpose_amd import build
    assert "kabsch.hip" in build.SOURCES


def test_driver_options_are_validated_without_a_gpu():
    from foundpose_amd import infer
    base = infer.load_opts({"infer_opts": dict(version="v", repre_version="r", object_dataset="d")})
    assert base.depth_pnp_inlier_thresh == 0.0 and base.pnp_type == "opencv"
    infer._check_driver_opts(base._replace(pnp_type="kabsch_depth", depth_pnp_inlier_thresh=7.5))
    for final in infer.FINAL_POSE_TYPES + infer.JOINT_POSE_TYPES:
        infer._check_driver_opts(base._replace(pnp_type="kabsch_depth", final_pose_type=final))
    with pytest.raises(ValueError, match="Unknown PnP type 'epnp'"):
        infer._check_driver_opts(base._replace(pnp_type="epnp"))
    for bad in (-1.0, float("nan"), float("inf"), "5", True):
        with pytest.raises(ValueError, match="depth_pnp_inlier_thresh"):
            infer._check_driver_opts(base._replace(pnp_type="kabsch_depth", depth_pnp_inlier_thresh=bad))

    class Repre:
        import torch
        vertices = torch.tensor([[0.0, 0.0, 0.0], [30.0, 40.0, 0.0], [10.0, 10.0, 0.0]])
    assert infer.depth_pnp_tau(base, Repre) == pytest.approx(0.05 * 50.0)
    assert infer.depth_pnp_tau(base._replace(depth_pnp_inlier_thresh=3.0), Repre) == 3.0
    frame = {"scene_id": 1, "im_id": 3, "camera": None}
    with pytest.raises(ValueError, match="scene 1 image 3: pnp_type 'kabsch_depth'"):
        infer._check_frame_depth(frame, infer._depth_reason(base._replace(pnp_type="kabsch_depth")))


def test_camera_pairs_and_missing_arguments_are_refused_without_a_gpu():
    from foundpose_amd import crop_util, pnp_util
    Tw = np.eye(4)
    Tw[:3, :3], Tw[:3, 3] = kr.rot_xyz(0.1, 0.2, 0.3), (100.0, 200.0, 300.0)
    frame = crop_util.PinholePlaneCameraModel(640, 480, (600.0, 600.0), (320.0, 240.0), Tw)
    crop = crop_util.construct_crop_camera(crop_util.AlignedBox2f(400.0, 100.0, 520.0, 200.0), frame, (420, 420), 0.2)
    A = pnp_util.solve_to_frame_rotations([frame, crop], [frame, frame])
    assert np.array_equal(A[0], np.eye(3)) and np.abs(A[1] @ A[1].T - np.eye(3)).max() < 1e-12 and abs(A[1][0, 2]) > 0.05
    # the crop camera's axis (0, 0, 1) is the frame camera's ray through the mean of the box's unit corner rays: near the box centre
    # (460, 150), a few pixels towards the image centre
    d = A[1] @ np.array([0.0, 0.0, 1.0])
    assert abs(600.0 * d[0] / d[2] + 320.0 - 460.0) < 3.0 and abs(600.0 * d[1] / d[2] + 240.0 - 150.0) < 3.0
    Ts = crop.T_world_from_eye.copy()
    Ts[:3, 3] += (0.0, 0.0, 1.0)   # a millimetre off the frame camera's centre
    moved = crop_util.PinholePlaneCameraModel(420, 420, crop.f, crop.c, Ts)
    with pytest.raises(ValueError, match="share their centre"):
        pnp_util.solve_to_frame_rotations([moved], [frame])

    class Res:
        pass
    with pytest.raises(ValueError, match="needs frame_cameras, depth, image_index, depth_inlier_thresh_mm"):
        import torch
        r = Res()
        r.template_ids = torch.zeros(1, 1, dtype=torch.int64)
        r.counts = torch.zeros(1, 1, dtype=torch.int32)
        pnp_util.estimate_poses(r, [frame], "kabsch_depth")
    with pytest.raises(ValueError, match="Unsupported PnP type"):
        pnp_util.estimate_poses(Res(), [frame], "epnp")


# ------------------------------------------------------------ the fixtures of tests/test_gpu_kabsch_restatement.py, conditions without a GPU
def test_sampler_allows_one_draw_and_sixty_four_redraws():
    """"at most 64 redraws per index, then the hypothesis fails" -- an index whose first acceptable value is its 65th
    draw succeeds, one draw later it fails.  The chain is mix64's, so the masks are made from it."""
    key, N = 99, 1 << 20     # (the restatement's sampler takes any N; 70 values of 2^20 are distinct here, asserted)
    chain, s = [], key
    for _ in range(70):
        s = kr.mix64(s)
        chain.append(s % N)
    assert len(set(chain)) == 70
    for first_ok, expect in ((65, 65), (64, 64), (66, kr.EXHAUSTED)):
        valid = np.zeros(N, bool)
        valid[chain[first_ok - 1:]] = True
        ids, draws = kr.sample3_draws(key, N, valid)
        assert draws[0] == expect and (ids is None) == (expect == kr.EXHAUSTED)
        if ids is not None:
            assert ids == chain[first_ok - 1:first_ok + 2] and draws[1:] == [1, 1]
    # the limit is per index: the second index has 65 draws of its own
    valid = np.zeros(N, bool)
    valid[[chain[0], chain[65]]] = True
    assert kr.sample3_draws(key, N, valid)[1] == [1, 65, kr.EXHAUSTED]


def test_triangle_margin_exempts_only_an_exact_zero():
    q = np.array([[0.0, 0, 0], [16.0, 0, 0], [48.0, 0, 0], [48.0, 1e-9, 0]])
    m = kr.Margin()
    assert kr.tri_frame(q[0], q[1], q[2], m) is None and m.value == 16.0 / 48.0  # exactly collinear on an axis: no margin but the first edge's own
    assert kr.tri_frame(q[0], q[1], q[3], m) is not None and m.value < 1e-10     # nearly collinear: decided, but within rounding of not
    m = kr.Margin()
    assert kr.tri_frame(q[0], q[0], q[2], m) is None and m.value == np.inf


def test_lift_rounds_half_to_even_and_refuses_what_is_no_measurement():
    cam = (128.0, 128.0, 32.0, 24.0)
    depth = np.zeros((48, 64), np.float32)
    depth[5, [10, 12, 0, 62, 63]] = 600.0
    depth[6, :4] = (0.0, -1.0, np.nan, np.inf)
    below = np.nextafter(np.float32(-0.5), np.float32(-1.0))
    uv = np.array([[10.5, 5.0], [11.5, 5.0], [9.5, 5.0], [12.5, 5.0], [-0.5, 5.0], [below, 5.0], [62.5, 5.0], [63.5, 5.0], [np.nan, 5.0], [10.0, np.nan],
                   [0.0, 6.0], [1.0, 6.0], [2.0, 6.0], [3.0, 6.0]], np.float32)
    m = kr.Margin()
    with np.errstate(invalid="ignore"):
        Y, valid = kr.lift(uv, cam, cam, np.eye(3), depth, m, tie_margin=False)
    # 10.5 and 9.5 -> 10, 11.5 and 12.5 -> 12: only pixels 10 and 12 hold depth, so any other rule loses one of the four
    assert valid.astype(int).tolist() == [1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 0, 1]
    assert m.value > 0.5 and np.isinf(Y[13, 2]) and Y[0, 2] == 600.0
    m = kr.Margin()
    kr.lift(uv[:1], cam, cam, np.eye(3), depth, m)
    assert m.value == 0.0      # with the tie margin a tie is what it is elsewhere: undecided


def test_sweep_fixture_conditions():
    fix = kr.sweep_fixture()
    ref = kr.run_ref_on(fix, False, fix["pair_keys"], cache={})
    print(f"hypothesis sweep: min_margin {ref['min_margin']:.3e}, {kr.sweep_classes(ref)}")
    assert kr.sweep_conditions(fix, ref) == []
    assert len(ref["success"]) == 4096 and fix["iters"] == 1 and (ref["num_valid"] == 44).all()
    # the cache changes nothing: a few pairs alone, without one
    some = [0, 17, 4095]
    sub = dict(fix, coord_2d=fix["coord_2d"][some], coord_3d=fix["coord_3d"][some], counts=fix["counts"][some], n_slots=3)
    alone = kr.run_ref_on(sub, False, fix["pair_keys"][some])
    for k in ("success", "quality", "inliers", "ransac_R", "ransac_t", "cnt", "draws"):
        assert np.array_equal(alone[k], ref[k][some]), k


def test_sparse_fixture_conditions():
    fix = kr.sparse_fixture()
    ref = kr.run_ref_on(fix, False, fix["pair_keys"], cache={})
    print(f"sparse-validity sweep: min_margin {ref['min_margin']:.3e}, {kr.sparse_classes(ref)}")
    assert kr.sparse_conditions(fix, ref) == []
    assert len(ref["success"]) == 2048


def test_stride_fixture_conditions():
    fix = kr.stride_fixture()
    refs = kr.stride_refs(fix)
    facts = kr.stride_facts(fix, refs)
    print(f"stride fixture: min_margin {min(r['min_margin'] for r in refs.values()):.3e}; beyond the budget {facts['beyond']}; ties {facts['ties']}; "
          f"shrinks {facts['shrinks']}")
    assert kr.stride_conditions(fix, refs) == []
    assert fix["counts"].tolist() == [700, 300, 257, 64, 757, 700] and fix["K"] == 700 and fix["iters"] == 1024
    assert np.array_equal(fix["A"][0], np.eye(3)) and not np.allclose(fix["A"][1], np.eye(3))
    assert abs(1.0 - fix["good"][5].sum() / 700.0 - 0.7) < 0.01
    # a restatement on the other confidence, or the other keys, is told apart by the comparison the GPU test uses
    as_dev = kr.as_device
    for (conf, keyed), ref in refs.items():
        assert kr.compare(as_dev(ref), ref)[0] == []
        assert kr.compare(as_dev(ref), refs[(0.5 if conf == 0.99 else 0.99, keyed)])[0]
        assert kr.compare(as_dev(ref), refs[(conf, not keyed)])[0]


def test_late_winner_fixture_conditions():
    fix = kr.late_winner_fixture()
    ref = kr.run_ref_on(fix)
    print(f"late winner: min_margin {ref['min_margin']:.3e}, best_h {ref['best_h'][0]}, {ref['quality'][0]} inliers")
    assert kr.late_conditions(fix, ref) == []
    assert ref["best_h"][0] >= 256 and ref["best_h"][0] % 256 != 0 and fix["iters"] == 1024 and fix["K"] == 64


def test_limit_fixture_conditions():
    fix = kr.limit_fixture()
    ref = kr.run_ref_on(fix)
    print(f"the limits: min_margin {ref['min_margin']:.3e}, best_h {ref['best_h'].tolist()}, quality {ref['quality'].tolist()}")
    assert kr.limit_conditions(fix, ref) == []
    assert fix["K"] == fix["iters"] == 4096 and fix["counts"].tolist() == [4096, 4196]


def test_edge_fixture_conditions_and_hand_list():
    fix = kr.edge_fixture()
    ref = kr.run_ref_on(fix)
    print(f"lift edges: min_margin (ties left out) {ref['min_margin']:.3e}")
    assert kr.edge_conditions(fix, ref) == []
    assert sum(kr.EDGE_VALID) == 21 and sum(kr.EDGE_INLIER) == 20 and len(kr.EDGE_VALID) == fix["K"] == 30
    # every tie point's residual is far inside tau, every refused one would have been an inlier had its pixel been read: the mask tells
    Y, valid = kr.lift(fix["coord_2d"][0], kr.camera_tuple(fix["solve"][0]), kr.camera_tuple(fix["frames"][0]), np.eye(3), fix["depth"][0])
    assert valid.astype(int).tolist() == kr.EDGE_VALID
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt(kr.residuals2(*fix["poses"][0], fix["coord_3d"][0], Y))
    assert d[np.array(kr.EDGE_INLIER, bool)].max() < 1e-3 * fix["tau"][0]


def test_conditioning_fixture_conditions():
    fix = kr.conditioning_fixture()
    ref = kr.run_ref_on(fix)
    print(f"refit conditioning: min_margin {ref['min_margin']:.3e}, eig_gap {ref['eig_gap'].round(3).tolist()}, quality {ref['quality'].tolist()}")
    assert kr.conditioning_conditions(fix, ref) == []
    assert (ref["eig_gap"] > 1e-6).all()
    assert np.array_equal(fix["poses"][2][0], np.eye(3)) and fix["poses"][5][1][2] == 5000.0
    for p in (3, 4):   # half-turns: R = R^T, trace -1 (the quaternion's w is 0)
        R = fix["poses"][p][0]
        assert np.abs(R - R.T).max() < 1e-15 and abs(np.trace(R) + 1.0) < 1e-15
