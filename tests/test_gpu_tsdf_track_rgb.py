"""GPU: frame-to-model tracking on shape and colour (csrc/tsdf_track.hip, fp_tsdf_track_rgb, ops.tsdf_track with colors; DESIGN.md section
31) against the numpy restatement tests/tsdf_track_rgb_ref.py.  The volume is tsdf_ref.integrate_fixture()'s five coloured frames fused
by ops.tsdf_integrate (37 x 29 x 23 voxels, tau = 10 mm); the restatement reads the planes the GPU wrote, so both sides start from the
same taps.  Points and colours are lifted from frame 0; tests/test_tsdf_track_rgb_cpu.py shows that no point of the fixture sits where
a last bit could decide a branch."""
import ctypes

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops
from tests import tsdf_track_ref as tr
from tests import tsdf_track_rgb_ref as rr

pytestmark = pytest.mark.gpu
MC, MD, W, CMAX = tr.TRACK_MIN_COUNT, tr.TRACK_MAX_DIST, rr.RGB_WEIGHT, rr.RGB_MAX


@pytest.fixture(scope="module")
def scene():
    fx = rr.track_fixture_rgb()
    f = fx["fx"]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    vol = ops.tsdf_new_volume(f["origin"], f["h"], f["dims"])
    ops.tsdf_integrate(vol, cuda(f["depth"]), cuda(f["mask"]), cuda(f["rgb"]), f["cams"], f["poses"], f["tau"])
    host = dict(vol, **{k: vol[k].cpu().numpy() for k in ops.TSDF_PLANES})
    return dict(vol=vol, host=host, tau=f["tau"], fx=fx)


def _run(scene, problems, iters=20, normal_eq=False, colour=True):
    """problems: list of dict(X, C, R, t, md=MD, has_pose=True) -> ops.tsdf_track's dict (cpu numpy); colour False: the geometric call."""
    X = np.concatenate([p["X"] for p in problems]).astype(np.float32)
    C = np.concatenate([p["C"] for p in problems]).astype(np.float32)
    n = np.array([len(p["X"]) for p in problems])
    rb = np.concatenate([[0], np.cumsum(n)[:-1]])
    cuda = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()   # noqa: E731
    kw = dict(colors=cuda(C), color_weight=W, color_max=CMAX) if colour else {}
    out = ops.tsdf_track(scene["vol"], cuda(X), cuda(rb, torch.int32), cuda(rb + n, torch.int32), cuda(np.stack([p["R"] for p in problems]), torch.float64),
                         cuda(np.stack([p["t"] for p in problems]), torch.float64), [p.get("md", MD) for p in problems], MC, scene["tau"], iters,
                         has_pose=cuda(np.array([p.get("has_pose", True) for p in problems])), want_normal_eq=normal_eq, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _x64(p):
    return p["X"].astype(np.float32).astype(np.float64)


def _ref(scene, p, iters=20):
    return rr.track(scene["host"], p["R"], p["t"], _x64(p), p["C"], scene["tau"], MC, p.get("md", MD), W, CMAX, iters, p.get("has_pose", True))


def _neq(scene, p):
    return rr.normal_equations(scene["host"], p["R"], p["t"], _x64(p), p["C"], scene["tau"], MC, MD, W, CMAX)


def _main(scene):
    fx = scene["fx"]
    return dict(X=fx["X"], C=fx["colors"], R=fx["R"], t=fx["t"])


def _close(got, b, ref):
    return np.radians(tr.rot_angle_deg(got["R"][b], ref["R"])), float(np.linalg.norm(got["t"][b] - ref["t"]))


def _blocks(got, want, tag):
    for lo, hi in ((0, 21), (21, 27), (27, 28)):
        assert np.abs(got[lo:hi] - want[lo:hi]).max() <= 1e-9 * np.abs(want[lo:hi]).max(), (tag, lo)


def test_at_the_input_pose(scene):
    """Both sides compute in fp64 from the same fp32 taps and differ in summation order and contraction only: section 30's bars."""
    p = _main(scene)
    out = _run(scene, [p], iters=0, normal_eq=True)
    want = _neq(scene, p)
    q = rr.point_terms(scene["host"], p["R"], p["t"], _x64(p), p["C"], scene["tau"], MC, MD, W, CMAX)
    inl = int(q["inlier"].sum())
    got = out["normal_eq"][0]
    print(f"{len(p['X'])} points, {inl} geometric inliers, channel inliers {q['channel'].sum(0).tolist()}: max |dH| {np.abs(got[:21] - want[:21]).max():.3e} of "
          f"{np.abs(want[:21]).max():.3e}, |dg| {np.abs(got[21:27] - want[21:27]).max():.3e} of {np.abs(want[21:27]).max():.3e}, cost {got[27]!r} vs {want[27]!r}")
    assert out["num_points"][0] == inl and 6 <= inl < len(p["X"]) and 0 < q["channel"].sum() < 3 * inl
    _blocks(got, want, "main")
    assert abs(out["cost_in"][0] - want[27]) <= 1e-9 * want[27]
    assert out["cost_in"][0] == out["cost_out"][0] == got[27] and out["iters_used"][0] == 0 and out["status"][0] == 1
    assert np.array_equal(out["R"][0], p["R"]) and np.array_equal(out["t"][0], p["t"])
    geo = _run(scene, [p], iters=0, normal_eq=True, colour=False)               # the joint system is not the geometric one
    assert geo["num_points"][0] == inl and got[27] > geo["normal_eq"][0][27] and np.abs(got[:21] - geo["normal_eq"][0][:21]).max() > 0


def test_after_twenty_iterations(scene):
    p = _main(scene)
    out, ref = _run(scene, [p], iters=20), _ref(scene, p, 20)
    rot, dt = _close(out, 0, ref)
    print(f"cost {out['cost_in'][0]:.6f} -> {out['cost_out'][0]:.6f} in {out['iters_used'][0]} iterations (restatement {ref['cost_out']:.6f} in "
          f"{ref['iters_used']}); pose differs by {rot:.3e} rad, {dt:.3e} mm")
    assert out["status"][0] == 0 and out["cost_out"][0] < out["cost_in"][0]
    assert rot < 1e-6 and dt < 1e-3


def test_sizes_that_stride_the_chunk_fold(scene):
    fx = scene["fx"]
    sizes = (6, 31, 32, 33, 65, 1000)
    probs = []
    for n in sizes:
        P, c = rr.sized_points_rgb(n)
        probs.append(dict(X=P, C=c, R=fx["R"], t=fx["t"]))
    out = _run(scene, probs, iters=20, normal_eq=True)
    for b, (n, p) in enumerate(zip(sizes, probs)):
        ref = _ref(scene, p, 20)
        rot, dt = _close(out, b, ref)
        print(f"{n} points, {out['num_points'][b]} inliers: cost {out['cost_in'][b]:.6f} -> {out['cost_out'][b]:.6f}, status {out['status'][b]}, "
              f"{out['iters_used'][b]} iterations; pose differs by {rot:.3e} rad, {dt:.3e} mm")
        assert out["num_points"][b] == ref["num_points"] >= 6 and out["status"][b] == ref["status"]
        _blocks(out["normal_eq"][b], _neq(scene, p), n)
        assert out["cost_out"][b] <= out["cost_in"][b] and rot < 1e-6 and dt < 1e-3


def test_batch_invariance_and_degenerate_problems(scene):
    fx = scene["fx"]
    p = _main(scene)
    Xu, cu = rr.uncoloured_points()
    P65, c65 = rr.sized_points_rgb(65)
    grey = dict(X=Xu, C=cu, R=fx["R"], t=fx["t"])                               # every point a geometric inlier, none colour-measurable
    probs = [dict(p, has_pose=False), grey, p, dict(p, md=float("nan")), dict(X=P65, C=c65, R=fx["R"], t=fx["t"])]
    batch, again = _run(scene, probs, normal_eq=True), _run(scene, probs, normal_eq=True)
    assert batch["status"].tolist() == [2, 0, 0, 2, 0] and batch["num_points"].tolist()[:2] == [0, len(Xu)]
    assert batch["iters_used"][2] > 2 and np.abs(batch["normal_eq"][2]).max() > 0
    for b, q in enumerate(probs):
        alone = _run(scene, [q], normal_eq=True)
        for key in batch:
            assert batch[key][b].tobytes() == alone[key][0].tobytes() == again[key][b].tobytes(), (b, key)
        if b in (0, 3):
            assert np.array_equal(batch["R"][b], q["R"]) and np.array_equal(batch["t"][b], q["t"]) and batch["iters_used"][b] == 0
    assert np.isnan(batch["cost_in"][3])                                       # max_dist^2 per point: a NaN, and no inlier
    # geometry still refines the problem colour has nothing to say about: its H and g are the geometric call's bit for bit (the same
    # source expressions, nothing added), its cost that plus 3 (weight color_max)^2 per point, its pose the restatement's
    geo = _run(scene, [grey], iters=0, normal_eq=True, colour=False)
    assert batch["normal_eq"][1][:27].tobytes() == geo["normal_eq"][0][:27].tobytes()
    assert abs(batch["cost_in"][1] - (geo["cost_in"][0] + 3.0 * (W * CMAX) ** 2)) <= 1e-9 * batch["cost_in"][1]
    rot, dt = _close(batch, 1, _ref(scene, grey))
    print(f"colour-unmeasurable problem: cost {batch['cost_in'][1]:.6f} -> {batch['cost_out'][1]:.6f} in {batch['iters_used'][1]} iterations; pose differs by "
          f"{rot:.3e} rad, {dt:.3e} mm")
    assert batch["cost_out"][1] < batch["cost_in"][1] and rot < 1e-6 and dt < 1e-3


def _raw(scene, **over):
    """fp_tsdf_track_rgb through ctypes with one valid problem of 40 points, `over` replacing arguments -> (rc, message, outputs dict)."""
    vol, fx = scene["vol"], scene["fx"]
    dev = "cuda"
    X, C = torch.from_numpy(fx["X"][:40].copy()).to(dev), torch.from_numpy(fx["colors"][:40].copy()).to(dev)
    a = dict(sdf_sum=_lib.ptr(vol["sdf_sum"]), sdf_cnt=_lib.ptr(vol["sdf_cnt"]), rgb_sum=_lib.ptr(vol["rgb_sum"]), rgb_cnt=_lib.ptr(vol["rgb_cnt"]),
             dims=vol["dims"], min_count=MC, tau=scene["tau"], points=_lib.ptr(X), colors=_lib.ptr(C), num_rows=40, rb=[0], re=[40], weight=W, cmax=CMAX,
             num_det=1, max_points=64, iters=3, scratch_bytes=None)
    a.update(over)
    B = a["num_det"]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731
    rb, re = i32(a["rb"]), i32(a["re"])
    R = torch.from_numpy(np.tile(fx["R"].reshape(1, 9), (B, 1))).to(dev)
    t = torch.from_numpy(np.tile(fx["t"].reshape(1, 3), (B, 1))).to(dev)
    hp, md = torch.ones(B, dtype=torch.int32, device=dev), torch.full((B,), MD, dtype=torch.float64, device=dev)
    outs = {"R": torch.full((B, 9), -7.0, dtype=torch.float64, device=dev), "t": torch.full((B, 3), -7.0, dtype=torch.float64, device=dev),
            "cost_in": torch.full((B,), -7.0, dtype=torch.float64, device=dev), "cost_out": torch.full((B,), -7.0, dtype=torch.float64, device=dev),
            "num_points": torch.full((B,), -7, dtype=torch.int32, device=dev), "iters_used": torch.full((B,), -7, dtype=torch.int32, device=dev),
            "status": torch.full((B,), -7, dtype=torch.int32, device=dev), "normal_eq": torch.full((B, 28), -7.0, dtype=torch.float64, device=dev)}
    need = _lib.tsdf_track_scratch_bytes(B, max(1, a["max_points"]))
    scratch = torch.zeros(need, dtype=torch.uint8, device=dev)
    box = np.array(list(vol["origin"]) + [vol["voxel_mm"]], np.float64)
    ptrs = {k: _lib.ptr(v) for k, v in outs.items()}
    ptrs.update(a.get("null_out", {}))
    rc = _lib.lib().fp_tsdf_track_rgb(a["sdf_sum"], a["sdf_cnt"], a["rgb_sum"], a["rgb_cnt"], box.ctypes.data_as(_lib.vp), *a["dims"], a["min_count"], a["tau"],
                                      a["points"], a["colors"], a["num_rows"], _lib.ptr(rb), _lib.ptr(re), _lib.ptr(R), _lib.ptr(t), _lib.ptr(hp), _lib.ptr(md),
                                      a["weight"], a["cmax"], B, a["max_points"], a["iters"], _lib.ptr(scratch),
                                      need if a["scratch_bytes"] is None else a["scratch_bytes"], *[ptrs[k] for k in outs], _lib.stream())
    torch.cuda.synchronize()
    return rc, _lib.lib().fp_last_error().decode(), {k: v.cpu().numpy() for k, v in outs.items()}


def test_refusals_write_nothing(scene):
    rc, _, outs = _raw(scene)
    assert rc == 0 and outs["status"][0] in (0, 1) and outs["num_points"][0] > 6         # the arguments below are this call's, one of them changed
    need = _lib.tsdf_track_scratch_bytes(1, 64)
    null = ctypes.c_void_p(0)
    cases = [(dict(colors=null), "null pointer"), (dict(rgb_cnt=null), "null pointer"), (dict(rgb_sum=null), "null pointer"),
             (dict(weight=0.0), "color_weight"), (dict(weight=-30.0), "color_weight"), (dict(weight=float("nan")), "color_weight"),
             (dict(weight=float("inf")), "color_weight"), (dict(cmax=0.0), "color_max"), (dict(cmax=float("nan")), "color_max"),
             (dict(re=[41]), "problem 0"), (dict(null_out={"status": null}), "null pointer"), (dict(iters=1001), "iters"),
             (dict(min_count=0), "min_count"), (dict(tau=float("nan")), "truncation"), (dict(scratch_bytes=need - 1), "scratch")]
    for over, word in cases:
        rc, msg, outs = _raw(scene, **over)
        assert rc == 1 and "fp_tsdf_track_rgb" in msg and word in msg, (over, rc, msg)
        for key, v in outs.items():
            assert np.all(v == -7), (over, key)
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device="cuda")           # noqa: E731
    good = dict(colors=z(10, 3, dt=torch.float32), color_weight=W, color_max=CMAX)
    for bad in (dict(colors=z(9, 3, dt=torch.float32)), dict(colors=z(10, 3)), dict(colors=torch.zeros(10, 3)), dict(color_weight=0.0),
                dict(color_weight=float("nan")), dict(color_max=0.0), dict(color_weight=True)):
        with pytest.raises(ValueError, match="color"):
            ops.tsdf_track(scene["vol"], z(10, 3, dt=torch.float32), z(1, dt=torch.int32), torch.full((1,), 10, dtype=torch.int32, device="cuda"), z(1, 3, 3),
                           z(1, 3), MD, MC, scene["tau"], 2, **dict(good, **bad))
    no_rgb = {k: v for k, v in scene["vol"].items() if k != "rgb_cnt"}
    with pytest.raises(ValueError, match="rgb_cnt"):
        ops.tsdf_track(no_rgb, z(10, 3, dt=torch.float32), z(1, dt=torch.int32), torch.full((1,), 10, dtype=torch.int32, device="cuda"), z(1, 3, 3), z(1, 3),
                       MD, MC, scene["tau"], 2, **good)
