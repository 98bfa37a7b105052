"""GPU: frame-to-model tracking against a TSDF volume (csrc/tsdf_track.hip, ops.tsdf_track) against the numpy
restatement tests/tsdf_track_ref.py.  The volume is tsdf_ref.integrate_fixture()'s five frames fused by ops.tsdf_integrate (37 x 29 x 23
voxels, tau = 10 mm); the restatement reads the planes the GPU wrote, so both sides start from the same taps.  The points are lifted
from frame 0; tests/test_tsdf_track_cpu.py shows that no point of the fixture sits where a last bit could decide a branch."""
import ctypes

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops
from tests import tsdf_track_ref as tr

pytestmark = pytest.mark.gpu
MC, MD = tr.TRACK_MIN_COUNT, tr.TRACK_MAX_DIST


@pytest.fixture(scope="module")
def scene():
    fx = tr.track_fixture()
    f = fx["fx"]
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    vol = ops.tsdf_new_volume(f["origin"], f["h"], f["dims"])
    ops.tsdf_integrate(vol, cuda(f["depth"]), cuda(f["mask"]), cuda(f["rgb"]), f["cams"], f["poses"], f["tau"])
    host = dict(vol, **{k: vol[k].cpu().numpy() for k in ops.TSDF_PLANES})
    return dict(vol=vol, host=host, tau=f["tau"], fx=fx)


def _run(scene, problems, iters=20, normal_eq=False):
    """problems: list of dict(X, R, t, md=MD, has_pose=True) -> ops.tsdf_track's dict (cpu numpy)."""
    X = np.concatenate([p["X"] for p in problems]).astype(np.float32)
    n = np.array([len(p["X"]) for p in problems])
    rb = np.concatenate([[0], np.cumsum(n)[:-1]])
    cuda = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()   # noqa: E731
    out = ops.tsdf_track(scene["vol"], cuda(X), cuda(rb, torch.int32), cuda(rb + n, torch.int32), cuda(np.stack([p["R"] for p in problems]), torch.float64),
                         cuda(np.stack([p["t"] for p in problems]), torch.float64), [p.get("md", MD) for p in problems], MC, scene["tau"], iters,
                         has_pose=cuda(np.array([p.get("has_pose", True) for p in problems])), want_normal_eq=normal_eq)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ref(scene, p, iters=20):
    return tr.track(scene["host"], p["R"], p["t"], p["X"].astype(np.float32).astype(np.float64), scene["tau"], MC, p.get("md", MD), iters, p.get("has_pose", True))


def _main(scene):
    fx = scene["fx"]
    return dict(X=fx["X"], R=fx["R"], t=fx["t"])


def _close(got, b, ref):
    rot = np.radians(tr.rot_angle_deg(got["R"][b], ref["R"]))
    dt = float(np.linalg.norm(got["t"][b] - ref["t"]))
    return rot, dt


def test_at_the_input_pose(scene):
    """Both sides compute in fp64 from the same fp32 taps and differ in summation order and contraction only: 1e-9 of the largest entry
    per block, as tests/test_gpu_depth_refine.py holds section 14."""
    p = _main(scene)
    out = _run(scene, [p], iters=0, normal_eq=True)
    X64 = p["X"].astype(np.float64)
    want = tr.normal_equations(scene["host"], p["R"], p["t"], X64, scene["tau"], MC, MD)
    inl = int(tr.system(scene["host"], p["R"], p["t"], X64, scene["tau"], MC, MD)[3].sum())
    got = out["normal_eq"][0]
    print(f"{len(X64)} points, {inl} inliers: max |dH| {np.abs(got[:21] - want[:21]).max():.3e} of {np.abs(want[:21]).max():.3e}, "
          f"|dg| {np.abs(got[21:27] - want[21:27]).max():.3e} of {np.abs(want[21:27]).max():.3e}, cost {got[27]!r} vs {want[27]!r}")
    assert out["num_points"][0] == inl and 6 <= inl < len(X64)
    for lo, hi in ((0, 21), (21, 27), (27, 28)):
        assert np.abs(got[lo:hi] - want[lo:hi]).max() <= 1e-9 * np.abs(want[lo:hi]).max(), lo
    assert abs(out["cost_in"][0] - want[27]) <= 1e-9 * want[27]
    assert out["cost_in"][0] == out["cost_out"][0] == got[27] and out["iters_used"][0] == 0 and out["status"][0] == 1
    assert np.array_equal(out["R"][0], p["R"]) and np.array_equal(out["t"][0], p["t"])


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
    probs = [dict(X=tr.sized_points(n), R=fx["R"], t=fx["t"]) for n in sizes]
    out = _run(scene, probs, iters=20, normal_eq=True)
    for b, (n, p) in enumerate(zip(sizes, probs)):
        ref = _ref(scene, p, 20)
        want = tr.normal_equations(scene["host"], p["R"], p["t"], p["X"].astype(np.float64), scene["tau"], MC, MD)
        rot, dt = _close(out, b, ref)
        print(f"{n} points, {out['num_points'][b]} inliers: cost {out['cost_in'][b]:.6f} -> {out['cost_out'][b]:.6f}, status {out['status'][b]}, "
              f"{out['iters_used'][b]} iterations; pose differs by {rot:.3e} rad, {dt:.3e} mm")
        assert out["num_points"][b] == ref["num_points"] >= 6 and out["status"][b] == ref["status"]
        for lo, hi in ((0, 21), (21, 27), (27, 28)):
            assert np.abs(out["normal_eq"][b][lo:hi] - want[lo:hi]).max() <= 1e-9 * np.abs(want[lo:hi]).max(), (n, lo)
        assert out["cost_out"][b] <= out["cost_in"][b] and rot < 1e-6 and dt < 1e-3


def test_batch_invariance_and_degenerate_problems(scene):
    fx = scene["fx"]
    p = _main(scene)
    far = fx["t"] + np.array([0.0, 0.0, 500.0])                                # the volume lies 500 mm in front of every point
    probs = [dict(p, has_pose=False), dict(X=tr.sized_points(5), R=fx["R"], t=fx["t"]), p, dict(p, md=float("nan")), dict(p, t=far)]
    batch, again = _run(scene, probs, normal_eq=True), _run(scene, probs, normal_eq=True)
    assert batch["status"].tolist() == [2, 2, 0, 2, 2] and batch["num_points"].tolist()[:2] == [0, 5] and batch["num_points"][4] == 0
    assert batch["iters_used"][2] > 2 and np.abs(batch["normal_eq"][2]).max() > 0
    for b, q in enumerate(probs):
        alone = _run(scene, [q], normal_eq=True)
        for key in batch:
            assert batch[key][b].tobytes() == alone[key][0].tobytes() == again[key][b].tobytes(), (b, key)
        if b != 2:
            assert np.array_equal(batch["R"][b], q["R"]) and np.array_equal(batch["t"][b], q["t"])
            assert batch["iters_used"][b] == 0
    assert np.isnan(batch["cost_in"][3])                                       # max_dist^2 per point: a NaN, and no inlier


def _raw(scene, **over):
    """fp_tsdf_track through ctypes with one valid problem of 40 points, `over` replacing arguments -> (rc, message, outputs dict)."""
    vol, fx = scene["vol"], scene["fx"]
    dev = "cuda"
    X = torch.from_numpy(fx["X"][:40].copy()).to(dev)
    a = dict(sdf_sum=_lib.ptr(vol["sdf_sum"]), sdf_cnt=_lib.ptr(vol["sdf_cnt"]), dims=vol["dims"], min_count=MC, tau=scene["tau"], points=_lib.ptr(X), num_rows=40,
             rb=[0], re=[40], num_det=1, max_points=64, iters=3, scratch_bytes=None)
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
    rc = _lib.lib().fp_tsdf_track(a["sdf_sum"], a["sdf_cnt"], box.ctypes.data_as(_lib.vp), *a["dims"], a["min_count"], a["tau"], a["points"], a["num_rows"],
                                  _lib.ptr(rb), _lib.ptr(re), _lib.ptr(R), _lib.ptr(t), _lib.ptr(hp), _lib.ptr(md), B, a["max_points"], a["iters"],
                                  _lib.ptr(scratch), need if a["scratch_bytes"] is None else a["scratch_bytes"], *[ptrs[k] for k in outs], _lib.stream())
    torch.cuda.synchronize()
    return rc, _lib.lib().fp_last_error().decode(), {k: v.cpu().numpy() for k, v in outs.items()}


def test_refusals_write_nothing(scene):
    rc, _, outs = _raw(scene)
    assert rc == 0 and outs["status"][0] in (0, 1) and outs["num_points"][0] > 6         # the arguments below are this call's, one of them changed
    nx, ny, nz = scene["vol"]["dims"]
    need = _lib.tsdf_track_scratch_bytes(1, 64)
    cases = [(dict(re=[41]), "problem 0"),                                               # past num_rows
             (dict(num_det=2, rb=[0, 0], re=[40, 30], max_points=38), "problem 0"),      # longer than max_points
             (dict(num_det=2, rb=[0, 30], re=[40, 41]), "problem 1"),
             (dict(rb=[-1]), "problem 0"),
             (dict(sdf_sum=ctypes.c_void_p(0)), "null pointer"), (dict(points=ctypes.c_void_p(0)), "null pointer"),
             (dict(null_out={"status": ctypes.c_void_p(0)}), "null pointer"),
             (dict(dims=(1, ny, nz)), "dimensions"), (dict(dims=(nx, ny, 1)), "dimensions"),
             (dict(iters=1001), "iters"), (dict(iters=-1), "iters"), (dict(min_count=0), "min_count"), (dict(tau=0.0), "truncation"),
             (dict(tau=float("nan")), "truncation"), (dict(scratch_bytes=need - 1), "scratch")]
    for over, word in cases:
        rc, msg, outs = _raw(scene, **over)
        assert rc == 1 and "fp_tsdf_track" in msg and word in msg, (over, rc, msg)
        for key, v in outs.items():
            assert np.all(v == -7), (over, key)
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device="cuda")           # noqa: E731
    with pytest.raises(_lib.FoundPoseNativeError, match="problem 0"):                     # the wrapper passes the message on
        ops.tsdf_track(scene["vol"], z(10, 3, dt=torch.float32), z(1, dt=torch.int32), torch.full((1,), 11, dtype=torch.int32, device="cuda"), z(1, 3, 3), z(1, 3),
                       MD, MC, scene["tau"], 2)
    for bad in (dict(min_count=0), dict(trunc_mm=-1.0), dict(iters=1001)):
        kw = dict(dict(min_count=MC, trunc_mm=scene["tau"], iters=2), **bad)
        with pytest.raises(ValueError):
            ops.tsdf_track(scene["vol"], z(10, 3, dt=torch.float32), z(1, dt=torch.int32), torch.full((1,), 10, dtype=torch.int32, device="cuda"), z(1, 3, 3),
                           z(1, 3), MD, **kw)
