"""fp_tsdf_track (csrc/tsdf_track.hip: the tracking step of reconstruct.py with pose_source "track") on the device: one 640 x 480 frame
tracked against a 256^3 volume, with track_max_points 16 384 and 4 096, beside the numpy restatement (tests/tsdf_track_ref.py) on the
same volume and points on one CPU thread -- which is all it is compared with.

    python tools/bench_reconstruct_track.py [--iters 10] [--no-cpu] [--dim 256] [--frames 16] [--out profiles/reconstruct_track_bench.txt]

The scene is bench_reconstruct.py's blob of radius 90 mm rendered by the HIP rasterizer, here from a ring of cameras 5 degrees apart at
600 mm over a background plane at 1 500 mm.  The first --frames views are fused at their true poses; the next view is the tracked frame,
started from the pose of the view before it ("hold": 5 degrees off), 20 iterations -- once on shape alone and once on shape and colour
(fp_tsdf_track_rgb with the frame's colours, weight 30 mm per unit, color_max 0.25).  Device time: HIP events around one ops.tsdf_track
call (its launches and the read-back of the range check; the allocation of its outputs is inside, the lifting of the points outside),
the median of --iters calls after 2 warm-up calls, one process.  The split into pass and solve launches is the sum of the kernels'
own durations from one more call under torch.profiler; what the events hold beyond those sums is the time between kernels."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_reconstruct import _look_at, _timed   # noqa: E402


def _kernel_split(fn, pass_kernel="tsdf_track_pass_kernel"):
    """One call under torch.profiler -> {"pass": (launches, ms), "solve": (launches, ms)} from the kernels' own durations, or None."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for name in ("pass", "solve"):
            evs = [e for e in prof.events() if (pass_kernel if name == "pass" else "tsdf_track_solve_kernel") in e.name]
            ms = sum(float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)) for e in evs) / 1e3
            if not evs or ms <= 0:
                return None
            out[name] = (len(evs), ms)
        return out
    except Exception as e:   # the profiler is an extra: the event times stand without it
        print(f"torch.profiler gave no kernel durations ({type(e).__name__}: {e})", flush=True)
        return None


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "reconstruct_track_bench.txt"))
    args = ap.parse_args()
    import torch
    from foundpose_amd import ops, reconstruct, synthetic
    from foundpose_amd.eval_bop19 import _Camera, _m2c
    from foundpose_amd.renderer import HipRasterizer
    assert torch.cuda.is_available(), "bench_reconstruct_track measures the MI355X"
    W, H, F, N, LM_ITERS = 640, 480, args.frames, args.dim, 20
    K = np.array([[900.0, 0.0, 320.3], [0.0, 900.0, 239.6], [0.0, 0.0, 1.0]])
    Kr = K.copy()
    Kr[0, 2] += 0.5   # the rasterizer samples at pixel centres x + 1/2, the frames' camera has them at integers
    Kr[1, 2] += 0.5
    mesh = synthetic.make_blob_mesh(50, 50, radius=90.0)
    az = np.radians(5.0 * np.arange(F + 1))
    poses = [_look_at(600.0 * np.array([np.cos(0.35) * np.cos(a), np.cos(0.35) * np.sin(a), np.sin(0.35)])) for a in az]
    ras = HipRasterizer("cuda")
    ras.add_object_model(1, mesh=mesh)
    depth, mask, rgb = [], [], []
    for b0 in range(0, F + 1, 16):
        r = ras.render_views(1, [_Camera(Kr, W, H, np.linalg.inv(_m2c(R, t))) for R, t in poses[b0:b0 + 16]])
        depth.append(torch.where(r["mask"] > 0, r["depth"], torch.full_like(r["depth"], 1500.0)))
        mask.append(r["mask"])
        rgb.append((r["color"] * 255.0).round().to(torch.uint8))
    depth, mask, rgb = torch.cat(depth), torch.cat(mask), torch.cat(rgb)
    cam = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    pose12 = np.stack([np.concatenate([R.reshape(-1), t]) for R, t in poses])
    lo, hi = mesh.vertices.min(0).astype(np.float64), mesh.vertices.max(0).astype(np.float64)
    h = float((hi - lo).max() * 1.25 / N)
    tau, md = 4.0 * h, 3.0 * h
    origin = (lo + hi) / 2 - N * h / 2
    vol = ops.tsdf_new_volume(origin, h, (N, N, N))
    ops.tsdf_integrate(vol, depth[:F], mask[:F], rgb[:F], np.tile(cam, (F, 1)), pose12[:F], tau)
    R0 = torch.from_numpy(poses[F - 1][0].copy()).cuda()[None]
    t0 = torch.from_numpy(poses[F - 1][1].copy()).cuda()[None]
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    lines = [f"# python tools/bench_reconstruct_track.py on one {torch.cuda.get_device_name(0)} (device: HIP events around one ops.tsdf_track call, median of "
             f"{args.iters} after 2 warm-up calls): one {W} x {H} frame against {N}^3 voxels of {h:.3f} mm fused from {F} frames, tau = {tau:.3f} mm, "
             f"inlier distance {md:.3f} mm, start 5 degrees off, {LM_ITERS} iterations = {2 * (1 + LM_ITERS) + 2} launches per call"]
    host_vol = None
    for cap in (16384, 4096):
        pts = reconstruct._lift(depth[F], mask[F], cam, cap)
        n = int(pts.shape[0])
        end = torch.full((1,), n, dtype=torch.int32, device="cuda")
        call = lambda: ops.tsdf_track(vol, pts, zero, end, R0, t0, md, 1, tau, LM_ITERS)   # noqa: E731
        ms, out = _timed(call, args.iters)
        used, inl, status = int(out["iters_used"][0]), int(out["num_points"][0]), int(out["status"][0])
        c = (np.trace(out["R"][0].cpu().numpy().T @ poses[F][0]) - 1.0) / 2.0
        err = (float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(out["t"][0].cpu().numpy() - poses[F][1])))
        line = (f"track_max_points {cap:5d}: {n:5d} points ({(n + 31) // 32} workgroups per pass)   {ms:7.3f} ms per tracked frame   {used} of {LM_ITERS} iterations used, "
                f"{inl} inliers at the start, status {status}, {err[0]:.3f} deg / {err[1]:.3f} mm from the true pose")
        split = _kernel_split(call)
        if split:
            (np_, mp), (ns, msol) = split["pass"], split["solve"]
            line += (f"\n    kernels' own durations: pass {mp:6.3f} ms in {np_} launches ({mp * 1e3 / np_:5.1f} us each), solve {msol:6.3f} ms in {ns} launches "
                     f"({msol * 1e3 / ns:5.1f} us each); between kernels and around them {ms - mp - msol:6.3f} ms = {100.0 * (ms - mp - msol) / ms:4.1f} % of the call")
            taps = 64.0 * n                                                     # sixteen 4-byte gathers per point and pass
            chunks = (n + 31) // 32
            line += (f"\n    a pass gathers at most {taps / 1e6:.2f} MB (sixteen 4-byte taps per point) and runs about {300.0 * n / 1e6:.1f} M fp64 operations: "
                     f"{taps / (mp * 1e-3 / np_) / 1e9:.1f} GB/s while a pass runs"
                     f"\n    a solve folds {chunks} partial records one after the other (lm_fold: one lane per term, chunk order): "
                     f"{msol * 1e6 / ns / chunks:5.0f} ns per record, about one load's latency each -- {100.0 * msol / ms:4.1f} % of the call")
        lines.append(line)
        # the same frame and volume on shape and colour (fp_tsdf_track_rgb): weight 30 mm per unit, color_max 0.25
        pts_c, cols = reconstruct._lift_rgb(depth[F], mask[F], rgb[F], cam, cap)
        assert torch.equal(pts_c, pts)
        call_c = lambda: ops.tsdf_track(vol, pts, zero, end, R0, t0, md, 1, tau, LM_ITERS, colors=cols, color_weight=30.0, color_max=0.25)   # noqa: E731
        ms_c, out_c = _timed(call_c, args.iters)
        c = (np.trace(out_c["R"][0].cpu().numpy().T @ poses[F][0]) - 1.0) / 2.0
        err_c = (float(np.degrees(np.arccos(np.clip(c, -1, 1)))), float(np.linalg.norm(out_c["t"][0].cpu().numpy() - poses[F][1])))
        line = (f"    with colours (weight 30, color_max 0.25): {ms_c:7.3f} ms per tracked frame   {int(out_c['iters_used'][0])} of {LM_ITERS} iterations used, "
                f"status {int(out_c['status'][0])}, {err_c[0]:.3f} deg / {err_c[1]:.3f} mm from the true pose")
        split = _kernel_split(call_c, "tsdf_track_rgb_pass_kernel")
        if split:
            (np_, mp), (ns, msol) = split["pass"], split["solve"]
            line += (f"\n        kernels' own durations: pass {mp:6.3f} ms in {np_} launches ({mp * 1e3 / np_:5.1f} us each; at most forty-eight 4-byte taps per point), "
                     f"solve {msol:6.3f} ms in {ns} launches ({msol * 1e3 / ns:5.1f} us each); between kernels and around them {ms_c - mp - msol:6.3f} ms")
        lines.append(line)
        if not args.no_cpu:
            from tests import tsdf_track_ref as tr
            if host_vol is None:
                host_vol = dict(vol, sdf_sum=vol["sdf_sum"].cpu().numpy(), sdf_cnt=vol["sdf_cnt"].cpu().numpy())
            X = pts.cpu().numpy().astype(np.float64)
            t_0 = time.perf_counter()
            ref = tr.track(host_vol, poses[F - 1][0], poses[F - 1][1], X, tau, 1, md, LM_ITERS)
            host = time.perf_counter() - t_0
            lines.append(f"    numpy restatement, the same frame on one CPU thread: {host:.3f} s ({ref['iters_used']} iterations) = {host * 1e3 / ms:.0f} x the device's time")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fobj:
        fobj.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
