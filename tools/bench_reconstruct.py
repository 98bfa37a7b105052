"""fp_tsdf_integrate, fp_tsdf_count_triangles and fp_tsdf_emit_triangles (csrc/tsdf.hip: the two stages of reconstruct.py) on the device:
64 frames of 640 x 480 fused into a 256^3 volume, then the extraction, beside the numpy restatement (tests/tsdf_ref.py) on a volume small
enough to run on this machine's CPU, scaled per voxel-frame.

    python tools/bench_reconstruct.py [--iters 10] [--no-cpu] [--dim 256] [--frames 64] [--out profiles/reconstruct_bench.txt]

The scene is a blob of radius 90 mm (synthetic.make_blob_mesh) rendered by the HIP rasterizer from --frames Fibonacci viewpoints at 600 mm,
with a background plane at 1 500 mm (mask 0: it carves); the volume is the blob's padded box cut into dim^3 voxels.  Device time: HIP
events around one call, the median of --iters calls after 2 warm-up calls, one process.  fuse: the frames in batches of 32 (two calls of
fp_tsdf_integrate; the uploads are outside the events).  Voxel traffic: the six planes are read and written once per call, 48 bytes per
voxel and call.  extract: fp_tsdf_count_triangles, torch.cumsum, fp_tsdf_emit_triangles, then the weld (torch.unique) separately."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _eyes(n, radius):
    i = np.arange(n, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / n
    lon = i * np.pi * (3.0 - np.sqrt(5.0))
    r = np.sqrt(1.0 - z * z)
    return radius * np.stack([r * np.cos(lon), r * np.sin(lon), z], 1)


def _look_at(eye):
    zc = -eye / np.linalg.norm(eye)
    xc = np.cross(zc, [0.0, 0.0, 1.0])
    xc = np.cross(zc, [0.0, 1.0, 0.0]) if np.linalg.norm(xc) < 1e-6 else xc
    xc /= np.linalg.norm(xc)
    R = np.stack([xc, np.cross(zc, xc), zc])
    return R, -R @ eye


def _timed(fn, iters, setup=None):
    import torch
    ts = []
    for it in range(iters + 2):
        state = setup() if setup else None
        torch.cuda.synchronize()
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        out = fn(state) if setup else fn()
        en.record()
        en.synchronize()
        if it >= 2:
            ts.append(st.elapsed_time(en))
    return float(np.median(ts)), out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "reconstruct_bench.txt"))
    args = ap.parse_args()
    import torch
    from foundpose_amd import ops, synthetic
    from foundpose_amd.eval_bop19 import _Camera, _m2c
    from foundpose_amd.renderer import HipRasterizer
    assert torch.cuda.is_available(), "bench_reconstruct measures the MI355X"
    W, H, F, N = 640, 480, args.frames, args.dim
    K = np.array([[900.0, 0.0, 320.3], [0.0, 900.0, 239.6], [0.0, 0.0, 1.0]])
    mesh = synthetic.make_blob_mesh(50, 50, radius=90.0)
    poses = [_look_at(e) for e in _eyes(F, 600.0)]
    ras = HipRasterizer("cuda")
    ras.add_object_model(1, mesh=mesh)
    depth, mask, rgb = [], [], []
    for b0 in range(0, F, 16):
        r = ras.render_views(1, [_Camera(K, W, H, np.linalg.inv(_m2c(R, t))) for R, t in poses[b0:b0 + 16]])
        depth.append(torch.where(r["mask"] > 0, r["depth"], torch.full_like(r["depth"], 1500.0)))
        mask.append(r["mask"])
        rgb.append((r["color"] * 255.0).round().to(torch.uint8))
    depth, mask, rgb = torch.cat(depth), torch.cat(mask), torch.cat(rgb)
    cams = np.tile([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], (F, 1))
    pose12 = np.stack([np.concatenate([R.reshape(-1), t]) for R, t in poses])
    lo, hi = mesh.vertices.min(0).astype(np.float64), mesh.vertices.max(0).astype(np.float64)
    h = float((hi - lo).max() * 1.25 / N)
    tau = 4.0 * h
    origin = (lo + hi) / 2 - N * h / 2

    def fuse(vol):
        for b0 in range(0, F, 32):
            ops.tsdf_integrate(vol, depth[b0:b0 + 32], mask[b0:b0 + 32], rgb[b0:b0 + 32], cams[b0:b0 + 32], pose12[b0:b0 + 32], tau)
        return vol

    lines = [f"# python tools/bench_reconstruct.py on one {torch.cuda.get_device_name(0)} (device: HIP events around the calls, median of {args.iters} after 2 "
             f"warm-up runs): {F} frames of {W} x {H} into {N}^3 voxels of {h:.3f} mm, tau = {tau:.3f} mm"]
    ms, vol = _timed(fuse, args.iters, setup=lambda: ops.tsdf_new_volume(origin, h, (N, N, N)))
    vf = float(N) ** 3 * F
    calls = (F + 31) // 32
    lines.append(f"fuse      {ms:9.3f} ms   {vf / ms / 1e6:8.2f} G voxel-frames/s   {ms * 1e6 / vf:7.4f} ns per voxel-frame   voxel planes "
                 f"{48.0 * N ** 3 * calls / ms / 1e9:6.3f} TB/s ({calls} calls x 48 B per voxel)   observed voxels {int((vol['sdf_cnt'] >= 2).sum())}")
    ms_x, (counts, keys, pos, col) = _timed(lambda: ops.tsdf_extract(vol, 2), args.iters)
    lines.append(f"extract   {ms_x:9.3f} ms   {int(counts.sum())} triangles from {counts.numel()} cells (count, cumsum, emit; one read-back of the total)")

    def weld():
        uniq, inv = torch.unique(keys, sorted=True, return_inverse=True)
        v = torch.empty(len(uniq), 3, dtype=torch.float32, device=pos.device)
        v[inv] = pos
        return v

    ms_w, v = _timed(weld, args.iters)
    lines.append(f"weld      {ms_w:9.3f} ms   {len(v)} vertices (torch.unique over {len(keys)} keys, scatter of the positions)")
    if not args.no_cpu:
        from tests import tsdf_ref as ref
        n, f = 48, 4
        hs = h * N / n
        small = ref.new_volume(origin, hs, (n, n, n))
        d, m, c = depth[:f].cpu().numpy(), mask[:f].cpu().numpy(), rgb[:f].cpu().numpy()
        t0 = time.perf_counter()
        ref.integrate(small, d, m, c, cams[:f], pose12[:f], 4.0 * hs)
        host = time.perf_counter() - t0
        per = host * 1e9 / (n ** 3 * f)
        lines.append(f"numpy restatement, {f} frames into {n}^3 voxels on one CPU thread: {host:.3f} s = {per:.1f} ns per voxel-frame; at that rate the "
                     f"{N}^3 x {F} fuse takes ~{per * vf / 1e9:.0f} s, {per * vf / 1e6 / ms:.0f} x the device's time")
        t0 = time.perf_counter()
        rc = ref.extract(small, 2)[0]
        lines.append(f"numpy restatement, extraction of the {n}^3 volume: {time.perf_counter() - t0:.3f} s for {int(rc.sum())} triangles")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fobj:
        fobj.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
