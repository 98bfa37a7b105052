"""reconstruct.fill_volume and fp_tsdf_diffuse (csrc/tsdf_fill.hip) on the device: a 256^3 volume fused as
tools/bench_reconstruct.py fuses its own, but from the viewpoints above the object only, so that there is an underside to fill.

    python tools/bench_reconstruct_fill.py [--iters 10] [--dim 256] [--frames 64] [--out profiles/reconstruct_fill_bench.txt]

Timed, each with HIP events around the calls in one process, two warm-up runs, then the median of --iters runs and their spread (lowest ..
highest): the 4 smoothing iterations on one channel and the 64 colour iterations on three channels, as fill_volume runs them but straight
through fp_tsdf_diffuse on buffers restored outside the events; the same iteration written with torch slices, as a yardstick; and
fill_volume as a whole (its elementwise torch, its read-backs for the statistics, both diffusions).  Bytes moved: what the algorithm
needs, 4 C + 1 bytes in and as many out per voxel and iteration.  The yardstick's result is compared with the kernel's, bit for bit."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ORDER = ((0, 0, 0), (0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0))   # (dz, dy, dx): centre, -x, +x, -y, +y, -z, +z


def torch_iteration(val, state):
    """One iteration of the contract in torch slices: val fp32 [C, nz, ny, nx], state uint8 [nz, ny, nx] -> (val', state')."""
    import torch
    import torch.nn.functional as F
    nz, ny, nx = state.shape
    known = F.pad(state != 0, (1, 1, 1, 1, 1, 1))
    pad = F.pad(val, (1, 1, 1, 1, 1, 1))
    n = torch.zeros(state.shape, dtype=torch.float32, device=val.device)
    acc = torch.zeros_like(val)
    for dz, dy, dx in ORDER:
        sl = (slice(1 + dz, nz + 1 + dz), slice(1 + dy, ny + 1 + dy), slice(1 + dx, nx + 1 + dx))
        k = known[sl]
        n += k
        acc = torch.where(k[None], acc + pad[(slice(None),) + sl], acc)
    fixed = state == 1
    zero = torch.zeros((), dtype=torch.float32, device=val.device)
    out = torch.where(fixed[None], val, torch.where((n > 0)[None], acc / n[None], zero))
    return out, torch.where(fixed, 1, torch.where(n > 0, 2, 0)).to(torch.uint8)


def _timed(fn, iters, setup):
    import torch
    ts = []
    for it in range(iters + 2):
        state = setup()
        torch.cuda.synchronize()
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        out = fn(state)
        en.record()
        en.synchronize()
        if it >= 2:
            ts.append(st.elapsed_time(en))
    return float(np.median(ts)), float(min(ts)), float(max(ts)), out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "reconstruct_fill_bench.txt"))
    args = ap.parse_args()
    import torch
    from bench_reconstruct import _eyes, _look_at
    from foundpose_amd import _lib, ops, reconstruct, synthetic
    from foundpose_amd.eval_bop19 import _Camera, _m2c
    from foundpose_amd.renderer import HipRasterizer
    assert torch.cuda.is_available(), "bench_reconstruct_fill measures the MI355X"
    W, H, N = 640, 480, args.dim
    K = np.array([[900.0, 0.0, 320.3], [0.0, 900.0, 239.6], [0.0, 0.0, 1.0]])
    mesh = synthetic.make_blob_mesh(50, 50, radius=90.0)
    poses = [_look_at(e) for e in _eyes(args.frames, 600.0) if e[2] > 0]
    F = len(poses)
    ras = HipRasterizer("cuda")
    ras.add_object_model(1, mesh=mesh)
    lo, hi = mesh.vertices.min(0).astype(np.float64), mesh.vertices.max(0).astype(np.float64)
    h = float((hi - lo).max() * 1.25 / N)
    tau = 4.0 * h
    origin = (lo + hi) / 2 - N * h / 2
    vol = ops.tsdf_new_volume(origin, h, (N, N, N))
    cam = [K[0, 0], K[1, 1], K[0, 2], K[1, 2]]
    for b0 in range(0, F, 16):
        r = ras.render_views(1, [_Camera(K, W, H, np.linalg.inv(_m2c(R, t))) for R, t in poses[b0:b0 + 16]])
        depth = torch.where(r["mask"] > 0, r["depth"], torch.full_like(r["depth"], 1500.0))
        ops.tsdf_integrate(vol, depth, r["mask"], (r["color"] * 255.0).round().to(torch.uint8), np.tile(cam, (len(depth), 1)),
                           np.stack([np.concatenate([R.reshape(-1), t]) for R, t in poses[b0:b0 + 16]]), tau)
    opts = reconstruct.load_opts({"voxel_mm": h, "fill": "carve"})
    lines = [f"# python tools/bench_reconstruct_fill.py on one {torch.cuda.get_device_name(0)} (device: HIP events around the calls, median of {args.iters} "
             f"after 2 warm-up runs, lowest .. highest of them in brackets): {F} frames of {W} x {H} from above into {N}^3 voxels of {h:.3f} mm"]

    # the two diffusions' inputs, made the way fill_volume makes them
    src = vol["sdf_cnt"] >= opts.min_count
    g = torch.where(vol["sdf_cnt"] > 0, (vol["sdf_sum"].double() / vol["sdf_cnt"].double()).float(), torch.tensor(-1.0, device="cuda"))
    outer = torch.zeros_like(src)
    outer[[0, -1]] = True
    outer[:, [0, -1]] = True
    outer[:, :, [0, -1]] = True
    g = torch.where(outer, torch.tensor(1.0, device="cuda"), g)[None].contiguous()
    g_state = torch.where(src | outer, 1, 2).to(torch.uint8)
    has = vol["rgb_cnt"] > 0
    m = torch.where(has[None], (vol["rgb_sum"].double() / vol["rgb_cnt"].double()[None]).float(), torch.tensor(0.0, device="cuda")).contiguous()
    m_state = torch.where(has, 1, 0).to(torch.uint8)
    vox = float(N) ** 3
    for name, val0, state0, T in (("smooth", g, g_state, int(opts.fill_smooth_iters)), ("colour", m, m_state, int(opts.fill_color_iters))):
        C = val0.shape[0]
        val, state, vt, st = val0.clone(), state0.clone(), torch.empty_like(val0), torch.empty_like(state0)

        def restore():
            val.copy_(val0), state.copy_(state0)

        def kernel(_):
            _lib.call("fp_tsdf_diffuse", _lib.ptr(val), _lib.ptr(state), _lib.ptr(vt), _lib.ptr(st), C, N, N, N, T, _lib.stream())

        def slices(_):
            v, s = val0, state0
            for _t in range(T):
                v, s = torch_iteration(v, s)
            return v, s

        ms, ms_lo, ms_hi, _ = _timed(kernel, args.iters, restore)
        by = 2.0 * (4 * C + 1) * vox * T
        lines.append(f"{name:7s} fp_tsdf_diffuse  {T:3d} iterations x {C} channel(s)  {ms:9.3f} ms [{ms_lo:.3f} .. {ms_hi:.3f}]   {ms / T:7.4f} ms per iteration   "
                     f"{by / ms / 1e9:6.3f} TB/s of the {2 * (4 * C + 1)} B per voxel and iteration the algorithm needs")
        ms_t, t_lo, t_hi, (tv, ts) = _timed(slices, args.iters, lambda: None)
        same = bool(torch.equal(tv.view(torch.int32), val.view(torch.int32)) and torch.equal(ts, state))
        lines.append(f"{name:7s} torch slices     {T:3d} iterations x {C} channel(s)  {ms_t:9.3f} ms [{t_lo:.3f} .. {t_hi:.3f}]   {ms_t / T:7.4f} ms per iteration   "
                     f"{ms_t / ms:5.1f} x the kernel's time; its result equals the kernel's bit for bit: {same}")
        del tv, ts
    ms, ms_lo, ms_hi, (_, stats) = _timed(lambda _: reconstruct.fill_volume(vol, opts), args.iters, lambda: None)
    lines.append(f"fill_volume as a whole {ms:9.3f} ms [{ms_lo:.3f} .. {ms_hi:.3f}]: " + ", ".join(f"{k} {v}" for k, v in stats.items() if k != "seconds"))
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fobj:
        fobj.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
