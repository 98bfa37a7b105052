"""Template rendering rate on the MI355X (gen_templates' device chain) at LM-O settings: a procedurally generated
vertex-coloured mesh of ~20k triangles, the lmo camera (630 x 630 templates, SSAA 4 -> 2520 x 2520 renders), 420 x 420
crops, 57 views x 14 in-plane rotations = 798 templates, 32 views per launch chain.

    python tools/bench_render.py [--templates N] [--batch 32] [--png] [--textured]

--textured: the same geometry as a textured model (per-corner spherical UVs, unmerged; a 2048 x 2048 procedural texture
with its mip pyramid, the default material), rendered by render_raster_kernel<true>.

Reports templates/s of the device chain (render -> boxes -> crop cameras -> warps -> downsample, wall clock between
device synchronisations, host work for the crop cameras included) with the device time of each stage from HIP events,
and, with --png, the PNG writing separately.  The per-kernel split comes from a `rocprofv3 --kernel-trace --stats` run
of this tool."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundpose_amd import gen_templates, synthetic  # noqa: E402
from foundpose_amd.renderer import HipRasterizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--templates", type=int, default=798)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--png", action="store_true")
    ap.add_argument("--textured", action="store_true")
    args = ap.parse_args()
    opts = gen_templates.GenTemplatesOpts(version="bench", object_dataset="lmo")
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    _, render_cam = gen_templates.base_cameras(K, (640, 480), opts)
    views = gen_templates.template_views(opts, (346.31, 1499.84))[:args.templates]
    if args.textured:
        mesh = synthetic.make_textured_blob_mesh(100, 100, radius=70.0, seed=0, tex_size=2048)
    else:
        mesh = synthetic.make_blob_mesh(100, 100, radius=70.0, seed=0)
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    print(f"mesh: {len(mesh.faces)} triangles, {len(mesh.vertices)} vertices; render {render_cam.width}^2, crop {opts.crop_size[0]}, "
          f"{len(views)} templates, batch {args.batch}" + (f", texture {mesh.texture.shape[1]}^2" if args.textured else ""), flush=True)
    gen_templates.render_templates(r, 1, views[:args.batch], render_cam, opts)     # warm-up (code objects, allocator)
    torch.cuda.synchronize()
    # stage split from HIP events on one batch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    cams = [gen_templates.view_camera(render_cam, v) for v in views[:args.batch]]
    ev[0].record()
    out = r.render_views(1, cams)
    ev[1].record()
    gen_templates.render_templates(r, 1, views[:args.batch], render_cam, opts)
    ev[2].record()
    torch.cuda.synchronize()
    n = len(cams)
    print(f"render_views (setup + raster), {n} views: {ev[0].elapsed_time(ev[1]):8.2f} ms  ({ev[0].elapsed_time(ev[1]) / n:.3f} ms/view)")
    print(f"whole chain, {n} views:                   {ev[1].elapsed_time(ev[2]):8.2f} ms  ({ev[1].elapsed_time(ev[2]) / n:.3f} ms/template)")
    del out
    t0 = time.perf_counter()
    kept = []
    for s in range(0, len(views), args.batch):
        t = gen_templates.render_templates(r, 1, views[s:s + args.batch], render_cam, opts)
        kept.append({k: t[k].cpu().numpy() for k in ("rgb", "depth", "mask")})
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"device chain: {len(views)} templates in {dt:.3f} s = {len(views) / dt:.1f} templates/s (results copied to the host)")
    if args.png:
        from concurrent.futures import ThreadPoolExecutor
        with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(8) as pool:
            t0 = time.perf_counter()
            futs = [pool.submit(gen_templates._save_pngs, b["rgb"][i], b["depth"][i], b["mask"][i],
                                tuple(os.path.join(d, f"{k}_{j}_{i}.png") for k in ("rgb", "depth", "mask")))
                    for j, b in enumerate(kept) for i in range(len(b["rgb"]))]
            for f in futs:
                f.result()
            dt = time.perf_counter() - t0
        print(f"PNG writing (8 threads): {len(futs)} templates in {dt:.3f} s = {len(futs) / dt:.1f} templates/s")


if __name__ == "__main__":
    main()
