"""Silhouette refinement at the driver's default shape: batch 32, 640 x 480 masks holding a disc of the object's
projected size, 4096 model points (a sphere), contour cap 1024, 30 iterations, starts 12 mm sideways and 40 mm along the ray off
the planted pose.  One process, HIP events, the median of --steps timed calls after --warmup: ops.mask_distance,
refine_util.mask_contours and refine_util.refine_mask each on their own, and refine_util.refine_depth at the shape of
tools/bench_depth_refine.py (449 points, max_points 480, 640 x 480 depth) beside them.  Writes the lines to --out.  No threshold.

    python tools/bench_mask_refine.py [--steps 20] [--warmup 3] [--iters 30] [--out profiles/mask_refine_bench.txt]
"""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sphere(n, radius):
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return (radius * np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], 1)).astype(np.float32)


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--max-contour", type=int, default=1024)
    ap.add_argument("--huber-px", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_refine_bench.txt"))
    args = ap.parse_args()
    import torch
    from foundpose_amd import ops, refine_util

    H, W, B, P = 480, 640, args.batch, args.points
    cam = (572.4, 573.6, 325.3, 242.0)
    radius = 60.0
    rng = np.random.default_rng(0)
    X = sphere(P, radius)
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    masks, t0, tg = [], [], []
    for b in range(B):
        z = rng.uniform(700, 1100)
        cu, cv = rng.uniform(150, W - 150), rng.uniform(120, H - 120)
        t = np.array([(cu - cam[2]) / cam[0] * z, (cv - cam[3]) / cam[1] * z, z])
        # the silhouette of a sphere is (to first order at this distance) the disc of radius f r / sqrt(z^2 - r^2) about its centre's projection
        rad = cam[0] * radius / np.sqrt(z * z - radius * radius)
        masks.append((((uu - cu) ** 2 + (vv - cv) ** 2) <= rad * rad).astype(np.uint8))
        ray = t / np.linalg.norm(t)
        side = np.cross(ray, [0.0, 1.0, 0.0])
        tg.append(t)
        t0.append(t + 12.0 * side / np.linalg.norm(side) + 40.0 * ray)
    dev = torch.device("cuda", 0)
    cuda = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    mk = cuda(np.stack(masks), torch.uint8)
    d2, dist_ms, dist_min = timed(lambda: ops.mask_distance(mk), args.steps, args.warmup)
    (rows, cb, ce), cont_ms, cont_min = timed(lambda: refine_util.mask_contours(mk, args.max_contour), args.steps, args.warmup)
    eye = np.tile(np.eye(3), (B, 1, 1))
    zeros, full = torch.zeros(B, dtype=torch.int32, device=dev), torch.full((B,), P, dtype=torch.int32, device=dev)
    a = (d2, rows, cb, ce, [cam] * B, cuda(eye, torch.float64), cuda(np.stack(t0), torch.float64), zeros, full, cuda(X, torch.float32),
         torch.ones(B, dtype=torch.bool, device=dev), args.huber_px)
    out, ref_ms, ref_min = timed(lambda: refine_util.refine_mask(*a, iters=args.iters, max_points=P, max_contour=args.max_contour), args.steps, args.warmup)
    st = out["status"].cpu().numpy()
    t = out["t"].cpu().numpy()
    lat = lambda tt: [float(np.linalg.norm((x - g) - ((x - g) @ (g / np.linalg.norm(g))) * g / np.linalg.norm(g))) for x, g in zip(tt, tg)]
    along = lambda tt: [float(abs((x - g) @ (g / np.linalg.norm(g)))) for x, g in zip(tt, tg)]
    med = lambda v: float(np.median(v))

    # refine_depth at the shape of tools/bench_depth_refine.py, in the same process
    Pd = 449
    depth, Xd, Rd, td = [], [], [], []
    for b in range(B):
        nx, ny = (uu - cam[2]) / cam[0], (vv - cam[3]) / cam[1]
        D = (rng.uniform(700, 1100) * (1.0 + rng.uniform(-0.2, 0.2) * nx + rng.uniform(-0.2, 0.2) * ny + 0.4 * ((nx - 0.01) ** 2 + 1.5 * (ny + 0.02) ** 2))).astype(np.float32)
        u, v = np.rint(rng.uniform(150, W - 150) + rng.uniform(-100, 100, Pd)), np.rint(rng.uniform(120, H - 120) + rng.uniform(-100, 100, Pd))
        z = D[v.astype(int), u.astype(int)].astype(np.float64)
        Xc = np.stack([(u - cam[2]) / cam[0] * z, (v - cam[3]) / cam[1] * z, z], 1)
        c = Xc.mean(0)
        dt = rng.normal(size=3)
        depth.append(D)
        Xd.append((Xc - c).astype(np.float32))
        Rd.append(np.eye(3))
        td.append(c + dt * 10.0 / np.linalg.norm(dt))
    rb = np.arange(B) * Pd
    ad = (cuda(np.stack(depth), torch.float32), cuda(np.arange(B), torch.int32), [cam] * B, cuda(np.stack(Rd), torch.float64), cuda(np.stack(td), torch.float64),
          cuda(rb, torch.int32), cuda(rb + Pd, torch.int32), cuda(np.concatenate(Xd), torch.float32), torch.ones(B, dtype=torch.bool, device=dev), 20.0)
    _, dep_ms, dep_min = timed(lambda: refine_util.refine_depth(*ad, iters=args.iters, max_points=480), args.steps, args.warmup)

    line = {"metric": "mask_refine", "date": datetime.date.today().isoformat(), "runs": 1, "steps": args.steps, "warmup": args.warmup, "batch": B, "masks": [H, W],
            "points": P, "max_contour": args.max_contour, "iters": args.iters, "huber_px": args.huber_px,
            "mask_distance_device_ms_median": dist_ms, "mask_distance_device_ms_min": dist_min,
            "mask_contours_ms_median": cont_ms, "mask_contours_ms_min": cont_min, "contour_rows_median": med((ce - cb).cpu().numpy()),
            "refine_mask_device_ms_median": ref_ms, "refine_mask_device_ms_min": ref_min,
            "refine_depth_device_ms_median": dep_ms, "refine_depth_device_ms_min": dep_min,
            "status_counts": {int(k): int((st == k).sum()) for k in (0, 1, 2)}, "iters_used_median": med(out["iters_used"].cpu().numpy()),
            "measurable_median": med(out["num_points"].cpu().numpy()), "cost_in_median": med(out["cost_in"].cpu().numpy()),
            "cost_out_median": med(out["cost_out"].cpu().numpy()), "lateral_mm_start_median": med(lat(t0)), "lateral_mm_refined_median": med(lat(t)),
            "along_ray_mm_start_median": med(along(t0)), "along_ray_mm_refined_median": med(along(t))}
    text = ("tools/bench_mask_refine.py on one MI355X: batch %d, %d x %d masks holding a disc of the object's projected size, %d points, contour cap %d, %d iterations,\n"
            "Huber delta %g px, %d timed calls after %d warm-up calls, one process (HIP events around ops.mask_distance, refine_util.mask_contours --\n"
            "which synchronises once, in nonzero() -- refine_util.refine_mask, and refine_util.refine_depth at the shape of tools/bench_depth_refine.py).\n"
            "This file holds ONE run of the tool, the last one made; DESIGN.md section 38 says how often the tool was run and what the other runs gave.\n\n%s\n"
            % (B, W, H, P, args.max_contour, args.iters, args.huber_px, args.steps, args.warmup, json.dumps(line)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
