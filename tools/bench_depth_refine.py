"""Depth refinement at the headline bank's template size: batch 32, 449 points per template (the headline
bank's mean; max_points 480 = its p_max), 640 x 480 depth images (one per detection), 30 iterations, starts 3 degrees / 10 mm off a
planted smooth surface.  Prints the device time per batch (HIP events around refine_depth) as one JSON line.  The bank's other
9 968 templates are not built: a detection reads its own rows only.

    python tools/bench_depth_refine.py [--steps 20] [--warmup 3] [--iters 30]

The per-kernel table comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rot_exp(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    return np.eye(3) if th < 1e-12 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=449)
    ap.add_argument("--max-points", type=int, default=480)
    ap.add_argument("--tau", type=float, default=20.0)
    args = ap.parse_args()
    import torch
    from foundpose_amd import refine_util

    H, W, B, P = 480, 640, args.batch, args.points
    cam = (572.4, 573.6, 325.3, 242.0)
    rng = np.random.default_rng(0)
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth, X, R0, t0, Rg, tg = [], [], [], [], [], []
    for b in range(B):
        nx, ny = (uu - cam[2]) / cam[0], (vv - cam[3]) / cam[1]
        z0 = rng.uniform(700, 1100)
        D = (z0 * (1.0 + rng.uniform(-0.2, 0.2) * nx + rng.uniform(-0.2, 0.2) * ny + 0.4 * ((nx - 0.01) ** 2 + 1.5 * (ny + 0.02) ** 2))).astype(np.float32)
        cu, cv = rng.uniform(150, W - 150), rng.uniform(120, H - 120)        # an object about 200 px across
        u, v = np.rint(cu + rng.uniform(-100, 100, P)), np.rint(cv + rng.uniform(-100, 100, P))
        z = D[v.astype(int), u.astype(int)].astype(np.float64)
        Xc = np.stack([(u - cam[2]) / cam[0] * z, (v - cam[3]) / cam[1] * z, z], 1)
        R = rot_exp(rng.normal(size=3) * 0.5)
        t = Xc.mean(0)
        ax, dt = rng.normal(size=3), rng.normal(size=3)
        depth.append(D)
        X.append(((Xc - t) @ R).astype(np.float32))
        Rg.append(R)
        tg.append(t)
        R0.append(rot_exp(ax / np.linalg.norm(ax) * np.radians(3.0)) @ R)
        t0.append(t + dt * 10.0 / np.linalg.norm(dt))
    dev = torch.device("cuda", 0)
    cuda = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    rb = np.arange(B) * P
    a = (cuda(np.stack(depth), torch.float32), cuda(np.arange(B), torch.int32), [cam] * B, cuda(np.stack(R0), torch.float64), cuda(np.stack(t0), torch.float64),
         cuda(rb, torch.int32), cuda(rb + P, torch.int32), cuda(np.concatenate(X), torch.float32), torch.ones(B, dtype=torch.bool, device=dev), args.tau)
    for _ in range(args.warmup):
        out = refine_util.refine_depth(*a, iters=args.iters, max_points=args.max_points)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = refine_util.refine_depth(*a, iters=args.iters, max_points=args.max_points)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    st = out["status"].cpu().numpy()
    R, t = out["R"].cpu().numpy(), out["t"].cpu().numpy()
    ang = lambda A, Bm: np.degrees(np.arccos(np.clip((np.einsum("bij,bij->b", A, Bm) - 1) / 2, -1, 1)))
    med = lambda v: float(np.median(v))
    print(json.dumps({"metric": "depth_refine", "batch": B, "points": P, "max_points": args.max_points, "depth": [H, W], "iters": args.iters, "tau_mm": args.tau,
                      "refine_device_ms_median": med(ms), "refine_device_ms_min": float(min(ms)),
                      "status_counts": {int(k): int((st == k).sum()) for k in (0, 1, 2)}, "inliers_median": med(out["num_points"].cpu().numpy()),
                      "iters_used_median": med(out["iters_used"].cpu().numpy()),
                      "rot_err_deg_start_median": med(ang(np.stack(R0), np.stack(Rg))), "rot_err_deg_refined_median": med(ang(R, np.stack(Rg))),
                      "trans_err_mm_start_median": med(np.linalg.norm(np.stack(t0) - np.stack(tg), axis=1)),
                      "trans_err_mm_refined_median": med(np.linalg.norm(t - np.stack(tg), axis=1))}))


if __name__ == "__main__":
    main()
