"""Joint feature + depth refinement at the headline shape of sections 11 and 14: batch 32, 449 points per
template (max_points 480), C = 256 and a 37 x 37 map of a 518 x 518 crop camera, 640 x 480 depth images (one per detection), 30
iterations, starts 3 degrees / 10 mm off a planted smooth surface with planted smooth features.  Prints, as one JSON line, the device
time per batch (HIP events, median of --steps calls) of one refine_rgbd call and, in the same process, of the sequential pair
refine_featuremetric -> refine_depth on the same inputs.

    python tools/bench_rgbd_refine.py [--steps 20] [--warmup 3] [--iters 30]
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


def smooth_field(g, C, rng):
    yy, xx = np.meshgrid(np.arange(g, dtype=np.float64), np.arange(g, dtype=np.float64), indexing="ij")
    M = np.zeros((g, g, C))
    for c in range(C):
        for _ in range(3):
            lam, th, ph = rng.uniform(6.0, 15.0), rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
            M[:, :, c] += rng.uniform(0.5, 1.0) * np.sin(2 * np.pi / lam * (np.cos(th) * xx + np.sin(th) * yy) + ph)
    return M.astype(np.float32)


def bilinear(M, xm, ym):
    g = M.shape[0]
    xm, ym = np.clip(xm, 0, g - 1), np.clip(ym, 0, g - 1)
    x0, y0 = np.minimum(np.floor(xm), g - 2).astype(int), np.minimum(np.floor(ym), g - 2).astype(int)
    al, be = (xm - x0).astype(np.float32)[:, None], (ym - y0).astype(np.float32)[:, None]
    return (1 - be) * ((1 - al) * M[y0, x0] + al * M[y0, x0 + 1]) + be * ((1 - al) * M[y0 + 1, x0] + al * M[y0 + 1, x0 + 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=449)
    ap.add_argument("--max-points", type=int, default=480)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--tau", type=float, default=20.0)
    ap.add_argument("--depth-weight", type=float, default=1.0)
    args = ap.parse_args()
    import torch
    from foundpose_amd import refine_util

    H, W, B, P, C, G, S = 480, 640, args.batch, args.points, args.channels, 37, 518
    cam = (572.4, 573.6, 325.3, 242.0)
    rng = np.random.default_rng(0)
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth, X, F, maps, fcams, As, avs, R0, t0, Rg, tg = [], [], [], [], [], [], [], [], [], [], []
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
        # the crop camera: looks at the object's centre, the 200 px of the object on 400 of its 518
        c = Xc.mean(0)
        zax = c / np.linalg.norm(c)
        xax = np.cross([0.0, 1.0, 0.0], zax)
        xax /= np.linalg.norm(xax)
        A = np.stack([xax, np.cross(zax, xax), zax])                          # rows: the crop camera's axes in the frame's camera
        ff = 2.0 * cam[0]
        fcam = (ff, ff, S / 2.0, S / 2.0)
        M = smooth_field(G, C, rng)
        Xf = Xc @ A.T
        xm, ym = (ff * Xf[:, 0] / Xf[:, 2] + S / 2.0) * (G / S) - 0.5, (ff * Xf[:, 1] / Xf[:, 2] + S / 2.0) * (G / S) - 0.5
        ax, dt = rng.normal(size=3), rng.normal(size=3)
        depth.append(D)
        X.append(((Xc - t) @ R).astype(np.float32))
        F.append(bilinear(M, xm, ym))
        maps.append(M)
        fcams.append(fcam)
        As.append(A)
        avs.append(np.zeros(3))
        Rg.append(R)
        tg.append(t)
        R0.append(rot_exp(ax / np.linalg.norm(ax) * np.radians(3.0)) @ R)
        t0.append(t + dt * 10.0 / np.linalg.norm(dt))
    dev = torch.device("cuda", 0)
    cuda = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    rb = np.arange(B) * P
    fmap, dstack, idx = cuda(np.stack(maps), torch.float32), cuda(np.stack(depth), torch.float32), cuda(np.arange(B), torch.int32)
    A_d, a_d = cuda(np.stack(As), torch.float64), cuda(np.stack(avs), torch.float64)
    Rc, tc = cuda(np.stack(R0), torch.float64), cuda(np.stack(t0), torch.float64)
    # the same start in the crop cameras, for the sequential pair's feature stage
    Rf = cuda(np.stack([A @ R for A, R in zip(As, R0)]), torch.float64)
    tf = cuda(np.stack([A @ t for A, t in zip(As, t0)]), torch.float64)
    rbd, red = cuda(rb, torch.int32), cuda(rb + P, torch.int32)
    feats, verts = cuda(np.concatenate(F), torch.float32), cuda(np.concatenate(X), torch.float32)
    ok = torch.ones(B, dtype=torch.bool, device=dev)
    At = A_d.transpose(1, 2)

    def joint():
        return refine_util.refine_rgbd(fmap, (S, S), fcams, A_d, a_d, dstack, idx, [cam] * B, Rc, tc, rbd, red, feats, verts, ok, args.tau,
                                       depth_weight=args.depth_weight, iters=args.iters, max_points=args.max_points)

    def sequential():
        f = refine_util.refine_featuremetric(fmap, (S, S), fcams, Rf, tf, rbd, red, feats, verts, ok, iters=args.iters, max_points=args.max_points)
        R1, t1 = At @ f["R"], (At @ f["t"][:, :, None])[:, :, 0]              # back into the frame's camera (a = 0)
        return refine_util.refine_depth(dstack, idx, [cam] * B, R1, t1, rbd, red, verts, ok, args.tau, iters=args.iters, max_points=args.max_points)

    def timed(fn):
        for _ in range(args.warmup):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return out, ms

    ang = lambda A, Bm: np.degrees(np.arccos(np.clip((np.einsum("bij,bij->b", A, Bm) - 1) / 2, -1, 1)))
    med = lambda v: float(np.median(v))
    line = {"metric": "rgbd_refine", "batch": B, "points": P, "max_points": args.max_points, "channels": C, "map": [G, G], "depth": [H, W],
            "iters": args.iters, "tau_mm": args.tau, "depth_weight": args.depth_weight, "launches_joint": 6 + 2 * args.iters,
            "launches_sequential": 10 + 4 * args.iters}
    for name, fn in (("joint", joint), ("sequential", sequential)):
        out, ms = timed(fn)
        R, t = out["R"].cpu().numpy(), out["t"].cpu().numpy()
        st = out["status"].cpu().numpy()
        line.update({f"{name}_device_ms_median": med(ms), f"{name}_device_ms_min": float(min(ms)),
                     f"{name}_status_counts": {int(k): int((st == k).sum()) for k in (0, 1, 2)},
                     f"{name}_iters_used_median": med(out["iters_used"].cpu().numpy()),
                     f"{name}_rot_err_deg_median": med(ang(R, np.stack(Rg))),
                     f"{name}_trans_err_mm_median": med(np.linalg.norm(t - np.stack(tg), axis=1))})
    print(json.dumps(line))


if __name__ == "__main__":
    main()
