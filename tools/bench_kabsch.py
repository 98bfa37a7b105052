"""fp_kabsch_ransac against fp_pnp_ransac on the same correspondences: batch 32 detections x 5 slots, K = 300,
1000 hypotheses, 640 x 480 depth, 50 % outliers; HIP events, median of 20 launches after 3 warm-up launches.  No pass bar.

    python tools/bench_kabsch.py [--out profiles/kabsch_bench.txt]
"""

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from foundpose_amd import pnp_util  # noqa: E402


def rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def scene(B=32, n=5, K=300, H=480, W=640, outliers=0.5, tau=5.0, seed=0):
    """Every pair: K model points at a planted pose in front of the frame camera (solve camera = frame camera); its depth image receives
    each point's z at the nearest pixel, half of the points displaced by 6 .. 20 tau (3D outliers) and their pixels by 15 .. 60 px."""
    rng = np.random.default_rng(seed)
    cam = (600.0, 600.0, 319.5, 239.5)
    depth = np.zeros((B, H, W), np.float32)
    c2, c3 = np.zeros((B, n, K, 2), np.float32), np.zeros((B, n, K, 3), np.float32)
    for b in range(B):
        for j in range(n):
            R, t = rot(rng), np.array([rng.uniform(-60, 60), rng.uniform(-40, 40), rng.uniform(700, 900)])
            X = rng.uniform(-80, 80, (K, 3))
            Y = X @ R.T + t
            uv = np.stack([cam[0] * Y[:, 0] / Y[:, 2] + cam[2], cam[1] * Y[:, 1] / Y[:, 2] + cam[3]], 1)
            bad = rng.permutation(K)[:int(outliers * K)]
            uv[bad] += rng.uniform(15, 60, (len(bad), 2)) * rng.choice([-1.0, 1.0], (len(bad), 2))
            z = Y[:, 2].copy()
            z[bad] += rng.uniform(6, 20, len(bad)) * tau * rng.choice([-1.0, 1.0], len(bad))
            px, py = np.clip(np.rint(uv[:, 0]).astype(int), 0, W - 1), np.clip(np.rint(uv[:, 1]).astype(int), 0, H - 1)
            depth[b, py, px] = z
            c2[b, j], c3[b, j] = uv, X
    return cam, depth, c2, c3


def median_ms(fn, reps=20, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "kabsch_bench.txt"))
    args = ap.parse_args()
    B, n, K, iters, tau = 32, 5, 300, 1000, 5.0
    cam, depth, c2, c3 = scene(B, n, K, tau=tau)
    dev = "cuda"
    c2d, c3d, dd = torch.from_numpy(c2).to(dev), torch.from_numpy(c3).to(dev), torch.from_numpy(depth).to(dev)
    counts = torch.full((B, n), K, dtype=torch.int32, device=dev)
    cams = [cam] * B
    idx = list(range(B))
    kab = lambda: pnp_util.solve_kabsch_ransac_batch(c2d, c3d, counts, cams, cams, dd, idx, tau, iters, 0.99, True, 0)
    pnp = lambda: pnp_util.solve_pnp_ransac_batch(c2d, c3d, counts, cams, iters, 10.0, 0.99, True, 0)
    ok_k, ok_p = kab(), pnp()
    torch.cuda.synchronize()
    lines = [f"shape: {B} detections x {n} slots, K = {K}, {iters} hypotheses, depth {depth.shape[2]} x {depth.shape[1]}, 50 % outliers; "
             "HIP events around the Python call (uploads of the per-detection tables included), median of 20 [min, max], ms",
             "fp_kabsch_ransac  %.3f [%.3f, %.3f]   success %d / %d, mean inliers %.1f" % (*median_ms(kab), int(ok_k["success"].sum()), B * n, float(ok_k["quality"].mean())),
             "fp_pnp_ransac     %.3f [%.3f, %.3f]   success %d / %d, mean inliers %.1f" % (*median_ms(pnp), int(ok_p["success"].sum()), B * n, float(ok_p["quality"].mean()))]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
