"""pnp_util.verify_poses_depth beside fp_pnp_ransac: what share of the coarse stage the depth check of every
hypothesis adds.  Verification: 32 detections x 5 slots, 4 objects of 16 384 vertices, all of them sampled (stride 1), G = 64, 640 x 480
depth; fp_pnp_ransac: the correspondences of tools/bench_kabsch.py (32 x 5 pairs, K = 300, 1000 hypotheses, 50 % outliers).  HIP events
around the Python calls, median of 20 launches after 3 warm-up launches.  No pass bar.

    python tools/bench_pose_verify.py [--out profiles/pose_verify_bench.txt]
"""

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_kabsch import median_ms, rot, scene  # noqa: E402
from foundpose_amd import bank as fb, pnp_util  # noqa: E402


class Samples:
    """What verify_poses_depth asks of a bank: verify_points(max_points), built by the bank's own host functions."""

    def __init__(self, vertices, row_ranges, device):
        self.vertices, self.row_ranges, self.device, self.cache = vertices, row_ranges, device, {}

    def verify_points(self, max_points):
        if max_points not in self.cache:
            pts, ranges = fb.sample_verify_points(self.vertices, self.row_ranges, max_points)
            self.cache[max_points] = fb.VerifyPoints(pts.to(self.device), ranges, *fb.sample_spheres(pts, ranges))
        return self.cache[max_points]


def verify_scene(B=32, n=5, objects=4, verts=16384, H=480, W=640, seed=0):
    """Bumpy spheres of radius about 60 mm at 700 .. 900 mm; every detection's own depth image is a plane through its object's centre, so
    the visible points split into confirmed, occluded and free ones; the slots of a detection are small perturbations of one pose."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(objects, verts, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    V = (d * (60.0 + 15.0 * np.sin(3.0 * d[..., :1]) * np.cos(2.0 * d[..., 1:2]))).astype(np.float32).reshape(-1, 3)
    R, t = np.zeros((B, n, 3, 3)), np.zeros((B, n, 3))
    depth = np.zeros((B, H, W), np.float32)
    for b in range(B):
        R0, t0 = rot(rng), np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(700, 900)])
        depth[b] = t0[2]
        for j in range(n):
            R[b, j], t[b, j] = R0, t0 + rng.normal(0.0, 4.0, 3)
    return torch.from_numpy(V), [(o * verts, (o + 1) * verts) for o in range(objects)], [b % objects for b in range(B)], R, t, depth


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "pose_verify_bench.txt"))
    args = ap.parse_args()
    dev = "cuda"
    B, n, G, max_points = 32, 5, 64, 16384
    cam = (600.0, 600.0, 319.5, 239.5)
    V, row_ranges, det_obj, R, t, depth = verify_scene(B, n)
    samples = Samples(V, row_ranges, dev)
    sampled = [e - b for b, e in samples.verify_points(max_points).ranges]
    print("sampled points per object:", sampled)
    assert all(m == max_points for m in sampled), sampled   # the shape the report names is the shape that runs
    poses = {"success": torch.ones(B, n, dtype=torch.bool, device=dev), "R": torch.from_numpy(R).to(dev), "t": torch.from_numpy(t).to(dev)}
    dd = torch.from_numpy(depth).to(dev)
    cams, idx = [cam] * B, list(range(B))
    ver = lambda: pnp_util.verify_poses_depth(poses, samples, det_obj, cams, cams, dd, idx, 5.0, max_points=max_points, grid=G)
    K, iters = 300, 1000
    _, _, c2, c3 = scene(B, n, K, tau=5.0)
    c2d, c3d = torch.from_numpy(c2).to(dev), torch.from_numpy(c3).to(dev)
    counts = torch.full((B, n), K, dtype=torch.int32, device=dev)
    pnp = lambda: pnp_util.solve_pnp_ransac_batch(c2d, c3d, counts, cams, iters, 10.0, 0.99, True, 0)
    out_v, out_p = ver(), pnp()
    torch.cuda.synchronize()
    cnt = out_v["counts"].reshape(-1, 6).double().mean(0).tolist()
    tv, tp = median_ms(ver), median_ms(pnp)
    lines = [f"verification: {B} detections x {n} slots, {sampled[0]} sampled points per object, G = {G}, depth {depth.shape[2]} x {depth.shape[1]}; "
             f"fp_pnp_ransac: {B} x {n} pairs, K = {K}, {iters} hypotheses, 50 % outliers; "
             "HIP events around the Python call (uploads of the per-detection tables included), median of 20 [min, max], ms",
             "verify_poses_depth  %.3f [%.3f, %.3f]   scored %d / %d, mean counts (vis, in, occ, free, hole, out) %s" % (
                 *tv, int((out_v["status"] == 0).sum()), B * n, [round(c, 1) for c in cnt]),
             "fp_pnp_ransac       %.3f [%.3f, %.3f]   success %d / %d" % (*tp, int(out_p["success"].sum()), B * n),
             "verification / fp_pnp_ransac = %.3f" % (tv[0] / tp[0])]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
