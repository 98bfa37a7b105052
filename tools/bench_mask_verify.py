"""pnp_util.verify_poses_mask beside verify_poses_depth and fp_pnp_ransac: what the mask check of every hypothesis
costs next to the depth check and next to solving the hypotheses.  Both verifiers: tools/bench_pose_verify.py's scene -- 32 detections x 5
slots, 4 objects of 16 384 vertices, all of them sampled (stride 1), G = 64, 640 x 480 images; each detection's mask is a disc of its
object's projected size (radius 60 mm) around its projected centre.  fp_pnp_ransac: the correspondences of tools/bench_kabsch.py (32 x 5
pairs, K = 300, 1000 hypotheses, 50 % outliers).  HIP events around the Python calls, median of 20 launches after 3 warm-up launches, all
three in one process.  No pass bar.

    python tools/bench_mask_verify.py [--out profiles/mask_verify_bench.txt]
"""

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_kabsch import median_ms, scene  # noqa: E402
from bench_pose_verify import Samples, verify_scene  # noqa: E402
from foundpose_amd import pnp_util  # noqa: E402


def disc_masks(t, cam, H, W, radius_mm=60.0):
    """uint8 [B, H, W]: for each detection the pixels within the projected radius of the projected centre of its first slot's pose."""
    fx, fy, cx, cy = cam
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((len(t), H, W), np.uint8)
    for b, tb in enumerate(t[:, 0]):
        u, v, r = fx * tb[0] / tb[2] + cx, fy * tb[1] / tb[2] + cy, fx * radius_mm / tb[2]
        masks[b] = (xx - u) ** 2 + (yy - v) ** 2 <= r * r
    return masks


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "mask_verify_bench.txt"))
    args = ap.parse_args()
    dev = "cuda"
    B, n, G, max_points = 32, 5, 64, 16384
    cam = (600.0, 600.0, 319.5, 239.5)
    V, row_ranges, det_obj, R, t, depth = verify_scene(B, n)
    H, W = depth.shape[1:]
    samples = Samples(V, row_ranges, dev)
    sampled = [e - b for b, e in samples.verify_points(max_points).ranges]
    print("sampled points per object:", sampled)
    assert all(m == max_points for m in sampled), sampled   # the shape the report names is the shape that runs
    poses = {"success": torch.ones(B, n, dtype=torch.bool, device=dev), "R": torch.from_numpy(R).to(dev), "t": torch.from_numpy(t).to(dev)}
    dd = torch.from_numpy(depth).to(dev)
    mm = torch.from_numpy(disc_masks(t, cam, H, W)).to(dev)
    cams, idx = [cam] * B, list(range(B))
    msk = lambda: pnp_util.verify_poses_mask(poses, samples, det_obj, cams, cams, mm, max_points=max_points, grid=G)
    ver = lambda: pnp_util.verify_poses_depth(poses, samples, det_obj, cams, cams, dd, idx, 5.0, max_points=max_points, grid=G)
    K, iters = 300, 1000
    _, _, c2, c3 = scene(B, n, K, tau=5.0)
    c2d, c3d = torch.from_numpy(c2).to(dev), torch.from_numpy(c3).to(dev)
    counts = torch.full((B, n), K, dtype=torch.int32, device=dev)
    pnp = lambda: pnp_util.solve_pnp_ransac_batch(c2d, c3d, counts, cams, iters, 10.0, 0.99, True, 0)
    out_m, out_v, out_p = msk(), ver(), pnp()
    torch.cuda.synchronize()
    cnt = out_m["counts"].reshape(-1, 4).double().mean(0).tolist()
    tm, tv, tp = median_ms(msk), median_ms(ver), median_ms(pnp)
    lines = [f"both verifiers: {B} detections x {n} slots, {sampled[0]} sampled points per object, G = {G}, images {W} x {H}, masks: discs of "
             f"{float(mm.flatten(1).sum(1).double().mean()):.0f} pixels on average; fp_pnp_ransac: {B} x {n} pairs, K = {K}, {iters} hypotheses, 50 % outliers; "
             "HIP events around the Python call (uploads of the per-detection tables and the masks' area sums included), median of 20 [min, max], ms",
             "verify_poses_mask   %.3f [%.3f, %.3f]   scored %d / %d, mean counts (both, model only, mask only, cells) %s, mean score %.3f" % (
                 *tm, int((out_m["status"] == 0).sum()), B * n, [round(c, 1) for c in cnt], float(out_m["score"].mean())),
             "verify_poses_depth  %.3f [%.3f, %.3f]   scored %d / %d" % (*tv, int((out_v["status"] == 0).sum()), B * n),
             "fp_pnp_ransac       %.3f [%.3f, %.3f]   success %d / %d" % (*tp, int(out_p["success"].sum()), B * n),
             "mask / depth verification = %.3f, mask verification / fp_pnp_ransac = %.3f" % (tm[0] / tv[0], tm[0] / tp[0])]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
