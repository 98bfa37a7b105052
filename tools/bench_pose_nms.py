"""The two launches of pose_nms.suppress_duplicates beside pnp_util.verify_poses_mask, for scale.  Duplicate
suppression: 32 frames x 16 poses of 8 objects (every object twice in every frame: a pose and a copy of it moved by a few mm), bumpy
spheres of radius about 60 mm with 4096 sampled points each (stride 1), G = 16, same-object pairs only: 512 ordered pairs, 32 frames.
Timed: pose_overlaps + nms_greedy (the one upload of the tables and the two launches, nothing read back), and suppress_duplicates as a
whole (the same plus the read-back and the host's bookkeeping).  verify_poses_mask: tools/bench_mask_verify.py's shape (32 detections x
5 slots, 16 384 points, G = 64, 640 x 480).  HIP events around the Python calls, median of 20 after 3 warm-up calls, all in one process.
No pass bar.

    python tools/bench_pose_nms.py [--out profiles/pose_nms_bench.txt]
"""

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_kabsch import median_ms, rot  # noqa: E402
from bench_mask_verify import disc_masks  # noqa: E402
from bench_pose_verify import Samples, verify_scene  # noqa: E402
from foundpose_amd import pnp_util, pose_nms  # noqa: E402


def nms_scene(frames=32, objects=8, verts=4096, seed=0):
    """-> vertices {obj_id: [verts, 3]}, rows: per frame every object twice, the second pose the first moved by N(0, 4 mm) per axis."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(objects, verts, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    V = (d * (60.0 + 15.0 * np.sin(3.0 * d[..., :1]) * np.cos(2.0 * d[..., 1:2]))).astype(np.float32)
    rows = []
    for f in range(frames):
        for o in range(objects):
            R0, t0 = rot(rng), np.array([rng.uniform(-300, 300), rng.uniform(-200, 200), rng.uniform(700, 900)])
            for k in range(2):
                rows.append(dict(scene_id=1, im_id=f, obj_id=o + 1, score=float(rng.random()), R=R0, t=t0 + k * rng.normal(0.0, 4.0, 3), time=0.0))
    return {o + 1: V[o] for o in range(objects)}, rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "pose_nms_bench.txt"))
    args = ap.parse_args()
    dev = "cuda"
    F, O, M, G, thr = 32, 8, 4096, 16, 0.3
    verts, rows = nms_scene(F, O, M)
    samples = pose_nms.samples_from_vertices(verts, M, dev)
    vp, lid_to_obj = samples
    assert all(e - b == M for b, e in vp.ranges)   # the shape the report names is the shape that runs
    order, group_off = pose_nms.rank_layout(rows)
    obj = np.asarray([lid_to_obj[rows[i]["obj_id"]] for i in order], np.int32)
    R, t = np.stack([rows[i]["R"] for i in order]), np.stack([rows[i]["t"] for i in order])
    pairs, pair_off = pose_nms.frame_pairs(group_off, obj)
    valid = np.ones(len(rows), np.int32)

    def two_launches():
        ov = pose_nms.pose_overlaps(vp.points, vp.ranges, vp.centers, vp.radii, obj, valid, R, t, pairs, G)
        return ov, pose_nms.nms_greedy(group_off, pair_off, pairs, ov["overlap"], ov["status"], thr)
    whole = lambda: pose_nms.suppress_duplicates(rows, samples, thr, G)
    ov, kept = two_launches()
    res = whole()
    torch.cuda.synchronize()
    assert np.array_equal(kept["keep"].cpu().numpy().astype(bool)[np.argsort(order)], res["keep"])

    # for scale: verify_poses_mask at its own bench shape
    B, n, Gm, mp = 32, 5, 64, 16384
    cam = (600.0, 600.0, 319.5, 239.5)
    Vm, row_ranges, det_obj, Rm, tm, depth = verify_scene(B, n)
    H, W = depth.shape[1:]
    msamples = Samples(Vm, row_ranges, dev)
    poses = {"success": torch.ones(B, n, dtype=torch.bool, device=dev), "R": torch.from_numpy(Rm).to(dev), "t": torch.from_numpy(tm).to(dev)}
    mm = torch.from_numpy(disc_masks(tm, cam, H, W)).to(dev)
    cams = [cam] * B
    msk = lambda: pnp_util.verify_poses_mask(poses, msamples, det_obj, cams, cams, mm, max_points=mp, grid=Gm)
    msk()
    torch.cuda.synchronize()
    t2, tw, tmk = median_ms(two_launches), median_ms(whole), median_ms(msk)
    st = ov["status"].cpu().numpy()
    lines = [f"duplicate suppression: {F} frames x {len(rows) // F} poses of {O} objects, {M} sampled points per object, G = {G}, thresh = {thr}, same-object "
             f"pairs: {len(pairs)} ordered pairs ({int((st == 0).sum())} scored, {int((st == 1).sum())} disjoint spheres); verify_poses_mask: {B} detections x {n} "
             f"slots, {mp} sampled points per object, G = {Gm}, images {W} x {H}; HIP events around the Python calls (the uploads of the tables included), "
             "median of 20 [min, max], ms; one run on one device",
             "pose_overlaps + nms_greedy   %.3f [%.3f, %.3f]   kept %d / %d poses, mean overlap of the scored pairs %.3f" % (
                 *t2, int(res["keep"].sum()), len(rows), float(ov["overlap"].cpu().numpy()[st == 0].mean())),
             "suppress_duplicates          %.3f [%.3f, %.3f]   (the same, the read-back and the host's bookkeeping)" % tw,
             "verify_poses_mask            %.3f [%.3f, %.3f]" % tmk,
             "two launches / verify_poses_mask = %.3f" % (t2[0] / tmk[0])]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
