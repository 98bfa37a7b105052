"""fp_pose_add_errors (ADD + ADI of a batch of (estimate, GT) pairs, brute-force nearest neighbours in fp64) at M = 4 096 and 30 000 points,
batches 1 and 32, on the device; and the host yardstick, scipy.spatial.cKDTree build + query of the same pairs on this machine's CPU.

    python tools/bench_pose_add.py [--iters 20] [--no-cpu] [--out profiles/pose_add_bench.txt]

Device time: HIP events around one call (the table upload and both kernels, pose_add_nn and pose_add_fold), the median of --iters calls after
3 warm-up calls, one process.  FP64 share: 9 fp64 VALU operations per (query, point) pair (3 subtractions, 3 products, 2 sums, 1 minimum:
the inner loop of pose_add_nn in its gfx950 ISA) x M^2 x pairs / time, over the FP64 vector issue rate 78.6 TFLOP/s / 2 (an FMA counts two
FLOPs, the peak is one FMA per lane-cycle), as tools/bench_pose_eval.py reports it.  The tree's mean and the device's ADI are compared
(1e-9 relative) at every shape, so the two columns time the same quantity.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (4096, 30000)
BATCHES = (1, 32)
OPS_PER_PAIR = 9
FP64_ISSUE_PEAK = 78.6e12 / 2


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "pose_add_bench.txt"))
    args = ap.parse_args()
    import torch
    from foundpose_amd import ops
    assert torch.cuda.is_available(), "bench_pose_add measures the MI355X"
    rng = np.random.default_rng(0)
    lines = [f"# python tools/bench_pose_add.py on one {torch.cuda.get_device_name(0)} (device: HIP events around one fp_pose_add_errors call, median of "
             f"{args.iters} after 3 warm-up calls; cKDTree: build + query per pair on the host CPU, one thread, scipy's defaults)",
             f"{'M':>7}{'pairs':>7}{'device us/call':>16}{'us/pair':>12}{'G point pairs/s':>17}{'fp64 share':>12}{'cKDTree s/call':>16}{'tree / device':>15}"]
    print("\n".join(lines), flush=True)
    for M in SIZES:
        pts = rng.normal(0, 40, (M, 3))
        for H in BATCHES:
            Rg, tg = _rot(rng), np.array([5.0, -3.0, 700.0])
            gt = np.tile(np.concatenate([Rg.ravel(), tg]), (H, 1))
            est = np.stack([np.concatenate([(_rot(rng) if h % 2 else Rg).ravel(), tg + rng.normal(0, 5, 3)]) for h in range(H)])
            d_pts, d_est, d_gt = (torch.from_numpy(a).cuda() for a in (pts, est, gt))
            ranges = np.array([(0, M)] * H, np.int64)
            for _ in range(3):
                err = ops.pose_add_errors(d_pts, d_est, d_gt, ranges)
            torch.cuda.synchronize()
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ts = []
            for _ in range(args.iters):
                st.record()
                err = ops.pose_add_errors(d_pts, d_est, d_gt, ranges)
                en.record()
                en.synchronize()
                ts.append(st.elapsed_time(en) * 1e3)
            us = float(np.median(ts))
            err = err.cpu().numpy()
            cpu = None
            if not args.no_cpu:
                from scipy.spatial import cKDTree
                t0 = time.perf_counter()
                tree_adi = []
                for h in range(H):
                    E = pts @ est[h, :9].reshape(3, 3).T + est[h, 9:]
                    G = pts @ gt[h, :9].reshape(3, 3).T + gt[h, 9:]
                    tree_adi.append(cKDTree(E).query(G, k=1)[0].mean())
                cpu = time.perf_counter() - t0
                assert np.all(np.abs(np.array(tree_adi) - err[:, 1]) <= 1e-9 * np.array(tree_adi)), "the tree and the device disagree"
            rate = H * float(M) * M / (us * 1e-6)
            line = (f"{M:>7}{H:>7}{us:>16.1f}{us / H:>12.1f}{rate / 1e9:>17.1f}{OPS_PER_PAIR * rate / FP64_ISSUE_PEAK:>12.1%}"
                    + (f"{cpu:>16.4f}{cpu / (us * 1e-6):>15.1f}" if cpu is not None else f"{'':>16}{'':>15}"))
            print(line, flush=True)
            lines.append(line)
    lines.append(f"# fp64 share: {OPS_PER_PAIR} fp64 VALU operations per (query, point) pair x M^2 x pairs / time over {FP64_ISSUE_PEAK / 1e12:.1f} T "
                 "lane-operations/s; the device time includes the fold kernel and the table upload.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(lines[-1])


if __name__ == "__main__":
    main()
