"""fp_multiview_refine (csrc/multiview.hip) on the device: one ops.multiview_refine call for 64 clusters x 32 views x
64 points at 20 iterations, the ops.pose_errors time of the clustering of the same scene, and the numpy restatement
(tests/multiview_ref.py) of one of the clusters on one CPU thread -- which is all it is compared with.  Nothing here is a bar.

    python tools/bench_multiview.py [--iters 10] [--no-cpu] [--out profiles/multiview_bench.txt]

The scene: 32 cameras on a ring of radius 800 mm, 64 objects of 64 points drawn from N(0, 30^2 mm^2) at random world poses; every view's
estimate of every object is pushed 2 .. 5 % of its distance along its own ray, plus 1 mm and 0.5 degrees of noise (the planted ring of
tests/multiview_ref.py).  Device time: HIP events (tools/bench_reconstruct._timed) around one call -- its launches, its validation
read-back and the allocation of its outputs --, the median of --iters calls after 2 warm-up calls, one process."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_reconstruct import _timed   # noqa: E402

CLUSTERS, VIEWS, POINTS, LM_ITERS = 64, 32, 64, 20


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "multiview_bench.txt"))
    args = ap.parse_args()
    import torch
    from foundpose_amd import multiview, ops
    from tests import multiview_ref as mv
    assert torch.cuda.is_available(), "bench_multiview measures the MI355X"
    rng = np.random.default_rng(0)
    cams = mv.ring_cameras(VIEWS)
    model = mv.cloud_model(rng, POINTS)
    X = mv.sample(model.pts, POINTS)
    cam = np.array([[600.0, 600.0, 160.0, 120.0]] * VIEWS)
    Tv = [mv.w2c(e) for e in cams.values()]
    view_T = np.stack([np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]) for T in Tv])
    Y, uv, vi, R0, t0, pairs = [], [], [], [], [], []
    for c in range(CLUSTERS):
        Wt = mv.random_pose(rng, 60.0)
        seed = None
        for v in range(VIEWS):
            est = mv.ray_noise(rng, Tv[v] @ Wt)
            Xc = X @ est[:3, :3].T + est[:3, 3]
            Y.append(X)
            uv.append(np.stack([cam[v, 0] * Xc[:, 0] / Xc[:, 2] + cam[v, 2], cam[v, 1] * Xc[:, 1] / Xc[:, 2] + cam[v, 3]], 1))
            vi.append(np.full(POINTS, v))
            W = np.linalg.inv(Tv[v]) @ est
            if seed is None:
                seed = W
            else:
                pairs.append((W, seed, 0))
        R0.append(seed[:3, :3])
        t0.append(seed[:3, 3])
    dev = "cuda"
    rows = VIEWS * POINTS
    a = dict(points=torch.from_numpy(np.concatenate(Y).astype(np.float32)).to(dev), targets=torch.from_numpy(np.concatenate(uv)).to(dev),
             view_index=torch.from_numpy(np.concatenate(vi).astype(np.int32)).to(dev), view_cam=torch.from_numpy(cam).to(dev),
             view_T=torch.from_numpy(view_T).to(dev), row_begin=torch.arange(CLUSTERS, dtype=torch.int32, device=dev) * rows,
             row_end=(torch.arange(CLUSTERS, dtype=torch.int32, device=dev) + 1) * rows, R=torch.from_numpy(np.stack(R0)).to(dev),
             t=torch.from_numpy(np.stack(t0)).to(dev))
    ms, out = _timed(lambda: ops.multiview_refine(**a, huber_px=10.0, iters=LM_ITERS), args.iters)
    used, st = out["iters_used"].cpu().numpy(), out["status"].cpu().numpy()
    cin, cout = out["cost_in"].cpu().numpy(), out["cost_out"].cpu().numpy()
    lines = [f"# python tools/bench_multiview.py on one {torch.cuda.get_device_name(0)} (device: HIP events around one call, median of {args.iters} after 2 "
             f"warm-up calls).  Nothing here is a bar.",
             f"ops.multiview_refine, {CLUSTERS} clusters x {VIEWS} views x {POINTS} points = {CLUSTERS * rows} rows, {LM_ITERS} iterations = "
             f"{2 * (1 + LM_ITERS) + 2} launches of up to {CLUSTERS * rows // 32} workgroups: {ms:7.3f} ms per call   (iterations used {used.min()} .. {used.max()}, "
             f"status 0 for {int((st == 0).sum())} of {CLUSTERS}, mean cost {cin.mean():.2f} -> {cout.mean():.2f} px^2)"]
    samples, stacks = [X], [multiview._sym_stack(model.syms)]
    ms_d, _ = _timed(lambda: multiview.seed_distances(pairs, samples, stacks, dev), args.iters)
    lines.append(f"the clustering's distances, multiview.seed_distances -> ops.pose_errors, {len(pairs)} (candidate, seed) pairs x {POINTS} points x 1 symmetry, "
                 f"host tables and read-back included: {ms_d:7.3f} ms per call")
    if not args.no_cpu:
        torch.set_num_threads(1)
        t = time.perf_counter()
        ref = mv.refine(R0[0], t0[0], np.concatenate(Y[:VIEWS]), np.concatenate(uv[:VIEWS]), np.concatenate(vi[:VIEWS]), cam, view_T, 10.0, LM_ITERS)
        cpu = time.perf_counter() - t
        dt = float(np.linalg.norm(ref["t"] - out["t"][0].cpu().numpy()))
        lines.append(f"tests/multiview_ref.refine, ONE cluster of {rows} rows on one CPU thread (numpy fp64): {cpu * 1e3:7.1f} ms ({ref['iters_used']} iterations; "
                     f"x {CLUSTERS} clusters = {cpu * CLUSTERS * 1e3:7.1f} ms); its pose lies {dt:.2e} mm from the device's")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
