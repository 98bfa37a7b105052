"""fp_pts_diameter and fp_directed_hausdorff (csrc/point_extremes.hip: the diameter and the symmetry candidates of models_info.py, brute force in
fp64) at V = 4 096, 30 000 and 100 000 vertices on the device, beside fp_pose_add_errors at the same V with 32 pairs in the same run, and the
host yardsticks on this machine's CPU: scipy.spatial.distance.pdist for the diameter where its V (V - 1) / 2 doubles fit (V <= 30 000), and
scipy.spatial.cKDTree (one build, one query per transform, one thread) for the Hausdorff pass.

    python tools/bench_models_info.py [--iters 20] [--no-cpu] [--sizes 4096 30000 100000] [--out profiles/models_info_bench.txt]

Device time: HIP events around one call, the median of --iters calls after 3 warm-up calls, one process.  Point pairs: V (V - 1) / 2 for the
diameter (the kernel evaluates whole 1 024 x 1 024 tile pairs a <= b: `evaluated` counts those), K x V x V for the Hausdorff pass at stride 1,
pairs x V x V for ADD / ADI.  FP64 share: 9 fp64 VALU operations per evaluated point pair over the FP64 vector issue rate 78.6 TFLOP/s / 2, as
tools/bench_pose_add.py.  The Hausdorff pass runs at K = 32 and at the tool's full candidate count (26 axes x 63 angle fractions x 2
directions = 3 276 at the default options for a model with three distinct principal moments, as the one here); the tree is timed on 32
transforms and its time at the full count is that, scaled (marked ~).
The last block times the tool's own symmetry search (object_symmetries with the device evaluation, host logic included, wall clock of one run
after one warm-up) on the same point set -- an ellipsoid with a rod, no symmetry -- with and without the prefilter, and how many of the
candidates the first pass rejected by its lower bound.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

OPS_PER_PAIR = 9
FP64_ISSUE_PEAK = 78.6e12 / 2
TILE = 1024


def _model(rng, V):
    """A model-like point set without a symmetry: V points on an ellipsoid of half axes (60, 40, 25) mm, one in twenty of them moved onto a rod
    of 3 mm noise from the centre to (90, 60, 50), at random indices.  (A Gaussian blob would do for the rates, but not for the tool: its
    sparse tail decides its Hausdorff distances and every stride-th vertex misses it, so the first pass rejects nothing.)"""
    u = rng.normal(size=(V, 3))
    pts = u / np.linalg.norm(u, axis=1, keepdims=True) * np.array([60.0, 40.0, 25.0])
    rod = rng.permutation(V)[:V // 20]
    pts[rod] = rng.uniform(size=(len(rod), 1)) * np.array([90.0, 60.0, 50.0]) + rng.normal(0, 3, (len(rod), 3))
    return pts


def _timed(fn, iters):
    import torch
    for _ in range(3):
        out = fn()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        st.record()
        out = fn()
        en.record()
        en.synchronize()
        ts.append(st.elapsed_time(en) * 1e3)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 30000, 100000])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "models_info_bench.txt"))
    args = ap.parse_args()
    import torch
    from foundpose_amd import models_info as mi, ops
    assert torch.cuda.is_available(), "bench_models_info measures the MI355X"
    rng = np.random.default_rng(0)
    lines = [f"# python tools/bench_models_info.py on one {torch.cuda.get_device_name(0)} (device: HIP events around one call, median of {args.iters} after 3 "
             "warm-up calls; host: scipy on one thread)",
             f"{'call':<22}{'V':>8}{'K':>6}{'device us/call':>16}{'G point pairs/s':>17}{'G evaluated/s':>15}{'fp64 share':>12}{'host s/call':>14}{'host / device':>15}"]
    print("\n".join(lines), flush=True)

    def row(name, V, K, us, pairs, evaluated, host, approx=False):
        line = (f"{name:<22}{V:>8}{K:>6}{us:>16.1f}{pairs / (us * 1e-6) / 1e9:>17.1f}{evaluated / (us * 1e-6) / 1e9:>15.1f}"
                f"{OPS_PER_PAIR * evaluated / (us * 1e-6) / FP64_ISSUE_PEAK:>12.1%}"
                + (f"{('~' if approx else '') + format(host, '.4f'):>14}{host / (us * 1e-6):>15.1f}" if host is not None else f"{'-':>14}{'-':>15}"))
        print(line, flush=True)
        lines.append(line)

    tool = []
    for V in args.sizes:
        pts = _model(rng, V)
        d_pts = torch.from_numpy(pts).cuda()
        # ---- the diameter
        us, (d, pair) = _timed(lambda: ops.pts_diameter(d_pts), args.iters)
        d = float(d.cpu()[0])
        host = None
        if not args.no_cpu and V <= 30000:
            from scipy.spatial.distance import pdist
            t0 = time.perf_counter()
            want = pdist(pts).max()
            host = time.perf_counter() - t0
            assert abs(d - want) <= 1e-9 * want, "pdist and the device disagree"
        tiles = (V + TILE - 1) // TILE
        row("pts_diameter", V, 1, us, V * (V - 1) / 2, tiles * (tiles + 1) / 2 * TILE * TILE, host)
        # ---- the Hausdorff pass: the tool's own candidates (rotations about its axes through the centre), both directions
        c, axes, fracs = mi.symmetry_centre(pts, None), mi.candidate_axes(pts), mi.angle_fractions(12, 36)
        tfs = np.array([mi.transform12(mi.rotation_about(f, a), c) for a in axes for f in fracs] +
                       [mi.transform12(mi.rotation_about(1 - f, a), c) for a in axes for f in fracs])
        tree_per = None
        for K in (32, len(tfs)):
            sub = tfs[:K] if K == len(tfs) else tfs[rng.permutation(len(tfs))[:K]]
            d_tf = torch.from_numpy(np.ascontiguousarray(sub)).cuda()
            us, (h, arg) = _timed(lambda: ops.directed_hausdorff(d_pts, d_tf, 1), args.iters if K == 32 or V < 100000 else max(3, args.iters // 4))
            host = None
            if not args.no_cpu:
                if K == 32:
                    from scipy.spatial import cKDTree
                    t0 = time.perf_counter()
                    tree = cKDTree(pts)
                    th = [tree.query(pts @ t[:9].reshape(3, 3).T + t[9:], k=1)[0].max() for t in sub]
                    host = time.perf_counter() - t0
                    tree_per = host / 32
                    assert np.all(np.abs(np.array(th) - h.cpu().numpy()) <= 1e-9 * np.array(th)), "the tree and the device disagree"
                else:
                    host = tree_per * K
            row("directed_hausdorff", V, K, us, K * float(V) * V, K * float(V) * (tiles * TILE), host, approx=K != 32)
        # ---- ADD / ADI at the same V, 32 pairs, in the same run
        pose = np.concatenate([np.eye(3).ravel(), [5.0, -3.0, 700.0]])
        est = np.stack([np.concatenate([mi.rotation_about(0.01 * (k + 1), [1.0, 2.0, 3.0]).ravel(), pose[9:] + rng.normal(0, 5, 3)]) for k in range(32)])
        d_est, d_gt = torch.from_numpy(est).cuda(), torch.from_numpy(np.tile(pose, (32, 1))).cuda()
        ranges = np.array([(0, V)] * 32, np.int64)
        us, _ = _timed(lambda: ops.pose_add_errors(d_pts, d_est, d_gt, ranges), args.iters)
        row("pose_add_errors", V, 32, us, 32 * float(V) * V, 32 * float(V) * (tiles * TILE), None)
        # ---- the tool's search on these points
        for prefilter in (True, False):
            if not prefilter and V >= 100000:
                continue   # the full-count row above is this pass
            ev = mi.device_evaluator(d_pts)
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                disc, cont, rep = mi.object_symmetries(pts, None, d, ev, prefilter=prefilter)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
            bound = sum(c["lower_bound"] for ax in rep["axes"] for c in ax["candidates"])
            tool.append(f"{V:>8}{len(rep['axes']):>6}{len(rep['axes']) * len(fracs):>12}{rep['query_stride']:>8}{bound:>10}{wall:>10.3f}{len(disc):>10}{len(cont):>12}")
    lines.append("# the tool's symmetry search on the same points (object_symmetries, device evaluation, host logic included; wall clock of the second run; "
                 "a candidate is a rotation, evaluated in both directions)")
    lines.append(f"{'V':>8}{'axes':>6}{'candidates':>12}{'stride':>8}{'by bound':>10}{'wall s':>10}{'discrete':>10}{'continuous':>12}")
    lines += tool
    lines.append(f"# fp64 share: {OPS_PER_PAIR} fp64 VALU operations per evaluated point pair / time over {FP64_ISSUE_PEAK / 1e12:.1f} T lane-operations/s; "
                 "device times include the fold kernels (and pose_add's table upload).")
    print("\n".join(lines[-(len(tool) + 3):]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
