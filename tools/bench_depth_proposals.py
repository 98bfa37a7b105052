"""depth_proposals.propose (mask proposals from depth) on synthetic table-top frames: the device time of each stage
(HIP events around the calls), the wall time of propose, and beside it the wall time of the numpy / scipy restatement on the same frames
-- the yardstick, because a new feature has no parent commit to compare with.

    python tools/bench_depth_proposals.py [--frames 32] [--scale 4] [--repeats 5] [--ref-frames 2] [--out profiles/depth_proposals_bench.txt]

The frames are tests/depth_proposals_ref.e2e_scene at `scale` times its 160 x 120 (scale 4: 640 x 480): a tilted plane, four spheres on
it, noise and a hole, one noise seed per frame, every other frame with a wall behind the plane.  One process; a warm-up call, then the
median of `repeats`; nothing here is a bar.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-frames", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from foundpose_amd import depth_proposals as dp, ops
    from tests import depth_proposals_ref as ref

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    frames = np.stack([ref.e2e_scene(wall=bool(f % 2), seed=100 + f, scale=a.scale)[0] for f in range(a.frames)])
    n, H, W = frames.shape
    cam = tuple(c * a.scale for c in ref.E2E_CAM)
    cams, keys = [cam] * n, [dp.frame_key(1, f) for f in range(n)]
    kw = dict(num_planes=2, min_pixels=12 * a.scale * a.scale)
    opts = dp.load_opts(kw)
    depth = torch.from_numpy(frames).cuda()
    say(f"depth_proposals bench: {n} frames of {W} x {H}, num_planes 2, {opts.plane_hypotheses} hypotheses at stride {opts.plane_stride}, one level; "
        f"device {torch.cuda.get_device_name(0)}")

    def timed(fn):
        """-> (result, device ms between two events, wall ms with a synchronisation at either end)."""
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return out, e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)

    def median(fn):
        fn()
        runs = [timed(fn) for _ in range(a.repeats)]
        return runs[-1][0], float(np.median([r[1] for r in runs])), float(np.median([r[2] for r in runs]))

    out, dev_all, wall_all = median(lambda: dp.propose(depth, cams, keys, opts))
    planes, num_planes = out["planes"], out["num_planes"]
    slope = (np.float64(opts.connect_slope) / np.array([cam[0]] * n)).astype(np.float32)
    zero = torch.zeros(n, dtype=torch.int32, device="cuda")
    stages = []
    _, d, w = median(lambda: ops.depth_plane_fit(depth, cams, keys, torch.zeros_like(planes), zero, opts.plane_hypotheses, opts.plane_stride,
                                                 opts.plane_thresh_mm, opts.max_depth_mm, opts.min_plane_share, opts.seed))
    stages.append(("fp_depth_plane_fit (one plane)", d, w))
    labels, d, w = median(lambda: ops.depth_components(depth, cams, slope, planes, num_planes, opts.max_depth_mm, opts.object_margin_mm, opts.levels()[0]))
    stages.append(("fp_depth_components", d, w))
    (table, counts, rank_map), d, w = median(lambda: ops.component_table(labels, opts.min_pixels, dp.max_area_of(opts, H, W), opts.max_proposals))
    stages.append(("fp_component_table", d, w))
    kept = counts[:, 2].contiguous()
    _, d, w = median(lambda: ops.component_runs(rank_map, kept, opts.max_proposals))
    stages.append(("fp_component_runs (two calls, the count read back, torch.sort)", d, w))
    say()
    say("| stage | device ms / batch | device us / frame | wall ms / batch |")
    say("|---|---|---|---|")
    for name, d, w in stages:
        say(f"| {name} | {d:.3f} | {1e3 * d / n:.1f} | {w:.3f} |")
    say(f"| propose, end to end (2 plane rounds) | {dev_all:.3f} | {1e3 * dev_all / n:.1f} | {wall_all:.3f} |")
    say()
    say(f"propose: {wall_all / n:.3f} ms wall per frame, {1e3 * n / wall_all:.0f} frames / s; planes accepted per frame: "
        f"{np.bincount(num_planes.cpu().numpy(), minlength=3).tolist()} frames with 0 / 1 / 2; proposals kept per frame: "
        f"{sorted(set(out['counts'][:, 0, 2].tolist()))}")
    say("(events around each Python call: a call uploads its frame table synchronously, so its interval holds that copy and the host's launch work)")

    # ---- the restatement on a few of the frames: numpy / scipy, one thread
    k = min(a.ref_frames, n)
    t0 = time.perf_counter()
    want = [ref.propose_frame(frames[f], cam, keys[f], ref.options(**kw)) for f in range(k)]
    t_ref = (time.perf_counter() - t0) / k
    t0 = time.perf_counter()
    on_device_planes = [ref.propose_frame(frames[f], cam, keys[f], ref.options(**kw), planes=list(planes[f, :int(num_planes[f])].cpu().numpy())) for f in range(k)]
    t_seg = (time.perf_counter() - t0) / k
    same = sum(np.array_equal(w_["levels"][0]["rank_map"], out["rank_maps"][f, 0].cpu().numpy()) for f, w_ in enumerate(on_device_planes))
    same_planes = sum(len(w_["planes"]) == int(num_planes[f]) for f, w_ in enumerate(want))
    say(f"numpy / scipy restatement (tests/depth_proposals_ref.py, one thread): {1e3 * t_ref:.0f} ms / frame with the planes, {1e3 * t_seg:.0f} ms / frame "
        f"on given planes, over {k} frames: {t_ref * 1e3 / (wall_all / n):.0f}x propose's wall time per frame; {same} of {k} rank maps equal the "
        f"device's on its planes, {same_planes} of {k} frames accept the same number of planes")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
