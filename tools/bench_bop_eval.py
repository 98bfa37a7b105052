"""The BOP19 evaluation (foundpose_amd.eval_bop19) at an LM-O-like shape, generated from a seed: 200 images of 640 x 480,
8 make_blob_mesh objects of 10-20k triangles, 7 objects (one GT instance each) and one estimate per target per image.

    python tools/bench_bop_eval.py [--out DIR] [--images 200] [--cpu-pairs 40] [--vsd-iters 20]

Reports: the wall time of evaluate_bop19 (csv, PNG decoding, rendering, VSD, MSSD / MSPD, matching); the device part alone
(HIP events around every render_views, fp_vsd_counts and fp_pose_errors call); fp_vsd_counts per pair (HIP events around
one call over every pair of a 32-image block, median of --vsd-iters); the numpy restatement (tests/vsd_ref.py) per pair on a
CPU subset, labelled as a CPU number.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="directory for the generated dataset (default: a temporary one)")
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--cpu-pairs", type=int, default=40)
    ap.add_argument("--vsd-iters", type=int, default=20)
    ap.add_argument("--json", default=None, help="also write the numbers here")
    args = ap.parse_args()
    import torch

    from foundpose_amd import eval_bop19 as eb, ops, synthetic
    from foundpose_amd.eval_bop19 import _Camera
    from foundpose_amd.renderer import HipRasterizer, load_ply
    from tests import vsd_ref
    assert torch.cuda.is_available(), "bench_bop_eval needs the MI355X"
    root = args.out or tempfile.mkdtemp(prefix="bop_eval_")
    t0 = time.perf_counter()
    meta = synthetic.make_bop_eval_scene(root, num_images=args.images, num_objects=8, width=640, height=480, mesh_res=90,
                                         gts_per_image=7, depth_scale=0.1, seed=2024)
    gen_s = time.perf_counter() - t0
    rng = np.random.default_rng(7)
    ests = []
    for im, inst in meta["images"]:
        for lid, T in inst:
            T2 = T.copy()
            a = rng.normal(size=3)
            a /= np.linalg.norm(a)
            ang = np.deg2rad(rng.uniform(0, 6))
            Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            T2[:3, :3] = (np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx) @ T[:3, :3]
            T2[:3, 3] += rng.normal(0, 0.04 * meta["diameters"][lid], 3)
            ests.append((1, im, lid, float(rng.uniform()), T2, 0.25))
    csv_path = os.path.join(root, "results.csv")
    synthetic.write_bop_results_csv(csv_path, ests)
    ntri = {lid: len(load_ply(os.path.join(meta["models_dir"], f"obj_{lid:06d}.ply")).faces) for lid in meta["diameters"]}

    eb.evaluate_bop19(csv_path, meta["split_dir"])          # warm-up: code objects, allocator, page cache
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores = eb.evaluate_bop19(csv_path, meta["split_dir"], timing=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev = scores["device_seconds"]

    # fp_vsd_counts alone: the pairs of the first 32 images (estimate vs its own GT), renders as the evaluator makes them
    ras = HipRasterizer("cuda")
    for lid in meta["diameters"]:
        ras.add_object_model(lid, mesh=load_ply(os.path.join(meta["models_dir"], f"obj_{lid:06d}.ply")))
    K, W, H = meta["K"], meta["width"], meta["height"]
    tests, de, dg, pairs, params, cpu_cases = [], [], [], [], [], []
    for n, (im, inst) in enumerate(meta["images"][:32]):
        tests.append(torch.from_numpy(eb.load_depth(os.path.join(meta["split_dir"], "000001", "depth", f"{im:06d}.png"), 0.1)))
        for lid, T in inst:
            Te = [e[4] for e in ests if e[1] == im and e[2] == lid][0]
            r = ras.render_views(lid, [_Camera(K, W, H, np.linalg.inv(Te)), _Camera(K, W, H, np.linalg.inv(T))], with_color=False)
            b = r["boxes"].cpu().numpy()
            x0, y0, x1, y1 = min(b[0, 0], b[1, 0]), min(b[0, 1], b[1, 1]), max(b[0, 2], b[1, 2]), max(b[0, 3], b[1, 3])
            if x0 > x1:
                x0, y0, x1, y1 = 0, 0, -1, -1
            pairs.append((n, len(de), len(dg), x0, y0, x1, y1))
            params.append((K[0, 0], K[1, 1], K[0, 2], K[1, 2], 15.0, meta["diameters"][lid]))
            de.append(r["depth"][0])
            dg.append(r["depth"][1])
    dt = torch.stack(tests).cuda()
    de, dg = torch.stack(de), torch.stack(dg)
    pairs, params = np.array(pairs), np.array(params)
    box_px = float(np.mean([(p[5] - p[3] + 1) * (p[6] - p[4] + 1) for p in pairs]))
    for _ in range(3):
        ops.vsd_counts(dt, de, dg, pairs, params, eb.VSD_TAUS)
    ts = []
    for _ in range(args.vsd_iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        counts = ops.vsd_counts(dt, de, dg, pairs, params, eb.VSD_TAUS)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / 1e3)
    vsd_call = float(np.median(ts))
    counts = counts.cpu().numpy()
    # the numpy restatement on a CPU subset, which must agree count for count
    m = min(args.cpu_pairs, len(pairs))
    dtn, den, dgn = dt.cpu().numpy(), de.cpu().numpy(), dg.cpu().numpy()
    t0 = time.perf_counter()
    ref = [vsd_ref.vsd_counts(dtn[p[0]], den[p[1]], dgn[p[2]], K, 15.0, q[5], eb.VSD_TAUS) for p, q in zip(pairs[:m], params[:m])]
    cpu_pair = (time.perf_counter() - t0) / m
    assert np.array_equal(np.stack(ref), counts[:m]), "fp_vsd_counts differs from the numpy restatement"

    res = {"images": args.images, "width": W, "height": H, "objects": len(ntri), "triangles": sorted(ntri.values()),
           "targets": scores["num_targets"], "estimates": scores["num_estimates_evaluated"], "gt_instances": scores["num_target_instances"],
           "dataset_generation_s": gen_s, "evaluate_bop19_wall_s": wall, "device_render_s": dev.get("render", 0.0),
           "device_vsd_s": dev.get("vsd", 0.0), "device_mssd_mspd_s": dev.get("mssd_mspd", 0.0),
           "device_total_s": sum(dev.values()), "vsd_call_pairs": len(pairs), "vsd_call_s": vsd_call,
           "vsd_us_per_pair": vsd_call / len(pairs) * 1e6, "mean_box_pixels": box_px,
           "vsd_gpix_per_s": box_px * len(pairs) / vsd_call / 1e9, "cpu_numpy_ms_per_pair": cpu_pair * 1e3, "cpu_pairs": m,
           "ar": scores["bop19_average_recall"], "ar_vsd": scores["bop19_average_recall_vsd"],
           "ar_mssd": scores["bop19_average_recall_mssd"], "ar_mspd": scores["bop19_average_recall_mspd"]}
    print(f"# python tools/bench_bop_eval.py (LM-O-like: {args.images} images {W}x{H}, {len(ntri)} objects of "
          f"{min(ntri.values())}-{max(ntri.values())} triangles, {res['estimates']} estimates, {res['gt_instances']} GT instances)")
    print(f"evaluate_bop19 wall                {wall:8.3f} s   (AR {res['ar']:.4f}: vsd {res['ar_vsd']:.4f} mssd {res['ar_mssd']:.4f} mspd {res['ar_mspd']:.4f})")
    print(f"device part (events)               {res['device_total_s']:8.3f} s   render {res['device_render_s']:.3f}  vsd {res['device_vsd_s']:.4f}  "
          f"mssd/mspd {res['device_mssd_mspd_s']:.4f}")
    print(f"fp_vsd_counts, {len(pairs)} pairs in one call  {vsd_call * 1e6:8.1f} us   {res['vsd_us_per_pair']:.2f} us/pair, mean box "
          f"{box_px:.0f} px, {res['vsd_gpix_per_s']:.1f} Gpixel/s")
    print(f"numpy restatement (CPU, {m} pairs)  {cpu_pair * 1e3:8.2f} ms/pair")
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
