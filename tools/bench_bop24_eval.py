"""The BOP24 6D detection evaluation (foundpose_amd.eval_bop24) at the LM-O-like volume of tools/bench_bop_eval.py,
generated from a seed: 200 images of 640 x 480, 8 make_blob_mesh objects, 7 objects per image (one GT instance each) and TEN estimates per
GT instance -- the GT pose perturbed by a growing amount, scores from the seed -- so that the precision-recall curve is not trivial.

    python tools/bench_bop24_eval.py [--out DIR] [--images 200] [--per-gt 10] [--iters 20] [--json FILE]

Reports: the wall time of evaluate_bop24 (csv, annotations, models, MSSD / MSPD, matching, AP); its device part by HIP events around
every fp_pose_errors call and around the matching and the AP call (uploads included); the two launches fp_detection_match +
fp_detection_ap alone on tables already on the device (HIP events, median of --iters); and the numpy restatement of matching + AP
(tests/detection_ap_ref.py) on the same tables on the HOST, labelled as a CPU number, which must agree bit for bit.
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
    ap.add_argument("--per-gt", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None, help="also write the numbers here")
    args = ap.parse_args()
    import torch

    from foundpose_amd import eval_bop24 as eb, ops, synthetic
    from tests import detection_ap_ref as ref
    assert torch.cuda.is_available(), "bench_bop24_eval needs the MI355X"
    root = args.out or tempfile.mkdtemp(prefix="bop24_eval_")
    t0 = time.perf_counter()
    meta = synthetic.make_bop_eval_scene(root, num_images=args.images, num_objects=8, width=640, height=480, mesh_res=90,
                                         gts_per_image=7, depth_scale=0.1, seed=2024)
    gen_s = time.perf_counter() - t0
    rng = np.random.default_rng(7)
    ests = []
    for im, inst in meta["images"]:
        for lid, T in inst:
            for k in range(args.per_gt):
                T2 = T.copy()
                a = rng.normal(size=3)
                a /= np.linalg.norm(a)
                ang = np.deg2rad(rng.uniform(0, 4 * (k + 1)))
                Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
                T2[:3, :3] = (np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx) @ T[:3, :3]
                T2[:3, 3] += rng.normal(0, 0.03 * (k + 1) * meta["diameters"][lid], 3)
                ests.append((1, im, lid, float(rng.uniform()), T2, 0.25))
    csv_path = os.path.join(root, "results.csv")
    synthetic.write_bop_results_csv(csv_path, ests)
    targets = [{"scene_id": 1, "im_id": im} for im, _ in meta["images"]]

    eb.evaluate_bop24(csv_path, meta["split_dir"], targets)          # warm-up: code objects, allocator, page cache
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores = eb.evaluate_bop24(csv_path, meta["split_dir"], targets, timing=True, details=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    dev, tb = scores["device_seconds"], scores["tables"]

    # the two launches alone, every table on the device already
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    err = d(tb["err"], np.float64)
    m_in = (d(tb["est_off"], np.int32), d(tb["gt_off"], np.int32), d(tb["pair_off"], np.int32), err, d(tb["gt_valid"], np.int32),
            d(tb["group_tab"], np.int32), d(tb["ths"], np.float64), int(tb["est_off"][-1]))
    a_in = (d(tb["obj_off"], np.int32), d(tb["order"], np.int32), d(tb["n_valid"], np.int32), d(eb.REC_THR, np.float64))
    for _ in range(3):
        flag, _m = ops.detection_match(*m_in)
        ops.detection_ap(a_in[0], a_in[1], flag, a_in[2], a_in[3])
    tm, ta = [], []
    for _ in range(args.iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        flag, matched = ops.detection_match(*m_in)
        e[1].record()
        ap_d, q_d, tot_d = ops.detection_ap(a_in[0], a_in[1], flag, a_in[2], a_in[3])
        e[2].record()
        torch.cuda.synchronize()
        tm.append(e[0].elapsed_time(e[1]) / 1e3)
        ta.append(e[1].elapsed_time(e[2]) / 1e3)
    match_s, ap_s = float(np.median(tm)), float(np.median(ta))

    # the numpy restatement on the host, on the same tables; it must agree bit for bit
    t0 = time.perf_counter()
    rflag, rmatched = ref.match_batch(tb["est_off"], tb["gt_off"], tb["pair_off"], tb["err"], tb["gt_valid"], tb["group_tab"], tb["ths"])
    cpu_match = time.perf_counter() - t0
    t0 = time.perf_counter()
    rap, rq, rtot = ref.ap_batch(tb["obj_off"], tb["order"], rflag, tb["n_valid"])
    cpu_ap = time.perf_counter() - t0
    assert np.array_equal(rflag, flag.cpu().numpy()) and np.array_equal(rmatched, matched.cpu().numpy()), "fp_detection_match differs from the restatement"
    assert np.array_equal(rap.view(np.int64), ap_d.cpu().numpy().view(np.int64)) and np.array_equal(rtot, tot_d.cpu().numpy()), \
        "fp_detection_ap differs from the restatement"

    res = {"images": args.images, "objects": 8, "estimates": scores["num_estimates_evaluated"], "gt_instances": scores["num_gt_instances"],
           "valid_gt_instances": scores["num_valid_gt_instances"], "groups": int(len(tb["groups"])), "pairs": int(tb["pair_off"][-1]),
           "dataset_generation_s": gen_s, "evaluate_bop24_wall_s": wall, "device_mssd_mspd_s": dev.get("mssd_mspd", 0.0),
           "device_match_call_s": dev.get("match", 0.0), "device_ap_call_s": dev.get("ap", 0.0), "device_total_s": sum(dev.values()),
           "match_launch_s": match_s, "ap_launch_s": ap_s, "cpu_numpy_match_s": cpu_match, "cpu_numpy_ap_s": cpu_ap,
           "ap": scores["bop24_average_precision"], "ap_mssd": scores["bop24_average_precision_mssd"], "ap_mspd": scores["bop24_average_precision_mspd"]}
    print(f"# python tools/bench_bop24_eval.py (LM-O-like: {args.images} images 640x480, 8 objects, {res['estimates']} estimates in "
          f"{res['groups']} groups, {res['gt_instances']} GT instances ({res['valid_gt_instances']} valid), {res['pairs']} (estimate, GT) pairs)")
    print(f"evaluate_bop24 wall                         {wall:8.3f} s   (AP {res['ap']:.4f}: mssd {res['ap_mssd']:.4f} mspd {res['ap_mspd']:.4f})")
    print(f"device part (events)                        {res['device_total_s']:8.4f} s   mssd/mspd {res['device_mssd_mspd_s']:.4f}  match call "
          f"{res['device_match_call_s']:.5f}  ap call {res['device_ap_call_s']:.5f} (table uploads included)")
    print(f"fp_detection_match alone (median of {args.iters})    {match_s * 1e6:8.1f} us")
    print(f"fp_detection_ap alone (median of {args.iters})       {ap_s * 1e6:8.1f} us")
    print(f"numpy restatement on the host (CPU)         {cpu_match:8.3f} s matching + {cpu_ap:.3f} s AP, equal bit for bit")
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
