"""Featuremetric refinement at the headline shape (planted workload, ViT-L/14-reg 518^2, batch 32, 10 000 templates, bf16, 30
iterations): (1) the refinement's device time per batch (HIP events around refine_best_coarse), (2) the infer_batch step with
keep_feature_map False and True, alternated in one process, (3) detections/s of the chain crops -> poses for final pose
types best_coarse and featuremetric, alternated.

    python tools/bench_refine.py [--steps 10] [--warmup 3] [--iters 30]

The per-kernel table comes from a separate `rocprofv3 --kernel-trace --stats` run of this script.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--templates", type=int, default=10000)
    args = ap.parse_args()
    import torch
    from foundpose_amd import engine as fe, feature_util, pnp_util, refine_util, workload
    from foundpose_amd.bank import DeviceBank

    dev = torch.device("cuda", 0)
    name = "dinov2_version=vitl14-reg_stride=14_facet=token_layer=18_norm=1"
    ex32 = feature_util.make_feature_extractor(name, random_init_seed=1234, precision="fp32").to(dev)
    wl = workload.build_planted_workload(ex32, args.batch, 518, 1, args.templates, 256, 2048, seed=7, crop_seed=0)
    del ex32
    bank = DeviceBank(wl.repres, device=dev)
    ex = feature_util.make_feature_extractor(name, random_init_seed=1234, precision="bf16").to(dev)
    eng = fe.FoundPoseEngine(ex, bank, 14.0, 5, 300, tie_order="torch")
    K = wl.K.cpu().numpy()
    cams = [K] * args.batch
    size = (518, 518)

    def chain(keep):
        res = eng.infer_batch(wl.crops, wl.masks, wl.det_obj, keep_feature_map=keep)
        best = pnp_util.select_best_coarse(pnp_util.estimate_poses(res, cams, "opencv", 1000, 10.0, 0.99, True))
        if keep:
            out = refine_util.refine_best_coarse(res, best, bank, wl.det_obj, cams, size, args.iters)
            return out["R"].cpu(), out["t"].cpu(), out
        return best["R"].cpu(), best["t"].cpu(), None

    for _ in range(args.warmup):
        chain(False)
        chain(True)
    torch.cuda.synchronize()

    # (1) refinement device time: the same coarse result refined `steps` times
    res = eng.infer_batch(wl.crops, wl.masks, wl.det_obj, keep_feature_map=True)
    best = pnp_util.select_best_coarse(pnp_util.estimate_poses(res, cams, "opencv", 1000, 10.0, 0.99, True))
    torch.cuda.synchronize()
    ref_ms = []
    for _ in range(args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = refine_util.refine_best_coarse(res, best, bank, wl.det_obj, cams, size, args.iters)
        b.record()
        b.synchronize()
        ref_ms.append(a.elapsed_time(b))
    st = out["status"].cpu().numpy()
    status = {int(k): int((st == k).sum()) for k in (0, 1, 2)}
    pts = out["num_points"].cpu().numpy()
    iters_used = out["iters_used"].cpu().numpy()
    # accuracy against the planted poses (coarse vs refined rotation error)
    def rot_err(R):
        Rg = wl.R.cpu().numpy()
        c = (np.einsum("bij,bij->b", R, Rg) - 1) / 2
        return np.degrees(np.arccos(np.clip(c, -1, 1)))
    e_coarse, e_ref = rot_err(best["R"].cpu().numpy()), rot_err(out["R"].cpu().numpy())

    # (2) infer_batch step, keep_feature_map False / True alternated
    step = {False: [], True: []}
    for _ in range(args.steps):
        for keep in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.infer_batch(wl.crops, wl.masks, wl.det_obj, keep_feature_map=keep)
            torch.cuda.synchronize()
            step[keep].append(1e3 * (time.perf_counter() - t0))

    # (3) chain crops -> poses, best_coarse / featuremetric alternated
    dps = {False: [], True: []}
    for _ in range(args.steps):
        for keep in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            chain(keep)
            torch.cuda.synchronize()
            dps[keep].append(args.batch / (time.perf_counter() - t0))

    med = lambda v: float(np.median(v))
    line = {"metric": "featuremetric_refine", "batch": args.batch, "templates": args.templates, "iters": args.iters,
            "refine_device_ms_median": med(ref_ms), "refine_device_ms_min": float(min(ref_ms)),
            "step_ms_keep_map_false": med(step[False]), "step_ms_keep_map_true": med(step[True]),
            "chain_det_per_s_best_coarse": med(dps[False]), "chain_det_per_s_featuremetric": med(dps[True]),
            "status_counts": status, "valid_points_median": med(pts), "iters_used_median": med(iters_used),
            "rot_err_deg_coarse_median": med(e_coarse), "rot_err_deg_refined_median": med(e_ref)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
