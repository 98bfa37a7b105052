"""The proposal-labelling stage at the size a user runs: --proposals mask proposals of one 640 x 480 frame against
--objects detector banks of --templates templates, ViT-L/14-reg (random_init_seed: the time does not depend on the weights) at 224 x 224.

Everything is generated here from a seed: a noise frame, ellipse proposals of 12 .. 220 pixels across, banks of random unit descriptors.
One warm-up pass, then --reps timed passes.  A pass runs the steps of detect_util.label_proposals one after the other with a device
synchronise after each, so the stage times are host clocks around finished device work: decode + boxes, crops, ViT (+ normalisation),
scores, suppression (rank + overlaps + greedy).  Then label_proposals itself, whole, as a user calls it (one read-back).  The report is the
median and the spread of every figure over the passes.

  python tools/bench_detect.py [--out profiles/detect_stage.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundpose_amd import _lib, detect_util as du, feature_util, infer_pose_util, ops  # noqa: E402

W, H = 640, 480
NAME = "dinov2_version=vitl14-reg_stride=14_facet=token_layer=23_norm=1"


def make_proposals(n, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(n):
        a, b = rng.integers(6, 110, 2)
        cx, cy = rng.integers(a, W - a), rng.integers(b, H - b)
        m = (((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= 1.0).astype(np.uint8)
        out.append({"scene_id": 1, "image_id": 0, "time": 0.0, "segmentation": infer_pose_util.binary_mask_to_rle(m)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--proposals", type=int, default=256)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--templates", type=int, default=798)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect needs the GPU: nothing is measured without one")
    ex = feature_util.make_feature_extractor(NAME, random_init_seed=1234, precision=args.precision).to("cuda")
    opts = du.DetectOpts(detector_extractor_name=NAME, detector_min_score=-1.0)   # random descriptors: nothing is dropped by its score
    g = torch.Generator().manual_seed(0)
    banks = {lid: {"descs": ops.normalize_rows(torch.randn(args.templates, ex.arch.dim, generator=g).cuda()),
                   "template_ids": torch.arange(args.templates), "extractor_name": NAME, "crop_size": opts.detector_crop_size}
             for lid in range(1, args.objects + 1)}
    bs = du.bank_set(banks)
    image = np.random.default_rng(1).integers(0, 256, (H, W, 3), dtype=np.uint8)
    proposals = make_proposals(args.proposals, 2)
    counts, run_off, _ = infer_pose_util.pack_rle(proposals)
    P = len(proposals)

    def sync():
        torch.cuda.synchronize()
        return time.perf_counter()

    def staged():
        t = [sync()]
        img = torch.from_numpy(image).cuda().float().div_(255.0)[None].contiguous()
        table = _lib.upload_async(torch.from_numpy(np.concatenate([counts, run_off])), "cuda")
        masks, _ = ops.detection_masks(table[:counts.size], table[counts.size:], (H, W), (H, W), open3x3=False)
        boxes, area = ops.mask_boxes(masks)
        t.append(sync())
        crops, status = ops.proposal_crops(img, masks, boxes, opts.detector_crop_size, torch.zeros(P, dtype=torch.int32, device="cuda"))
        t.append(sync())
        desc = du.cls_descriptors(ex, crops, opts.detector_batch)
        t.append(sync())
        _, bo, bsc, bt = ops.proposal_scores(desc, bs.descs, bs.obj_off, bs.max_templates, opts.detector_topk)
        t.append(sync())
        dec, order, goff, poff, pairs, ranked = ops.proposal_rank(bo, bsc, area, status, boxes, len(bs.lids), 0, -1.0, du.MAX_GROUP)
        ov, st = ops.box_iou(ranked, pairs)
        keep, by = ops.pose_nms_greedy(goff, poff, pairs, ov, st, P, opts.detector_nms_thresh)
        t.append(sync())
        return dict(zip(("decode_boxes_ms", "crops_ms", "vit_ms", "scores_ms", "suppression_ms"), (1e3 * (b - a) for a, b in zip(t[:-1], t[1:]))))

    def whole():
        t0 = sync()
        dets, _ = du.label_proposals(opts, image, proposals, bs, ex)
        return {"label_proposals_ms": 1e3 * (sync() - t0), "kept": sum(len(v) for v in dets.values())}

    staged(), whole()   # warm-up: code objects, workspaces, the allocator
    runs = [dict(staged(), **whole()) for _ in range(args.reps)]
    report = {"config": {"proposals": P, "objects": args.objects, "templates": args.templates, "frame": [W, H], "crop": opts.detector_crop_size,
                         "extractor": NAME, "precision": args.precision, "vit_batch": opts.detector_batch, "reps": args.reps,
                         "device": torch.cuda.get_device_name(0)},
              "median": {k: float(np.median([r[k] for r in runs])) for k in runs[0]},
              "min": {k: float(np.min([r[k] for r in runs])) for k in runs[0]},
              "max": {k: float(np.max([r[k] for r in runs])) for k in runs[0]}}
    print(json.dumps(report))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
