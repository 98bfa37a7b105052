"""The proposal-labelling stage at the size a user runs: --proposals mask proposals of one 640 x 480 frame against
--objects detector banks of --templates templates, ViT-L/14-reg (random_init_seed: the time does not depend on the weights) at 224 x 224.

Everything is generated here from a seed: a noise frame, ellipse proposals of 12 .. 220 pixels across, banks of random unit descriptors.
One warm-up pass, then --reps timed passes.  A pass runs the steps of detect_util.label_proposals one after the other with a device
synchronise after each, so the stage times are host clocks around finished device work: decode + boxes, crops, ViT (+ normalisation),
scores, suppression (rank + overlaps + greedy).  Then label_proposals itself, whole, as a user calls it (one read-back).  The report is the
median and the spread of every figure over the passes.

--score-type semantic_appearance adds the two steps of the appearance score -- patch coverage, and the score itself
against banks of random unit patch descriptors (objects x templates x 256 x 1024 floats: 6.7 GB at the default size; --templates 42 is
detector_template_stride = 19) -- times the ViT step through patch_descriptors, and reports label_proposals whole in BOTH modes.

  python tools/bench_detect.py [--out profiles/detect_stage.json]
  python tools/bench_detect.py --score-type semantic_appearance [--out profiles/detect_stage_appearance.json]
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
    ap.add_argument("--score-type", default="semantic", choices=list(du.SCORE_TYPES))
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
    appearance = args.score_type == "semantic_appearance"
    if appearance:
        ps = du.patch_size_of(ex)
        Np = (opts.detector_crop_size // ps) ** 2
        gd = torch.Generator(device="cuda").manual_seed(0)
        for b in banks.values():
            rows = torch.randn(args.templates * Np, ex.arch.dim, generator=gd, device="cuda")
            b["patch_descs"] = ops.normalize_rows(rows).view(args.templates, Np, ex.arch.dim)
            b["patch_cover"] = torch.randint(0, ps * ps + 1, (args.templates, Np), generator=gd, device="cuda", dtype=torch.int32)
            b["patch_size"] = ps
            del rows
        app_opts = opts._replace(detector_score_type="semantic_appearance")
        min_cover = du.min_cover_pixels(opts.detector_patch_min_cover, ps)
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
        index = torch.zeros(P, dtype=torch.int32, device="cuda")
        crops, status = ops.proposal_crops(img, masks, boxes, opts.detector_crop_size, index)
        t.append(sync())
        if appearance:
            desc, patches = du.patch_descriptors(ex, crops, opts.detector_batch)
        else:
            desc = du.cls_descriptors(ex, crops, opts.detector_batch)
        t.append(sync())
        _, bo, bsc, bt = ops.proposal_scores(desc, bs.descs, bs.obj_off, bs.max_templates, opts.detector_topk)
        t.append(sync())
        dec, order, goff, poff, pairs, ranked = ops.proposal_rank(bo, bsc, area, status, boxes, len(bs.lids), 0, -1.0, du.MAX_GROUP)
        ov, st = ops.box_iou(ranked, pairs)
        keep, by = ops.pose_nms_greedy(goff, poff, pairs, ov, st, P, opts.detector_nms_thresh)
        t.append(sync())
        names = ("decode_boxes_ms", "crops_ms", "vit_ms", "scores_ms", "suppression_ms")
        if appearance:   # (timed behind the suppression so that the five steps above stay what they are in the other mode)
            cover = ops.proposal_patch_cover(masks, boxes, opts.detector_crop_size, ps, index, 1)
            t.append(sync())
            ops.proposal_appearance(patches, cover, bs.patch_descs, bs.patch_cover, bs.obj_off, bo, bt, bsc, min_cover)
            t.append(sync())
            names += ("patch_cover_ms", "appearance_ms")
        return dict(zip(names, (1e3 * (b - a) for a, b in zip(t[:-1], t[1:]))))

    def whole():
        t0 = sync()
        dets, _ = du.label_proposals(opts, image, proposals, bs, ex)
        out = {"label_proposals_ms": 1e3 * (sync() - t0), "kept": sum(len(v) for v in dets.values())}
        if appearance:
            t0 = sync()
            dets, _ = du.label_proposals(app_opts, image, proposals, bs, ex)
            out.update({"label_proposals_appearance_ms": 1e3 * (sync() - t0), "kept_appearance": sum(len(v) for v in dets.values())})
        return out

    staged(), whole()   # warm-up: code objects, workspaces, the allocator
    runs = [dict(staged(), **whole()) for _ in range(args.reps)]
    report = {"config": {"proposals": P, "objects": args.objects, "templates": args.templates, "frame": [W, H], "crop": opts.detector_crop_size,
                         "extractor": NAME, "precision": args.precision, "vit_batch": opts.detector_batch, "reps": args.reps, "score_type": args.score_type,
                         "patch_bank_bytes": int(bs.patch_descs.numel()) * 4 if appearance else 0,
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
