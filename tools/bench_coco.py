"""The COCO scorer's device chain (foundpose_amd.eval_coco) at the workload's own shape, generated from a seed: a few
hundred 640 x 480 frames, about 100 detections and 8 objects per frame with --inst-per-object instances each; detections are jittered
copies of the instances' rectangles plus false positives, as COCO run lengths.

    python tools/bench_coco.py [--frames 200] [--dets 100] [--objects 8] [--inst-per-object 1] [--image-block 32] [--iters 5]
                               [--variant-lib foundpose_amd/lib/coco_tile1.so] [--json FILE]

Per stage (fp_detection_masks, fp_mask_pack of detections and of ground truth, fp_group_mask_iou, fp_coco_match, fp_detection_ap): the
device time by HIP events (the sum over the blocks, median of --iters passes after one warm-up pass), the bytes the stage has to read
(computed from the shapes: every row of a tile once) and that rate as a fraction of the HBM bandwidth (8.0 TB/s spec; a block's packed
masks fit the 256 MiB Infinity Cache, so this is a rate, not a statement about HBM traffic).  The same overlaps are computed on the HOST by
numpy on the packed bits (bitwise_and + bitwise_count, at most 16 threads), labelled as a CPU number, and must agree exactly.
--variant-lib: another build of the library (tools/build_variant.sh coco_tile1 coco_eval.hip -DFP_COCO_TILE_A=1 -DFP_COCO_TILE_B=1: the
same kernel with one pair per workgroup); its fp_group_mask_iou is timed in alternation with the shipped one and must give the same
bytes.  The byte-per-pixel form of the kernel is tools/ubench/mask_iou_bytes.hip, a program of its own.
"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC = 8.0e12


def rect_rle(H, W, x0, y0, x1, y1):
    """The column-major run lengths of the rectangle [x0, x1) x [y0, y1) on an H x W canvas."""
    h, w = y1 - y0, x1 - x0
    counts = [x0 * H + y0]
    for _ in range(w - 1):
        counts += [h, H - h]
    counts += [h, (W - x1) * H + (H - y1)]
    return {"size": [H, W], "counts": counts}


def make_frames(args, rng):
    """-> per frame: (gt [(obj, x0, y0, x1, y1)], dets [(obj, score, x0, y0, x1, y1)])."""
    H, W = args.height, args.width
    frames = []
    for _ in range(args.frames):
        gt = []
        for o in range(args.objects):
            for _i in range(args.inst_per_object):
                w, h = int(rng.integers(40, 160)), int(rng.integers(40, 160))
                x0, y0 = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
                gt.append((o + 1, x0, y0, x0 + w, y0 + h))
        dets = []
        for k in range(args.dets):
            o, x0, y0, x1, y1 = gt[k % len(gt)]
            j = int(rng.integers(0, 4 + 6 * (k // len(gt))))     # later copies of an instance are jittered further
            dx, dy = (int(v) for v in rng.integers(-j, j + 1, 2))
            bx0, by0 = min(max(x0 + dx, 0), W - 2), min(max(y0 + dy, 0), H - 2)
            bx1, by1 = min(max(x1 + dx + int(rng.integers(-j, j + 1)), bx0 + 1), W), min(max(y1 + dy + int(rng.integers(-j, j + 1)), by0 + 1), H)
            dets.append((o, float(rng.uniform()), bx0, by0, bx1, by1))
        frames.append((gt, dets))
    return frames


def block_tables(frames, H, W):
    """One block's host tables: groups = (frame, object) with a detection, the detections in rank order."""
    est_off, gt_off, pair_off, rles, gt_rects, obj_of, score_of = [0], [0], [0], [], [], [], []
    for gt, dets in frames:
        for o in sorted({d[0] for d in dets}):
            ds = sorted((d for d in dets if d[0] == o), key=lambda d: -d[1])
            gs = [g for g in gt if g[0] == o]
            rles += [rect_rle(H, W, *d[2:]) for d in ds]
            obj_of += [o] * len(ds)
            score_of += [d[1] for d in ds]
            gt_rects += [g[1:] for g in gs]
            est_off.append(est_off[-1] + len(ds))
            gt_off.append(gt_off[-1] + len(gs))
            pair_off.append(pair_off[-1] + len(ds) * len(gs))
    return (np.array(est_off, np.int64), np.array(gt_off, np.int64), np.array(pair_off, np.int64)), rles, gt_rects, obj_of, score_of


def tile_rows(est_off, gt_off, ta=4, tb=4):
    """The mask rows a tiled pass has to read: every row of a tile once."""
    rows = 0
    for E, G in zip(np.diff(est_off), np.diff(gt_off)):
        E, G = int(E), int(G)
        if E and G:
            na, nb = -(-E // ta), (1 if G == 1 else -(-G // tb))
            rows += nb * E + na * G
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--inst-per-object", type=int, default=1)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--image-block", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--variant-lib", default=None)
    ap.add_argument("--json", default=None, help="also write the numbers here")
    args = ap.parse_args()
    import torch

    from foundpose_amd import _lib, eval_coco, ops
    from foundpose_amd.infer_pose_util import pack_rle
    assert torch.cuda.is_available(), "bench_coco needs the MI355X"
    assert args.host_threads <= 16
    H, W = args.height, args.width
    L = H * ((W + 63) // 64)
    dev = torch.device("cuda")
    rng = np.random.default_rng(2024)
    t0 = time.perf_counter()
    frames = make_frames(args, rng)
    blocks = []
    for b0 in range(0, len(frames), args.image_block):
        offs, rles, gt_rects, obj_of, score_of = block_tables(frames[b0:b0 + args.image_block], H, W)
        counts, run_off, _ = pack_rle(rles)
        gt = np.zeros((len(gt_rects), H, W), np.uint8)
        for i, (x0, y0, x1, y1) in enumerate(gt_rects):
            gt[i, y0:y1, x0:x1] = 255
        blocks.append(dict(offs=offs, counts=torch.from_numpy(counts).to(dev), run_off=torch.from_numpy(run_off).to(dev), gt=torch.from_numpy(gt).to(dev),
                           d_offs=[torch.from_numpy(o.astype(np.int32)).to(dev) for o in offs], ign=np.zeros(len(gt_rects), np.int64),
                           obj_of=obj_of, score_of=score_of))
    gen_s = time.perf_counter() - t0
    ths = torch.from_numpy(eval_coco.IOU_THS).to(dev)

    variant = None
    if args.variant_lib:
        variant = ctypes.CDLL(os.path.abspath(args.variant_lib))
        variant.fp_group_mask_iou.argtypes = _lib._PROTOS["fp_group_mask_iou"]
        variant.fp_group_mask_iou.restype = ctypes.c_int

    def variant_iou(wa, wb, d_offs, P):
        counts = torch.zeros(P, 2, dtype=torch.int32, device=dev)
        overlap = torch.zeros(P, dtype=torch.float64, device=dev)
        status = torch.full((P,), 2, dtype=torch.int32, device=dev)
        tiles = torch.empty(d_offs[0].shape[0], dtype=torch.int32, device=dev)
        rc = variant.fp_group_mask_iou(_lib.ptr(wa), int(wa.shape[0]), _lib.ptr(wb), int(wb.shape[0]), L, _lib.ptr(d_offs[0]), _lib.ptr(d_offs[1]),
                                       _lib.ptr(d_offs[2]), int(d_offs[0].shape[0]) - 1, P, _lib.ptr(tiles), _lib.ptr(counts), _lib.ptr(overlap),
                                       _lib.ptr(status), _lib.stream())
        assert rc == 0
        return counts, overlap, status

    stages = ("decode", "pack_det", "pack_gt", "overlap", "match", "ap") + (("overlap_variant",) if variant else ())
    times = {k: [] for k in stages}
    keep = {}
    for it in range(args.iters + 1):
        ev = {k: [] for k in stages}

        def timed(kind, fn, *a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            ev[kind].append((e0, e1))
            return out

        flags = []
        for bi, b in enumerate(blocks):
            P = int(b["offs"][2][-1])
            masks, _ = timed("decode", ops.detection_masks, b["counts"], b["run_off"], (H, W), (H, W), open3x3=False)
            wa, area_a = timed("pack_det", ops.mask_pack, masks)
            wb, area_b = timed("pack_gt", ops.mask_pack, b["gt"])
            del masks
            cnt, overlap, status = timed("overlap", ops.group_mask_iou, wa, wb, *b["d_offs"], P)
            if variant:
                cnt2, ov2, st2 = timed("overlap_variant", variant_iou, wa, wb, b["d_offs"], P)
                if it == 0:
                    assert torch.equal(cnt, cnt2) and torch.equal(ov2.view(torch.int64), overlap.view(torch.int64)) and torch.equal(status, st2), \
                        "the variant library's overlaps differ"
            d_ign = torch.zeros(len(b["ign"]), dtype=torch.int32, device=dev)
            flag, _m = timed("match", ops.coco_match, *b["d_offs"], overlap, d_ign, ths, int(b["offs"][0][-1]))
            flags.append(flag)
            if it == 0 and bi == 0:
                keep = dict(wa=wa.cpu().numpy().view(np.uint64).reshape(len(wa), L), wb=wb.cpu().numpy().view(np.uint64).reshape(len(wb), L),
                            counts=cnt.cpu().numpy(), offs=b["offs"])
        if it == 0:   # the AP tables once: per object the global rank order
            obj = np.concatenate([np.array(b["obj_of"]) for b in blocks])
            score = np.concatenate([np.array(b["score_of"]) for b in blocks])
            obj_ids = sorted(set(obj.tolist()))
            order = np.concatenate([np.flatnonzero(obj == o)[np.argsort(-score[obj == o], kind="stable")] for o in obj_ids])
            obj_off = np.cumsum([0] + [int((obj == o).sum()) for o in obj_ids])
            n_valid = np.full(len(obj_ids), args.frames * args.inst_per_object)
            d_ap = [torch.from_numpy(np.asarray(x, np.int32)).to(dev) for x in (obj_off, order, n_valid)] + [torch.from_numpy(eval_coco.REC_THR).to(dev)]
        ap_d, _q, tot = timed("ap", ops.detection_ap, d_ap[0], d_ap[1], torch.cat(flags), d_ap[2], d_ap[3])
        torch.cuda.synchronize()
        if it:   # pass 0 warms up: code objects, allocator
            for k in stages:
                times[k].append(sum(e0.elapsed_time(e1) for e0, e1 in ev[k]) / 1e3)
    ap_host = ap_d.cpu().numpy()

    # ---- the first block's overlaps on the HOST: numpy on the packed bits, at most 16 threads; must agree exactly
    wa, wb, (est_off, gt_off, pair_off) = keep["wa"], keep["wb"], keep["offs"]

    def host_group(g):
        A, B = wa[est_off[g]:est_off[g + 1]], wb[gt_off[g]:gt_off[g + 1]]
        inter = np.array([[int(np.bitwise_count(a & b).sum()) for b in B] for a in A], np.int64).reshape(len(A), len(B))
        aa, ab = np.bitwise_count(A).sum(1, dtype=np.int64), np.bitwise_count(B).sum(1, dtype=np.int64)
        return inter, aa[:, None] + ab[None, :] - inter
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=args.host_threads) as ex:
        host = list(ex.map(host_group, range(len(est_off) - 1)))
    host_s = time.perf_counter() - t0
    for g, (inter, union) in enumerate(host):
        sl = keep["counts"][pair_off[g]:pair_off[g + 1]]
        assert np.array_equal(sl[:, 0], inter.reshape(-1)) and np.array_equal(sl[:, 1], union.reshape(-1)), "the device's counts differ from numpy's"
    host_all_s = host_s * len(blocks)

    n_det = sum(int(b["offs"][0][-1]) for b in blocks)
    n_gt = sum(int(b["offs"][1][-1]) for b in blocks)
    pairs = sum(int(b["offs"][2][-1]) for b in blocks)
    runs = sum(int(b["counts"].numel()) for b in blocks)
    rows4 = sum(tile_rows(b["offs"][0], b["offs"][1]) for b in blocks)
    bytes_read = {"decode": 4.0 * runs, "pack_det": float(n_det) * H * W, "pack_gt": float(n_gt) * H * W, "overlap": rows4 * L * 8.0,
                  "match": pairs * 8.0, "ap": n_det * 10.0, "overlap_variant": 2.0 * pairs * L * 8.0}
    res = {"frames": args.frames, "width": W, "height": H, "detections": n_det, "gt_instances": n_gt, "pairs": pairs, "groups": sum(len(b["offs"][0]) - 1 for b in blocks),
           "image_block": args.image_block, "words_per_mask": L, "generation_s": gen_s, "iters": args.iters, "stages": {},
           "overlap_bytes_per_pair_tiled": rows4 * L * 8.0 / max(pairs, 1), "overlap_bytes_per_pair_one_pair_per_workgroup": 2.0 * L * 8.0,
           "overlap_bytes_per_pair_byte_masks": 2.0 * H * W,
           "host_numpy_overlap_first_block_s": host_s, "host_numpy_overlap_all_blocks_extrapolated_s": host_all_s, "host_threads": args.host_threads,
           "ap_mean": float(ap_host.mean())}
    print(f"# python tools/bench_coco.py: {args.frames} frames {W}x{H}, {n_det} detections, {n_gt} GT instances, {pairs} pairs in {res['groups']} groups, "
          f"blocks of {args.image_block} frames, L = {L} words")
    for k in stages:
        med, lo, hi = float(np.median(times[k])), float(np.min(times[k])), float(np.max(times[k]))
        res["stages"][k] = {"device_s_median": med, "min": lo, "max": hi, "bytes_read": bytes_read[k], "bytes_per_s": bytes_read[k] / med,
                            "fraction_of_hbm_spec": bytes_read[k] / med / HBM_SPEC}
        print(f"{k:16s} {med * 1e3:9.3f} ms [{lo * 1e3:.3f}, {hi * 1e3:.3f}]  reads {bytes_read[k] / 1e6:10.1f} MB  {bytes_read[k] / med / 1e9:8.1f} GB/s  "
              f"{100 * bytes_read[k] / med / HBM_SPEC:5.1f} % of 8.0 TB/s")
    print(f"host numpy on packed bits ({args.host_threads} threads, CPU): first block {host_s:.3f} s, x {len(blocks)} blocks = {host_all_s:.2f} s; counts equal")
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=2)


if __name__ == "__main__":
    main()
