"""The two inference drivers on one synthetic BOP split: infer.infer (one object after the other, one batch per (image, object)) against
infer.infer_batched (one pass over the images, N detections per batch across frames and objects).  DESIGN.md section 13.

The split is generated here (workload.py + synthetic.py, nothing external) and written to disk in the BOP layout, so both drivers read it
the way the CLI does (PNG decoding included: once per image and object for infer(), once per image for infer_batched()):
  * --objects banks of --templates templates from workload.build_planted_workload (ViT-L/14-reg, random_init_seed, 518 px crops);
  * --frames images of 640 x 480 noise; every (frame, object) has 1 or 2 instances (alternating), each a planted crop of its object shrunk
    into its box with a disc mask -- so the crop producer, the backbone, the matching and the PnP tail all have work of the usual size.
One warm-up pass and one timed pass per driver; the report is detections/s over the timed pass (wall clock, loading included), the time
spent loading frames, in select_instances (detection masks: RLE decoding and the 3x3 opening, on the host) and in _record_poses (the
correspondences of every pose to the host, scores, evaluator) -- host work outside the stage clocks -- and the mean of every per-detection
`times` stage of estimated-poses.json.

--device-masks: after the runs above, infer_batched(<first of --batches>) with the host masks and with device_masks=True
on the same split in the same process, in the order host, device, host, device; the report gains "device_masks": the four runs (the device
ones with select_instances_device_s), the mean and the spread of the two repeats of each path, and the ratios device / host.

  python tools/bench_infer_drivers.py [--out profiles/infer_drivers.json]
  python tools/bench_infer_drivers.py --batches 32 --device-masks --out profiles/infer_drivers_device_masks.json
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundpose_amd import feature_util, infer, infer_pose_util, workload  # noqa: E402

W, H = 640, 480
# box slots (x, y, side) of a frame: 4 columns x 3 rows (8 objects with 1 or 2 instances in turn = 12 instances per frame)
SLOTS = [(10 + 155 * (i % 4), 5 + 155 * (i // 4), 140 + 4 * (i % 3)) for i in range(12)]


def make_split(root, wl, num_frames, seed=0):
    """-> (split dir, targets, detections path); the planted crops of `wl` (two per object) are the instances' appearance."""
    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    num_objects = len(wl.repres)
    by_obj = {o: [b for b, d in enumerate(wl.det_obj) if d == o] for o in range(num_objects)}
    sdir = os.path.join(root, "synth", "test", "000001")
    os.makedirs(os.path.join(sdir, "rgb"))
    cams, targets, dets = {}, [], []
    crops = wl.crops.cpu()
    for f in range(num_frames):
        img = (torch.rand(H, W, 3, generator=g) * 255).to(torch.uint8)
        slot = 0
        for o in range(num_objects):
            n_inst = 1 + (f + o) % 2
            targets.append({"scene_id": 1, "im_id": f, "obj_id": o + 1, "inst_count": n_inst})
            for i in range(n_inst):
                x, y, s = SLOTS[slot % len(SLOTS)]
                slot += 1
                src = crops[by_obj[o][i % len(by_obj[o])]][None]
                small = torch.nn.functional.interpolate(src, size=(s, s), mode="bilinear", align_corners=False, antialias=True)[0]
                yy, xx = torch.meshgrid(torch.arange(s), torch.arange(s), indexing="ij")
                disc = ((yy - (s - 1) / 2) ** 2 + (xx - (s - 1) / 2) ** 2) <= (0.42 * s) ** 2
                patch = img[y:y + s, x:x + s]
                patch[disc] = (small.permute(1, 2, 0)[disc] * 255).to(torch.uint8)
                mask = np.zeros((H, W), np.uint8)
                mask[y:y + s, x:x + s] = disc.numpy()
                dets.append({"scene_id": 1, "image_id": f, "category_id": o + 1, "bbox": [x, y, s, s], "score": 0.9 - 0.1 * i, "time": 0.1,
                             "segmentation": infer_pose_util.binary_mask_to_rle(mask)})
        Image.fromarray(img.numpy()).save(os.path.join(sdir, "rgb", f"{f:06d}.png"))
        cams[str(f)] = {"cam_K": [600.0, 0, W / 2.0, 0, 600.0, H / 2.0, 0, 0, 1], "depth_scale": 1.0}
    with open(os.path.join(sdir, "scene_camera.json"), "w") as fh:
        json.dump(cams, fh)
    det_path = os.path.join(root, "cnos.json")
    with open(det_path, "w") as fh:
        json.dump(dets, fh)
    return os.path.dirname(sdir), targets, det_path


class TimedFrames:
    """Wraps a frame generator and adds up the time spent producing frames (disk read + PNG decode)."""

    def __init__(self):
        self.seconds, self.frames = 0.0, 0

    def __call__(self, gen):
        it = iter(gen)
        while True:
            t = time.perf_counter()
            try:
                frame = next(it)
            except StopIteration:
                self.seconds += time.perf_counter() - t
                return
            self.seconds += time.perf_counter() - t
            self.frames += 1
            yield frame


class TimedCalls:
    """Adds up the wall time of a function of the infer module (host work the per-detection `times` do not cover)."""

    def __init__(self, name):
        self.name, self.fn, self.seconds = name, getattr(infer, name), 0.0
        setattr(infer, name, self)

    def __call__(self, *a, **kw):
        t = time.perf_counter()
        try:
            return self.fn(*a, **kw)
        finally:
            self.seconds += time.perf_counter() - t


def stage_means(out_dir, lids):
    entries = [e for lid in lids for e in json.load(open(os.path.join(out_dir, str(lid), "estimated-poses.json")))]
    keys = sorted({k for e in entries for k in e["time"]})
    return len(entries), {k: float(np.mean([e["time"].get(k, 0.0) for e in entries])) for k in keys}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=8)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--templates", type=int, default=800, help="templates per object")
    ap.add_argument("--version", default="vitl14-reg")
    ap.add_argument("--layer", type=int, default=18)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--batches", default="32,256", help="batch_detections values of infer_batched")
    ap.add_argument("--device-masks", action="store_true", help="also run infer_batched(first of --batches) host, device, host, device (see above)")
    ap.add_argument("--out", default=None, help="also write the JSON report here")
    args = ap.parse_args()
    name = f"dinov2_version={args.version}_stride=14_facet=token_layer={args.layer}_norm=1"
    ex32 = feature_util.make_feature_extractor(name, random_init_seed=1234, precision="fp32").to("cuda")
    wl = workload.build_planted_workload(ex32, 2 * args.objects, args.size, args.objects, args.templates, 256, 2048, seed=7)
    del ex32
    ex = feature_util.make_feature_extractor(name, random_init_seed=1234, precision=args.precision).to("cuda")
    lids = list(range(1, args.objects + 1))
    repres = {lid: wl.repres[lid - 1] for lid in lids}
    opts = infer.InferOpts(version="v", repre_version="v", object_dataset="synth", object_lids=lids, crop_size=(args.size, args.size),
                           extractor_name=name, grid_cell_size=14.0, vis_results=False)
    report = {"objects": args.objects, "frames": args.frames, "templates_per_object": args.templates, "extractor": name, "crop_size": args.size,
              "precision": args.precision, "pnp_ransac_iter": opts.pnp_ransac_iter, "runs": []}
    with tempfile.TemporaryDirectory() as root:
        split, targets, det_path = make_split(root, wl, args.frames)
        detections = infer_pose_util.load_detections_in_bop_format(det_path)
        n_inst = {}
        for t in targets:
            n_inst.setdefault(t["obj_id"], {})[(t["scene_id"], t["im_id"])] = t["inst_count"]

        def per_object(out_dir, timer):
            infer.infer(opts, lambda lid: timer(infer.load_bop_frames(split, targets, lid)), detections, repres, out_dir, extractor=ex, num_target_insts=n_inst)

        def batched(n, **kw):
            def run(out_dir, timer):
                infer.infer_batched(opts, timer(infer.load_bop_frames_all(split, targets)), detections, repres, out_dir, batch_detections=n, extractor=ex,
                                    num_target_insts=n_inst, **kw)
            return run
        select, record = TimedCalls("select_instances"), TimedCalls("_record_poses")
        select_dev = TimedCalls("select_instances_device")
        drivers = [("infer", per_object)] + [(f"infer_batched({int(n)})", batched(int(n))) for n in args.batches.split(",")]

        def measure(label, run, tag=""):
            for phase in ("warmup", "timed"):
                out_dir = os.path.join(root, "out", label.replace("(", "_").replace(")", "").replace(", ", "_") + tag, phase)
                timer = TimedFrames()
                select.seconds = record.seconds = select_dev.seconds = 0.0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(out_dir, timer)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
            n_poses, means = stage_means(out_dir, lids)
            n_det = sum(t["inst_count"] for t in targets)
            r = {"driver": label, "detections": n_det, "poses_found": n_poses, "wall_s": wall, "detections_per_s": n_det / wall,
                 "frame_loading_s": timer.seconds, "frames_loaded": timer.frames, "detections_per_s_without_loading": n_det / (wall - timer.seconds),
                 "select_instances_s": select.seconds, "record_poses_s": record.seconds,
                 "stage_means_ms": {k: 1e3 * v for k, v in means.items()}}
            if select_dev.seconds:   # a device_masks run: the selection ran in select_instances_device (select_instances is not called there)
                r["select_instances_device_s"] = select_dev.seconds
            print(json.dumps(r), flush=True)
            return r
        for label, run in drivers:
            report["runs"].append(measure(label, run))
        if args.device_masks:
            n = int(args.batches.split(",")[0])
            runs = []
            for rep_no in (0, 1):
                for label, kw in ((f"infer_batched({n})", {}), (f"infer_batched({n}, device_masks)", {"device_masks": True})):
                    r = measure(label, batched(n, **kw), tag=f"_rep{rep_no}")
                    r["repeat"] = rep_no
                    runs.append(r)
            summary = {}
            for path, key in (("host", "select_instances_s"), ("device", "select_instances_device_s")):
                mine = [r for r in runs if ("device_masks" in r["driver"]) == (path == "device")]
                summary[path] = {out: {"mean": float(np.mean([r[k] for r in mine])), "spread": float(abs(mine[0][k] - mine[1][k]))}
                                 for out, k in (("select_s", key), ("record_poses_s", "record_poses_s"), ("wall_s", "wall_s"), ("detections_per_s", "detections_per_s"))}
            summary["device_over_host"] = {k: summary["device"][k]["mean"] / summary["host"][k]["mean"] for k in summary["host"]}
            report["device_masks"] = {"runs": runs, "summary": summary}
            print(json.dumps(summary), flush=True)
    base = report["runs"][0]["detections_per_s"]
    report["speedup_vs_infer"] = {r["driver"]: r["detections_per_s"] / base for r in report["runs"][1:]}
    print(json.dumps(report["speedup_vs_infer"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(report, fh, indent=1)


if __name__ == "__main__":
    main()
