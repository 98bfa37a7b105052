"""gt_info.write_gt_info (scene_gt_info.json and the instance masks from GT poses) on an LM-O-like tree from
synthetic.make_bop_eval_scene: wall time with and without the masks, the device time of the renders and of fp_gt_visibility (HIP events
around the calls, as the tool's summary reports them), and the numpy restatement's time per instance on a subset.

    python tools/bench_gt_info.py [--images 200] [--width 640] [--height 480] [--instances 7] [--ref-instances 16] [--out profiles/gt_info_bench.txt]

One process, one run of each configuration after a warm-up run on a small tree (library load, first launches); nothing here is a bar.
The restatement (tests/gt_info_ref.py) is timed on renders fetched the way the tool makes them, one thread, renders excluded.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--instances", type=int, default=7)
    ap.add_argument("--mesh-res", type=int, default=40)
    ap.add_argument("--ref-instances", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from foundpose_amd import eval_bop19 as eb, gt_info, synthetic
    from foundpose_amd.renderer import HipRasterizer, load_ply
    from tests import gt_info_ref

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp(prefix="gt_info_bench_")
    try:
        warm = synthetic.make_bop_eval_scene(os.path.join(root, "warm"), num_images=2, num_objects=2, width=64, height=48, mesh_res=12, seed=1)
        gt_info.write_gt_info(warm["split_dir"], warm["models_dir"], output_dir=os.path.join(root, "warm_out", "test"))
        t0 = time.perf_counter()
        meta = synthetic.make_bop_eval_scene(os.path.join(root, "lmo_like"), num_images=a.images, num_objects=a.instances + 1, width=a.width,
                                             height=a.height, mesh_res=a.mesh_res, gts_per_image=a.instances, seed=3)
        t_scene = time.perf_counter() - t0
        tris = sum(len(load_ply(os.path.join(meta["models_dir"], f"obj_{lid:06d}.ply")).faces) for lid in meta["diameters"]) / len(meta["diameters"])
        say(f"gt_info bench: {a.images} images of {a.width} x {a.height}, {a.instances} instances each ({a.images * a.instances} instances), "
            f"{len(meta['diameters'])} objects of about {tris:.0f} triangles; device {torch.cuda.get_device_name(0)}")
        say(f"(the tree itself took {t_scene:.2f} s to generate; render window {3 * a.width} x {3 * a.height}, {gt_info.chunk_views(a.width, a.height)} views per chunk)")
        say()
        say("| configuration | wall s | ms / instance | device s, renders | device s, fp_gt_visibility | kernel share of wall |")
        say("|---|---|---|---|---|---|")
        results = {}
        from PIL import Image
        os.makedirs(os.path.join(meta["split_dir"], "000001", "rgb"))      # depth_from_gt takes the image size from rgb/: blank frames
        for im, _ in meta["images"]:
            Image.new("RGB", (a.width, a.height)).save(os.path.join(meta["split_dir"], "000001", "rgb", f"{im:06d}.png"))
        for name, kw in (("scene_gt_info.json only", dict(write_masks=False)), ("with mask/ and mask_visib/ PNGs", dict(write_masks=True)),
                         ("depth_from_gt, no masks", dict(write_masks=False, depth_from_gt=True))):
            out = os.path.join(root, "out_" + str(len(results)), "test")
            s = gt_info.write_gt_info(meta["split_dir"], meta["models_dir"], output_dir=out, **kw)
            results[name] = s
            d = s["device_seconds"]
            say(f"| {name} | {s['wall_seconds']:.2f} | {1e3 * s['wall_seconds'] / s['num_instances']:.2f} | {d['render']:.3f} | {d['gt_visibility']:.4f} | "
                f"{100 * d['gt_visibility'] / s['wall_seconds']:.2f} % |")
        s = results["with mask/ and mask_visib/ PNGs"]
        say()
        say(f"instances below visib_fract 0.1: {s['num_instances_below_min_visib']} of {s['num_instances']}")

        # ---- the restatement on a subset: the same renders, numpy on one thread
        ras = HipRasterizer("cuda")
        for lid in meta["diameters"]:
            ras.add_object_model(lid, mesh=load_ply(os.path.join(meta["models_dir"], f"obj_{lid:06d}.ply")))
        sd = os.path.join(meta["split_dir"], "000001")
        gts, cams = json.load(open(os.path.join(sd, "scene_gt.json"))), json.load(open(os.path.join(sd, "scene_camera.json")))
        info = json.load(open(os.path.join(root, "out_1", "test", "000001", "scene_gt_info.json")))
        W, H, K = a.width, a.height, meta["K"]
        Kw = K.copy()
        Kw[0, 2] += W
        Kw[1, 2] += H
        todo = [(im, g) for im in sorted(int(k) for k in gts) for g in range(len(gts[str(im)]))][:a.ref_instances]
        t_ref, same = 0.0, 0
        for im, g in todo:
            e = gts[str(im)][g]
            cam = eb._Camera(Kw, 3 * W, 3 * H, np.linalg.inv(eb._m2c(e["cam_R_m2c"], e["cam_t_m2c"])))
            large = ras.render_views(int(e["obj_id"]), [cam], with_color=False)["depth"][0].cpu().numpy()
            test = eb.load_depth(os.path.join(sd, "depth", f"{im:06d}.png"), cams[str(im)]["depth_scale"])
            t0 = time.perf_counter()
            row, _, _ = gt_info_ref.gt_visibility(test, large, K, 15.0, W, H)
            rec = gt_info_ref.record(row)
            t_ref += time.perf_counter() - t0
            same += rec == info[str(im)][g]
        say(f"numpy restatement (tests/gt_info_ref.py, one thread, renders excluded): {1e3 * t_ref / len(todo):.1f} ms / instance over {len(todo)} "
            f"instances; {same} of {len(todo)} records equal the tool's")
        for name in ("scene_gt_info.json only", "with mask/ and mask_visib/ PNGs"):
            r = results[name]
            say(f"{name}: fp_gt_visibility {1e6 * r['device_seconds']['gt_visibility'] / r['num_instances']:.1f} us / instance, renders "
                f"{1e3 * r['device_seconds']['render'] / r['num_instances']:.3f} ms / instance")
        say("(events around each call: for fp_gt_visibility two memsets, the synchronous table upload and two kernels, so a host kept busy by the "
            "PNG encoders stretches the interval)")
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
