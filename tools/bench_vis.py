"""Times the result pictures at the headline shape: batch 32, 518 x 518 crops, 5 templates, 100 matches,
ViT-L/14-reg with random weights.  Prints the device time of one vis_inference_results_batch call (HIP events), the share of
the extra extractor forward over the 32 best templates, the device -> pinned host copy and the host PNG encoding, next to the
derived yardsticks.

    python tools/bench_vis.py [--batch 32] [--size 518] [--reps 5] > profiles/vis_bench.txt
"""
import argparse
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundpose_amd import feature_util, projector_util, repre_util, synthetic, vis_util  # noqa: E402
from foundpose_amd.crop_util import PinholePlaneCameraModel  # noqa: E402
from foundpose_amd.matching import MatchResult  # noqa: E402
from foundpose_amd.renderer import HipRasterizer  # noqa: E402


def _events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--extractor", default="dinov2_version=vitl14-reg_stride=14_facet=token_layer=18_norm=1")
    args = ap.parse_args()
    B, S, n, K, T, C = args.batch, args.size, 5, 300, 16, 256
    g = torch.Generator(device="cuda").manual_seed(0)
    ex = feature_util.make_feature_extractor(args.extractor, random_init_seed=1234, precision="bf16").to("cuda")
    gs = S // ex.patch_size
    proj = projector_util.PCAProjector(n_components=C)
    proj.components, proj.mean = torch.linalg.qr(torch.randn(ex.arch.dim, C))[0].t().contiguous(), torch.zeros(ex.arch.dim)
    T_c2m = np.eye(4)
    T_c2m[2, 3] = -600.0                                        # the template camera 600 mm in front of the model origin
    cam = {"f": torch.tensor([700.0, 700.0]), "c": torch.tensor([S / 2, S / 2]), "width": S, "height": S, "T_world_from_eye": torch.from_numpy(T_c2m)}
    repre = repre_util.FeatureBasedObjectRepre(templates=torch.randint(0, 256, (T, 3, S, S), dtype=torch.uint8), feat_raw_projectors=[proj],
                                               feat_vis_projectors=[proj], template_cameras_cam_from_model=[cam] * T)
    ras = HipRasterizer("cuda")
    ras.add_object_model(1, mesh=synthetic.make_blob_mesh(50, 50, radius=55.0, seed=7))
    crops = torch.rand(B, 3, S, S, generator=g, device="cuda")
    masks = torch.zeros(B, S, S, dtype=torch.uint8, device="cuda")
    masks[:, S // 4:3 * S // 4, S // 4:3 * S // 4] = 1
    cams = [PinholePlaneCameraModel(S, S, (700.0, 700.0), (S / 2, S / 2), np.eye(4))] * B
    res = MatchResult(template_ids=torch.randint(0, T, (B, n), generator=g, device="cuda", dtype=torch.int32),
                      template_scores=torch.rand(B, n, generator=g, device="cuda"), counts=torch.full((B, n), K, dtype=torch.int32, device="cuda"),
                      q_ids=torch.zeros(B, n, K, dtype=torch.int32, device="cuda"), feat_ids=torch.zeros(B, n, K, dtype=torch.int32, device="cuda"),
                      dists=torch.zeros(B, n, K, device="cuda"), conf=torch.rand(B, n, K, generator=g, device="cuda"),
                      coord_2d=torch.rand(B, n, K, 2, generator=g, device="cuda") * S,
                      coord_3d=(torch.rand(B, n, K, 3, generator=g, device="cuda") - 0.5) * 100.0,
                      feature_map=torch.randn(B, gs, gs, C, generator=g, device="cuda"))
    pose = np.eye(4)
    pose[2, 3] = 600.0
    poses = [pose] * B
    tpl_dev = repre.templates.cuda()

    def run(feat=True):
        return vis_util.vis_inference_results_batch(crops, masks, cams, res, [True] * B, [0] * B, poses, poses, repre, ras, 1, extractor=ex,
                                                    vis_corresp_top_n=100, vis_feat_map=feat, templates=tpl_dev)[0]
    total = _events(run, args.reps)
    fwd = _events(lambda: vis_util._projected_map(ex, tpl_dev[:B].float() / 255.0, [proj]), args.reps)
    no_feat = _events(lambda: run(False), args.reps)
    tiles = run()
    rows = {"mask_tint": lambda: vis_util.mask_tint(tiles[:, :S, :S].contiguous(), masks),
            "contour": lambda: vis_util.contour(tiles[:, :S, :S].contiguous(), masks, (0, 255, 0)),
            "resize_area": lambda: vis_util.resize_area(tiles[:, :S, :].repeat(1, 1, 3, 1)[:, :, :n * S].contiguous(), (int(S * 2 / n), 2 * S)),
            "pca_colorize": lambda: vis_util.pca_colorize(res.feature_map, (S, S), dim=(9, 10)),
            "draw_matches": lambda: vis_util.draw_matches(tiles[:, :S].contiguous(), torch.rand(B, 100, 4, device="cuda") * S + torch.tensor([0.0, 0, S, 0], device="cuda"),
                                                          torch.full((B,), 100, dtype=torch.int32, device="cuda"))}
    per_kernel = {k: _events(f, args.reps) for k, f in rows.items()}   # (each includes the input copy it makes: an upper bound)
    t0 = time.perf_counter()
    host = vis_util.tiles_to_host(tiles)
    d2h = time.perf_counter() - t0
    from PIL import Image
    t0 = time.perf_counter()
    for b in range(B):
        Image.fromarray(host[b]).save(io.BytesIO(), format="PNG")
    png = time.perf_counter() - t0
    mb = tiles.numel() / 1e6
    floor_ms = 2 * tiles.numel() / 2e12 * 1e3
    print(f"shape: batch {B}, crops {S} x {S}, {n} templates, 100 matches, tile {tuple(tiles.shape[1:])}, {args.extractor}")
    print(f"vis_inference_results_batch, device time (HIP events, median of {args.reps}): {total:.3f} ms per batch, {total / B:.3f} ms per detection")
    print(f"  extra extractor forward over the {B} best templates + projection: {fwd:.3f} ms ({100 * fwd / total:.1f} % of the call)")
    print(f"  the same call with vis_feat_map=False (no extractor forward, no PCA pictures): {no_feat:.3f} ms")
    print(f"  compositing = call - forward: {total - fwd:.3f} ms; byte floor (tiles written + as much read, {2 * mb:.0f} MB at 2 TB/s): {floor_ms:.3f} ms "
          f"-> {(total - fwd) / floor_ms:.1f} x the floor (includes the rasterizer's views, torch gathers / concatenations and launch gaps)")
    for k, v in per_kernel.items():
        print(f"  kernel alone (with its input copy) {k}: {v:.3f} ms")
    print(f"device -> pinned host, one copy of {mb:.1f} MB: {d2h * 1e3:.3f} ms ({mb / 1e3 / d2h:.1f} GB/s)")
    print(f"host PNG encoding (PIL, default compression): {png * 1e3:.1f} ms per batch, {png / B * 1e3:.1f} ms per detection")


if __name__ == "__main__":
    main()
