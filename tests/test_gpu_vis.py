"""GPU: the result pictures (csrc/vis.hip, foundpose_amd/vis_util.py, the driver's renderer= switch) against the numpy
restatement tests/vis_ref.py.  Integer-defined outputs must be equal; float-defined ones (pca_colorize,
resize_area, draw_matches) may differ from the fp64 restatement by one level: an fp32 chain of <= 3 * 1024 blend steps errs by
< 1e-3 of the 0..255 range, which can only move a value across a truncation / rounding boundary it was already next to.  The
mean absolute difference must stay below 0.05 levels (expected ~0.005: the share of values that close to a boundary, times ten
for clustering), so that a systematic off-by-one fails.

The end-to-end scene is tests/test_gpu_infer_driver.py's (detections at planted poses, tiny ViT, the instances' own crops as
templates 3 and 7) with a blob mesh for the contours and template images / cameras added to its bank.

Every comparison prints its observed figures before it asserts."""
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, synthetic, vis_util
from foundpose_amd.crop_util import PinholePlaneCameraModel
from tests import vis_ref as vr

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (1, 7), (5, 3), (37, 53), (64, 128), (67, 129)]


def _cuda(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()


def _close(got, want, what):
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(f"{what}: max |diff| {int(d.max(initial=0))} levels, mean |diff| {float(d.mean()) if d.size else 0.0:.5f} levels over {d.size} values")
    assert d.max(initial=0) <= 1, what
    assert (float(d.mean()) if d.size else 0.0) < 0.05, what


def _blob_mask(rng, H, W):
    yy, xx = np.mgrid[:H, :W]
    m = np.zeros((H, W), np.uint8)
    for _ in range(3):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.5, max(H, W) / 2 + 0.5)
        m |= ((yy - cy) ** 2 + (xx - cx) ** 2 < r * r).astype(np.uint8)
    return m * 255


# ---------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("H,W", SIZES)
def test_integer_kernels_equal_the_restatement(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    B = 3
    img = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    masks = np.stack([_blob_mask(rng, H, W) for _ in range(B)])
    masks[0] = 255 if H * W > 1 else masks[0]                       # a full mask: no edge at the image border
    got = vis_util.mask_tint(_cuda(img), _cuda(masks)).cpu().numpy()
    assert np.array_equal(got, np.stack([vr.mask_tint(img[b], masks[b]) for b in range(B)]))
    # an unaligned view takes the byte path
    flat = torch.zeros(B * H * W * 3 + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = _cuda(img).reshape(-1)
    assert np.array_equal(vis_util.mask_tint(flat[1:].view(B, H, W, 3), _cuda(masks)).cpu().numpy(), got)
    for dil in (0, 1, 2):
        painted = vis_util.contour(_cuda(img).clone(), _cuda(masks), (0, 255, 0), dil).cpu().numpy()
        assert np.array_equal(painted, np.stack([vr.contour(img[b], masks[b], (0, 255, 0), dil) for b in range(B)])), dil
    K = 4
    depth = rng.uniform(300, 900, (K, H, W)).astype(np.float32) * (rng.random((K, H, W)) < 0.6)
    depth[1] = np.where(rng.random((H, W)) < 0.3, depth[0], depth[1])   # ties between layers 0 and 1
    colours = rng.integers(0, 256, (K, 3)).astype(np.uint8)
    out, ids = vis_util.scene_composite(_cuda(img[0]), _cuda(depth), _cuda(colours))
    want, want_ids = vr.scene_composite(img[0], depth, colours)
    assert np.array_equal(ids.cpu().numpy(), want_ids) and np.array_equal(out.cpu().numpy(), want)


def test_hand_cases_on_the_device():
    m = np.zeros((1, 9, 9), np.uint8)
    m[0, 3:6, 3:6] = 1
    out = vis_util.contour(torch.zeros(1, 9, 9, 3, dtype=torch.uint8, device="cuda"), _cuda(m), (0, 255, 0)).cpu().numpy()[0]
    want = np.zeros((9, 9), bool)
    want[2:7, 2:7] = True
    assert np.array_equal(out[..., 1] == 255, want)
    d = np.zeros((2, 1, 4), np.float32)
    d[0, 0], d[1, 0] = [500, 600, 0, 0], [500, 500, 700, 0]
    _, ids = vis_util.scene_composite(torch.full((1, 4, 3), 100, dtype=torch.uint8, device="cuda"), _cuda(d), _cuda(np.array([[255, 0, 0], [0, 0, 201]], np.uint8)))
    assert ids.cpu().tolist() == [[0, 1, 1, -1]]
    assert not vis_util.pca_colorize(torch.full((2, 3, 4, 8), 2.5, device="cuda"), (7, 9)).any()
    t = vis_util.draw_matches(torch.zeros(1, 9, 9, 3, dtype=torch.uint8, device="cuda"), _cuda(np.array([[[4.5, -10.0, 4.5, 20.0]]], np.float32)),
                              _cuda(np.array([1], np.int32)), colour=(200, 100, 50), radius=0.0).cpu().numpy()[0]
    assert np.array_equal(t[:, 4], np.tile(np.array([200, 100, 50], np.uint8), (9, 1))) and not t[:, 3].any() and not t[:, 5].any()
    src = np.random.default_rng(0).integers(0, 256, (1, 6, 8, 3)).astype(np.uint8)
    want = np.floor(src[0].reshape(3, 2, 4, 2, 3).astype(np.float64).mean(axis=(1, 3)) + 0.5).astype(np.uint8)
    assert np.array_equal(vis_util.resize_area(_cuda(src), (3, 4)).cpu().numpy()[0], want)
    with pytest.raises(_lib.FoundPoseNativeError, match="downscaling"):
        vis_util.resize_area(_cuda(src), (7, 8))
    with pytest.raises(_lib.FoundPoseNativeError):
        vis_util.contour(torch.zeros(1, 9, 9, 3, dtype=torch.uint8, device="cuda"), _cuda(m), (0, 255, 0), 99)


@pytest.mark.parametrize("H,W", SIZES)
def test_float_kernels_within_one_level(H, W):
    rng = np.random.default_rng(H * 77 + W)
    B = 2
    gh, gw, C = max(1, H // 14), max(1, W // 14), 5
    fmap = rng.normal(size=(B, gh, gw, C)).astype(np.float32)
    got = vis_util.pca_colorize(_cuda(fmap), (H, W)).cpu().numpy()
    want = np.stack([vr.pca_colorize(fmap[b], H, W) for b in range(B)])
    _close(got, want, f"pca_colorize {H}x{W}")
    dim = vis_util.pca_colorize(_cuda(fmap), (H, W), dim=(9, 10)).cpu().numpy()
    assert np.array_equal(dim, vr.darken(got))                              # (9 q) // 10: integer, exact
    src = rng.integers(0, 256, (B, 2 * H + 1, 3 * W + 2, 3)).astype(np.uint8)
    got = vis_util.resize_area(_cuda(src), (H, W)).cpu().numpy()
    _close(got, np.stack([vr.resize_area(src[b], H, W) for b in range(B)]), f"resize_area -> {H}x{W}")
    N = 24
    segs = np.stack([rng.uniform(-3, W + 3, (B, N)), rng.uniform(-3, H + 3, (B, N)), rng.uniform(-3, W + 3, (B, N)), rng.uniform(-3, H + 3, (B, N))], -1).astype(np.float32)
    segs[0, 0, 2:] = segs[0, 0, :2]                                         # a zero-length segment
    counts = np.array([N, 5], np.int32)
    tile = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    for alpha in (1.0, 0.6):
        got = vis_util.draw_matches(_cuda(tile).clone(), _cuda(segs), _cuda(counts), alpha=alpha).cpu().numpy()
        want = np.stack([vr.draw_matches(tile[b], segs[b, :counts[b]], alpha=alpha) for b in range(B)])
        _close(got, want, f"draw_matches {H}x{W} alpha {alpha}")


def _pictures(img, masks, fmap, strip, segs, counts, H, W):
    """The kernel chain of one tile (without the rasterizer and the extractor): rows 1..3 stacked."""
    left1 = vis_util.mask_tint(img, masks)
    right1 = vis_util.contour(img.clone(), masks, vis_util.COLOUR_FINAL)
    h2 = int(strip.shape[1] * 2 * W / strip.shape[2])
    row2 = vis_util.resize_area(strip, (h2, 2 * W))
    row3 = torch.cat([vis_util.pca_colorize(fmap, (H, W), dim=(9, 10)), vis_util.pca_colorize(fmap.flip(1), (H, W))], dim=2)
    vis_util.draw_matches(row3, segs, counts)
    return torch.cat([torch.cat([left1, right1], dim=2), row2, row3], dim=1)


def test_batch_invariance_at_production_shape():
    """Batch 32 at 518 x 518, 5 templates, 100 matches: detection 6 is bit-identical alone and as the 7th of 32, and within a level of the restatement."""
    g = torch.Generator(device="cuda").manual_seed(3)
    B, H, W, n = 32, 518, 518, 5
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    cx = torch.rand(B, generator=g, device="cuda") * W
    masks = (((yy[None] - 260) ** 2 + (xx[None] - cx[:, None, None]) ** 2) < 150 ** 2).to(torch.uint8)
    fmap = torch.randn(B, 37, 37, 256, generator=g, device="cuda")
    strip = torch.randint(0, 256, (B, H, n * W, 3), generator=g, device="cuda", dtype=torch.uint8)
    segs = torch.rand(B, 100, 4, generator=g, device="cuda") * torch.tensor([W, H, W, H], device="cuda") + torch.tensor([0, 0, W, 0], device="cuda")
    counts = torch.randint(60, 101, (B,), generator=g, device="cuda", dtype=torch.int32)
    batch = _pictures(img, masks, fmap, strip, segs, counts, H, W)
    again = _pictures(img, masks, fmap, strip, segs, counts, H, W)
    assert torch.equal(batch, again)
    k = 6
    alone = _pictures(img[k:k + 1], masks[k:k + 1], fmap[k:k + 1], strip[k:k + 1], segs[k:k + 1], counts[k:k + 1], H, W)
    assert batch.shape == (B, H + int(H * 2 * W / (n * W)) + H, 2 * W, 3) and torch.equal(alone[0], batch[k])
    i, m, f, s = img[k].cpu().numpy(), masks[k].cpu().numpy(), fmap[k].cpu().numpy(), strip[k].cpu().numpy()
    q = vr.pca_colorize(f, H, W)
    want = vr.tile(vr.mask_tint(i, m), vr.contour(i, m, vis_util.COLOUR_FINAL), [s[:, j * W:(j + 1) * W] for j in range(n)], vr.darken(q),
                   vr.pca_colorize(f[::-1], H, W), segs[k, :int(counts[k])].cpu().numpy())
    got = batch[k].cpu().numpy()
    assert np.array_equal(got[:H], want[:H])                                # row 1: integer
    _close(got[H:], want[H:], "rows 2 and 3 at 518 x 518")


def test_match_selection_matches_the_restatement():
    rng = np.random.default_rng(5)
    B, K, W, H = 4, 40, 32, 24
    conf = rng.integers(0, 6, (B, K)).astype(np.float32) / 5                # many ties
    conf[1, 3] = conf[1, 9] = np.nan
    counts = np.array([40, 17, 0, 3], np.int32)
    left = rng.uniform(0, W, (B, K, 2))
    right = rng.uniform(-6, W + 6, (B, K, 2))
    segs, kept = vis_util.select_matches(_cuda(conf), _cuda(counts), _cuda(left), _cuda(right), 10, W, H)
    for b in range(B):
        want = vr.select_matches(conf[b, :counts[b]], left[b, :counts[b]], right[b, :counts[b]], 10, W, H)
        assert int(kept[b]) == len(want)
        assert np.array_equal(segs[b, :len(want)].cpu().numpy(), want.astype(np.float32)), b


# ---------------------------------------------------------------------------------------------------- frame summary
def _rasterizer():
    from foundpose_amd.renderer import HipRasterizer
    ras = HipRasterizer("cuda")
    ras.add_object_model(1, mesh=synthetic.make_blob_mesh(30, 30, radius=55.0, seed=7))
    ras.add_object_model(2, mesh=synthetic.make_blob_mesh(24, 24, radius=40.0, seed=9))
    return ras


def _pose(rx, t):
    c, s = np.cos(rx), np.sin(rx)
    T = np.eye(4)
    T[:3, :3] = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    T[:3, 3] = t
    return T


def test_frame_summary_two_objects_with_occlusion():
    ras = _rasterizer()
    H, W = 96, 128
    cam = PinholePlaneCameraModel(W, H, (150.0, 150.0), (64.0, 48.0), np.eye(4))
    image = np.random.default_rng(1).integers(0, 256, (H, W, 3)).astype(np.uint8)
    poses = [(1, _pose(0.4, [-15.0, 0.0, 420.0]), None), (2, _pose(1.1, [20.0, 5.0, 330.0]), (10, 20, 250)),   # object 2 in front of part of object 1
             (1, _pose(2.0, [0.0, 0.0, 50.0]), None)]                                                          # within the near plane: skipped
    pic, ids, notes = vis_util.vis_frame_summary(image, cam, poses, ras)
    assert len(notes) == 1 and "pose 2" in notes[0]
    depth = np.zeros((3, H, W), np.float32)
    for k, (obj, T, _) in enumerate(poses[:2]):
        view = PinholePlaneCameraModel(W, H, cam.f, cam.c, np.linalg.inv(T))
        depth[k] = ras.render_views(obj, [view], with_color=False)["depth"][0].cpu().numpy()
    z = np.where(depth > 0, depth, np.inf)
    want_ids = np.where(np.isfinite(z.min(0)), z.argmin(0), -1)
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, want_ids)
    both = (depth[0] > 0) & (depth[1] > 0)
    assert both.sum() > 50 and (ids[both] == 1).all() and (ids == 0).sum() > 50    # a real occlusion, decided for the nearer object
    colours = [vis_util.palette_colour(1), (10, 20, 250), vis_util.palette_colour(1)]
    want, _ = vr.scene_composite(image, depth, colours)
    for k in range(3):
        want = vr.contour(want, ids == k, colours[k])
    assert np.array_equal(pic.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- the driver
def _vis_scene(tmp_path):
    from foundpose_amd import feature_util, repre_util
    from tests.test_gpu_infer_driver import NAME, _scene
    ex = feature_util.make_feature_extractor(NAME, random_init_seed=1234, precision="fp32").to("cuda")
    sc = _scene(tmp_path, ex)
    repre = repre_util.load_object_repre(sc["rdir"])
    # what gen_repre adds for the pictures: the template images, their cameras (model -> camera), the visualisation projector
    img = torch.from_numpy(sc["image"]).cuda().float() / 255.0
    from foundpose_amd import crop_util
    crops, cmasks, cams = crop_util.crop_detections(img, torch.from_numpy(sc["masks"]).cuda(), sc["boxes_xyxy"], sc["cam"], (224, 224), 0.2)
    tpl = torch.randint(0, 256, (12, 3, 224, 224), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    tcams = [{"f": torch.tensor(cams[0].f), "c": torch.tensor(cams[0].c), "width": 224, "height": 224, "T_world_from_eye": torch.eye(4, dtype=torch.float64)} for _ in range(12)]
    for b, s in enumerate((3, 7)):
        tpl[s] = (crops[b] * 255.0 + 0.5).clamp(0, 255).to(torch.uint8).cpu()
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = sc["R"][b].numpy(), sc["t"][b].numpy()
        tcams[s] = {"f": torch.tensor(cams[b].f), "c": torch.tensor(cams[b].c), "width": 224, "height": 224, "T_world_from_eye": torch.from_numpy(np.linalg.inv(T))}
    repre.templates, repre.template_cameras_cam_from_model = tpl, tcams
    repre.feat_vis_projectors = [repre.feat_raw_projectors[0]]
    return ex, sc, repre, (crops, cmasks, cams)


def _strip_times(entries):
    return [{k: (sorted(v) if k == "time" else v) for k, v in e.items()} for e in entries]


def test_driver_writes_tiles_and_summary_and_changes_nothing_without_a_renderer(tmp_path):
    from PIL import Image
    from foundpose_amd import infer, infer_pose_util
    ex, sc, repre, (crops, cmasks, cams) = _vis_scene(tmp_path)
    ras = _rasterizer()
    frames = lambda lid: iter([{"scene_id": 1, "im_id": 3, "image": sc["image"], "camera": sc["cam"]}])
    dets = infer_pose_util.load_detections_in_bop_format(str(sc["det_path"]))
    run = lambda name, opts, **kw: infer.infer(opts, frames, dets, {1: repre}, str(tmp_path / name), extractor=ex, num_target_insts={1: {(1, 3): 1}}, **kw)
    on = sc["opts"]._replace(vis_results=True, vis_corresp_top_n=30)
    run("off", sc["opts"]._replace(vis_results=False))
    run("plain", on)                                        # vis_results true, no renderer: nothing changes
    paths = run("vis", on, renderer=ras)
    run("quiet", sc["opts"]._replace(vis_results=False), renderer=ras)   # a renderer, vis_results false: nothing is written either

    def listing(name):
        return sorted(os.path.relpath(os.path.join(d, f), tmp_path / name) for d, _, fs in os.walk(tmp_path / name) for f in fs)
    load = lambda name: json.load(open(tmp_path / name / "1" / "estimated-poses.json"))
    assert listing("off") == listing("plain") == listing("quiet")
    # (the "time" values are wall-clock measurements and differ between any two runs: their keys are compared, every other field is equal)
    assert _strip_times(load("off")) == _strip_times(load("plain")) == _strip_times(load("quiet"))
    est = load("vis")
    assert len(est) == 2 and all(set(e["time"]) == set(load("off")[0]["time"]) | {"vis"} and e["time"]["vis"] > 0 for e in est)
    for a, b in zip(est, load("off")):                      # keep_feature_map turns the token selection off: same poses to solver tolerance
        assert np.abs(np.array(a["R"]) - np.array(b["R"])).max() < 1e-2
    want_files = sorted([os.path.join("1", f"1_3_1_{e['inst_id']}_0.png") for e in est] + [os.path.join("vis", "1_3.png")])
    assert sorted(set(listing("vis")) - set(listing("off"))) == want_files
    assert paths[-1].endswith(os.path.join("vis", "1_3.png"))
    H = W = 224
    h2 = int(224 * 2 * W / (5 * 224))
    summary = np.asarray(Image.open(tmp_path / "vis" / "vis" / "1_3.png"))
    assert summary.shape == sc["image"].shape and (summary != sc["image"]).any()

    # ---- the same chain by hand
    from foundpose_amd import engine as fe, pnp_util
    from foundpose_amd.bank import DeviceBank
    o = on
    eng = fe.FoundPoseEngine(ex, DeviceBank([repre]), o.grid_cell_size, o.match_top_n_templates, o.match_top_k_buddies, tie_order="torch")
    res = eng.infer_batch(crops, cmasks, [0, 0], keep_feature_map=True)
    poses = pnp_util.estimate_poses(res, cams, o.pnp_type, o.pnp_ransac_iter, o.pnp_inlier_thresh, o.pnp_required_ransac_conf, o.pnp_refine_lm)
    best = pnp_util.select_best_coarse(poses)
    assert best["found"].all()
    cid = best["corresp_id"].cpu().tolist()
    crop_u8 = (crops.permute(0, 2, 3, 1) * 255.0 + 0.5).clamp(0, 255).to(torch.uint8).cpu().numpy()
    for e in est:
        b = int(e["inst_id"])
        tile = np.asarray(Image.open(tmp_path / "vis" / "1" / f"1_3_1_{b}_0.png"))
        assert tile.shape == (H + h2 + H, 2 * W, 3)
        # row 1: tinted mask | the green contour of the rasterizer's own mask at the returned pose, nothing else painted
        assert np.array_equal(tile[:H, :W], vr.mask_tint(crop_u8[b], cmasks[b].cpu().numpy()))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = best["R"][b].cpu().numpy(), best["t"][b].cpu().numpy()
        view = PinholePlaneCameraModel(W, H, cams[b].f, cams[b].c, np.linalg.inv(T))
        mask = ras.render_views(1, [view], with_color=False)["mask"][0].cpu().numpy()
        assert mask.any()
        assert np.array_equal(tile[:H, W:], vr.contour(crop_u8[b], mask, vis_util.COLOUR_FINAL))
        # row 2: the retrieved templates, area-resized
        ids = res.template_ids[b].cpu().tolist()
        strip = np.concatenate([repre.templates[i].permute(1, 2, 0).numpy() for i in ids], axis=1)
        _close(tile[H:H + h2], vr.resize_area(strip, h2, 2 * W), f"template strip of instance {b}")
        # row 3: (9 q) // 10 of the query's PCA picture on the left, and the match colour at both ends of every kept match
        j = cid[b]
        assert ids[j] == (3, 7)[b]
        n = int(res.counts[b, j])
        X = res.coord_3d[b, j, :n].cpu().numpy().astype(np.float64)
        Xc = X @ sc["R"][b].numpy().T + sc["t"][b].numpy()
        right = Xc[:, :2] / Xc[:, 2:] * np.array(cams[b].f) + np.array(cams[b].c)
        segs = vr.select_matches(res.conf[b, j, :n].cpu().numpy(), res.coord_2d[b, j, :n].cpu().numpy(), right, 30, W, H)
        assert len(segs) >= 10
        q = vr.darken(vr.pca_colorize(res.feature_map[b].cpu().numpy(), H, W))
        untouched = (vr.draw_matches(np.zeros((H, 2 * W, 3), np.uint8), segs, colour=(255, 255, 255)) == 0).all(-1)[:, :W]
        d = np.abs(tile[H + h2:, :W].astype(int) - q.astype(int))[untouched]
        assert d.max() <= 1 and d.mean() < 0.05
        for x0, y0, x1, y1 in segs:
            for x, y in ((x0, y0), (x1, y1)):
                assert tile[H + h2 + min(int(y), H - 1), min(int(x), 2 * W - 1)].tolist() == list(vis_util.MATCH_COLOUR), (b, x, y)


def test_refused_pose_and_unbuilt_layout(tmp_path):
    """A pose within the near plane skips its contour with a note instead of raising; the labelled layout is refused."""
    ex, sc, repre, (crops, cmasks, cams) = _vis_scene(tmp_path)
    from foundpose_amd import engine as fe
    from foundpose_amd.bank import DeviceBank
    ras = _rasterizer()
    res = fe.FoundPoseEngine(ex, DeviceBank([repre]), 14.0, 5, 300, tie_order="torch").infer_batch(crops, cmasks, [0, 0], keep_feature_map=True)
    far, near = _pose(0.3, [0.0, 0.0, 900.0]), _pose(0.3, [0.0, 0.0, 60.0])
    kw = dict(repre=repre, rasterizer=ras, object_id=1, extractor=ex, vis_corresp_top_n=20)
    tiles, rec = vis_util.vis_inference_results_batch(crops, cmasks, cams, res, [True, True], [0, 0], [far, far], [far, near], poses_gt=[near, None],
                                                      draw_coarse=True, **kw)
    assert tiles.shape[0] == 2 and not rec[0]["notes"] == [] and len(rec[1]["notes"]) == 1 and "final pose of detection 1" in rec[1]["notes"][0]
    right = tiles[:, :224, 224:].cpu().numpy()
    is_col = lambda img, c: (img == np.array(c, np.uint8)).all(-1)
    assert is_col(right[0], vis_util.COLOUR_FINAL).sum() > 20 and is_col(right[1], vis_util.COLOUR_COARSE).sum() > 20
    assert is_col(right[1], vis_util.COLOUR_FINAL).sum() == 0                # its final pose was refused
    plain, _ = vis_util.vis_inference_results_batch(crops, cmasks, cams, res, [True, True], [0, 0], [far, far], [far, far], vis_feat_map=False, **kw)
    assert plain.shape == tiles.shape
    with pytest.raises(NotImplementedError):
        vis_util.vis_inference_results_batch(crops, cmasks, cams, res, [True, True], [0, 0], [far, far], [far, far], vis_for_paper=False, **kw)
