"""GPU end to end with a textured model: a BOP tree holding a binary textured PLY and its PNG -> gen_templates (depth and
mask identical to the same geometry saved untextured, rgb from the texture) -> gen_repre -> a template as the query ->
PnP recovers its pose, as tests/test_gpu_onboarding.py does for a vertex-coloured model."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from foundpose_amd import engine as fe
from foundpose_amd import feature_util, gen_repre, gen_templates, pnp_util, repre_util, synthetic
from foundpose_amd.bank import DeviceBank
from foundpose_amd.crop_util import PinholePlaneCameraModel
from foundpose_amd.renderer import Mesh, load_ply, save_ply

pytestmark = pytest.mark.gpu
NAME = "dinov2_version=vits14-reg_stride=14_facet=token_layer=9_logbin=0_norm=1"


def _bop_root(root, name, mesh):
    d = os.path.join(root, name)
    os.makedirs(os.path.join(d, "models"))
    save_ply(os.path.join(d, "models", "obj_000001.ply"), mesh)
    with open(os.path.join(d, "models", "models_info.json"), "w") as f:
        json.dump({"1": {"diameter": 200.0}}, f)
    with open(os.path.join(d, "camera.json"), "w") as f:
        json.dump({"cx": 325.26, "cy": 242.05, "fx": 572.41, "fy": 573.57, "width": 640, "height": 480, "depth_scale": 1.0}, f)


def _rot_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def _png(path):
    return np.asarray(Image.open(path))


def test_textured_mesh_to_pose(tmp_path):
    root = str(tmp_path)
    mesh = synthetic.make_textured_blob_mesh(50, 50, radius=55.0, seed=7, tex_size=512)
    _bop_root(root, "tex", mesh)
    _bop_root(root, "plain", Mesh(mesh.vertices, mesh.faces, mesh.colors, mesh.normals))
    ply = os.path.join(root, "tex", "models", "obj_000001.ply")
    assert open(ply, "rb").read(40).startswith(b"ply\nformat binary_little_endian") and os.path.exists(ply[:-4] + ".png")
    assert load_ply(ply, textured=True).texture.shape == (512, 512, 3)
    held = {}
    for ds in ("tex", "plain"):
        opts = gen_templates.load_opts({"gen_templates_opts": {"version": "v1", "object_dataset": ds, "object_lids": None,
                                                               "min_num_viewpoints": 9, "num_inplane_rotations": 2, "crop_size": [224, 224]}})
        held[ds] = gen_templates.synthesize_templates(opts, root, root, (450.0, 550.0), return_templates=True)
    dirs = {ds: os.path.join(root, "templates", "v1", ds, "1") for ds in ("tex", "plain")}
    meta = json.load(open(os.path.join(dirs["tex"], "metadata.json")))
    assert len(meta) == 18
    textured_px = 0
    for k in range(18):
        for kind in ("depth", "mask"):
            a = _png(os.path.join(dirs["tex"], kind, f"template_{k:04d}.png"))
            b = _png(os.path.join(dirs["plain"], kind, f"template_{k:04d}.png"))
            assert a.dtype == b.dtype and np.array_equal(a, b), (kind, k)
        m = _png(os.path.join(dirs["tex"], "mask", f"template_{k:04d}.png")) > 0
        rgb = _png(os.path.join(dirs["tex"], "rgb", f"template_{k:04d}.png")).astype(np.int32)
        plain = _png(os.path.join(dirs["plain"], "rgb", f"template_{k:04d}.png")).astype(np.int32)
        assert m.sum() > 1000
        # the texture, not the vertex colours and not grey: the rgb differs from the vertex-coloured template and is coloured
        assert np.abs(rgb - plain)[m].mean() > 5.0
        spread = rgb[m].max(1) - rgb[m].min(1)
        textured_px += int((spread > 30).sum())
    assert textured_px > 18 * 1000
    for k in ("depth", "mask"):
        assert torch.equal(held["tex"][1][k], held["plain"][1][k])
    ro = gen_repre.load_opts({"gen_repre_opts": {"version": "v1", "templates_version": "v1", "object_dataset": "tex", "object_lids": [1],
                                                 "extractor_name": NAME, "pca_components": 64, "cluster_num": 32,
                                                 "template_desc_opts": {"desc_type": "tfidf"}}})
    ex = feature_util.make_feature_extractor(NAME, random_init_seed=1234, precision="fp32").to("cuda")
    out_dir = gen_repre.generate_repre(ro, "tex", 1, root, extractor=ex)
    assert os.path.exists(os.path.join(out_dir, "repre.pth"))
    disk = repre_util.load_object_repre(out_dir)
    eng = fe.FoundPoseEngine(ex, DeviceBank([disk]), 14.0, 5, 300, tie_order="torch")
    for k in (5, 12):
        crop = disk.templates[k:k + 1].cuda().float() / 255.0
        mask = torch.from_numpy(_png(meta[k]["binary_mask_path"])[None].copy()).cuda()
        res = eng.infer_batch(crop, mask)
        assert int(res.template_ids[0, 0]) == k
        c = meta[k]["cameras"]
        cam = PinholePlaneCameraModel(c["ImageSizeX"], c["ImageSizeY"], (c["fx"], c["fy"]), (c["cx"], c["cy"]), np.array(c["T_WorldFromCamera"]))
        corr = res.corresp_list(0)[0]
        assert int(corr["template_id"]) == k
        ok, R, t, inl, q = pnp_util.estimate_pose(corr, cam, "opencv", 1000, 10.0, 0.99, True)
        assert ok
        T_cw = np.linalg.inv(cam.T_world_from_eye)
        assert _rot_deg(R, T_cw[:3, :3]) < 1.0, _rot_deg(R, T_cw[:3, :3])
        assert np.linalg.norm(t.reshape(3) - T_cw[:3, 3]) < 2.0, (t.reshape(3), T_cw[:3, 3])
