"""GPU end to end: mesh -> gen_templates -> gen_repre -> correspondences -> PnP recovers the template's pose.  The first
check that the template camera, the depth units, the 3D registration and PnP agree on one convention; it holds with any
backbone weights, because the query crop IS a template."""
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import engine as fe
from foundpose_amd import feature_util, gen_repre, gen_templates, pnp_util, repre_util, synthetic
from foundpose_amd.bank import DeviceBank
from foundpose_amd.crop_util import PinholePlaneCameraModel
from foundpose_amd.renderer import save_ply

pytestmark = pytest.mark.gpu
NAME = "dinov2_version=vits14-reg_stride=14_facet=token_layer=9_logbin=0_norm=1"


def _bop_root(root):
    d = os.path.join(root, "synth")
    os.makedirs(os.path.join(d, "models"))
    mesh = synthetic.make_blob_mesh(50, 50, radius=55.0, seed=7)       # ~4.9k triangles, asymmetric, vertex-coloured
    save_ply(os.path.join(d, "models", "obj_000001.ply"), mesh)
    with open(os.path.join(d, "models", "models_info.json"), "w") as f:
        json.dump({"1": {"diameter": 200.0}}, f)
    with open(os.path.join(d, "camera.json"), "w") as f:
        json.dump({"cx": 325.26, "cy": 242.05, "fx": 572.41, "fy": 573.57, "width": 640, "height": 480, "depth_scale": 1.0}, f)
    return mesh


def _rot_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def test_mesh_to_pose(tmp_path):
    root = str(tmp_path)
    _bop_root(root)
    opts = gen_templates.load_opts({"gen_templates_opts": {"version": "v1", "object_dataset": "synth", "object_lids": None,
                                                           "min_num_viewpoints": 9, "num_inplane_rotations": 2, "crop_size": [224, 224]}})
    held = gen_templates.synthesize_templates(opts, root, root, (450.0, 550.0), return_templates=True)
    tdir = os.path.join(root, "templates", "v1", "synth", "1")
    meta = json.load(open(os.path.join(tdir, "metadata.json")))
    assert len(meta) == 18 and os.path.exists(os.path.join(tdir, "rgb", "template_0017.png"))
    assert meta[3]["cameras"]["ImageSizeX"] == 224 and meta[3]["pose"]["R"] == np.eye(3).tolist()
    ro = gen_repre.load_opts({"gen_repre_opts": {"version": "v1", "templates_version": "v1", "object_dataset": "synth", "object_lids": [1],
                                                 "extractor_name": NAME, "pca_components": 64, "cluster_num": 32,
                                                 "template_desc_opts": {"desc_type": "tfidf"}}})
    ex = feature_util.make_feature_extractor(NAME, random_init_seed=1234, precision="fp32").to("cuda")
    disk = repre_util.load_object_repre(gen_repre.generate_repre(ro, "synth", 1, root, extractor=ex))
    # the in-memory handoff builds the same bank
    mem_dir = gen_repre.generate_repre(ro._replace(version="mem"), "synth", 1, root, extractor=ex, templates=held[1])
    mem = repre_util.load_object_repre(mem_dir)
    for k in ("vertices", "feat_vectors", "feat_to_template_ids", "feat_to_vertex_ids", "templates", "template_descs",
              "feat_cluster_centroids", "feat_cluster_idfs"):
        assert torch.equal(getattr(disk, k), getattr(mem, k)), k
    # a template as the query: it is retrieved first, and PnP on its correspondences returns its camera pose
    eng = fe.FoundPoseEngine(ex, DeviceBank([disk]), 14.0, 5, 300, tie_order="torch")
    from PIL import Image
    for k in (5, 12):
        crop = disk.templates[k:k + 1].cuda().float() / 255.0
        mask = torch.from_numpy(np.asarray(Image.open(meta[k]["binary_mask_path"]))[None].copy()).cuda()
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
