"""GPU: foundpose_amd.reconstruct with fill "carve" through its command line, on the blob of
tests/test_gpu_reconstruct.py seen from its six upper viewpoints only: the mesh that comes out is closed, has the original's volume, is
coloured all over, and is the mesh the numpy restatement (tests/tsdf_ref.py, tests/tsdf_fill_ref.py) makes from the same files."""
import json

import numpy as np
import pytest
import torch

from foundpose_amd import reconstruct, synthetic
from foundpose_amd.eval_bop19 import _Camera, _m2c
from foundpose_amd.renderer import HipRasterizer, load_ply
from tests import tsdf_fill_ref as fill, tsdf_ref as ref

pytestmark = pytest.mark.gpu
H_MM = 2.5


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    root = tmp_path_factory.mktemp("reconstruct_fill")
    original = synthetic.make_blob_mesh(24, 24, radius=40)
    ras = HipRasterizer("cuda")
    ras.add_object_model(1, mesh=original)
    r = ras.render_views(1, [_Camera(ref.SEQ_K, ref.SEQ_W, ref.SEQ_H, np.linalg.inv(_m2c(R, t))) for R, t in ref.sequence_poses()])
    r = {k: r[k].cpu().numpy() for k in ("color", "depth", "mask")}
    upper = [i for i, e in enumerate(ref.fibonacci_eyes()) if e[2] > 0]
    assert len(upper) == 6
    ref.write_scene(str(root / "upper" / "000001"), upper, r["color"], r["depth"], r["mask"])
    return dict(root=root, original=original, sequence=str(root / "upper" / "000001"))


def _run(scene, name, opts):
    root = scene["root"]
    (root / f"{name}.json").write_text(json.dumps(opts))
    args = ["--sequence", scene["sequence"], "--obj-id", "1", "--output", str(root / name), "--opts", str(root / f"{name}.json"), "--report",
            str(root / f"{name}_report.json")]
    assert reconstruct.main(args) == 0
    return json.load(open(root / f"{name}_report.json")), load_ply(str(root / name / "obj_000001.ply"))


@pytest.mark.parametrize("with_plane", (False, True))
def test_the_filled_mesh_is_closed_coloured_and_the_restatements(scene, with_plane):
    original = scene["original"]
    plane = [0.0, 0.0, -1.0, float(original.vertices[:, 2].min())] if with_plane else None
    rep, mesh = _run(scene, "plane" if with_plane else "carve", {"voxel_mm": H_MM, "fill": "carve", "fill_plane": plane})
    print("dims", rep["dims"], "fill", rep["fill"], "boundary edges", rep["boundary_edges"])
    assert rep["watertight"] is True and rep["boundary_edges"] == 0 and rep["nonmanifold_edges"] == 0 and rep["note"] is None
    fl = rep["fill"]
    assert fl["filled_voxels"] > 0 and fl["uncoloured_voxels"] == 0 and (fl["smooth_iters"], fl["color_iters"]) == (4, 64) and fl["seconds"] > 0
    assert (fl["plane_voxels"] > 0) == with_plane and 0 < fl["last_change"] < 1
    assert rep["opts"]["fill"] == "carve" and rep["opts"]["fill_plane"] == plane and rep["frames_used"] == 6
    assert len(mesh.vertices) == rep["vertices"] > 1000 and len(mesh.faces) == rep["triangles"] > 2000
    # the restatement's mesh from the same files, in the volume the tool chose
    frames = reconstruct.read_sequence(scene["sequence"], 1, "mask_visib")
    vol = ref.new_volume(rep["bounds"][0], H_MM, tuple(rep["dims"]))
    ref.integrate(vol, np.stack([f.depth for f in frames]), np.stack([f.mask for f in frames]), np.stack([f.rgb for f in frames]),
                  np.array([f.cam for f in frames]), np.stack([f.pose for f in frames]), 4 * H_MM)
    filled, w_st = fill.fill_volume(vol, 2, 4, 64, plane)
    _, keys, pos, col = ref.extract(filled, 1)
    rv, rc, rf = ref.weld(keys, pos, col)
    rf = rf[reconstruct.largest_component(rf, len(rv))]
    used = np.zeros(len(rv), bool)
    used[rf.reshape(-1)] = True
    rv, rc, rf = rv[used], np.clip(rc[used], 0, 1), (np.cumsum(used) - 1)[rf].astype(np.int32)
    assert len(rv) == len(mesh.vertices) and np.array_equal(rf, mesh.faces)
    ulp = np.spacing(np.float32(np.abs(rv).max()))
    d = np.abs(rv.astype(np.float64) - mesh.vertices.astype(np.float64)).max()
    print("vertices differ by at most", d, "mm of", 2 * ulp, "; restatement's stats", w_st)
    assert d <= 2 * ulp
    assert {k: fl[k] for k in ("filled_voxels", "plane_voxels", "clipped_voxels", "snapped_voxels", "uncoloured_voxels")} == \
           {k: w_st[k] for k in ("filled_voxels", "plane_voxels", "clipped_voxels", "snapped_voxels", "uncoloured_voxels")}
    v0 = ref.signed_volume(original.vertices, original.faces)
    v1 = ref.signed_volume(mesh.vertices, mesh.faces)
    print("signed volume", v1, "of the original", v0, f"({100 * (v1 / v0 - 1):+.2f} %)")
    assert abs(v1 / v0 - 1) <= 0.04
    grey = np.float32(128.0) / np.float32(255.0)                        # what the 0.5 of an edge without colour is in the file
    assert not np.any(np.all(mesh.colors == grey, axis=1)) and not np.any(np.all(rc == np.float32(0.5), axis=1))
    torch.cuda.synchronize()


def test_the_default_path_still_reports_an_open_surface(scene):
    rep, _ = _run(scene, "none", {"voxel_mm": H_MM})
    assert rep["opts"]["fill"] == "none" and "fill" not in rep
    assert rep["boundary_edges"] > 0 and rep["watertight"] is False and "open" in rep["note"] and "nothing is filled" in rep["note"]
    torch.cuda.synchronize()
