"""GPU: foundpose_amd.reconstruct end to end through its command line, on a sequence rendered here: a blob seen from twelve viewpoints
all round, written as a BOP scene directory.  The mesh that comes out loads, has the original's diameter, and renders back onto the
input frames as well as the mesh the numpy restatement (tests/tsdf_ref.py) makes from the same files."""
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import models_info, reconstruct, synthetic
from foundpose_amd.eval_bop19 import _Camera, _m2c
from foundpose_amd.renderer import HipRasterizer, Mesh, load_ply, vertex_normals
from tests import tsdf_ref as ref

pytestmark = pytest.mark.gpu
H_MM = 2.5


def _cameras():
    return [_Camera(ref.SEQ_K, ref.SEQ_W, ref.SEQ_H, np.linalg.inv(_m2c(R, t))) for R, t in ref.sequence_poses()]


def _render(mesh):
    ras = HipRasterizer("cuda")
    ras.add_object_model(1, mesh=mesh)
    r = ras.render_views(1, _cameras())
    return {k: r[k].cpu().numpy() for k in ("color", "depth", "mask")}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    root = tmp_path_factory.mktemp("reconstruct")
    original = synthetic.make_blob_mesh(24, 24, radius=40)
    r = _render(original)
    upper = [i for i, e in enumerate(ref.fibonacci_eyes()) if e[2] > 0]
    assert len(upper) == 6
    ref.write_scene(str(root / "all" / "000001"), range(ref.SEQ_VIEWS), r["color"], r["depth"], r["mask"])
    ref.write_scene(str(root / "upper" / "000001"), upper, r["color"], r["depth"], r["mask"])
    (root / "opts.json").write_text(json.dumps({"voxel_mm": H_MM}))
    args = ["--sequence", str(root / "all" / "000001"), "--obj-id", "1", "--output", str(root / "models"), "--opts", str(root / "opts.json"),
            "--report", str(root / "report.json")]
    assert reconstruct.main(args) == 0
    return dict(root=root, original=original, args=args, report=json.load(open(root / "report.json")))


def test_the_mesh_serves_downstream_and_matches_the_restatement(run):
    root, rep = run["root"], run["report"]
    path = str(root / "models" / "obj_000001.ply")
    assert rep["output"] == path and rep["frames_used"] == 12 and rep["opts"]["voxel_mm"] == H_MM and rep["observed_voxels"] > 0
    mesh = load_ply(path)
    assert len(mesh.vertices) == rep["vertices"] > 1000 and len(mesh.faces) == rep["triangles"] > 2000
    assert np.ptp(mesh.colors, axis=0).min() > 0.3                     # vertex colours came through, not one grey
    v = run["original"].vertices.astype(np.float64)
    d0 = np.sqrt(((v[:, None] - v[None]) ** 2).sum(-1).max())
    d1 = models_info.calc_models_info(str(root / "models"))[1]["diameter"]
    print("diameter", d1, "of the original", d0)
    assert abs(d1 - d0) <= 2 * H_MM
    # the restatement's mesh from the same files, in the volume the tool chose
    frames = reconstruct.read_sequence(str(root / "all" / "000001"), 1, "mask_visib")
    rv, rc, rf = ref.mesh_from_frames(frames, rep["bounds"][0], H_MM, tuple(rep["dims"]), 4 * H_MM, 2, reconstruct.largest_component)
    assert len(rv) == len(mesh.vertices) and np.array_equal(rf, mesh.faces)
    print("vertices differ by at most", np.abs(rv - mesh.vertices).max(), "mm")
    in_depth, in_mask = np.stack([f.depth for f in frames]), np.stack([f.mask for f in frames])
    got = _render(mesh)
    want = _render(Mesh(rv, rf, rc.astype(np.float32), vertex_normals(rv, rf)))
    g = ref.render_agreement(got["depth"], got["mask"], in_depth, in_mask)
    w = ref.render_agreement(want["depth"], want["mask"], in_depth, in_mask)
    print("median |d depth|, 95th percentile, silhouette IoU: kernel", g, "restatement", w)
    assert g[0] <= w[0] + 1e-3 and g[1] <= w[1] + 1e-3 and g[2] >= w[2] - 1e-3
    assert g[0] <= H_MM                                                # a sign or pose-direction error lands tau = 4 h away


def test_a_second_run_is_refused(run):
    path = run["root"] / "models" / "obj_000001.ply"
    before = os.stat(path).st_mtime_ns
    with pytest.raises(FileExistsError):
        reconstruct.main(run["args"])
    assert os.stat(path).st_mtime_ns == before
    assert reconstruct.main(run["args"] + ["--overwrite"]) == 0
    assert json.load(open(run["root"] / "report.json"))["vertices"] == run["report"]["vertices"]


def test_the_report_tells_a_closed_surface_from_an_open_one(run):
    rep, root = run["report"], run["root"]
    assert rep["boundary_edges"] == 0 and rep["watertight"] is True and rep["note"] is None
    r = reconstruct.reconstruct([str(root / "upper" / "000001")], 1, str(root / "models_upper"), {"voxel_mm": H_MM})
    assert r["frames_used"] == 6 and r["boundary_edges"] > 0 and r["watertight"] is False and "open" in r["note"]
    torch.cuda.synchronize()
