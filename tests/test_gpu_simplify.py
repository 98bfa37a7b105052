"""GPU: fp_mesh_cell_keys and fp_mesh_cluster (csrc/simplify.hip), the face rules and the command line of foundpose_amd/simplify.py against
the numpy restatement tests/simplify_ref.py, on the fixtures whose conditions tests/test_simplify_cpu.py asserts: no grid coordinate on
a cell border, no eigenvalue at the truncation threshold, no solve at the box test's bounds.  The comparison therefore has no exclusions."""
import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops, simplify
from foundpose_amd.renderer import Mesh, load_ply, save_ply
from foundpose_amd.synthetic import make_blob_mesh
from tests import simplify_ref as ref

pytestmark = pytest.mark.gpu
OUTPUTS = ("positions", "colors", "quadrics", "means", "err", "status")
TABLES = ("cells", "rank", "vert_order", "vert_begin", "corner_order", "corner_begin")


def _blob():
    m = make_blob_mesh(24, 24, radius=40)
    return m.vertices, m.faces, m.colors


def _fixture(name):
    if name == "cube":
        v, f = ref.cube_mesh()
        return v, f, ref.fixture_colors(len(v), 1), 7.3
    if name == "stride":
        v, f = ref.stride_mesh()
        return v, f, ref.fixture_colors(len(v), 4), ref.STRIDE_CELL
    return (*_blob(), 9.0)


def _device_cluster(v, f, col, c, origin=None, dims=None):
    v64 = v.astype(np.float64)
    if origin is None:
        origin, dims = simplify.grid_for(v64.min(0), v64.max(0), c)
    dv, df, dc = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), torch.from_numpy(col).cuda()
    keys = ops.mesh_cell_keys(dv, origin, c, dims)
    tb = ops.mesh_cluster_tables(keys, df)
    out = ops.mesh_cluster(dv, dc, df, tb, origin, c, dims)
    return keys.cpu().numpy(), {k: t.cpu().numpy() for k, t in tb.items()}, {k: t.cpu().numpy() for k, t in out.items()}, origin, dims


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("name", ["cube", "blob"])
def test_keys_equal_the_restatement(name):
    v, f, col, c = _fixture(name)
    origin, dims = ref.grid_for(v, c)
    got_origin, got_dims = simplify.grid_for(v.astype(np.float64).min(0), v.astype(np.float64).max(0), c)
    assert np.array_equal(origin, got_origin) and dims == got_dims
    keys = ops.mesh_cell_keys(torch.from_numpy(v).cuda(), origin, c, dims).cpu().numpy()
    assert keys.dtype == np.int64 and np.array_equal(keys, ref.cell_keys(v, origin, c, dims))
    assert len(v) % 256 != 0 and len(v) > 256                      # a ragged last workgroup, and more than one


@pytest.mark.parametrize("name", ["cube", "blob", "stride"])
def test_cluster_equals_the_restatement(name):
    """The ten sums and the mean bit for bit, the status equal, positions within 2 fp32 ulp of the coordinate, colours within 1e-6.
    err = x'Ax + 2 b'x + s cancels three terms of the size of s, and the positions agree to about 1e-12 relative: 1e-9 (s + 1)."""
    v, f, col, c = _fixture(name)
    keys, tb, got, origin, dims = _device_cluster(v, f, col, c)
    w_tb = ref.tables(ref.cell_keys(v, origin, c, dims), f)
    for k in TABLES:
        assert tb[k].dtype == np.int64 and np.array_equal(tb[k], w_tb[k]), k
    want = ref.cluster(v, col, f, w_tb, origin, c, dims)
    corners, verts = np.diff(w_tb["corner_begin"]), np.diff(w_tb["vert_begin"])
    if name == "stride":
        assert {1, 63, 64, 65} <= set(corners.tolist()) and corners.max() >= 129 and (verts[corners == 0] == 130).any()
        assert -1 in want["status"]
    assert np.array_equal(_bits(got["quadrics"]), _bits(want["quadrics"]))
    assert np.array_equal(_bits(got["means"]), _bits(want["means"]))
    assert got["status"].dtype == np.int32 and np.array_equal(got["status"], want["status"])
    dpos = np.abs(got["positions"].astype(np.float64) - want["positions"].astype(np.float64))
    ulp = np.spacing(np.abs(want["positions"])).astype(np.float64)
    dcol = np.abs(got["colors"].astype(np.float64) - want["colors"].astype(np.float64)).max()
    derr = np.abs(got["err"] - want["err"])
    print(name, "cells", len(want["status"]), "positions: differing", int((dpos > 0).sum()), "largest", dpos.max(), "mm,", (dpos / ulp).max(), "ulp;",
          "colours", dcol, "; err", derr.max(), "of", (1e-9 * (want["quadrics"][:, 9] + 1)).min())
    assert (dpos <= 2 * ulp).all()
    assert dcol <= 1e-6
    assert (derr <= 1e-9 * (want["quadrics"][:, 9] + 1)).all()


def test_a_cell_depends_on_its_own_records_only():
    """The blob alone, then with the cube 10 000 mm away in one call: the grid keeps its origin, so the blob's cells come first in key
    order, and every output of theirs is the same bits."""
    v, f, col = _blob()
    cv, cf = ref.cube_mesh()
    _, tb1, one, origin, _ = _device_cluster(v, f, col, 9.0)
    v2, f2 = np.concatenate([v, cv + np.float32(10000.0)]), np.concatenate([f, cf + np.int32(len(v))])
    _, tb2, two, origin2, _ = _device_cluster(v2, f2, np.concatenate([col, ref.fixture_colors(len(cv), 1)]), 9.0)
    n = len(tb1["cells"])
    assert np.array_equal(origin, origin2) and len(tb2["cells"]) > n and np.array_equal(tb2["rank"][:len(v)], tb1["rank"])
    for k in OUTPUTS:
        assert np.array_equal(_bits(one[k]), _bits(two[k][:n])), k


def test_point_cloud():
    v, _, col = _blob()
    _, tb, got, origin, dims = _device_cluster(v, np.zeros((0, 3), np.int32), col, 9.0)
    assert (got["status"] == 0).all() and np.array_equal(got["positions"], got["means"].astype(np.float32))
    assert not got["quadrics"].any() and not got["err"].any()
    want = ref.cluster(v, col, np.zeros((0, 3), np.int32), ref.tables(ref.cell_keys(v, origin, 9.0, dims), np.zeros((0, 3), np.int32)), origin, 9.0, dims)
    assert np.array_equal(_bits(got["means"]), _bits(want["means"]))
    mesh, report = simplify.simplify_mesh(Mesh(v, np.zeros((0, 3), np.int32), col, np.zeros_like(v)), simplify.SimplifyOpts(cell_mm=9.0))
    assert len(mesh.vertices) == report["cells"] == len(tb["cells"]) and np.array_equal(mesh.vertices, got["positions"]) and len(mesh.faces) == 0
    assert report["status_counts"] == {"0": len(tb["cells"])}


@pytest.mark.parametrize("name,c", [("plate", 11.3), ("cube", 7.3)])
def test_face_rules_equal_the_restatement(name, c):
    v, f = ref.plate_mesh() if name == "plate" else ref.cube_mesh()
    col = ref.fixture_colors(len(v), 2)
    want = ref.simplify(v, col, f, c)
    mesh, report = simplify.simplify_mesh(Mesh(v, f, col, np.zeros_like(v)), simplify.SimplifyOpts(cell_mm=c))
    assert mesh.faces.dtype == np.int32 and np.array_equal(mesh.faces, want["faces"])
    assert np.abs(mesh.vertices.astype(np.float64) - want["vertices"].astype(np.float64)).max() <= 4e-6
    assert np.abs(mesh.colors - want["colors"]).max() <= 1e-6
    assert report["cells"] == len(want["tables"]["cells"]) and report["vertices_out"] == len(want["vertices"]) and report["triangles_out"] == len(want["faces"])
    assert report["grid_dims"] == list(want["dims"]) and report["cell_mm"] == c and "manifold" in report["limits"]
    if name == "plate":
        assert report["triangles_out"] == 50 and report["vertices_out"] == 36
    else:
        assert report["topology"] == {"boundary_edges": 0, "nonmanifold_edges": 0, "watertight": True}
        # every vertex lies on its planes: what is left is the rounding of three terms of about w d^2, sqrt(2^-52 900) = 4e-7 mm
        assert report["status_counts"] == {"1": 294, "2": 84, "3": 8} and report["rms_quadric_error_mm"] < 1e-5
        far = np.array([[500, 500, 500], [530, 500, 500], [500, 530, 500]], np.float32)        # one more component, 30 mm wide
        two = Mesh(np.concatenate([v, far]), np.concatenate([f, [[3458, 3459, 3460]]]).astype(np.int32), np.concatenate([col, col[:3]]),
                   np.zeros((3461, 3), np.float32))
        for keep, nv, nf in ((False, 389, 769), (True, 386, 768)):
            out, _ = simplify.simplify_mesh(two, simplify.SimplifyOpts(cell_mm=c, keep_largest=keep))
            assert (len(out.vertices), len(out.faces)) == (nv, nf)


def test_refusals_write_nothing(tmp_path):
    v, f = ref.plate_mesh()
    col = np.full(v.shape, 0.5, np.float32)
    dv = torch.from_numpy(v).cuda()
    nan = v.copy()
    nan[3, 0] = np.nan
    bad_f = f.copy()
    bad_f[0, 0] = len(v)
    opts = simplify.SimplifyOpts(cell_mm=11.3)
    for mesh in (Mesh(nan, f, col, v), Mesh(v, bad_f, col, v)):
        with pytest.raises(ValueError):
            simplify.simplify_mesh(mesh, opts)
    for c in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ops.mesh_cell_keys(dv, (0.0, 0.0, 0.0), c, (8, 8, 8))
    with pytest.raises(ValueError):
        ops.mesh_cell_keys(dv, (0.0, 0.0, 0.0), 1.0, ((1 << 20) + 1, 8, 8))
    with pytest.raises(ValueError):
        simplify.simplify_mesh(Mesh(v, f, col, v), simplify.SimplifyOpts(cell_mm=1e-5))        # 60 mm / 1e-5 mm > 2^20 cells
    for bad in (simplify.SimplifyOpts(), simplify.SimplifyOpts(cell_mm=5.0, target_vertices=100)):
        with pytest.raises(ValueError):
            simplify.simplify_mesh(Mesh(v, f, col, v), bad)
    with pytest.raises(_lib.FoundPoseNativeError):
        ops.mesh_cell_keys(torch.from_numpy(v), (0.0, 0.0, 0.0), 1.0, (8, 8, 8))
    with pytest.raises(_lib.FoundPoseNativeError):
        ops.mesh_cluster_tables(torch.zeros(4, dtype=torch.int64), torch.zeros(0, 3, dtype=torch.int32))
    # the C entry points themselves: FP_ERR_INVALID (1), and the outputs keep their bytes
    L = _lib.lib()
    keys = torch.full((len(v),), -7, dtype=torch.int64, device="cuda")
    p = _lib.ptr
    for grid, dims in (([0, 0, 0, 0.0], (8, 8, 8)), ([0, 0, 0, -2.0], (8, 8, 8)), ([0, 0, 0, float("nan")], (8, 8, 8)), ([0, float("inf"), 0, 1.0], (8, 8, 8)),
                       ([0, 0, 0, 1.0], (8, (1 << 20) + 1, 8)), ([0, 0, 0, 1.0], (0, 8, 8))):
        g = np.array(grid, np.float64)
        assert L.fp_mesh_cell_keys(p(dv), len(v), g.ctypes.data_as(_lib.vp), *dims, p(keys), _lib.stream()) == 1
    assert L.fp_mesh_cell_keys(None, len(v), np.array([0, 0, 0, 1.0]).ctypes.data_as(_lib.vp), 8, 8, 8, p(keys), _lib.stream()) == 1
    origin, dims = ref.grid_for(v, 11.3)
    tb = ops.mesh_cluster_tables(ops.mesh_cell_keys(dv, origin, 11.3, dims), torch.from_numpy(f).cuda())
    dc, df = torch.from_numpy(col).cuda(), torch.from_numpy(f).cuda()
    n = len(tb["cells"])
    outs = [torch.full((n, 3), -7.0, device="cuda"), torch.full((n, 3), -7.0, device="cuda"), torch.full((n, 10), -7.0, dtype=torch.float64, device="cuda"),
            torch.full((n, 3), -7.0, dtype=torch.float64, device="cuda"), torch.full((n,), -7.0, dtype=torch.float64, device="cuda"),
            torch.full((n,), -7, dtype=torch.int32, device="cuda")]
    g = np.array([*origin, 11.3], np.float64)

    def cluster(num_v=len(v), num_f=len(f), num_c=n, grid=g, d=dims, eps=1e-3, faces=df):
        return L.fp_mesh_cluster(p(dv), p(dc), num_v, p(faces), num_f, p(tb["cells"]), num_c, p(tb["vert_order"]), p(tb["vert_begin"]), p(tb["corner_order"]),
                                 p(tb["corner_begin"]), grid.ctypes.data_as(_lib.vp), *d, eps, *(p(t) for t in outs), _lib.stream())
    assert cluster(num_v=0) == 1 and cluster(num_f=-1) == 1 and cluster(num_c=0) == 1 and cluster(num_c=len(v) + 1) == 1
    assert cluster(grid=np.array([*origin, 0.0])) == 1 and cluster(d=(dims[0], dims[1], (1 << 20) + 1)) == 1
    assert cluster(eps=1.0) == 1 and cluster(eps=float("nan")) == 1 and cluster(faces=None) == 1
    torch.cuda.synchronize()
    assert (keys == -7).all() and all(bool((t == -7).all()) for t in outs)
    assert cluster() == 0
    torch.cuda.synchronize()
    assert not any(bool((t == -7).any()) for t in outs)


def _diameter(v):
    v = v.astype(np.float64)
    return max(float(np.sqrt(((v[i:i + 256, None] - v[None]) ** 2).sum(-1).max())) for i in range(0, len(v), 256))


def test_command_line(tmp_path):
    from foundpose_amd.eval_util import load_eval_model
    blob = make_blob_mesh(60, 60)
    src, dst = tmp_path / "models", tmp_path / "models_eval"
    src.mkdir()
    save_ply(str(src / "obj_000003.ply"), blob)
    info = {"3": {"diameter": 187.25, "min_x": -1.0, "min_y": -2.0, "min_z": -3.0, "size_x": 4.0, "size_y": 5.0, "size_z": 6.0,
                  "symmetries_discrete": [[1, 0, 0, 0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]]}}
    (src / "models_info.json").write_text(json.dumps(info))
    v_in = load_ply(str(src / "obj_000003.ply")).vertices
    args = ["--models-dir", str(src), "--output-dir", str(dst), "--target-vertices", "400", "--report", str(tmp_path / "r.json")]
    assert simplify.main(args) == 0
    report = json.loads((tmp_path / "r.json").read_text())["3"]
    c = ref.choose_cell(v_in, 400)
    assert report["cell_mm"] == c                                   # bit for bit: it depends on integer counts only
    out = load_ply(str(dst / "obj_000003.ply"))
    assert 300 < len(out.vertices) <= 400 and report["vertices_out"] == len(out.vertices) and report["vertices_in"] == 3542
    assert len(out.faces) == report["triangles_out"] > 600 and out.faces.max() == len(out.vertices) - 1
    d = np.sqrt(((out.vertices.astype(np.float64)[:, None] - v_in.astype(np.float64)[None]) ** 2).sum(-1)).min(1)
    print("cell", c, "vertices", len(out.vertices), "farthest output vertex from the input's", d.max(), "of", 1.5 * np.sqrt(3) * c, report["topology"])
    assert d.max() <= 1.5 * np.sqrt(3) * c
    assert json.loads((dst / "models_info.json").read_text()) == info
    model = load_eval_model(str(dst), 3)
    assert model.diameter == 187.25 and model.pts.shape == (len(out.vertices), 3) and len(model.syms) == 2
    before = {n: (os.stat(dst / n).st_mtime_ns, (dst / n).read_bytes()) for n in ("obj_000003.ply", "models_info.json")}
    with pytest.raises(FileExistsError):
        simplify.main(args)
    assert before == {n: (os.stat(dst / n).st_mtime_ns, (dst / n).read_bytes()) for n in before}
    assert simplify.main(args + ["--overwrite"]) == 0              # and the result is the same bytes from run to run
    assert (dst / "obj_000003.ply").read_bytes() == before["obj_000003.ply"][1]
    # without a source models_info.json one is written from the output
    (src / "models_info.json").unlink()
    dst2 = tmp_path / "models_eval2"
    assert simplify.main(["--models-dir", str(src), "--output-dir", str(dst2), "--cell-mm", repr(c), "--object-ids", "3"]) == 0
    written = json.loads((dst2 / "models_info.json").read_text())
    assert set(written) == {"3"} and abs(written["3"]["diameter"] - _diameter(v_in)) <= 2 * 1.5 * np.sqrt(3) * c
    assert (dst2 / "obj_000003.ply").read_bytes() == before["obj_000003.ply"][1]
