"""GPU: foundpose_amd.models_info on PLY files written into tmp_path -- bounds, diameter and symmetry lists equal to the host logic driven by the
numpy restatement (tests/models_info_ref.py), the prefilter changing nothing, load_eval_model reading the written file, the command-line tool."""

import json

import numpy as np
import pytest

from foundpose_amd import eval_util, models_info as mi
from foundpose_amd.renderer import load_ply
from tests import models_info_ref as ref

pytestmark = pytest.mark.gpu

EPS = 0.5


def _cap_fans(n, levels=5):
    """Triangles of the two caps of ref.prism(n): a surface whose area-weighted centroid lies on the axis, halfway up."""
    bottom, top = levels * n, levels * n + 1
    return [(bottom, (i + 1) % n, i) for i in range(n)] + [(top, (levels - 1) * n + i, (levels - 1) * n + (i + 1) % n) for i in range(n)]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """1: a 5 x 5 x 9 box (7 entries), 2: a 4 x 6 x 9 box with one outlier (none), 3: a 7-sided prism with capped ends (13), 4: a cube of 2 168
    boundary points (23; more than 2 048 vertices, so the first pass queries every second one).  The expected lists of 1-3 come from the host
    logic driven by the restatement, computed once; 4 is too large for that and is compared with itself."""
    d = tmp_path_factory.mktemp("models")
    ref.write_ply(d / "obj_000001.ply", ref.box_lattice(5, 5, 9))
    ref.write_ply(d / "obj_000002.ply", ref.box_lattice(4, 6, 9, extra=[[100.0, 3.0, 5.0]]))
    ref.write_ply(d / "obj_000003.ply", ref.prism(7), _cap_fans(7))
    ref.write_ply(d / "obj_000004.ply", ref.box_lattice(20, 20, 20))
    want = {}
    for oid in (1, 2, 3):
        mesh = load_ply(str(d / f"obj_{oid:06d}.ply"), geometry_only=True)
        v = mesh.vertices.astype(np.float64)
        diam, _ = ref.diameter(v)
        disc, cont, _ = mi.object_symmetries(v, mesh.faces, diam, ref.evaluator(v), sym_thresh=EPS)
        lo, hi = v.min(0), v.max(0)
        e = {"min_x": lo[0], "min_y": lo[1], "min_z": lo[2], "size_x": hi[0] - lo[0], "size_y": hi[1] - lo[1], "size_z": hi[2] - lo[2], "diameter": diam}
        e = {k: float(x) for k, x in e.items()}
        if disc:
            e["symmetries_discrete"] = disc
        if cont:
            e["symmetries_continuous"] = cont
        want[oid] = e
    return d, want


def test_bounds_diameter_and_symmetry_lists_equal_the_host_logic_on_the_restatement(models):
    d, want = models
    got, rep = mi.calc_models_info(str(d), object_ids=[1, 2, 3], symmetries=True, sym_thresh=EPS, report=True)
    print({o: (e["diameter"], len(e.get("symmetries_discrete", []))) for o, e in got.items()})
    assert got == want
    assert [len(got[o].get("symmetries_discrete", [])) for o in (1, 2, 3)] == [7, 0, 13] and "symmetries_discrete" not in got[2]
    assert rep[3]["closure"]["axis_pass"] == 7 and rep[3]["closure"]["failed_products"] == 0 and np.allclose(rep[3]["centre"], ref.SHIFT + [0, 0, 50.0])
    assert mi.calc_models_info(str(d), object_ids=[1, 2, 3], symmetries=True, sym_thresh=EPS, prefilter=False) == want
    plain = mi.calc_models_info(str(d), object_ids=[3, 1])          # the default writes no symmetry lists, as the toolkit's tool
    assert list(plain) == [3, 1] and all(plain[o] == {k: x for k, x in want[o].items() if not k.startswith("symmetries")} for o in (1, 3))


def test_the_prefilter_changes_nothing_where_it_rejects(models):
    d, _ = models
    a, ra = mi.calc_models_info(str(d), object_ids=[4], symmetries=True, sym_thresh=EPS, report=True)
    b, rb = mi.calc_models_info(str(d), object_ids=[4], symmetries=True, sym_thresh=EPS, prefilter=False, report=True)
    assert a == b and len(a[4]["symmetries_discrete"]) == 23 and ra[4]["query_stride"] == 2 and rb[4]["query_stride"] == 1
    assert a[4]["diameter"] == float(np.sqrt(np.float64(3 * 152.0 * 152.0))) and ra[4]["vertices"] == 2168
    bounds = 0
    for ax, bx in zip(ra[4]["axes"], rb[4]["axes"]):
        for ca, cb in zip(ax["candidates"], bx["candidates"]):
            assert (EPS <= ca["value"] <= cb["value"]) if ca["lower_bound"] else ca["value"] == cb["value"]
            bounds += ca["lower_bound"]
    assert bounds > 0


def test_load_eval_model_reads_the_written_file_and_mssd_sees_the_symmetry(models):
    d, want = models
    info = mi.calc_models_info(str(d), object_ids=[1, 2], symmetries=True, sym_thresh=EPS)
    with open(d / "models_info.json", "w") as f:
        json.dump({str(k): v for k, v in info.items()}, f)
    sym_box, asym = eval_util.load_eval_model(str(d), 1), eval_util.load_eval_model(str(d), 2)
    assert len(sym_box.syms) == 8 and len(asym.syms) == 1 and sym_box.diameter == want[1]["diameter"]
    R_gt, t_gt = eval_util._rotation_matrix(0.7, [1.0, -2.0, 0.5]), np.array([20.0, -30.0, 700.0])
    K = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1.0]])
    S = sym_box.syms[3]          # a found symmetry of the box (0 is the identity); the outlier object is the 4 x 6 x 9 box, which it does not fit
    items = [{"R_est": R_gt @ S["R"], "t_est": R_gt @ S["t"].ravel() + t_gt, "R_gt": R_gt, "t_gt": t_gt, "K": K, "pts": m.pts, "syms": m.syms}
             for m in (sym_box, asym)]
    err, _ = eval_util.pose_errors_batch(items)
    print("mssd with the symmetry listed", err[0, 0], "without", err[1, 0])
    assert err[0, 0] < EPS < err[1, 0]


def test_the_command_line_tool_writes_the_same_json_and_refuses_to_overwrite(models, tmp_path):
    d, want = models
    out, report = tmp_path / "models_info.json", tmp_path / "report.json"
    args = ["--models-dir", str(d), "--output", str(out), "--object-ids", "1", "2", "3", "--symmetries", "--sym-thresh", str(EPS), "--report", str(report)]
    assert mi.main(args) == 0
    assert json.loads(out.read_text()) == json.loads(json.dumps({str(k): v for k, v in want.items()}))
    rep = json.loads(report.read_text())
    assert set(rep) == {"1", "2", "3"} and rep["1"]["eps"] == EPS and len(rep["1"]["axes"]) == 13 and len(rep["1"]["axes"][0]["candidates"]) == 63
    before = out.read_text()
    with pytest.raises(FileExistsError):
        mi.main(args)
    assert out.read_text() == before
    assert mi.main(args + ["--force"]) == 0 and out.read_text() == before
