"""CPU: the numpy restatement of fp_pts_diameter / fp_directed_hausdorff (tests/models_info_ref.py) against scipy, and the host decision logic of
foundpose_amd.models_info -- axis list, fraction set, per-axis decision, combination, closure -- driven by that restatement on shapes whose
symmetry groups are known; the file format's round trip and the refusals that need no device."""

import json
from fractions import Fraction

import numpy as np
import pytest

from foundpose_amd import eval_util, models_info as mi
from tests import models_info_ref as ref

EPS = 0.5


def _tf(R, t):
    return np.concatenate([np.asarray(R, np.float64).ravel(), np.asarray(t, np.float64).ravel()])


# ---------------------------------------------------------------------------------------------------- restatement against scipy
@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 1500])
def test_restatement_agrees_with_pdist_and_the_kd_tree(V):
    from scipy.spatial import cKDTree
    from scipy.spatial.distance import pdist
    rng = np.random.default_rng(100 + V)
    pts = rng.normal(size=(V, 3)) * 40.0 + ref.SHIFT
    d, (i, j) = ref.diameter(pts)
    want = pdist(pts).max() if V > 1 else 0.0
    assert abs(d - want) <= 1e-9 * want and (i < j or V == 1)
    assert abs(np.linalg.norm(pts[i] - pts[j]) - want) <= 1e-9 * max(want, 1.0)
    tree = cKDTree(pts)
    for stride in (1, 3, 7):
        for k in range(3):
            tf = _tf(eval_util._rotation_matrix(0.3 * (k + 1), rng.normal(size=3)), rng.normal(size=3) * 5.0)
            h, v = ref.directed_hausdorff(pts, tf, stride)
            dist, _ = tree.query(ref.place(tf, pts[::stride]), k=1)
            assert abs(h - dist.max()) <= 1e-9 * dist.max() and v % stride == 0 and v < V
            assert abs(dist[v // stride] - dist.max()) <= 1e-9 * dist.max()


def test_a_nan_never_wins():
    rng = np.random.default_rng(1)
    pts = rng.normal(size=(300, 3)) * 40.0
    bad = pts.copy()
    bad[[0, 17, 299]] = np.nan
    d, pair = ref.diameter(bad)
    keep = np.delete(np.arange(300), [0, 17, 299])
    wd, wpair = ref.diameter(pts[keep])
    assert d == wd and pair == (keep[wpair[0]], keep[wpair[1]])
    assert ref.diameter(np.full((4, 3), np.nan)) == (0.0, (0, 0))
    q = rng.normal(size=(50, 3)) * 40.0
    assert np.array_equal(ref.nn_sq(q, bad), ref.nn_sq(q, pts[keep]))
    assert np.all(np.isinf(ref.nn_sq(q, np.full((4, 3), np.nan))))


def test_ties_go_to_the_lowest_pair_and_the_lowest_vertex():
    g = (np.arange(7, dtype=np.float64) - 3) * 16.0
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    assert ref.diameter(pts) == (float(np.sqrt(np.float64(3 * 96.0 * 96.0))), (0, 342))      # four body diagonals tie
    assert ref.directed_hausdorff(pts, _tf(np.eye(3), [3.0, -4.0, 0.0])) == (5.0, 0)         # every vertex ties
    assert ref.directed_hausdorff(pts, _tf(np.eye(3), [3.0, -4.0, 0.0]), 5) == (5.0, 0)
    assert ref.directed_hausdorff(pts, _tf(np.diag([-1.0, -1.0, 1.0]), [0.0, 0.0, 0.0])) == (0.0, 0)
    assert ref.diameter(pts[:1]) == (0.0, (0, 0)) and ref.directed_hausdorff(pts[:1], _tf(np.eye(3), [0.0, 3.0, 4.0]), 9) == (5.0, 0)


# ---------------------------------------------------------------------------------------------------- the pure parts
def test_axis_list_and_fraction_set():
    f = mi.angle_fractions(12, 36)
    assert len(f) == 63 and f == sorted(f) and all(1 - x in f for x in f) and f[0] == Fraction(1, 36) and Fraction(1, 2) in f
    assert mi.angle_fractions(2, 2) == [Fraction(1, 2)]
    box = ref.box_lattice(4, 6, 9)
    axes = mi.candidate_axes(box)      # the principal frame of a box is its own frame: all 13 principal-frame axes are duplicates
    assert axes.shape == (13, 3) and np.allclose(np.linalg.norm(axes, axis=1), 1.0)
    assert np.array_equal(axes[:3], np.eye(3)) and np.allclose(axes[3], [2 ** -0.5, 2 ** -0.5, 0]) and np.allclose(axes[9], np.ones(3) / 3 ** 0.5)
    assert mi.candidate_axes(ref.prism(7)).shape == (13, 3)          # two equal eigenvalues: no principal frame
    R = eval_util._rotation_matrix(0.4, [1.0, 2.0, 3.0])
    turned = mi.candidate_axes((box - box.mean(0)) @ R.T)            # a box in general position: 13 + 13
    assert turned.shape == (26, 3)
    want = np.eye(3) @ R.T                                            # the box's own axes are among the principal-frame ones
    assert all(np.max(np.abs(turned[13:] @ w)) > 1 - 1e-9 for w in want)


def test_centre_is_the_area_weighted_centroid_when_there_is_a_surface():
    v = np.array([[0.0, 0, 0], [4, 0, 0], [4, 4, 0], [0, 4, 0], [2, 0, 0]])        # a square; the extra vertex splits one triangle
    coarse = np.array([[0, 1, 2], [0, 2, 3]])
    fine = np.array([[0, 4, 2], [4, 1, 2], [0, 2, 3]])
    assert np.allclose(mi.symmetry_centre(v[:4], coarse), [2, 2, 0]) and np.allclose(mi.symmetry_centre(v, fine), [2, 2, 0])
    assert np.allclose(mi.symmetry_centre(v, None), v.mean(0)) and np.allclose(mi.symmetry_centre(v, np.zeros((0, 3), int)), v.mean(0))
    assert np.allclose(mi.symmetry_centre(v, np.array([[0, 4, 1]])), v.mean(0))    # zero area: the vertex mean


def test_axis_decision_rules():
    F = mi.angle_fractions(6, 6)
    H = {f: 1.0 for f in F}
    assert mi.axis_decision(H, 0.5, 6, 6) == (False, [])
    H.update({Fraction(1, 2): 0.1, Fraction(1, 4): 0.1, Fraction(3, 4): 0.49})
    assert mi.axis_decision(H, 0.5, 6, 6) == (False, [Fraction(1, 4), Fraction(1, 2), Fraction(3, 4)])
    H[Fraction(3, 4)] = 0.5                                         # strict: 0.5 is not below eps
    assert mi.axis_decision(H, 0.5, 6, 6) == (False, [Fraction(1, 2)])
    assert mi.axis_decision({f: 0.2 for f in F}, 0.5, 6, 6) == (True, [])
    assert mi.axis_decision({f: (0.2 if f.denominator in (2, 3, 6) else 9.0) for f in F}, 0.5, 6, 6) == (True, [])   # every j / 6


# ---------------------------------------------------------------------------------------------------- shapes with known groups
def _run(pts, prefilter=True, **kw):
    d, _ = ref.diameter(pts)
    return mi.object_symmetries(pts, None, d, ref.evaluator(pts), prefilter=prefilter, **kw)


@pytest.fixture(scope="module")
def round_prism():
    """The 64-sided prism at the default threshold, computed once: (pts, diameter, discrete, continuous, report)."""
    pts = ref.prism(64)
    return (pts, ref.diameter(pts)[0]) + _run(pts)


@pytest.mark.parametrize("dims,extra,want", [((4, 6, 9), None, 3), ((5, 5, 9), None, 7), ((5, 5, 5), None, 23), ((4, 6, 9), [[100.0, 3.0, 5.0]], 0)])
def test_lattice_boxes(dims, extra, want):
    pts = ref.box_lattice(*dims, extra=extra)
    assert len(pts) == {(4, 6, 9): 160, (5, 5, 9): 162, (5, 5, 5): 98}[dims] + (1 if extra else 0)
    disc, cont, rep = _run(pts, sym_thresh=EPS)
    print(dims, extra, "discrete", len(disc), "continuous", len(cont), "axis pass", rep["axis_pass"], rep.get("closure", {}).get("rounds"))
    assert len(disc) == want and cont == []
    assert rep["closure"]["failed_products"] == 0 and not rep["closure"]["abandoned"]
    for m in disc:      # every entry maps the set onto itself exactly enough
        m = np.array(m).reshape(4, 4)
        assert ref.directed_hausdorff(pts, _tf(m[:3, :3], m[:3, 3]))[0] < EPS


@pytest.mark.parametrize("n,axis_pass,closed", [(5, 5, 9), (6, 7, 11), (7, 7, 13), (64, 11, 15)])
def test_prisms_axis_pass_and_closure(n, axis_pass, closed):
    pts = ref.prism(n)
    disc, cont, rep = _run(pts, sym_thresh=EPS)
    print(n, "axis pass", rep["axis_pass"], "closed", len(disc), rep["closure"]["rounds"] and [(r["tested"], r["passed"]) for r in rep["closure"]["rounds"]])
    assert rep["axis_pass"] == axis_pass and len(disc) == closed and cont == []
    assert rep["closure"]["failed_products"] == 0 and not rep["closure"]["abandoned"]
    if n <= 7:
        assert _run(pts, prefilter=False, sym_thresh=EPS)[:2] == (disc, cont)


def test_a_round_prism_at_the_default_threshold_has_one_continuous_axis_and_one_discrete_entry(round_prism):
    pts, d, disc, cont, rep = round_prism
    assert abs(d - 128.06) < 0.01
    assert rep["eps"] == 15.0 and len(cont) == 1 and len(disc) == 1 and "closure" not in rep
    assert np.allclose(np.abs(cont[0]["axis"]), [0, 0, 1]) and np.allclose(cont[0]["offset"], ref.SHIFT + [0, 0, 50.0])
    assert np.allclose(np.array(disc[0]).reshape(4, 4)[:3, :3] @ [0, 0, 1.0], [0, 0, -1.0])      # it turns the axis over


def test_the_prefilter_rejects_by_a_lower_bound_and_changes_nothing(monkeypatch):
    monkeypatch.setattr(mi, "PREFILTER_QUERIES", 64)      # 162 points: every third vertex in the first pass
    pts = ref.box_lattice(5, 5, 9)
    with_pf, without = _run(pts, sym_thresh=EPS), _run(pts, prefilter=False, sym_thresh=EPS)
    assert with_pf[:2] == without[:2] and len(with_pf[0]) == 7 and with_pf[2]["query_stride"] == 3 and without[2]["query_stride"] == 1
    a, b = with_pf[2]["axes"], without[2]["axes"]
    for ax, bx in zip(a, b):
        for ca, cb in zip(ax["candidates"], bx["candidates"]):
            assert not cb["lower_bound"]
            assert (ca["value"] <= cb["value"] and ca["value"] >= EPS) if ca["lower_bound"] else ca["value"] == cb["value"]
    assert any(c["lower_bound"] for ax in a for c in ax["candidates"])


def test_closure_drops_failing_products_and_gives_up_past_120():
    I = np.eye(3)
    quarter = [mi.rotation_about(Fraction(1, 4), I[0]), mi.rotation_about(Fraction(1, 4), I[1])]   # generate the cube group: 24
    accept = lambda tfs, stride: np.zeros(len(tfs))
    held, rep = mi.close_group(quarter, np.zeros(3), accept, EPS, 1)
    assert len(held) == 23 and rep["closed"] == 23 and rep["failed_products"] == 0 and len(rep["rounds"]) >= 2
    refuse = lambda tfs, stride: np.ones(len(tfs))
    held, rep = mi.close_group(quarter, np.zeros(3), refuse, EPS, 1)
    assert len(held) == 2 and rep["failed_products"] == 4 and len(rep["rounds"]) == 1            # a a, a b, b a, b b
    big = [mi.rotation_about(Fraction(1, 97), I[2]), mi.rotation_about(Fraction(1, 2), I[0])]     # a dihedral group of 194 elements
    held, rep = mi.close_group(big, np.zeros(3), accept, EPS, 1)
    assert rep["abandoned"] and len(held) == 2


# ---------------------------------------------------------------------------------------------------- file format, refusals
@pytest.mark.parametrize("shape", ["box", "round"])
def test_round_trip_through_get_symmetry_transformations(shape, tmp_path, round_prism):
    if shape == "box":
        pts = ref.box_lattice(5, 5, 9)
        d, (disc, cont, rep) = ref.diameter(pts)[0], _run(pts, sym_thresh=EPS)
    else:
        pts, d, disc, cont, rep = round_prism
    entry = {"diameter": d}
    if disc:
        entry["symmetries_discrete"] = disc
    if cont:
        entry["symmetries_continuous"] = cont
    path = tmp_path / "models_info.json"
    path.write_text(json.dumps({"1": entry}))
    info = json.loads(path.read_text())["1"]
    assert info == entry and all(len(m) == 16 for m in info.get("symmetries_discrete", []))
    trans = eval_util.get_symmetry_transformations(info, 0.01)
    assert len(trans) == (8 if shape == "box" else 2 * 314)
    h = ref.batch_hausdorff(pts, np.array([_tf(t["R"], t["t"].ravel()) for t in trans]))[0]
    print(shape, "eps", rep["eps"], "largest distance of a listed transform", h.max())
    assert np.all(h < rep["eps"])


def test_refusals(tmp_path):
    for bad in (dict(sym_thresh=0.0), dict(sym_thresh=-1.0), dict(sym_thresh=float("nan")), dict(sym_thresh="15"), dict(max_order=1), dict(max_order=2.5),
                dict(continuous_steps=1), dict(continuous_steps=True), dict(max_order=1000)):
        with pytest.raises(ValueError):
            mi.calc_models_info(str(tmp_path), **bad)
        with pytest.raises(ValueError):
            mi.object_symmetries(ref.prism(5), None, 128.0, ref.evaluator(ref.prism(5)), **bad)
    with pytest.raises(FileNotFoundError):
        mi.calc_models_info(str(tmp_path))                      # no model files
    with pytest.raises(FileNotFoundError):
        mi.calc_models_info(str(tmp_path / "absent"))
    ref.write_ply(tmp_path / "obj_000001.ply", ref.prism(5))
    with pytest.raises(FileNotFoundError):
        mi.calc_models_info(str(tmp_path), object_ids=[1, 2])
    bad = ref.prism(5)
    bad[3, 1] = np.inf
    ref.write_ply(tmp_path / "obj_000002.ply", bad)
    with pytest.raises(ValueError, match="non-finite"):
        mi.calc_models_info(str(tmp_path))
    out = tmp_path / "models_info.json"
    out.write_text("{}")
    with pytest.raises(FileExistsError):
        mi.main(["--models-dir", str(tmp_path), "--output", str(out), "--object-ids", "1"])
    assert out.read_text() == "{}"
    report = tmp_path / "report.json"
    report.write_text("kept")
    with pytest.raises(FileExistsError):
        mi.main(["--models-dir", str(tmp_path), "--output", str(tmp_path / "new.json"), "--report", str(report), "--object-ids", "1"])
    assert report.read_text() == "kept" and not (tmp_path / "new.json").exists()


def test_there_is_no_cpu_path(tmp_path):
    import torch
    from foundpose_amd import _lib
    if torch.cuda.is_available():
        return      # on a device the tool runs: tests/test_gpu_models_info.py
    ref.write_ply(tmp_path / "obj_000001.ply", ref.prism(5))
    with pytest.raises(_lib.FoundPoseNativeError):
        mi.calc_models_info(str(tmp_path))
    with pytest.raises(_lib.FoundPoseNativeError):
        mi.main(["--models-dir", str(tmp_path), "--output", str(tmp_path / "models_info.json")])
    assert not (tmp_path / "models_info.json").exists()
