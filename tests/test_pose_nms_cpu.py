"""frame_select_type "pose_nms" without a GPU: the numpy restatement (tests/pose_nms_ref.py) on the GPU tests' fixture (far from every
decision boundary) and on hand-made conflict matrices, pose_nms.frame_pairs, the rank layout, the csv writer's round trip, the argument
checks that come before any device work, the drivers' option checks and the C ABI's declarations."""

import json
import os
import re

import numpy as np
import pytest
import torch

from tests import pose_nms_ref as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[8, 16])
def fix(request):
    return pn.gpu_fixture(seed=6, grid=request.param)


def test_the_fixture_is_far_from_every_boundary(fix):
    """Seeds tried (min_margin at G = 8 / G = 16): 6 gives 5.8e-6 / 5.8e-6 (kept: the seed of pose_verify_ref's own tests), 7 3.1e-6 /
    1.3e-6, 8 2.6e-6 / 2.6e-6, 9 1.3e-5 / 2.6e-6, 10 6.1e-7 / 6.1e-7 (below the bar, not used), 11 7.9e-6 / 1.2e-6."""
    ref = fix["ref"]
    print("G =", fix["grid"], "min_margin", ref["min_margin"])
    assert ref["min_margin"] > 1e-6, ref["min_margin"]
    assert [e - b for b, e in fix["ranges"]] == [600, 602]   # more than two rounds of a 256-thread loop
    assert len(fix["pairs"]) == 56 and fix["pair_off"].tolist() == [0, 56]


def test_restatement_facts_on_the_fixture(fix):
    ref, G = fix["ref"], fix["grid"]
    at = lambda i, j: pn.pair_index(fix, i, j)
    # the same pose twice: every point of i falls into the cell it set itself -- the fixture's value is 1.0 exactly, both ways
    for i, j in ((0, 1), (1, 0)):
        assert ref["status"][at(i, j)] == 0 and ref["overlap"][at(i, j)] == 1.0 and ref["counts"][at(i, j), 0] == 600
    # n_cells is j's own and does not depend on i or on the poses
    for j in range(4):
        assert ref["counts"][at(4, j), 1] == ref["counts"][at(0, 1), 1]
    # the overlap falls with the shift: rho / 16 (half a cell at G = 16), rho / 2
    o = [ref["overlap"][at(0, j)] for j in (1, 2, 3)]
    print("G =", G, "overlap of the planted pose with itself / shifted by rho / 16 / by rho / 2:", o, "object 1 in object 0:", ref["overlap"][at(4, 0)])
    assert o[0] > o[1] > o[2] > 0
    assert {8: (0.9333333333333333, 0.3233333333333333), 16: (0.7466666666666667, 0.11166666666666666)}[G] == (o[1], o[2])
    assert 0 < ref["overlap"][at(4, 0)] < o[1] and 0 < ref["overlap"][at(0, 4)] < o[1]   # the two objects' surfaces cross
    # disjoint spheres and a NaN pose: status 1, nothing counted; an invalid pose: status 2 -- in both directions
    for i in range(8):
        for j in range(8):
            if i == j:
                continue
            want = 2 if 6 in (i, j) else 1 if (5 in (i, j) or 7 in (i, j)) else 0
            assert ref["status"][at(i, j)] == want, (i, j)
            if want:
                assert not ref["counts"][at(i, j)].any() and ref["overlap"][at(i, j)] == 0.0
    keep, by = pn.nms_greedy_ref(fix["group_off"], fix["pair_off"], fix["pairs"], ref["overlap"], ref["status"], fix["thr"])
    # at G = 8 the cells are rho / 4 and the rho / 2 shift still overlaps by 0.32 >= 0.3; at G = 16 it does not (limits)
    assert keep.tolist() == {8: [1, 0, 0, 0, 1, 1, 1, 1], 16: [1, 0, 0, 1, 1, 1, 1, 1]}[G]
    assert by.tolist() == {8: [-1, 0, 0, 0, -1, -1, -1, -1], 16: [-1, 0, 0, -1, -1, -1, -1, -1]}[G]


def test_restatement_on_a_case_counted_by_hand():
    """G = 8, c = 0, rho = 4: x0 = -4, h = 1, cell = floor(x + 4).  j's sample occupies cells (4,4,4), (5,4,4) and -- a point outside the
    cube, clamped -- (7,4,4).  i = the same object at t = (1, 0, 0): its points land at x + 1."""
    X = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [9.5, 0.5, 0.5]], np.float32)
    I, z = np.eye(3), np.zeros(3)
    n_in, n_cells, ov, st = pn.overlap_pair(X, X, z, 4.0, z, 4.0, I, np.array([1.0, 0.0, 0.0]), I, z, 8)
    # (1.5, .5, .5) -> cell (5,4,4) set; (2.5, ...) -> (6,4,4) clear; (10.5, ...) -> q = 14: outside the cube, NOT clamped into (7,4,4)
    assert (n_in, n_cells, ov, st) == (1, 3, 1.0 / 3.0, 0)
    n_in, _, ov, _ = pn.overlap_pair(X, X, z, 4.0, z, 4.0, I, np.array([-1.0, 0.0, 0.0]), I, z, 8)   # -> (3,4,4) clear, (4,4,4) set, q = 12 outside
    assert (n_in, ov) == (1, 1.0 / 3.0)
    assert pn.overlap_pair(X, X, z, 4.0, z, 4.0, I, np.array([8.0, 0.0, 0.1]), I, z, 8)[3] == 1      # d^2 = 64.01 > 64
    assert pn.overlap_pair(X, X, z, 4.0, z, 4.0, I, np.array([8.0, 0.0, 0.0]), I, z, 8)[3] == 0      # d^2 = s^2: touching spheres are scored
    assert pn.overlap_pair(X, X, z, 4.0, z, 0.0, I, z, I, z, 8)[3] == 2                               # rho_j = 0
    assert pn.overlap_pair(X, X, z, 4.0, z, 4.0, I, np.array([np.nan, 0.0, 0.0]), I, z, 8)[3] == 1


def test_reference_greedy_on_hand_made_matrices():
    def run(n, edges):
        conf = np.zeros((n, n), bool)
        for a, b in edges:
            conf[a, b] = conf[b, a] = True
        keep, by = pn.greedy_from_conflicts(conf)
        return keep.tolist(), by.tolist()
    # a chain a - b - c: b goes, and c, whose only conflict is with the suppressed b, stays
    assert run(3, [(0, 1), (1, 2)]) == ([True, False, True], [-1, 0, -1])
    # suppressed_by is the FIRST kept pose in rank order that conflicts
    assert run(4, [(0, 3), (2, 3)]) == ([True, True, True, False], [-1, -1, -1, 0])
    assert run(4, [(0, 1), (1, 3), (2, 3)]) == ([True, False, True, False], [-1, 0, -1, 2])
    assert run(0, []) == ([], []) and run(1, []) == ([True], [-1])
    # the conflict is the max of the two directions, status 0 only, >= thr
    pairs = np.array([[0, 1], [1, 0], [1, 2], [2, 1], [0, 2], [2, 0]])
    keep, by = pn.nms_greedy_ref([0, 3], [0, 6], pairs, np.array([0.1, 0.3, 0.9, 0.9, 0.29, 0.2]), np.array([0, 0, 1, 2, 0, 0]), 0.3)
    assert keep.tolist() == [1, 0, 1] and by.tolist() == [-1, 0, -1]


def test_a_score_tie_keeps_the_earlier_row():
    from foundpose_amd import pose_nms
    rows = [dict(scene_id=1, im_id=2, obj_id=5, score=s) for s in (0.5, 0.9, 0.9, 0.7)] + [dict(scene_id=1, im_id=1, obj_id=5, score=0.1)]
    order, group_off = pose_nms.rank_layout(rows)
    assert order.tolist() == [1, 2, 3, 0, 4] and group_off.tolist() == [0, 4, 5]   # frames in the order of their first row; the tie in input order
    # rows 1 and 2 conflict: the reference greedy on this layout keeps row 1, the earlier one
    keep, by = pn.nms_greedy_ref(group_off, [0, 2, 2], np.array([[0, 1], [1, 0]]), np.array([0.8, 0.8]), np.array([0, 0]), 0.3)
    assert [int(order[i]) for i in np.nonzero(keep == 0)[0]] == [2] and int(order[by[1]]) == 1


def test_frame_pairs():
    from foundpose_amd import pose_nms
    group_off, obj = [0, 3, 3, 4, 6], [0, 1, 0, 2, 1, 1]
    pairs, pair_off = pose_nms.frame_pairs(group_off, obj)
    assert pairs.dtype == np.int32 and pair_off.dtype == np.int32
    assert pairs.tolist() == [[0, 2], [2, 0], [4, 5], [5, 4]] and pair_off.tolist() == [0, 2, 2, 2, 4]
    pairs, pair_off = pose_nms.frame_pairs(group_off, obj, cross_object=True)
    assert pairs.tolist() == [[0, 1], [0, 2], [1, 0], [1, 2], [2, 0], [2, 1], [4, 5], [5, 4]] and pair_off.tolist() == [0, 6, 6, 6, 8]
    pairs, pair_off = pose_nms.frame_pairs([0], [])
    assert pairs.shape == (0, 2) and pair_off.tolist() == [0]
    for bad in ([0, 3], [1, 6], [0, 4, 3, 6]):
        with pytest.raises(ValueError, match="group_off"):
            pose_nms.frame_pairs(bad, obj)


def test_csv_round_trip_of_the_writer(tmp_path):
    from foundpose_amd import eval_bop19, pose_nms
    rng = np.random.default_rng(3)
    rows = [dict(scene_id=48, im_id=i // 2, obj_id=1 + i % 3, score=float(rng.random()), R=rng.normal(size=(3, 3)), t=rng.normal(size=3) * 1e3,
                 time=float(rng.random())) for i in range(7)]
    a, b = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    pose_nms.write_results_csv(a, rows)
    back = eval_bop19.load_results_csv(a)
    assert len(back) == 7
    for r, q in zip(rows, back):
        assert all(r[k] == q[k] for k in ("scene_id", "im_id", "obj_id", "score", "time")) and np.array_equal(r["R"], q["R"]) and np.array_equal(r["t"], q["t"])
    pose_nms.write_results_csv(b, back)
    assert open(a, "rb").read() == open(b, "rb").read()
    # the same bytes as the drivers' own writer for the same entries
    from foundpose_amd import eval_util
    d = tmp_path / "out" / "1"
    d.mkdir(parents=True)
    entries = [dict(scene_id=r["scene_id"], img_id=r["im_id"], obj_id=1, score=r["score"], R=r["R"].tolist(), t=r["t"].reshape(3, 1).tolist(), cnos_time=0.0,
                    time={"all": 0.0}) for r in rows]
    json.dump(entries, open(d / "estimated-poses.json", "w"))
    ours = str(tmp_path / "ours.csv")
    pose_nms.write_results_csv(ours, [dict(r, obj_id=1, time=0.0) for r in rows])
    assert open(eval_util.prepare_bop_submission(str(tmp_path / "out"), "d", [1]), "rb").read() == open(ours, "rb").read()
    pose_nms.write_results_csv(b, [])
    assert eval_bop19.load_results_csv(b) == []
    # the decisions' records
    result = {"keep": np.array([True, False] + [True] * 5), "suppressed_by": np.array([-1, 0] + [-1] * 5), "overlap": np.array([np.nan, 0.5] + [np.nan] * 5)}
    rec = json.loads(json.dumps(pose_nms.decision_records(rows, result)))
    assert rec[1] == dict(row=1, scene_id=48, im_id=0, obj_id=2, keep=False, suppressed_by=0, overlap=0.5) and rec[0]["overlap"] is None and rec[0]["keep"]


def test_argument_checks_that_come_before_any_device_work(monkeypatch):
    from foundpose_amd import ops, pose_nms
    launched = []
    monkeypatch.setattr(ops, "call", lambda *a: launched.append(a[0]))
    monkeypatch.setattr(pose_nms, "upload_async", lambda *a: launched.append("upload"))
    N = 3
    good = dict(points=torch.zeros(10, 3), ranges=[(0, 4), (4, 10)], centers=np.zeros((2, 3)), radii=np.ones(2), pose_obj=[0, 1, 0], valid=[1, 1, 1],
                R=np.tile(np.eye(3), (N, 1, 1)), t=np.zeros((N, 3)), pairs=[[0, 1], [1, 0]])
    run = lambda **kw: pose_nms.pose_overlaps(**dict(good, **kw))
    for bad in (7, 33, 16.0, True, "16"):
        with pytest.raises(ValueError, match="grid"):
            run(grid=bad)
    for bad in (torch.zeros(10, 3, dtype=torch.float64), torch.zeros(10, 4), torch.zeros(30), np.zeros((10, 3), np.float32)):
        with pytest.raises(ValueError, match=r"points must be a float32 tensor \[M_total, 3\]"):
            run(points=bad)
    with pytest.raises(ValueError, match="same O objects"):
        run(radii=np.ones(3))
    with pytest.raises(ValueError, match="same N poses"):
        run(t=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="same N poses"):
        run(valid=[1, 1])
    with pytest.raises(ValueError, match="must hold integers"):
        run(pose_obj=[0.0, 1.0, 0.0])
    for bad in ([0, 2, 0], [-1, 0, 0]):
        with pytest.raises(ValueError, match=r"outside the samples' \[0, 2\)"):
            run(pose_obj=bad)
    for bad in ([[0, 3]], [[-1, 0]]):
        with pytest.raises(ValueError, match="names a pose outside"):
            run(pairs=bad)
    with pytest.raises(ValueError, match=r"pairs must be int32 \[P, 2\]"):
        run(pairs=[[0, 1, 2]])
    with pytest.raises(ValueError, match="on the device"):   # everything else in order: a host tensor is refused, not copied
        run()
    # the greedy pass: the threshold, the offsets and a frame of 257 poses
    ov, st = torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), float("inf"), True, "0.3"):
        with pytest.raises(ValueError, match="thresh"):
            pose_nms.nms_greedy([0, 3], [0, 2], good["pairs"], ov, st, bad)
    with pytest.raises(ValueError, match="at most 256 per frame"):
        pose_nms.nms_greedy([0, 1, 258], [0, 0, 2], [[1, 2], [2, 1]], ov, st)
    for go, po in (([0, 3], [0, 1]), ([1, 3], [0, 2]), ([0, 3, 2], [0, 2, 2]), ([0, 3], [0, 1, 2])):
        with pytest.raises(ValueError, match="group_off|pair_off"):
            pose_nms.nms_greedy(go, po, good["pairs"], ov, st)
    with pytest.raises(ValueError, match="outside its own frame"):
        pose_nms.nms_greedy([0, 1, 3], [0, 0, 2], [[0, 1], [1, 0]], ov, st)
    with pytest.raises(ValueError, match="overlap must be"):
        pose_nms.nms_greedy([0, 3], [0, 2], good["pairs"], ov.float(), st)
    with pytest.raises(ValueError, match="on the device"):
        pose_nms.nms_greedy([0, 3], [0, 2], good["pairs"], ov, st)
    # suppress_duplicates: an object without a sample, a frame of 257 rows; no rows and a single row need no device
    from foundpose_amd.bank import VerifyPoints
    samples = (VerifyPoints(torch.zeros(10, 3), [(0, 10)], np.zeros((1, 3)), np.ones(1)), {5: 0})
    row = dict(scene_id=1, im_id=1, obj_id=5, score=1.0, R=np.eye(3), t=np.zeros(3), time=0.0)
    with pytest.raises(ValueError, match="no point sample for object 6"):
        pose_nms.suppress_duplicates([row, dict(row, obj_id=6)], samples)
    with pytest.raises(ValueError, match="257 poses: at most 256 per frame"):
        pose_nms.suppress_duplicates([row] * 257, samples)
    for bad in (0.0, 1.01, True):
        with pytest.raises(ValueError, match="thresh"):
            pose_nms.suppress_duplicates([row], samples, thresh=bad)
    assert pose_nms.suppress_duplicates([], samples)["keep"].shape == (0,)
    one = pose_nms.suppress_duplicates([row, dict(row, im_id=2)], samples)   # two frames of one row each: no pair
    assert one["keep"].tolist() == [True, True] and one["suppressed_by"].tolist() == [-1, -1] and np.isnan(one["overlap"]).all()
    assert launched == []


def test_samples_from_vertices_are_the_banks_stride_samples():
    from foundpose_amd import pose_nms
    rng = np.random.default_rng(1)
    verts = {7: rng.normal(size=(10, 3)).astype(np.float32), 3: torch.from_numpy(rng.normal(size=(5, 3)))}
    vp, lid_to_obj = pose_nms.samples_from_vertices(verts, max_points=4, device="cpu")
    assert lid_to_obj == {3: 0, 7: 1} and vp.ranges == [(0, 3), (3, 7)]           # strides ceil(5 / 4) = 2 and ceil(10 / 4) = 3
    assert np.array_equal(vp.points.numpy(), np.concatenate([verts[3].numpy()[::2].astype(np.float32), verts[7][::3]]))
    P = vp.points.numpy().astype(np.float64)
    assert np.array_equal(vp.centers[1], (P[3:7].min(0) + P[3:7].max(0)) / 2.0)
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError, match="max_points"):
            pose_nms.samples_from_vertices(verts, max_points=bad, device="cpu")


def test_driver_options_are_validated_without_a_gpu():
    from foundpose_amd import infer
    base = infer.load_opts({"infer_opts": dict(version="v", repre_version="r", object_dataset="d")})
    assert (base.frame_select_type, base.pose_nms_thresh, base.pose_nms_grid, base.pose_nms_max_points, base.pose_nms_cross_object) == ("none", 0.3, 16, 4096, False)
    assert infer.FRAME_SELECT_TYPES == ("none", "pose_nms")
    for sel in infer.FRAME_SELECT_TYPES:
        for coarse in infer.COARSE_SELECT_TYPES:
            infer._check_driver_opts(base._replace(frame_select_type=sel, coarse_select_type=coarse))
    for bad in ("nms", "", None, True):
        with pytest.raises(ValueError, match="frame select type"):
            infer._check_driver_opts(base._replace(frame_select_type=bad))
    for good in (0.01, 1, 1.0):
        infer._check_driver_opts(base._replace(pose_nms_thresh=good))
    for bad in (0, 0.0, -0.3, 1.0001, float("nan"), float("inf"), "0.3", True, None):
        with pytest.raises(ValueError, match="pose_nms_thresh"):
            infer._check_driver_opts(base._replace(pose_nms_thresh=bad))
    for good in (8, 16, 32):
        infer._check_driver_opts(base._replace(pose_nms_grid=good))
    for bad in (7, 33, 0, -16, 16.0, "16", True):
        with pytest.raises(ValueError, match="pose_nms_grid"):
            infer._check_driver_opts(base._replace(pose_nms_grid=bad))
    for bad in (0, -3, 2.5, "9", True):
        with pytest.raises(ValueError, match="pose_nms_max_points"):
            infer._check_driver_opts(base._replace(pose_nms_max_points=bad))
    for bad in (0, 1, "false", None):
        with pytest.raises(ValueError, match="pose_nms_cross_object"):
            infer._check_driver_opts(base._replace(pose_nms_cross_object=bad))
    # the options are checked whatever frame_select_type says, like the mask_verify_* ones
    assert infer.load_opts({"infer_opts": dict(version="v", repre_version="r", object_dataset="d", frame_select_type="pose_nms", pose_nms_grid=8)}).pose_nms_grid == 8


def test_header_and_binding_declare_both_entries():
    from foundpose_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    assert int(re.search(r"#define\s+FP_ABI_VERSION\s+(\d+)", header).group(1)) == 20 == _lib.ABI_VERSION
    api = open(os.path.join(ROOT, "foundpose_amd", "csrc", "api.cpp")).read()
    for name, n_args in (("fp_pose_overlap", 18), ("fp_pose_nms_greedy", 12)):
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in the header"
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        proto = _lib._PROTOS[name]
        assert len(args) == len(proto) == n_args
        for a, ty in zip(args, proto):
            want = _lib.vp if ("*" in a or a.startswith("fp_stream_t")) else {"int": _lib.i32, "double": _lib.f64}[a.split()[0]]
            assert ty is want, a
        assert f"int {name}(" in api and name in _lib.exported_symbols()
    assert "pose_nms.hip" in build.SOURCES
    src = open(os.path.join(ROOT, "foundpose_amd", "csrc", "pose_nms.hip")).read()
    assert '#include "verify_grid.hpp"' in src and "contract(off)" in src
    kernels = open(os.path.join(ROOT, "foundpose_amd", "csrc", "kernels.hpp")).read()
    from foundpose_amd import pose_nms
    assert f"PN_MIN_GRID = {pose_nms.MIN_GRID}, PN_MAX_GRID = {pose_nms.MAX_GRID}" in kernels and f"PN_MAX_GROUP = {pose_nms.MAX_GROUP}" in kernels
