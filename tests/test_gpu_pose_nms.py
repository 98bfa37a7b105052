"""fp_pose_overlap and fp_pose_nms_greedy (foundpose_amd/pose_nms.py) against their numpy restatement (tests/pose_nms_ref.py) on the smallest
frame that reaches every path: the blob objects of tests/pose_verify_ref.py -- 600 and 602 sampled points, more than two rounds of the
256-thread point loops -- and 8 poses: the planted pose of object 0, the same pose again, a shift by rho / 16 and by rho / 2, object 1
interpenetrating, disjoint spheres, an invalid pose and a NaN in t; every ordered pair (56), G = 8 and G = 16.  The fixture is far from
every decision boundary (min_margin, asserted on the CPU too), every output is an integer count or the fp64 quotient of two of them, so
counts, status and overlap must be EQUAL, bit for bit; and the same bits alone, in the batch and in the reversed batch.  The greedy pass is
compared on the GPU's own overlaps and on seeded random ones (frames of 0, 1, 2, 65 and 256 poses).

The restatement's figures, which the GPU's equal (seed 6): the same pose twice overlaps by 1.0 (600 / 600) at both grids; the rho / 16
shift by 0.933 at G = 8 and 0.747 at G = 16, the rho / 2 shift by 0.323 and 0.112; at thr = 0.3 the greedy pass therefore removes poses 1,
2 and 3 at G = 8 and poses 1 and 2 at G = 16."""

import numpy as np
import pytest
import torch

from tests import pose_nms_ref as pn

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[8, 16])
def fix(request):
    out = pn.gpu_fixture(seed=6, grid=request.param)
    assert out["ref"]["min_margin"] > 1e-6
    return out


@pytest.fixture(scope="module")
def points(fix):
    return torch.from_numpy(fix["points"]).to("cuda")


def _run(fix, points, pairs=None, **kw):
    from foundpose_amd import pose_nms
    args = dict(ranges=fix["ranges"], centers=fix["centers"], radii=fix["radii"], pose_obj=fix["pose_obj"], valid=fix["valid"], R=fix["R"], t=fix["t"],
                pairs=fix["pairs"] if pairs is None else pairs, grid=fix["grid"])
    args.update(kw)
    out = pose_nms.pose_overlaps(points, **args)
    torch.cuda.synchronize()
    assert out["counts"].dtype == torch.int32 and out["status"].dtype == torch.int32 and out["overlap"].dtype == torch.float64
    return out


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_equal(out, want):
    assert np.array_equal(out["counts"], want["counts"])
    assert np.array_equal(out["status"], want["status"])
    assert np.array_equal(out["overlap"].view(np.int64), np.asarray(want["overlap"]).view(np.int64))   # the same division of the same integers


def test_overlaps_match_the_restatement(fix, points):
    ref = fix["ref"]
    out = _np(_run(fix, points))
    show = [pn.pair_index(fix, 0, j) for j in (1, 2, 3, 4, 5, 6, 7)]
    print("G =", fix["grid"], "pairs (0, j): counts GPU", out["counts"][show].tolist(), "restatement", ref["counts"][show].tolist())
    print("overlap GPU", out["overlap"][show].tolist(), "restatement", ref["overlap"][show].tolist(), "status GPU", out["status"][show].tolist())
    _assert_equal(out, ref)
    assert out["overlap"][pn.pair_index(fix, 0, 1)] == 1.0 and sorted(set(out["status"].tolist())) == [0, 1, 2]


def test_alone_in_the_batch_and_reversed_are_the_same_bits(fix, points):
    both = _np(_run(fix, points))
    rev = _np(_run(fix, points, pairs=fix["pairs"][::-1].copy()))
    for k, v in both.items():
        assert np.array_equal(v, rev[k][::-1]), k
    for p, pair in enumerate(fix["pairs"]):
        alone = _np(_run(fix, points, pairs=pair[None]))
        for k, v in alone.items():
            assert np.array_equal(v[0], both[k][p]), (p, k)


def test_greedy_on_the_gpus_own_overlaps_equals_the_reference(fix, points):
    from foundpose_amd import pose_nms
    ref = fix["ref"]
    out = _run(fix, points)
    want_keep, want_by = pn.nms_greedy_ref(fix["group_off"], fix["pair_off"], fix["pairs"], ref["overlap"], ref["status"], fix["thr"])
    for pairs in (fix["pairs"], torch.from_numpy(fix["pairs"]).to("cuda")):   # the pairs as a host table, and as the tensor an upload left
        got = _np(pose_nms.nms_greedy(fix["group_off"], fix["pair_off"], pairs, out["overlap"], out["status"], fix["thr"]))
        assert got["keep"].dtype == np.int32 and got["suppressed_by"].dtype == np.int32
        assert np.array_equal(got["keep"], want_keep) and np.array_equal(got["suppressed_by"], want_by)
    assert want_keep.tolist() == {8: [1, 0, 0, 0, 1, 1, 1, 1], 16: [1, 0, 0, 1, 1, 1, 1, 1]}[fix["grid"]]
    # the whole stage on the same poses as csv rows (same-object pairs only: object 1's pose is compared with nothing)
    rows = [dict(scene_id=1, im_id=1, obj_id=int(o) + 10, score=float(s), R=R, t=t) for o, s, R, t in zip(fix["pose_obj"], fix["scores"], fix["R"], fix["t"])]
    rows = [rows[i] for i in (3, 0, 4, 1, 2, 5, 7)]   # any input order (the invalid pose is no row); the tie 0 / 1 keeps its order
    from foundpose_amd.bank import VerifyPoints
    samples = (VerifyPoints(points, fix["ranges"], fix["centers"], fix["radii"]), {10: 0, 11: 1})
    res = pose_nms.suppress_duplicates(rows, samples, thresh=fix["thr"], grid=fix["grid"])
    gone = {8: {3: 1, 4: 1, 0: 1}, 16: {3: 1, 4: 1}}[fix["grid"]]   # input row -> the input row that suppressed it (row 1 is pose 0)
    assert res["keep"].tolist() == [i not in gone for i in range(7)]
    assert res["suppressed_by"].tolist() == [gone.get(i, -1) for i in range(7)]
    at = lambda i, j: pn.pair_index(fix, i, j)
    assert res["overlap"][3] == 1.0 and res["overlap"][4] == max(ref["overlap"][at(0, 2)], ref["overlap"][at(2, 0)])
    assert np.isnan(res["overlap"][[i for i in range(7) if i not in gone]]).all()


def test_greedy_on_seeded_random_overlaps_equals_the_reference():
    from foundpose_amd import pose_nms
    syn = pn.synthetic_groups(seed=0)
    assert np.diff(syn["group_off"]).tolist() == [0, 1, 2, 65, 256] and len(syn["pairs"]) == 2 + 65 * 64 + 256 * 255
    want_keep, want_by = pn.nms_greedy_ref(syn["group_off"], syn["pair_off"], syn["pairs"], syn["overlap"], syn["status"], syn["thr"])
    dev = "cuda"
    got = _np(pose_nms.nms_greedy(syn["group_off"], syn["pair_off"], syn["pairs"], torch.from_numpy(syn["overlap"]).to(dev),
                                  torch.from_numpy(syn["status"]).to(dev), syn["thr"]))
    sizes = np.diff(syn["group_off"])
    print("kept per frame:", [int(want_keep[b:b + n].sum()) for b, n in zip(syn["group_off"][:-1], sizes)], "of", sizes.tolist())
    assert np.array_equal(got["keep"], want_keep) and np.array_equal(got["suppressed_by"], want_by)
    # the case is not trivial: poses are suppressed in both larger frames, some by a pose that is not the frame's first, and some pose
    # outlives a conflict with a suppressed one
    for g in (3, 4):
        b, e = syn["group_off"][g], syn["group_off"][g + 1]
        assert 0 < want_keep[b:e].sum() < e - b and (want_by[b:e] > b).any()
    b, pb = int(syn["group_off"][4]), int(syn["pair_off"][4])
    conf = pn.conflicts(256, b, syn["pairs"][pb:], syn["overlap"][pb:], syn["status"][pb:], syn["thr"])
    kept = want_keep[b:] == 1
    assert (np.triu(conf, 1) & ~kept[:, None] & kept[None, :]).any()


def test_bad_arguments_raise_before_anything_is_launched(fix, points, monkeypatch):
    from foundpose_amd import ops, pose_nms
    launched = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda *a: (launched.append(a[0]), real(*a))[1])
    for bad in (7, 33, 16.0):
        with pytest.raises(ValueError, match="grid"):
            _run(fix, points, grid=bad)
    with pytest.raises(ValueError, match="outside the samples'"):
        _run(fix, points, pose_obj=np.array([0, 0, 0, 0, 2, 0, 0, 0]))
    with pytest.raises(ValueError, match="names a pose outside"):
        _run(fix, points, pairs=np.array([[0, 8]]))
    with pytest.raises(ValueError, match="host table"):
        _run(fix, points, R=torch.from_numpy(fix["R"]).to("cuda"))
    with pytest.raises(ValueError, match="float32"):
        _run(fix, points.double())
    empty = _run(fix, points, pairs=np.zeros((0, 2), np.int32))   # no pair: empty tensors, no launch
    assert tuple(empty["counts"].shape) == (0, 2) and tuple(empty["overlap"].shape) == (0,) and tuple(empty["status"].shape) == (0,)
    ov, st = torch.zeros(2, dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="257 poses: at most 256 per frame"):
        pose_nms.nms_greedy([0, 257], [0, 2], [[0, 1], [1, 0]], ov, st)
    from foundpose_amd.bank import VerifyPoints
    samples = (VerifyPoints(points, fix["ranges"], fix["centers"], fix["radii"]), {1: 0})
    row = dict(scene_id=1, im_id=1, obj_id=1, score=1.0, R=fix["R"][0], t=fix["t"][0], time=0.0)
    with pytest.raises(ValueError, match="257 poses: at most 256 per frame"):
        pose_nms.suppress_duplicates([row] * 257, samples)
    assert launched == []
    res = pose_nms.suppress_duplicates([row] * 256, samples)   # the largest frame: the first row keeps, every other is its duplicate
    assert res["keep"].tolist() == [True] + [False] * 255 and set(res["suppressed_by"][1:].tolist()) == {0} and (res["overlap"][1:] == 1.0).all()
    assert launched == ["fp_pose_overlap", "fp_pose_nms_greedy"]


def test_the_c_entries_refuse_a_bad_grid_and_clamp_bad_indices(fix, points):
    """The entry point itself: a grid outside [8, 32] is an error; indices the Python layer would have refused are skipped (status 2) and
    read nothing."""
    from foundpose_amd import _lib, ops
    dev = "cuda"
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
    rng, cen, rad = t(fix["ranges"], torch.int32), t(fix["centers"], torch.float64), t(fix["radii"], torch.float64)
    obj, ok, R, tt = t(fix["pose_obj"], torch.int32), t(fix["valid"], torch.int32), t(fix["R"], torch.float64), t(fix["t"], torch.float64)
    for bad in (7, 33):
        with pytest.raises(_lib.FoundPoseNativeError, match="grid"):
            ops.pose_overlap(points, rng, cen, rad, obj, ok, R, tt, t(fix["pairs"], torch.int32), bad)
    pairs = t([[0, 1], [0, 8], [-1, 0], [4, 0]], torch.int32)
    bad_obj = obj.clone()
    bad_obj[4] = 2
    counts, overlap, status = ops.pose_overlap(points, rng, cen, rad, bad_obj, ok, R, tt, pairs, fix["grid"])
    torch.cuda.synchronize()
    assert status.tolist() == [0, 2, 2, 2] and overlap.tolist() == [1.0, 0.0, 0.0, 0.0] and not counts[1:].any()


def _write_ply(path, verts):
    """An ascii PLY of the vertices (9 significant digits: float32 round-trips) and one face, which the loader asks for."""
    lines = ["ply", "format ascii 1.0", f"element vertex {len(verts)}", "property float x", "property float y", "property float z",
             "element face 1", "property list uchar int vertex_indices", "end_header"]
    lines += [" ".join("%.9g" % c for c in v) for v in verts] + ["3 0 1 2"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_the_command_line_tool_filters_a_csv(tmp_path):
    """python -m foundpose_amd.pose_nms on a csv of the fixture's poses and PLY files of its objects: the kept rows in their input order,
    with their bytes, and one decision per input row."""
    import json
    from foundpose_amd import eval_bop19, pose_nms
    from tests import pose_verify_ref as pv
    fix = pn.gpu_fixture(seed=6, grid=16)
    for lid, verts in zip((10, 11), pv.gpu_fixture(6)["verts"]):
        _write_ply(str(tmp_path / f"obj_{lid:06d}.ply"), verts)
    poses = (3, 0, 4, 1, 2, 5, 7)   # any input order; pose 7 has a NaN in t, which a csv can hold
    rows = [dict(scene_id=1, im_id=1, obj_id=int(fix["pose_obj"][p]) + 10, score=float(fix["scores"][p]), R=fix["R"][p], t=fix["t"][p], time=0.5) for p in poses]
    rows.append(dict(rows[1], im_id=2))   # the planted pose alone in a second frame
    src, out = str(tmp_path / "in.csv"), str(tmp_path / "out.csv")
    pose_nms.write_results_csv(src, rows)
    pose_nms.main(["--result-csv", src, "--models-dir", str(tmp_path), "--output", out, "--max-points", "700"])   # 1203 vertices: every second
    gone = {3: 1, 4: 1}   # poses 1 and 2 are duplicates of pose 0 (row 1) at G = 16, thr = 0.3
    lines = open(src).read().splitlines()
    assert open(out).read().splitlines() == [lines[0]] + [l for i, l in enumerate(lines[1:]) if i not in gone]
    assert len(eval_bop19.load_results_csv(out)) == 6
    rec = json.load(open(out + ".nms.json"))
    assert [r["row"] for r in rec] == list(range(8)) and [r["keep"] for r in rec] == [i not in gone for i in range(8)]
    assert [r["suppressed_by"] for r in rec] == [gone.get(i, -1) for i in range(8)] and rec[3]["overlap"] == 1.0 and rec[0]["overlap"] is None
    # a coarser grid through the options: at G = 8 the rho / 2 shift (row 0) goes too
    pose_nms.main(["--result-csv", src, "--models-dir", str(tmp_path), "--output", out, "--max-points", "700", "--grid", "8", "--thresh", "0.3"])
    assert [r["keep"] for r in json.load(open(out + ".nms.json"))] == [False, True, True, False, False, True, True, True]
