"""Multi-view pose consensus on the device (csrc/multiview.hip, foundpose_amd/multiview.py, the driver's scene_select_type; DESIGN.md
section 37) against the numpy restatement (tests/multiview_ref.py)."""

import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, eval_bop19, multiview, ops, pose_nms
from tests import lm_steps
from tests import multiview_ref as mv
from tests.test_gpu_depth_refine import driver_split  # noqa: F401  (the planted split of the depth drivers' tests)

pytestmark = pytest.mark.gpu

NAMES = list(mv.KERNEL_SPECS)
FEW, NOPOSE = "few", "nopose"


def _dets(names):
    """The fixtures' problems by name; "few": the first 5 rows of five_views (status 2), "nopose": five_views without a pose."""
    out = []
    for n in names:
        if n == FEW:
            d = mv.kernel_fixture("five_views").det
            out.append(dict(d, Y=d["Y"][:5], uv=d["uv"][:5], view=d["view"][:5]))
        elif n == NOPOSE:
            out.append(dict(mv.kernel_fixture("five_views").det, has_pose=False))
        else:
            out.append(mv.kernel_fixture(n).det)
    return out


def _tensors(dets):
    cam, T = mv.view_tables()
    dev = "cuda"
    ends = np.cumsum([len(d["Y"]) for d in dets])
    return dict(points=torch.from_numpy(np.concatenate([d["Y"] for d in dets]).astype(np.float32)).to(dev),
                targets=torch.from_numpy(np.concatenate([d["uv"] for d in dets])).to(dev),
                view_index=torch.from_numpy(np.concatenate([d["view"] for d in dets]).astype(np.int32)).to(dev),
                view_cam=torch.from_numpy(cam).to(dev), view_T=torch.from_numpy(T).to(dev),
                row_begin=torch.from_numpy((ends - [len(d["Y"]) for d in dets]).astype(np.int32)).to(dev),
                row_end=torch.from_numpy(ends.astype(np.int32)).to(dev),
                R=torch.from_numpy(np.stack([d["R"] for d in dets])).to(dev), t=torch.from_numpy(np.stack([d["t"] for d in dets])).to(dev),
                has_pose=torch.tensor([bool(d.get("has_pose", True)) for d in dets], device=dev))


def _run(names, iters, **kw):
    out = ops.multiview_refine(**_tensors(_dets(names)), huber_px=mv.DELTA, iters=iters, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _ref(name, iters):
    (d,) = _dets([name])
    cam, T = mv.view_tables()
    return mv.refine(d["R"], d["t"], d["Y"].astype(np.float64), d["uv"], d["view"], cam, T, mv.DELTA, iters, d.get("has_pose", True))


def _rot_rad(Ra, Rb):
    return float(np.arccos(np.clip(0.5 * (np.trace(Ra @ Rb.T) - 1.0), -1.0, 1.0)))


BATCH = NAMES + [NOPOSE, FEW]


def test_normal_equations_at_the_input_pose():
    got = _run(BATCH, 0, want_normal_eq=True)
    cam, T = mv.view_tables()
    for b, (name, d) in enumerate(zip(BATCH, _dets(BATCH))):
        if name == NOPOSE:
            assert not got["normal_eq"][b].any() and got["status"][b] == 2 and got["num_points"][b] == 0
            continue
        want = mv.normal_equations(d["R"], d["t"], d["Y"].astype(np.float64), d["uv"], d["view"], cam, T, mv.DELTA)
        for lo, hi in ((0, 21), (21, 27), (27, 28)):
            err = np.abs(got["normal_eq"][b, lo:hi] - want[lo:hi]).max() / np.abs(want[lo:hi]).max()
            print(name, (lo, hi), f"{err:.2e}")
            assert err < 1e-9, (name, lo, hi, err)
        ref = _ref(name, 0)
        assert got["num_points"][b] == ref["num_points"] and got["status"][b] == (2 if name == FEW else 1) and got["iters_used"][b] == 0
        assert np.array_equal(got["R"][b], d["R"]) and np.array_equal(got["t"][b], d["t"])          # no step: the input bit for bit


@pytest.mark.parametrize("name", NAMES)
def test_final_poses_over_the_pinned_prefix(name):
    fx = mv.kernel_fixture(name)
    sweep = sorted({0, 1, 2, fx.K // 2, fx.K})
    for iters in sweep:
        got, ref = _run([name], iters), _ref(name, iters)
        dr, dt = _rot_rad(got["R"][0], ref["R"]), float(np.linalg.norm(got["t"][0] - ref["t"]))
        print(name, iters, f"{dr:.2e} rad {dt:.2e} mm", got["iters_used"][0], got["status"][0], got["cost_in"][0], got["cost_out"][0])
        assert dr < lm_steps.POSE_RAD and dt < lm_steps.POSE_MM, (name, iters, dr, dt)
        assert got["iters_used"][0] == ref["iters_used"] and got["status"][0] == ref["status"] and got["num_points"][0] == ref["num_points"]
        assert abs(got["cost_out"][0] - ref["cost_out"]) <= 1e-9 * ref["cost_in"] and got["cost_out"][0] <= got["cost_in"][0]


def test_mixed_batch_statuses_and_untouched_poses():
    got = _run(BATCH, 20)
    for b, name in enumerate(BATCH):
        ref = _ref(name, 20)
        assert got["status"][b] == ref["status"], name
        if name in (NOPOSE, FEW):
            d = _dets([name])[0]
            assert got["status"][b] == 2 and np.array_equal(got["R"][b], d["R"]) and np.array_equal(got["t"][b], d["t"])
            assert got["num_points"][b] == ref["num_points"] and got["iters_used"][b] == 0


def test_a_problem_gives_the_same_bits_alone_first_and_last():
    iters = 6
    alone = {n: _run([n], iters, want_normal_eq=True) for n in BATCH}
    for order in (BATCH, BATCH[::-1], BATCH[2:] + BATCH[:2]):
        got = _run(order, iters, want_normal_eq=True)
        for b, n in enumerate(order):
            for k, v in got.items():
                assert np.array_equal(v[b], alone[n][k][0]), (n, k, order.index(n))
    assert {order.index(n) for order in (BATCH, BATCH[::-1]) for n in BATCH[:1]} == {0, len(BATCH) - 1}


# ---------------------------------------------------------------------------------------------------------- refused calls
def _bad_calls():
    T = lambda: _tensors(_dets(["two_views", "five_views"]))   # noqa: E731
    def put(key, fn):
        def make():
            a = T()
            a[key] = fn(a[key])
            return a, {}
        return make
    cases = {
        "points on the host": put("points", lambda x: x.cpu()), "points fp64": put("points", lambda x: x.double()),
        "points [N, 2]": put("points", lambda x: x[:, :2]), "targets fp32": put("targets", lambda x: x.float()),
        "targets short": put("targets", lambda x: x[:-1]), "view_index int64": put("view_index", lambda x: x.long()),
        "view_index on the host": put("view_index", lambda x: x.cpu()), "view_cam [V, 3]": put("view_cam", lambda x: x[:, :3]),
        "view_cam fp32": put("view_cam", lambda x: x.float()), "view_T rows": put("view_T", lambda x: x[:-1]),
        "row_begin int64": put("row_begin", lambda x: x.long()), "row_end shape": put("row_end", lambda x: x[:1]),
        "R fp32": put("R", lambda x: x.float()), "R [B, 9]": put("R", lambda x: x.reshape(-1, 9)), "t on the host": put("t", lambda x: x.cpu()),
        "has_pose float": put("has_pose", lambda x: x.float()), "has_pose shape": put("has_pose", lambda x: x[:1]),
        "row_end beyond the rows": put("row_end", lambda x: x + 1), "row_begin negative": put("row_begin", lambda x: x - 1),
        "row_end before row_begin": put("row_end", lambda x: x * 0), "view index == V": put("view_index", lambda x: x + (torch.arange(len(x), device=x.device) == 100).int() * 6),
        "view index negative": put("view_index", lambda x: x - (torch.arange(len(x), device=x.device) == 3).int() * 7),
    }
    for name, kw in (("huber_px zero", dict(huber_px=0.0)), ("huber_px nan", dict(huber_px=float("nan"))), ("huber_px inf", dict(huber_px=float("inf"))),
                     ("huber_px bool", dict(huber_px=True)), ("iters negative", dict(iters=-1)), ("iters 1001", dict(iters=1001)), ("iters float", dict(iters=2.5)),
                     ("max_points below the longest range", dict(max_points=69)), ("max_points zero", dict(max_points=0))):
        cases[name] = (lambda kw=kw: (T(), kw))
    return cases


def test_every_refused_call_raises_before_a_launch(monkeypatch):
    calls = []
    real = _lib.call
    monkeypatch.setattr(ops, "call", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    for name, make in _bad_calls().items():
        args, kw = make()
        kw = dict(dict(huber_px=mv.DELTA, iters=3), **kw)
        with pytest.raises(ValueError, match="multiview_refine"):
            ops.multiview_refine(**args, **kw)
        assert not calls, name
    ops.multiview_refine(**_tensors(_dets(["two_views"])), huber_px=mv.DELTA, iters=1, max_points=70)
    assert calls == ["fp_multiview_refine"]


def test_the_c_entry_refuses_and_leaves_poisoned_outputs_untouched():
    a = _tensors(_dets(["two_views", "five_views"]))
    B, N, V, dev = 2, 140, 6, "cuda"
    outs = [torch.full(s, 7.5, dtype=torch.float64, device=dev) for s in ((B, 9), (B, 3), (B,), (B,))] + \
           [torch.full((B,), -77, dtype=torch.int32, device=dev) for _ in range(3)] + [torch.full((B, 28), 7.5, dtype=torch.float64, device=dev)]
    nbytes = _lib.multiview_scratch_bytes(B, 70)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    hp = torch.ones(B, dtype=torch.int32, device=dev)
    p = _lib.ptr

    def call(**kw):
        v = dict(points=a["points"], targets=a["targets"], view_index=a["view_index"], N=N, view_cam=a["view_cam"], view_T=a["view_T"], V=V,
                 row_begin=a["row_begin"], row_end=a["row_end"], huber=mv.DELTA, B=B, cap=70, iters=3, nbytes=nbytes, R_out=outs[0])
        v.update(kw)
        _lib.call("fp_multiview_refine", p(v["points"]), p(v["targets"]), p(v["view_index"]), v["N"], p(v["view_cam"]), p(v["view_T"]), v["V"],
                  p(v["row_begin"]), p(v["row_end"]), p(a["R"].reshape(B, 9).contiguous()), p(a["t"]), p(hp), v["huber"], v["B"], v["cap"], v["iters"],
                  p(scratch), v["nbytes"], p(v["R_out"]), *(p(o) for o in outs[1:]), _lib.stream())

    vi_bad = a["view_index"].clone()
    vi_bad[120] = 6
    rb_bad = a["row_begin"].clone()
    rb_bad[1] = -1
    refused = {"huber_px": dict(huber=0.0), "huber_px must": dict(huber=float("nan")), "iters": dict(iters=-1), "iters ": dict(iters=1001),
               "num_views": dict(V=0), "num_det": dict(B=0), "max_points": dict(cap=0), "scratch": dict(nbytes=nbytes - 1), "null pointer": dict(points=None),
               "null pointer ": dict(R_out=None), "view index": dict(view_index=vi_bad), "rows outside": dict(row_begin=rb_bad),
               "more than max_points": dict(cap=69, nbytes=_lib.multiview_scratch_bytes(B, 69)), "rows outside ": dict(N=139)}
    for text, kw in refused.items():
        with pytest.raises(_lib.FoundPoseNativeError, match=text.strip()):
            call(**kw)
        torch.cuda.synchronize()
        assert all(bool((o == 7.5).all()) for o in outs if o.dtype == torch.float64) and all(bool((o == -77).all()) for o in outs if o.dtype == torch.int32), text
    call()
    torch.cuda.synchronize()
    assert not any(bool((o == 7.5).any()) for o in outs[:2]) and not bool((outs[6] == -77).any())


# ---------------------------------------------------------------------------------------------------------- fuse_results, the tool
def _compare_fusion(rows, sc, models, out, rep, want_out, want_rep):
    assert len(rep["clusters"]) == len(want_rep["clusters"])
    for c, w in zip(rep["clusters"], want_rep["clusters"]):
        assert (c["seed_row"], c["rows"], c["status"], c["dropped_rows"]) == (w["seed"], w["members"], w["status"], w["dropped"])
        if w["status"] is not None:
            assert c["inliers"] == w["num_points"] and abs(c["cost_in"] - w["cost_in"]) <= 1e-9 * w["cost_in"]
    for i, (r, w) in enumerate(zip(rep["rows"], want_rep["rows"])):
        assert (r["cluster"], r["seed_row"], r["views"], r["sym"], r["fused"]) == (w["cluster"], w["seed"], w["views"], w["sym"], w["fused"]), i
        if w["d"] is not None:
            assert abs(r["dist_to_seed_mm"] - w["d"]) <= 1e-9 * max(w["d"], 1.0)
        if w["fused"]:
            dr, dt = _rot_rad(out[i]["R"], want_out[i]["R"]), float(np.linalg.norm(out[i]["t"] - want_out[i]["t"]))
            assert dr < lm_steps.POSE_RAD and dt < lm_steps.POSE_MM, (i, dr, dt)
        else:
            assert out[i]["R"] is rows[i]["R"] and out[i]["t"] is rows[i]["t"] and r["moved_mm"] == 0.0
    assert [(o["scene_id"], o["im_id"], o["obj_id"], o["score"], o["time"]) for o in out] == [(o["scene_id"], o["im_id"], o["obj_id"], o["score"], o["time"]) for o in rows]


@pytest.mark.parametrize("name", list(mv.SCENES))
def test_fuse_results_equals_the_restatement(name, tmp_path):
    rows, sc, models, _ = mv.SCENES[name]()
    kw = mv.SCENE_OPTS.get(name, {})
    want_out, want_rep = mv.fuse(rows, sc, models, **kw)
    out, rep = multiview.fuse_results(rows, sc, models, **kw)
    _compare_fusion(rows, sc, models, out, rep, want_out, want_rep)
    assert [u["scene_id"] for u in rep["unfused_scenes"]] == list(want_rep["unfused_scenes"])
    keep = [i for i, w in enumerate(want_rep["rows"]) if not w["fused"]]
    pose_nms.write_results_csv(str(tmp_path / "a.csv"), [out[i] for i in keep])
    pose_nms.write_results_csv(str(tmp_path / "b.csv"), [rows[i] for i in keep])
    assert (tmp_path / "a.csv").read_bytes() == (tmp_path / "b.csv").read_bytes()


def _write_tree(root, rows, sc, models):
    """A split directory, a models directory (ascii plys + models_info.json) and the results csv."""
    for sid, cams in sc.items():
        os.makedirs(root / "test" / f"{sid:06d}", exist_ok=True)
        (root / "test" / f"{sid:06d}" / "scene_camera.json").write_text(json.dumps(cams))
    os.makedirs(root / "models", exist_ok=True)
    info = {}
    for lid, m in models.items():
        P = m.pts.astype(np.float32)
        (root / "models" / f"obj_{lid:06d}.ply").write_text(
            "ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
            % len(P) + "".join(f"{float(x)!r} {float(y)!r} {float(z)!r}\n" for x, y, z in P) + "3 0 1 2\n")
        info[str(lid)] = {"diameter": m.diameter}
        sy = [np.concatenate([np.concatenate([s["R"], np.asarray(s["t"]).reshape(3, 1)], 1), [[0, 0, 0, 1.0]]]).reshape(16).tolist() for s in m.syms[1:]]
        if sy:
            info[str(lid)]["symmetries_discrete"] = sy
    (root / "models" / "models_info.json").write_text(json.dumps(info))
    pose_nms.write_results_csv(str(root / "in.csv"), rows)


def test_the_tool_writes_what_fuse_results_gives(tmp_path, capsys):
    rows, sc, models, _ = mv.SCENES["fourfold"]()
    _write_tree(tmp_path, rows, sc, models)
    argv = ["--result-csv", str(tmp_path / "in.csv"), "--dataset-dir", str(tmp_path / "test"), "--models-dir", str(tmp_path / "models"), "--output",
            str(tmp_path / "out.csv"), "--huber-px", "8", "--iters", "15"]
    multiview.main(argv)
    assert "6 of 6 rows fused in 1 clusters" in capsys.readouterr().out
    read = eval_bop19.load_results_csv(str(tmp_path / "in.csv"))
    loaded = multiview.load_models(str(tmp_path / "models"), [1])
    assert len(loaded[1].syms) == 4 and np.array_equal(loaded[1].pts, models[1].pts.astype(np.float32).astype(np.float64))
    out, rep = multiview.fuse_results(read, multiview.load_scene_cameras(str(tmp_path / "test"), [1]), loaded, huber_px=8.0, iters=15)
    pose_nms.write_results_csv(str(tmp_path / "want.csv"), out)
    assert (tmp_path / "out.csv").read_bytes() == (tmp_path / "want.csv").read_bytes()
    assert json.load(open(tmp_path / "out.csv.fuse.json")) == json.loads(json.dumps(rep))
    got = json.load(open(tmp_path / "out.csv.fuse.json"))
    assert set(got["rows"][0]) >= {"cluster", "seed_row", "views", "sym", "dist_to_seed_mm", "moved_mm", "moved_deg", "fused", "reason"}
    assert set(got["clusters"][0]) >= {"cost_in", "cost_out", "iters_used", "inliers", "status"}
    os.remove(tmp_path / "models" / "models_info.json")
    with pytest.raises(FileNotFoundError, match="models_info.json"):
        multiview.main(argv)


# ---------------------------------------------------------------------------------------------------------- the driver
def _drive(tmp, tag, driver_split, opts, **kw):
    from foundpose_amd import infer
    from tests.test_gpu_infer_batched import TARGETS
    ex, split, _, _ = driver_split
    d = str(tmp / tag)
    paths = infer.infer(opts, lambda lid: iter([split.frame(f, [lid]) for f in range(3)]), split.dets, split.repres, d, extractor=ex,
                        num_target_insts={lid: TARGETS[lid] for lid in (1, 2)}, **kw)
    csv = next(p for p in paths if p.endswith(".csv"))
    return d, csv, paths


def _strip_time(path):
    return [line.rsplit(",", 1)[0] for line in open(path).read().splitlines()]


def test_driver_scene_select(tmp_path, driver_split):
    from foundpose_amd import eval_util, infer
    from tests.test_gpu_infer_batched import IM_IDS
    ex, split, opts, _ = driver_split
    rng = np.random.default_rng(5)
    models = {lid: eval_util.EvalModel(split.repres[lid].vertices.cpu().numpy().astype(np.float64), [{"R": np.eye(3), "t": np.zeros((3, 1))}], 400.0)
              for lid in (1, 2)}
    plain = {str(im): {"cam_K": [c.f[0], 0, c.c[0], 0, c.f[1], c.c[1], 0, 0, 1], "depth_scale": 1.0} for im, c in zip(IM_IDS, split.cams)}
    base_dir, base_csv, base_paths = _drive(tmp_path, "base", driver_split, opts)
    # absent or "none": the files of the run without the field
    none_dir, none_csv, none_paths = _drive(tmp_path, "none", driver_split, opts._replace(scene_select_type="none"), scene_cameras={1: plain}, scene_models=models)
    assert _strip_time(none_csv) == _strip_time(base_csv)
    assert [os.path.relpath(p, none_dir) for p in none_paths] == [os.path.relpath(p, base_dir) for p in base_paths]
    assert not os.path.exists(os.path.join(none_dir, "scene-fuse.json"))
    # "multiview" without camera poses: the csv keeps its bytes and the report says why
    mopts = opts._replace(scene_select_type="multiview")
    d, csv, paths = _drive(tmp_path, "nopose", driver_split, mopts, scene_cameras={1: plain}, scene_models=models)
    assert _strip_time(csv) == _strip_time(base_csv) and paths[-1] == os.path.join(d, "scene-fuse.json")
    rep = json.load(open(paths[-1]))
    assert rep["unfused_scenes"][0]["scene_id"] == 1 and "cam_R_w2c" in rep["unfused_scenes"][0]["reason"] and not any(r["fused"] for r in rep["rows"])
    before = open(csv, "rb").read()
    multiview_rows = eval_bop19.load_results_csv(csv)
    pose_nms.write_results_csv(str(tmp_path / "again.csv"), multiview_rows)
    assert (tmp_path / "again.csv").read_bytes() == before
    # with camera poses: the three images become views of one static scene in which the planted objects stand still, so that the
    # estimates of object 1 from different images agree in the world up to a small error (each image's camera pose is chosen to make
    # them so, then turned by 0.3 degrees and moved by 3 mm)
    rows = eval_bop19.load_results_csv(base_csv)
    anchor = {}
    posed = {}
    for im in IM_IDS:
        mine = [r for r in rows if r["im_id"] == im and r["obj_id"] == 1]
        T = mv.mat(mine[0]["R"], mine[0]["t"])
        if not anchor:
            anchor["W"] = T                                        # object 1's pose in the first image's camera is the world pose
            T_w2c = np.eye(4)
        else:
            T_w2c = T @ np.linalg.inv(anchor["W"]) @ mv.mat(mv.lm_ref.rot_exp(rng.normal(size=3) * np.radians(0.3)), rng.normal(size=3) * 3.0)
        posed[str(im)] = dict(plain[str(im)], cam_R_w2c=T_w2c[:3, :3].reshape(9).tolist(), cam_t_w2c=T_w2c[:3, 3].tolist())
    d, csv, paths = _drive(tmp_path, "posed", driver_split, mopts, scene_cameras={1: posed}, scene_models=models)
    want, want_rep = multiview.fuse_results(rows, {1: posed}, models)
    assert any(r["fused"] for r in want_rep["rows"]) and len(want) == len(rows)
    pose_nms.write_results_csv(str(tmp_path / "want.csv"), want)
    assert _strip_time(csv) == _strip_time(str(tmp_path / "want.csv"))
    got_rep = json.load(open(os.path.join(d, "scene-fuse.json")))
    assert got_rep == json.loads(json.dumps(want_rep))
    assert eval_bop19.average_time_per_image(eval_bop19.load_results_csv(csv)) > 0       # the stage's share leaves one time per image
    assert json.load(open(os.path.join(d, "1", "estimated-poses.json"))) is not None and \
        [{k: v for k, v in e.items() if k != "time"} for e in json.load(open(os.path.join(d, "2", "estimated-poses.json")))] == \
        [{k: v for k, v in e.items() if k != "time"} for e in json.load(open(os.path.join(base_dir, "2", "estimated-poses.json")))]
    # with pose_nms as well: fusion sees the suppressed csv
    nopts = mopts._replace(frame_select_type="pose_nms", pose_nms_thresh=0.05)
    nms_dir, nms_csv, _ = _drive(tmp_path, "nms_only", driver_split, nopts._replace(scene_select_type="none"))
    d, csv, paths = _drive(tmp_path, "nms_fuse", driver_split, nopts, scene_cameras={1: posed}, scene_models=models)
    kept = eval_bop19.load_results_csv(nms_csv)
    want, want_rep = multiview.fuse_results(kept, {1: posed}, models)
    pose_nms.write_results_csv(str(tmp_path / "want2.csv"), want)
    assert _strip_time(csv) == _strip_time(str(tmp_path / "want2.csv"))
    assert [os.path.basename(p) for p in paths[-2:]] == ["pose-nms.json", "scene-fuse.json"]
    assert len(json.load(open(paths[-1]))["rows"]) == len(kept)
    # the models are required
    with pytest.raises(ValueError, match="needs the objects' models"):
        infer._fuse_scene_poses(mopts, {1: posed}, None, base_csv)
    with pytest.raises(ValueError, match="needs the objects' models"):
        infer._fuse_scene_poses(mopts, {1: posed}, {1: models[1]}, base_csv)
