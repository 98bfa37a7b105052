"""GPU: the depth proposals (csrc/depth_proposals.hip behind fp_depth_plane_fit, fp_depth_components, fp_component_table and
fp_component_runs) against the numpy restatement tests/depth_proposals_ref.py.  Everything that is an integer
-- label maps, hypothesis counts, winners, tables, rank maps, run lengths -- must be EQUAL; only the refitted plane has a tolerance, and
that one is measured from the restatement's own sensitivity to the order of summation (the rule of section 7).  What follows a plane is
tested on the kernel's own planes handed to the restatement, so the refit's last bits cannot flip a pixel between the two.

Measured on an MI355X (the figures the refit's tolerance is made of, and what the kernel used of it) are in DESIGN.md section 28."""

import json
import os

import numpy as np
import pytest
import torch

from foundpose_amd import _lib, depth_proposals as dp, detect, detect_util as du, infer_pose_util, ops, synthetic
from tests import depth_proposals_ref as ref

pytestmark = pytest.mark.gpu
CAM = ref.E2E_CAM


def _planes(n, planes=()):
    """The plane records of n frames that all have `planes`."""
    t = torch.zeros(n, 4, 4, dtype=torch.float64)
    for k, p in enumerate(planes):
        t[:, k] = torch.from_numpy(np.asarray(p, np.float64))
    return t.cuda(), torch.full((n,), len(planes), dtype=torch.int32, device="cuda")


def _labels(D, slope_fx, planes=(), margin=15.0, max_depth=0.0, cmm=ref.PATTERN_CMM):
    pl, cnt = _planes(len(D), planes)
    return ops.depth_components(torch.from_numpy(D).cuda(), [CAM] * len(D), slope_fx, pl, cnt, max_depth, margin, float(cmm))


@pytest.fixture(scope="module")
def patterns():
    """[(name, D, slope_fx, the restatement's label maps)]: computed once, shared, never changed."""
    return [(name, D, s, np.stack([ref.components(D[f], D[f] > 0, ref.PATTERN_CMM, s[f]) for f in range(len(D))]))
            for name, D, s in ref.pattern_batches()]


# ------------------------------------------------------------------------------------------------------------------------ 1. components
def test_label_maps_equal_the_restatement_at_shapes_that_stride(patterns):
    for name, D, s, want in patterns:
        got = _labels(D, s).cpu().numpy()
        assert np.array_equal(got, want), name
        for f in range(len(D)):   # a frame alone is its slice of the batch
            assert np.array_equal(_labels(D[f:f + 1], s[f:f + 1]).cpu().numpy()[0], got[f]), (name, f)


# ------------------------------------------------------------------------------------------------------------------------ 2. foreground
def test_foreground_is_exact_at_the_margin_and_at_max_depth():
    for D, planes, margin, max_depth, want in ref.foreground_frames():
        got = _labels(D[None], np.array([ref.PATTERN_SLOPE_FX]), planes, margin, max_depth).cpu().numpy()[0]
        assert np.array_equal(got >= 0, want)
        assert np.array_equal(ref.foreground(D, CAM, planes, margin, max_depth), want)


# ---------------------------------------------------------------------------------------------------------------------------- 3. planes
PLANE_CROP = (24, 32, 72, 96)   # y0, x0, H, W of the 96 x 72 window of the analytic scene
PLANE_CAM = (CAM[0], CAM[1], CAM[2] - 32, CAM[3] - 24)
PLANE_KEYS = [ref.E2E_KEY, (7 << 32) + 3, (1 << 63) + 5]


@pytest.fixture(scope="module")
def plane_case():
    y0, x0, H, W = PLANE_CROP
    full, sparse = ref.e2e_scene()[0], ref.sparse_scene()[0]
    few = np.zeros((H, W), np.float32)
    few[3, 5], few[40, 60] = 900.0, 950.0
    D = np.stack([full[y0:y0 + H, x0:x0 + W], sparse[y0:y0 + H, x0:x0 + W], few])
    o = ref.options()
    want = [ref.fit_plane(D[f], PLANE_CAM, PLANE_KEYS[f], 0, [], o) for f in range(3)]
    sens = [ref.refit_sensitivity(D[f], PLANE_CAM, PLANE_KEYS[f], 0, [], o) for f in range(2)]
    pl, cnt = _planes(3)
    got = ops.depth_plane_fit(torch.from_numpy(D).cuda(), [PLANE_CAM] * 3, PLANE_KEYS, pl, torch.zeros_like(cnt), want_counts=True)
    return D, o, want, sens, [t.cpu().numpy() for t in got]


def test_every_hypothesis_count_and_the_winner_equal_the_restatement(plane_case):
    D, o, want, _, (plane, info, counts) = plane_case
    assert (D[1] > 0).mean() < 0.45                                     # the second frame is 60 % holes: the sampler redraws
    for f in range(3):
        assert np.array_equal(counts[f], want[f]["counts"]), f        # dead hypotheses count 0 on both sides
        assert info[f, 0] == want[f]["winner"] and info[f, 1] == want[f]["subgrid_count"]
        assert info[f, 3] == want[f]["eligible"] and info[f, 4] == want[f]["valid"] and info[f, 6] == 0
    assert want[0]["counts"].max() > 100 and want[1]["counts"].max() > 40
    # fewer than three valid pixels: every hypothesis is dead, no plane, not accepted, no fault
    assert not counts[2].any() and info[2, 5] == 0 and info[2, 2] == 0 and not plane[2].any() and all(i is None for i in want[2]["ids"])


def test_the_refit_is_the_restatements_within_its_own_sensitivity(plane_case):
    D, o, want, sens, (plane, info, _) = plane_case
    for f in range(2):
        angle, offset = ref.plane_difference(plane[f], want[f]["plane"])
        tol_angle, tol_offset = max(1e-9, 1000 * sens[f][0]), max(1e-6, 1000 * sens[f][1])
        print(f"frame {f}: kernel vs restatement {angle:.3e} rad {offset:.3e} mm; summation order alone {sens[f][0]:.3e} rad {sens[f][1]:.3e} mm")
        assert angle <= tol_angle and offset <= tol_offset
        assert abs(np.linalg.norm(plane[f, :3]) - 1) < 1e-12 and plane[f, 3] > 0
        # support and acceptance are exact functions of the kernel's own plane
        el = ref.eligible_mask(D[f], PLANE_CAM, [], o["plane_thresh_mm"])
        support = int((el & (np.abs(ref.height(plane[f], ref.points(D[f], PLANE_CAM))) <= o["plane_thresh_mm"])).sum())
        assert info[f, 2] == support and info[f, 5] == 1 and want[f]["accepted"]


def test_a_frame_fits_the_same_plane_alone_and_in_a_batch(plane_case):
    D, o, want, _, (plane, info, counts) = plane_case
    for f in (1, 0):
        pl, cnt = _planes(1)
        p1, i1, c1 = ops.depth_plane_fit(torch.from_numpy(D[f:f + 1]).cuda(), [PLANE_CAM], PLANE_KEYS[f:f + 1], pl, torch.zeros_like(cnt), want_counts=True)
        assert p1.cpu().numpy().tobytes() == plane[f:f + 1].tobytes() and np.array_equal(i1.cpu().numpy(), info[f:f + 1])
        assert np.array_equal(c1.cpu().numpy(), counts[f:f + 1])


# ----------------------------------------------------------------------------------------------------------------- 5. tables, ranks, runs
def _check_levels(out, f, want, H, W, P):
    """segment()'s entries of frame f against the restatement's propose_frame."""
    L = len(want["levels"])
    runs, off = out["runs"].cpu().numpy(), out["run_off"].cpu().numpy()
    for lv, w in enumerate(want["levels"]):
        assert np.array_equal(out["labels"][f, lv].cpu().numpy(), w["labels"])
        kept = len(w["table"])
        assert tuple(out["counts"][f, lv].tolist()) == tuple(w["counts"])
        table = out["tables"][f, lv].cpu().numpy()
        assert np.array_equal(table[:kept], w["table"]) and np.all(table[kept:, 0] == -1) and not table[kept:, 1:].any()
        assert np.array_equal(out["rank_maps"][f, lv].cpu().numpy(), w["rank_map"])
        for r in range(P):
            g = (f * L + lv) * P + r
            counts = runs[off[g]:off[g + 1]].tolist()
            assert counts == (w["runs"][r] if r < kept else [])
            if r < kept:
                assert sum(counts) == H * W and (counts[0] == 0) == bool(w["rank_map"][0, 0] == r)


def test_tables_rank_maps_and_runs_equal_the_restatement_on_the_patterns(patterns):
    P = 64
    o = dp.DepthProposalOpts(num_planes=0, min_pixels=1, max_area_share=1.0, max_proposals=P, connect_mm=float(ref.PATTERN_CMM))
    for name, D, s, want_labels in patterns:
        n, H, W = D.shape
        lab = _labels(D, s)
        table, counts, rank_map = ops.component_table(lab, 1, H * W, P)
        runs, off = ops.component_runs(rank_map, counts[:, 2].contiguous(), P)
        out = {"labels": lab[:, None], "tables": table[:, None], "counts": counts[:, None], "rank_maps": rank_map[:, None], "runs": runs, "run_off": off}
        for f in range(n):
            rows, cnt, rk = ref.table(want_labels[f], 1, H * W, P)
            _check_levels(out, f, {"levels": [dict(labels=want_labels[f], table=rows, counts=cnt, rank_map=rk, runs=ref.runs(rk, len(rows)))]}, H, W, P)
        if name.startswith("borders"):   # the ring holds pixel (0, 0) and runs down the first column into the second: [0, H + 1, ...]
            first = runs[off[0]:off[1]].tolist()
            assert first[0] == 0 and first[1] == H + 1
        if name.startswith("dense"):     # the checkerboard: far more components than max_proposals, all of area 1, the lowest labels win
            assert counts[0].tolist() == [(H * W + 1) // 2, (H * W + 1) // 2, P, 0] and table[0, :, 0].tolist() == np.flatnonzero(D[0].reshape(-1) > 0)[:P].tolist()


@pytest.fixture(scope="module")
def e2e():
    """The analytic scene, the same with a wall, and the grooved one on three levels: the device's results and the restatement's on the
    device's planes."""
    D0, plane, visible = ref.e2e_scene()
    D1 = ref.e2e_scene(wall=True)[0]
    D2 = D0.copy()
    D2[60:62, 70:90] = D2[60:62, 70:90] + np.float32(40.0)
    cases = []
    for D, kw in ((D0, dict(min_pixels=12)), (D1, dict(min_pixels=12, num_planes=3)), (D2, dict(min_pixels=12, connect_mm=[2.0, 5.0, 60.0]))):
        opts = dp.load_opts(kw)
        out = dp.propose(torch.from_numpy(D[None]).cuda(), [CAM], [ref.E2E_KEY], opts)
        n_pl = int(out["num_planes"][0])
        planes = out["planes"][0, :n_pl].cpu().numpy()
        want = ref.propose_frame(D, CAM, ref.E2E_KEY, ref.options(**{k: (tuple(v) if isinstance(v, list) else v) for k, v in kw.items()}), planes=list(planes))
        cases.append((D, opts, out, want))
    return cases, plane, visible


def test_two_and_three_levels_drop_duplicates_and_nest(e2e):
    (D, opts, out, want), = [c for c in e2e[0] if len(c[1].levels()) == 3]
    _check_levels(out, 0, want, *D.shape, opts.max_proposals)
    lab = out["labels"][0].cpu().numpy()
    for a, b in ((lab[0], lab[1]), (lab[1], lab[2])):
        pairs = np.unique(np.stack([a[a >= 0], b[a >= 0]]), axis=1)
        assert np.array_equal(a >= 0, b >= 0) and len(np.unique(pairs[0])) == pairs.shape[1]
    assert int(out["counts"][0, :, 3].sum()) > 0
    rows = [tuple(r[:2]) for lv in range(3) for r in out["tables"][0, lv].cpu().numpy() if r[0] >= 0]
    assert len(rows) == len(set(rows))


# -------------------------------------------------------------------------------------------------------------------------- 6. end to end
def test_the_analytic_scene_gives_its_four_spheres_and_the_restatements_bits(e2e):
    cases, plane, visible = e2e
    for D, opts, out, want in cases[:2]:
        _check_levels(out, 0, want, *D.shape, opts.max_proposals)
        rk = out["rank_maps"][0, 0].cpu().numpy()
        assert int(out["counts"][0, 0, 2]) == 4
        for m in visible:
            assert max(ref.iou(rk == r, m) for r in range(4)) >= 0.95
    angle, offset = ref.plane_difference(cases[0][2]["planes"][0, 0].cpu().numpy(), plane)
    assert angle < np.deg2rad(0.01) and offset < 0.05
    rounds = cases[1][2]["plane_rounds"]
    assert [int(i[0, 5]) for _, i, _ in rounds] == [1, 1, 0] and int(cases[1][2]["num_planes"][0]) == 2
    shares = [int(i[0, 2]) / int(i[0, 4]) for _, i, _ in rounds]
    assert 0.7 < shares[0] < 0.8 and 0.2 < shares[1] < 0.3 and shares[2] < 0.05
    # a frame whose sequence has ended is skipped: a fourth round reports plane index -1 and writes zeros
    out4 = dp.propose(torch.from_numpy(cases[1][0][None]).cuda(), [CAM], [ref.E2E_KEY], dp.load_opts(dict(min_pixels=12, num_planes=4)))
    p4, i4, _ = out4["plane_rounds"][3]
    assert i4[0].tolist() == [-1, 0, 0, i4[0, 3].item(), i4[0, 4].item(), 0, -1, 0] and not p4.cpu().numpy().any()
    assert torch.equal(out4["rank_maps"], cases[1][2]["rank_maps"])


# ----------------------------------------------------------------------------------------------------------------------- 7. the tool chain
@pytest.fixture(scope="module")
def split(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("depth_split"))
    scene = synthetic.make_bop_eval_scene(root, num_images=3, num_objects=2, width=64, height=48, mesh_res=12)
    from PIL import Image
    rng = np.random.default_rng(5)
    os.makedirs(os.path.join(scene["split_dir"], "000001", "rgb"))
    for im, _ in scene["images"]:
        Image.fromarray(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)).save(os.path.join(scene["split_dir"], "000001", "rgb", f"{im:06d}.png"))
    opts_path = os.path.join(root, "depth_opts.json")
    with open(opts_path, "w") as f:
        json.dump({"depth_proposal_opts": {"min_pixels": 10, "max_area_share": 0.95}}, f)
    return root, scene, opts_path


def test_the_command_line_writes_proposals_that_decode_to_the_rank_maps(split, tmp_path):
    root, scene, opts_path = split
    out_path, report_path = str(tmp_path / "p" / "proposals.json"), str(tmp_path / "report.json")
    dp.main(["--dataset-dir", scene["split_dir"], "--output", out_path, "--opts", opts_path, "--report", report_path])
    records = json.load(open(out_path))
    assert len(records) > 0 and set(records[0]) == {"scene_id", "image_id", "segmentation", "bbox", "score", "time"}
    report = json.load(open(report_path))
    assert [(f["scene_id"], f["image_id"]) for f in report["frames"]] == [(1, im) for im, _ in scene["images"]]
    assert sum(f["levels"][0]["kept"] for f in report["frames"]) == len(records) and all(len(f["planes"]) == 1 for f in report["frames"])
    opts = dp.load_opts(opts_path)
    for im, _ in scene["images"]:
        mine = [r for r in records if r["image_id"] == im]
        D = dp.load_depth(os.path.join(scene["split_dir"], "000001", "depth", f"{im:06d}.png"), 0.1)
        K = scene["K"]
        out = dp.propose(torch.from_numpy(D[None]).cuda(), [(K[0, 0], K[1, 1], K[0, 2], K[1, 2])], [dp.frame_key(1, im)], opts)
        rk = out["rank_maps"][0, 0].cpu().numpy()
        assert len(mine) == int(out["counts"][0, 0, 2])          # a frame gives the same alone as in the split's batch
        if not mine:
            continue
        counts, run_off, size = infer_pose_util.pack_rle(mine)   # what the decoder of section 19 takes
        assert size == (48, 64) and run_off[-1] == len(counts)
        for r, rec in enumerate(mine):
            m = infer_pose_util.rle_to_binary_mask(rec["segmentation"])
            assert np.array_equal(m, rk == r)
            ys, xs = np.nonzero(m)
            assert rec["bbox"] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1] and rec["score"] == m.sum() / (48 * 64)


def _strip_time(records):
    return json.dumps([{k: v for k, v in r.items() if k != "time"} for r in records])


def test_detect_run_takes_its_proposals_from_depth_or_from_a_file_and_never_both(split, tmp_path):
    from tests.test_gpu_detect import World
    root, scene, opts_path = split
    world = World(str(tmp_path / "world"))
    (tmp_path / "detect.json").write_text(json.dumps({"detect_opts": dict(world.opts._asdict(), detector_min_score=-1.0)}))
    common = ["--opts", str(tmp_path / "detect.json"), "--output-path", world.root, "--precision", "fp32", "--weights", world.weights]
    detect.main(["onboard"] + common)
    tail = ["--dataset-dir", scene["split_dir"]]
    prop_path = str(tmp_path / "proposals.json")
    dp.main(["--dataset-dir", scene["split_dir"], "--output", prop_path, "--opts", opts_path])
    detect.main(["run"] + common + tail + ["--proposals-from-depth", opts_path, "--output", str(tmp_path / "a" / "detections.json")])
    detect.main(["run"] + common + tail + ["--proposals", prop_path, "--output", str(tmp_path / "b" / "detections.json")])
    a, b = (json.load(open(tmp_path / d / "detections.json")) for d in "ab")
    assert len(a) > 0 and _strip_time(a) == _strip_time(b)
    assert open(tmp_path / "a" / "detector-decisions.json").read() == open(tmp_path / "b" / "detector-decisions.json").read()
    # --proposals with a hand-written file: what the unchanged run() and label_proposals give
    m = np.zeros((48, 64), np.uint8)
    m[10:30, 8:40] = 1
    hand = [{"scene_id": 1, "image_id": scene["images"][0][0], "time": 0.5, "segmentation": infer_pose_util.binary_mask_to_rle(m)}]
    (tmp_path / "hand.json").write_text(json.dumps(hand))
    detect.main(["run"] + common + tail + ["--proposals", str(tmp_path / "hand.json"), "--output", str(tmp_path / "c" / "detections.json")])
    opts = du.load_opts(str(tmp_path / "detect.json"))
    image = detect._load_frame_image(scene["split_dir"], 1, hand[0]["image_id"])
    memory = du.detections_to_list(du.label_proposals(opts, image, hand, world.banks, world.ex)[0])
    assert _strip_time(json.load(open(tmp_path / "c" / "detections.json"))) == _strip_time(memory) and len(memory) == 1
    for flags in ([], ["--proposals", prop_path, "--proposals-from-depth"]):
        with pytest.raises(SystemExit):
            detect.main(["run"] + common + tail + flags + ["--output", str(tmp_path / "d" / "detections.json")])
    assert not os.path.exists(tmp_path / "d")


# --------------------------------------------------------------------------------------------------------------------------- 8. refusals
SENTINEL = 0x5a


def _filled(nbytes):
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")


def _untouched(*ts):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in ts)


def test_every_refusal_comes_from_its_argument_and_writes_nothing():
    N, H, W, HYP, P = 2, 40, 48, 16, 8
    L, vp = _lib.lib(), _lib.vp
    depth = torch.full((N, H, W), 1000.0, device="cuda")
    cams = np.array([CAM] * N, np.float64)
    keys = np.arange(N, dtype=np.uint64)
    slope = np.full(N, 0.03, np.float32)
    planes, nplanes = _planes(N)
    host = lambda a: a.ctypes.data_as(vp)
    ptr, stream = _lib.ptr, _lib.stream

    def plane_fit(**kw):
        a = dict(depth=ptr(depth), n=N, h=H, w=W, cams=host(cams), keys=host(keys), prior=ptr(planes), nprior=ptr(nplanes), hyp=HYP, stride=4, thresh=10.0,
                 maxd=0.0, share=0.05, seed=0, scratch_bytes=_lib.depth_plane_scratch_bytes(N, H * W, HYP), outs=3)
        a.update(kw)
        scratch = _filled(_lib.depth_plane_scratch_bytes(N, H * W, HYP))
        outs = [_filled(N * 32), _filled(N * 32), _filled(N * HYP * 4)]
        o = [ptr(t) if i < a["outs"] else None for i, t in enumerate(outs)]
        rc = L.fp_depth_plane_fit(a["depth"], a["n"], a["h"], a["w"], a["cams"], a["keys"], a["prior"], a["nprior"], a["hyp"], a["stride"], a["thresh"],
                                  a["maxd"], a["share"], a["seed"], ptr(scratch), a["scratch_bytes"], o[0], o[1], o[2], stream())
        return rc, _untouched(scratch, *outs)

    bad_cam, nan_cam = cams.copy(), cams.copy()
    bad_cam[1, 0], nan_cam[0, 2] = 0.0, np.nan
    for kw in (dict(depth=None), dict(cams=None), dict(keys=None), dict(prior=None), dict(nprior=None), dict(outs=0), dict(outs=1), dict(n=0),
               dict(n=4097), dict(h=0), dict(w=0), dict(h=65536, w=65536), dict(hyp=0), dict(hyp=4097), dict(stride=0), dict(stride=65),
               dict(thresh=0.0), dict(thresh=float("nan")), dict(maxd=-1.0), dict(share=1.5), dict(share=float("nan")), dict(cams=host(bad_cam)),
               dict(cams=host(nan_cam)), dict(scratch_bytes=_lib.depth_plane_scratch_bytes(N, H * W, HYP) - 1)):
        assert plane_fit(**kw) == (1, True), kw
    assert plane_fit(outs=2)[0] == 0 and plane_fit()[0] == 0          # hyp_counts may be NULL; the good call passes

    def components(**kw):
        a = dict(depth=ptr(depth), n=N, h=H, w=W, cams=host(cams), slope=host(slope), planes=ptr(planes), nplanes=ptr(nplanes), maxd=0.0, margin=15.0,
                 cmm=5.0, scratch_bytes=_lib.depth_components_scratch_bytes(N, H * W), out=True)
        a.update(kw)
        scratch, labels = _filled(_lib.depth_components_scratch_bytes(N, H * W)), _filled(N * H * W * 4)
        rc = L.fp_depth_components(a["depth"], a["n"], a["h"], a["w"], a["cams"], a["slope"], a["planes"], a["nplanes"], a["maxd"], a["margin"], a["cmm"],
                                   ptr(scratch), a["scratch_bytes"], ptr(labels) if a["out"] else None, stream())
        return rc, _untouched(scratch, labels)

    bad_slope = slope.copy()
    bad_slope[1] = -1.0
    for kw in (dict(depth=None), dict(cams=None), dict(slope=None), dict(planes=None), dict(nplanes=None), dict(out=False), dict(n=0), dict(h=0),
               dict(w=-1), dict(maxd=float("inf")), dict(margin=float("nan")), dict(cmm=-1.0), dict(cmm=float("inf")), dict(slope=host(bad_slope)),
               dict(cams=host(bad_cam)), dict(scratch_bytes=_lib.depth_components_scratch_bytes(N, H * W) - 1)):
        assert components(**kw) == (1, True), kw
    assert components()[0] == 0

    labels = _labels(depth.cpu().numpy(), slope)

    def table(**kw):
        a = dict(labels=ptr(labels), n=N, h=H, w=W, minp=1, maxa=H * W, p=P, level=0, finer=None, nf=0,
                 scratch_bytes=_lib.component_table_scratch_bytes(N, H * W), outs=3)
        a.update(kw)
        scratch = _filled(_lib.component_table_scratch_bytes(N, H * W))
        outs = [_filled(N * P * 28), _filled(N * 16), _filled(N * H * W * 4)]
        o = [ptr(t) if i < a["outs"] else None for i, t in enumerate(outs)]
        rc = L.fp_component_table(a["labels"], a["n"], a["h"], a["w"], a["minp"], a["maxa"], a["p"], a["level"], a["finer"], a["nf"], ptr(scratch),
                                  a["scratch_bytes"], o[0], o[1], o[2], stream())
        return rc, _untouched(scratch, *outs)

    for kw in (dict(labels=None), dict(outs=0), dict(outs=1), dict(outs=2), dict(n=0), dict(h=0), dict(w=0), dict(minp=0), dict(maxa=0), dict(p=0),
               dict(p=1025), dict(level=3), dict(level=-1), dict(nf=3), dict(nf=1), dict(finer=ptr(labels)),
               dict(scratch_bytes=_lib.component_table_scratch_bytes(N, H * W) - 1)):
        assert table(**kw) == (1, True), kw
    assert table()[0] == 0

    rank_map = torch.zeros(N, H, W, dtype=torch.int32, device="cuda")
    kept = torch.ones(N, dtype=torch.int32, device="cuda")

    def run_events(**kw):
        a = dict(maps=ptr(rank_map), m=N, h=H, w=W, kept=ptr(kept), p=P, cap=16, events=True, count=True)
        a.update(kw)
        events, count = _filled(16 * 8), _filled(4)
        rc = L.fp_component_runs(a["maps"], a["m"], a["h"], a["w"], a["kept"], a["p"], a["cap"], ptr(events) if a["events"] else None,
                                 ptr(count) if a["count"] else None, stream())
        return rc, _untouched(events, count)

    for kw in (dict(maps=None), dict(kept=None), dict(count=False), dict(events=False), dict(m=0), dict(h=0), dict(w=0), dict(p=0), dict(p=1025),
               dict(cap=-1), dict(h=32768, w=32768), dict(m=65536, h=1, w=1)):
        assert run_events(**kw) == (1, True), kw
    assert run_events()[0] == 0 and run_events(cap=0, events=False)[0] == 0
    # the wrappers turn FP_ERR_INVALID into ValueError
    with pytest.raises(ValueError, match="max_proposals"):
        ops.component_table(labels, 1, H * W, 0)
    with pytest.raises(ValueError, match="device"):
        ops.depth_components(depth.cpu(), cams, slope, planes, nplanes)
