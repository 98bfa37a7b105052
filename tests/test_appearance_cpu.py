"""The yardstick of the appearance score (tests/appearance_ref.py) checked on the host: the restated patch coverage against a brute-force
loop over pixel centres and against the true pixel count at scale 1, the fp32 replay on hand-made similarity matrices (ties, NaN, the
statuses); and the declarations the stage adds (header, binding, options, refusals of CPU tensors, _select's old call).  No GPU."""
import os
import re
import time
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import appearance_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, PS = 28, 14
SHAPES = [(9, 50), (50, 9), (1, 1), (28, 28), (200, 131)]   # (h, w) of the box


def _brute_force_cover(mask, box, size, ps):
    """Every crop pixel of the window looks at the source pixel under its centre, in exact rational arithmetic."""
    x1, y1, x2, y2 = box
    w, h = x2 - x1, y2 - y1
    L = max(w, h)
    wo, ho = max(1, int(Fraction(w * size, L) + Fraction(1, 2))), max(1, int(Fraction(h * size, L) + Fraction(1, 2)))   # rounded half up
    ox, oy = (size - wo) // 2, (size - ho) // 2
    g = size // ps
    out = np.zeros((g, g), np.int32)
    for Y in range(size):
        for X in range(size):
            if not (ox <= X < ox + wo and oy <= Y < oy + ho):
                continue
            u, v = (Fraction(X - ox) + Fraction(1, 2)) * Fraction(w, wo), (Fraction(Y - oy) + Fraction(1, 2)) * Fraction(h, ho)
            sx, sy = x1 + int(u), y1 + int(v)
            assert x1 <= sx < x2 and y1 <= sy < y2
            out[Y // ps, X // ps] += int(mask[sy, sx] != 0)
    return out.reshape(-1)


@pytest.mark.parametrize("h,w", SHAPES)
def test_restated_coverage_is_the_brute_force_loop(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    mask = (rng.random((h + 5, w + 7)) < 0.6).astype(np.uint8) * 255
    box = (3, 2, 3 + w, 2 + h)
    got = ar.patch_cover(mask, box, S, PS)
    assert got.dtype == np.int32 and got.shape == (4,)
    assert got.tolist() == _brute_force_cover(mask, box, S, PS).tolist()
    wo, ho, ox, oy = ar.crop_window(box, S)
    assert max(wo, ho) == S and 0 <= got.min() and got.max() <= PS * PS and got.sum() <= wo * ho
    full = ar.patch_cover(np.ones_like(mask), box, S, PS)
    assert full.sum() == wo * ho                      # a full mask covers exactly the window


def test_at_scale_one_coverage_is_the_pixel_count():
    rng = np.random.default_rng(5)
    mask = (rng.random((40, 45)) < 0.5).astype(np.uint8)
    box = (6, 4, 6 + 28, 4 + 28)
    assert ar.crop_window(box, S) == (28, 28, 0, 0)
    got = ar.patch_cover(mask, box, S, PS).reshape(2, 2)
    for cy in range(2):
        for cx in range(2):
            assert got[cy, cx] == mask[4 + 14 * cy:4 + 14 * cy + 14, 6 + 14 * cx:6 + 14 * cx + 14].sum()


def test_refused_boxes_cover_nothing():
    mask = np.ones((6, 8), np.uint8)
    for box in ((0, 0, 0, 0), (2, 2, 2, 5), (-1, 0, 3, 3), (0, 0, 9, 3), (0, 0, 3, 7)):
        assert not ar.patch_cover(mask, box, S, PS).any()
    assert not ar.patch_cover(mask, (0, 0, 4, 4), S, PS, image_index=1, n_img=1).any()
    assert not ar.patch_cover(mask, (0, 0, 4, 4), S, PS, image_index=-1, n_img=1).any()
    assert ar.patch_cover(mask, (0, 0, 4, 4), S, PS).sum() == S * S


def test_replay_ties_nan_and_validity():
    f = np.float32
    sim = np.array([[[0.5, 0.9, 0.9, 0.2],          # a tie: the lower column
                     [np.nan, 0.1, 0.3, 0.99],      # a NaN never wins; column 3 is invalid
                     [0.7, 0.7, 0.7, 0.7],          # an invalid query patch
                     [np.nan, -0.5, -0.25, 1.0]]], np.float64)
    q_cover = np.array([[5, 5, 4, 9]], np.int32)
    bank_cover = np.array([[5, 5, 7, 4]], np.int32)
    bs, bp, app, nv, st, score = ar.replay(sim, q_cover, bank_cover, [0], np.array([0.5], f), 5)
    assert bp.tolist() == [[1, 2, -1, 2]] and bs.tolist() == [[f(0.9), f(0.3), 0.0, f(-0.25)]]
    assert nv.tolist() == [3] and st.tolist() == [0]
    want = f(f(f(f(0.9) + f(0.3)) + f(-0.25)) / f(3))
    assert app[0] == want and score[0] == f((f(0.5) + want) * f(0.5))
    # the same from the best similarities alone
    app2, nv2, st2, score2 = ar.replay_from_best(bs, q_cover, bank_cover, [0], np.array([0.5], f), 5)
    assert app2.tobytes() == app.tobytes() and score2.tobytes() == score.tobytes() and nv2.tolist() == [3] and st2.tolist() == [0]
    # all valid columns NaN: nothing wins
    bs, bp, app, nv, st, _ = ar.replay(np.full((1, 1, 1), np.nan), np.array([[1]], np.int32), np.array([[1]], np.int32), [0], np.zeros(1, f), 1)
    assert bp.tolist() == [[-1]] and bs[0, 0] == -np.inf and st.tolist() == [0]


def test_replay_statuses():
    f = np.float32
    sim = np.full((4, 2, 2), 0.5)
    q_cover = np.array([[0, 0], [3, 0], [3, 3], [3, 3]], np.int32)
    bank_cover = np.array([[3, 3], [0, 2]], np.int32)
    rows = ar.template_rows([0, 1, 2], 2, [0, 0, 1, 2], [0, 0, 0, 0])
    assert rows == [0, 0, 1, -1]
    bs, bp, app, nv, st, score = ar.replay(sim, q_cover, bank_cover, rows, np.array([0.25, 0.25, -np.inf, 0.25], f), 3)
    assert st.tolist() == [1, 0, 3, 2] and nv.tolist() == [0, 1, 2, 0] and app.tolist() == [0.0, 0.5, 0.0, 0.0]
    assert bp.tolist() == [[-1, -1], [0, -1], [-1, -1], [-1, -1]] and bs.tolist() == [[0, 0], [0.5, 0], [0, 0], [0, 0]]
    assert score.tolist() == [0.125, 0.375, -np.inf, 0.125]
    # rows: offsets clamped into the bank and made non-decreasing, ids outside their object refused
    assert ar.template_rows([-3, 9, 1, 2], 4, [0, 0, 1, 2, -1, 3, 0], [0, 3, 0, 0, 0, 0, 4]) == [0, 3, -1, -1, -1, -1, -1]


def test_header_and_binding_declare_the_entries():
    from foundpose_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    assert int(re.search(r"#define\s+FP_ABI_VERSION\s+(\d+)", header).group(1)) == 20 == _lib.ABI_VERSION
    api = open(os.path.join(ROOT, "foundpose_amd", "csrc", "api.cpp")).read()
    kinds = {"int": _lib.i32, "float": _lib.f32}
    for name, n_args in (("fp_proposal_patch_cover", 11), ("fp_proposal_appearance", 21)):
        m = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert m, f"{name} is not declared in the header"
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        proto = _lib._PROTOS[name]
        assert len(args) == len(proto) == n_args, name
        for a, ty in zip(args, proto):
            want = _lib.vp if ("*" in a or a.startswith("fp_stream_t")) else kinds[a.split()[0]]
            assert ty is want, (name, a)
        assert f"int {name}(" in api and name in _lib.exported_symbols()
    assert "proposals.hip" in build.SOURCES
    flat = re.sub(r"\s*\n \* ", " ", header)
    section = flat.split("The appearance score of a proposal", 1)[1].split("int fp_proposal_appearance(", 1)[0]
    assert len(re.findall(r"the same bits alone, in any batch and at any position", section)) == 2
    assert header.index("int fp_box_iou(") < header.index("int fp_proposal_patch_cover(") < header.index("COCO average precision of a detections file")


def test_options_defaults_and_refusals():
    from foundpose_amd import detect_util as du
    o = du.load_opts({"detect_opts": {"version": "v", "templates_version": "t", "object_dataset": "d", "object_lids": [1]}})
    assert (o.detector_score_type, o.detector_patch_min_cover) == ("semantic", 0.5)
    assert du.DetectOpts._fields[-2:] == ("detector_score_type", "detector_patch_min_cover")   # new fields at the end
    assert du.load_opts({"detector_score_type": "semantic_appearance", "detector_patch_min_cover": 1}).detector_score_type == "semantic_appearance"
    for bad in ({"detector_score_type": "appearance"}, {"detector_score_type": None}, {"detector_patch_min_cover": 0.0},
                {"detector_patch_min_cover": 1.5}, {"detector_patch_min_cover": float("nan")}, {"detector_patch_min_cover": True},
                {"detector_patch_min_cover": "0.5"}):
        with pytest.raises(ValueError):
            du.load_opts(bad)
    assert [du.min_cover_pixels(c, 14) for c in (0.5, 1.0, 0.001, 0.501)] == [98, 196, 1, 99]
    assert du.BankSet._fields[-2:] == ("patch_descs", "patch_cover") and du.BankSet([1], None, None, [], 1, 224).patch_descs is None


def test_cpu_tensors_are_refused():
    from foundpose_amd import detect_util as du, ops
    i32 = torch.int32
    with pytest.raises(ValueError, match="no CPU path"):
        ops.proposal_patch_cover(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, dtype=i32), 28, 14)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.proposal_appearance(torch.zeros(1, 4, 8), torch.zeros(1, 4, dtype=i32), torch.zeros(2, 4, 8), torch.zeros(2, 4, dtype=i32),
                                torch.tensor([0, 2], dtype=i32), torch.zeros(1, dtype=i32), torch.zeros(1, dtype=i32), torch.zeros(1), 1)
    with pytest.raises(ValueError, match="no CPU path"):
        du.patch_descriptors(None, torch.zeros(1, 3, 28, 28), 4)
    with pytest.raises(ValueError, match="no CPU path"):
        du.build_detector_bank(None, torch.zeros(1, 3, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8), 28, with_patches=True)


def test_select_keeps_its_old_call_and_names_the_parts_in_the_new_mode():
    from foundpose_amd import detect_util as du
    n = 3
    code, order = np.zeros(n, np.int32), np.array([0, 1, 2], np.int32)
    keep, by = np.ones(n, np.int32), np.full(n, -1, np.int32)
    obj, tpl, area = np.array([0, 0, 1], np.int32), np.array([1, 0, 2], np.int32), np.full(n, 9, np.int32)
    boxes = np.array([[0, 0, 3, 3], [10, 10, 13, 13], [20, 20, 23, 23]], np.int32)
    score = np.array([0.9, 0.5, 0.7], np.float32)
    opts = du.DetectOpts()
    bs = du.BankSet([7, 9], None, None, [np.array([10, 20, 30]), np.array([11, 21, 31])], 3, 224)
    proposals = [{"scene_id": 2, "image_id": 5, "time": 1.0, "segmentation": {"counts": [i], "size": [1, 1]}} for i in range(n)]
    dets, decs = du._select(opts, proposals, bs, code, order, keep, by, obj, tpl, area, boxes, score, time.perf_counter())   # 13 positional
    assert [d["decision"] for d in decs] == ["kept"] * 3 and all("appearance_score" not in d and "semantic_score" not in d for d in decs)
    assert set(decs[0]) == {"proposal", "decision", "category_id", "score", "template_id", "area", "bbox", "suppressed_by"}
    dets2, decs2 = du._select(opts, proposals, bs, code, order, keep, by, obj, tpl, area, boxes, score, time.perf_counter(),
                              semantic=np.array([0.8, -np.inf, 0.6], np.float32), appearance=np.array([1.0, 0.0, 0.8], np.float32),
                              valid_patches=np.array([4, 0, 3], np.int32), appearance_status=np.array([0, 1, 0], np.int32))
    assert [(d["semantic_score"], d["appearance_score"], d["valid_patches"]) for d in decs2] == \
        [(float(np.float32(0.8)), 1.0, 4), (None, None, 0), (float(np.float32(0.6)), float(np.float32(0.8)), 3)]
    assert [{k: v for k, v in d.items() if k not in ("semantic_score", "appearance_score", "valid_patches")} for d in decs2] == decs
    assert sorted(dets2) == sorted(dets)
