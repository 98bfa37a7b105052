"""The yardstick of the proposal-labelling stage (tests/proposal_ref.py) checked on the host: the restated crop against CPU torch's
antialiased bilinear interpolation, the restated suppression against a brute-force loop, the selection rules on a hand-made case; and the
declarations the stage adds (header, binding, build list, options).  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import proposal_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 28
# (h, w) of the box: wide, tall, tiny, one pixel, odd, scale > 7, identity
SHAPES = [(9, 50), (50, 9), (3, 2), (1, 1), (37, 53), (200, 131), (28, 28)]


def _torch_crop(image, mask, box, size):
    """Crop the masked image, F.interpolate(bilinear, antialias) to the window, zero-pad: the semantics the contract restates."""
    x1, y1, x2, y2 = box
    wo, ho, ox, oy = pr.crop_window(box, size)
    src = torch.from_numpy((image[y1:y2, x1:x2] * (mask[y1:y2, x1:x2, None] != 0)).astype(np.float32)).permute(2, 0, 1)[None]
    win = torch.nn.functional.interpolate(src, size=(ho, wo), mode="bilinear", antialias=True, align_corners=False)[0]
    out = torch.zeros(3, size, size)
    out[:, oy:oy + ho, ox:ox + wo] = win
    return out.numpy().astype(np.float64)


@pytest.mark.parametrize("h,w", SHAPES)
def test_restated_crop_is_torch_antialiased_bilinear(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    H, W = h + 5, w + 7
    image = rng.random((H, W, 3)).astype(np.float32)
    mask = (rng.random((H, W)) < 0.8).astype(np.uint8)
    box = (3, 2, 3 + w, 2 + h)
    mask[box[1], box[0]:box[2]] = 1
    ref, status = pr.proposal_crop(image, mask, box, S)
    assert status == 0
    wo, ho, ox, oy = pr.crop_window(box, S)
    assert max(wo, ho) == S and (wo == S if w >= h else ho == S)
    err = float(np.abs(ref - _torch_crop(image, mask, box, S)).max())
    print(f"box {h} x {w} -> window {ho} x {wo}: max |restated - torch| = {err:.3g}")
    assert err <= 2e-6   # torch's own fp32 rounding of weights and sums
    outside = np.ones((S, S), bool)
    outside[oy:oy + ho, ox:ox + wo] = False
    assert not ref[:, outside].any()


def test_crop_window_rounds_half_up_and_never_vanishes():
    assert pr.crop_window((0, 0, 50, 9), S)[:2] == (28, 5)          # 9 * 28 / 50 = 5.04
    assert pr.crop_window((0, 0, 2, 3), S)[:2] == (19, 28)          # 2 * 28 / 3 = 18.67
    assert pr.crop_window((0, 0, 1, 100), S)[:2] == (1, 28)         # 0.28 -> at least one column
    assert pr.crop_window((0, 0, 4, 8), 7)[:2] == (4, 7)            # 3.5 rounds up
    assert pr.crop_window((0, 0, 50, 9), S)[2:] == (0, 11)          # centred: (28 - 5) // 2
    for n_in, n_out in ((200, 28), (9, 5), (2, 19), (1, 1), (28, 28)):
        sup = max(n_in / n_out, 1.0)
        assert pr.max_taps(n_in, n_out) <= 2 * sup + 1
        assert all(abs(wt.sum() - 1.0) < 1e-12 and (wt >= 0).all() for _, wt in pr.axis_weights(n_in, n_out))


def test_refused_boxes_give_status_2_and_zeros():
    image, mask = np.ones((6, 8, 3)), np.ones((6, 8), np.uint8)
    for box in ((0, 0, 0, 0), (2, 2, 2, 5), (-1, 0, 3, 3), (0, 0, 9, 3), (0, 0, 3, 7)):
        crop, status = pr.proposal_crop(image, mask, box, 4)
        assert status == 2 and not crop.any()


def _brute_force_nms(boxes, scores, thresh):
    """The textbook loop on one class: take the best remaining box, drop everything that overlaps it by >= thresh."""
    def iou(a, b):
        ix = max(min(a[2], b[2]) - max(a[0], b[0]), 0)
        iy = max(min(a[3], b[3]) - max(a[1], b[1]), 0)
        u = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - ix * iy
        return ix * iy / u if u > 0 else 0.0
    left = sorted(range(len(boxes)), key=lambda i: (-scores[i], i))
    kept = []
    while left:
        best = left.pop(0)
        kept.append(best)
        left = [i for i in left if not iou(boxes[best], boxes[i]) >= thresh]
    return kept


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restated_suppression_is_the_brute_force_loop(seed):
    rng = np.random.default_rng(seed)
    n, num_obj = 40, 3
    xy = rng.integers(0, 30, (n, 2))
    wh = rng.integers(1, 25, (n, 2))
    boxes = np.concatenate([xy, xy + wh], 1)
    boxes[5] = boxes[4]                                  # identical boxes
    scores = rng.random(n).astype(np.float32)
    scores[7] = scores[6]                                # equal scores: input order decides
    obj = rng.integers(0, num_obj, n)
    names, by, kept = pr.select(obj, scores, np.full(n, 10), np.zeros(n, int), boxes, num_obj, 0, 0.0, 0.25, n)
    want = []
    for o in range(num_obj):
        idx = [i for i in range(n) if obj[i] == o]
        want += [idx[j] for j in _brute_force_nms(boxes[idx], scores[idx], 0.25)]
    assert sorted(kept) == sorted(want)
    assert kept == sorted(kept, key=lambda p: (-scores[p], p))
    for p in range(n):
        assert names[p] == ("kept" if p in want else "suppressed")
        if names[p] == "suppressed":
            q = by[p]
            assert names[q] == "kept" and obj[q] == obj[p] and (scores[q], -q) > (scores[p], -p)
            assert pr.box_iou(boxes, [(q, p)])[0][0] >= 0.25


def test_selection_names_every_reason():
    #            0 kept  1 twin   2 small  3 empty  4 none  5 low    6 other object  7 over the per-image cut
    best_obj = [0,      0,       0,       0,       -1,     0,       1,              1]
    score = np.array([0.9, 0.8, 0.95, 0.99, -np.inf, 0.1, 0.7, 0.6], np.float32)
    area = [50, 50, 3, 0, 50, 50, 50, 50]
    status = [0, 0, 0, 2, 0, 0, 0, 0]
    boxes = [(0, 0, 10, 10), (0, 0, 10, 10), (0, 0, 2, 2), (0, 0, 0, 0), (0, 0, 9, 9), (0, 0, 9, 9), (0, 0, 10, 10), (20, 20, 30, 30)]
    names, by, kept = pr.select(best_obj, score, area, status, boxes, 2, 4, 0.2, 0.25, 2)
    assert names == ["kept", "suppressed", "small", "small", "no_object", "low_score", "kept", "max_per_image"]
    assert by[1] == 0 and kept == [0, 6]
    names, _, _ = pr.select(best_obj, score, area, status, boxes, 2, 0, 0.2, 0.25, 8)
    assert names[2] == "kept" and names[3] == "empty" and names[7] == "kept"
    # the group limit: rank >= max_group never reaches the suppression
    names, _, _ = pr.select([0] * 5, np.arange(5, 0, -1, dtype=np.float32), [9] * 5, [0] * 5,
                            [(10 * i, 0, 10 * i + 5, 5) for i in range(5)], 1, 0, 0.0, 0.25, 5, max_group=3)
    assert names == ["kept", "kept", "kept", "group_limit", "group_limit"]


def test_overlap_is_one_division_of_two_integers():
    boxes = [(0, 0, 4, 4), (0, 0, 4, 4), (1, 1, 3, 3), (4, 0, 8, 4), (0, 0, 0, 5), (0, 0, 5, 2), (0, 1, 5, 3)]
    ov, st = pr.box_iou(boxes, [(0, 1), (0, 2), (0, 3), (4, 4), (5, 6), (0, 9), (4, 0)])
    assert ov.tolist() == [1.0, 0.25, 0.0, 0.0, 5 / 15, 0.0, 0.0]
    assert st.tolist() == [0, 0, 0, 2, 0, 2, 0]


def test_scores_follow_the_stated_fp32_order():
    sims = np.array([[0.5, 0.25, 0.5, 0.1, 0.9, 0.9]], np.float32)
    scores, bo, bs, bt = pr.proposal_scores(sims, [0, 4, 4, 6], 2)
    assert scores.tolist() == [[0.5, -np.inf, np.float32(0.9)]] and bo[0] == 2 and bt[0] == 0
    scores, bo, bs, bt = pr.proposal_scores(sims, [0, 4, 4, 6], 3)
    assert scores[0, 0] == np.float32(np.float32(np.float32(0.5) + np.float32(0.5)) + np.float32(0.25)) / np.float32(3)
    assert scores[0, 2] == np.float32(0.9)   # T = 2 < k: m = 2
    _, bo, _, bt = pr.proposal_scores(np.array([[0.3, 0.3]], np.float32), [0, 1, 2], 1)
    assert bo[0] == 0 and bt[0] == 0         # equal scores: the lower object
    _, bo, bs, bt = pr.proposal_scores(np.zeros((1, 0), np.float32), [0, 0], 1)
    assert (bo[0], bs[0], bt[0]) == (-1, -np.inf, -1)


def test_header_binding_and_build_declare_the_entries():
    from foundpose_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    assert int(re.search(r"#define\s+FP_ABI_VERSION\s+(\d+)", header).group(1)) == 20 == _lib.ABI_VERSION
    api = open(os.path.join(ROOT, "foundpose_amd", "csrc", "api.cpp")).read()
    kinds = {"int": _lib.i32, "float": _lib.f32, "size_t": __import__("ctypes").c_size_t}
    for name, n_args in (("fp_mask_boxes", 7), ("fp_proposal_crops", 12), ("fp_proposal_scores", 16), ("fp_proposal_rank", 18), ("fp_box_iou", 7)):
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
    flat = re.sub(r"\s*\n \* ", " ", header)   # comment lines joined
    section = flat.split("Labelling of class-agnostic mask proposals", 1)[1].split("int fp_box_iou(", 1)[0]
    assert len(re.findall(r"the same bits alone, in any batch and at any position", section)) == 4   # boxes, crops, scores, overlaps
    assert int(re.search(r"#define\s+FP_PROPOSAL_MAX_SIZE\s+(\d+)", header).group(1)) == _lib.PROPOSAL_MAX_SIZE
    assert int(re.search(r"#define\s+FP_PROPOSAL_MAX_K\s+(\d+)", header).group(1)) == _lib.PROPOSAL_MAX_K
    assert int(re.search(r"#define\s+FP_PROPOSAL_MAX_RANKED\s+(\d+)", header).group(1)) == _lib.PROPOSAL_MAX_RANKED
    for i, name in enumerate(_lib.PROPOSAL_DECISIONS):
        assert int(re.search(r"#define\s+FP_PROPOSAL_%s\s+(\d+)" % name.upper(), header).group(1)) == i
    assert tuple(_lib.PROPOSAL_DECISIONS) == pr.DECISIONS


def test_scratch_size_matches_the_header_macro():
    from foundpose_amd import _lib
    up16 = lambda b: (b + 15) // 16 * 16
    for P, O, D, T, k in ((5, 4, 20, 70, 5), (1, 1, 128, 1, 1), (256, 8, 1024, 798, 5)):
        rows = P * O
        want = (up16(4 * (2 * rows * T + 17 * rows + 2)) + up16(4 * rows * D) + 2 * up16(4 * (O + 1)) + up16(4 * rows) + 2 * up16(4 * rows * k))
        assert _lib.proposal_score_scratch_bytes(P, O, D, T, k) == want


def test_options_defaults_and_refusals():
    from foundpose_amd import detect_util as du
    o = du.load_opts({"detect_opts": {"version": "v", "templates_version": "t", "object_dataset": "d", "object_lids": [1]}})
    assert (o.detector_extractor_name, o.detector_crop_size, o.detector_topk, o.detector_min_score, o.detector_nms_thresh, o.detector_min_area,
            o.detector_max_per_image, o.detector_batch, o.detector_template_stride) == \
        ("dinov2_version=vitl14-reg_stride=14_facet=token_layer=23_norm=1", 224, 5, 0.2, 0.25, 0, 100, 32, 1)
    with pytest.raises(TypeError):
        du.load_opts({"detector_typo": 1})
    for bad in ({"detector_topk": 0}, {"detector_topk": 17}, {"detector_crop_size": 0}, {"detector_nms_thresh": 0.0}, {"detector_batch": 0},
                {"detector_min_score": float("nan")}, {"detector_max_per_image": 0}, {"detector_template_stride": 0}, {"detector_min_area": -1}):
        with pytest.raises(ValueError):
            du.load_opts(bad)


def test_cpu_tensors_are_refused():
    from foundpose_amd import detect_util as du, ops
    with pytest.raises(ValueError, match="no CPU path"):
        ops.mask_boxes(torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no CPU path"):
        ops.proposal_crops(torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.proposal_scores(torch.zeros(1, 16), torch.zeros(2, 16), torch.tensor([0, 2], dtype=torch.int32), 2, 1)
    with pytest.raises(ValueError, match="no CPU path"):
        ops.box_iou(torch.zeros(1, 4, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(ValueError, match="no CPU path"):
        du.build_detector_bank(None, torch.zeros(1, 3, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8), 8)


def test_the_host_half_of_label_proposals_names_what_the_restatement_names():
    """detect_util._select on the tables the device would hand back (made here by the restatement): names, suppressors, records."""
    import time
    from foundpose_amd import _lib, detect_util as du
    rng = np.random.default_rng(4)
    n, num_obj = 30, 2
    obj = rng.integers(-1, num_obj, n).astype(np.int32)
    score = rng.random(n).astype(np.float32)
    area = rng.integers(0, 30, n).astype(np.int32)
    status = np.where(area == 0, 2, 0).astype(np.int32)
    xy = rng.integers(0, 20, (n, 2))
    boxes = np.concatenate([xy, xy + rng.integers(1, 20, (n, 2))], 1).astype(np.int32)
    tpl = rng.integers(0, 3, n).astype(np.int32)
    names, order, group_off = pr.decide(obj, score, area, status, num_obj, 5, 0.3)
    keep, by = pr.nms_greedy(boxes[order], group_off, 0.25)
    code = np.array([pr.DECISIONS.index(x) for x in names], np.int32)
    order_d = np.array(order + [-1] * (n - len(order)), np.int32)
    keep_d, by_d = np.ones(n, np.int32), np.full(n, -1, np.int32)
    keep_d[:len(order)], by_d[:len(order)] = keep, by
    opts = du.DetectOpts(detector_min_area=5, detector_min_score=0.3, detector_max_per_image=4)
    bs = du.BankSet([7, 9], None, None, [np.array([10, 20, 30]), np.array([11, 21, 31])], 3, 224)
    proposals = [{"scene_id": 2, "image_id": 5, "time": 1.0, "segmentation": {"counts": [i], "size": [1, 1]}} for i in range(n)]
    dets, decs = du._select(opts, proposals, bs, code, order_d, keep_d, by_d, obj, tpl, area, boxes, score, time.perf_counter())
    want_names, want_by, want_kept = pr.select(obj, score, area, status, boxes, num_obj, 5, 0.3, 0.25, 4)
    assert [d["decision"] for d in decs] == want_names and [d["suppressed_by"] for d in decs] == want_by
    assert "suppressed" in want_names and "max_per_image" in want_names and "small" in want_names and "no_object" in want_names
    flat = [(k, d) for k, ds in dets.items() for d in ds]
    assert sorted(d["segmentation"]["counts"][0] for _, d in flat) == sorted(want_kept)
    for k, d in flat:
        p = d["segmentation"]["counts"][0]
        assert k == (2, 5, [7, 9][obj[p]]) and d["bbox"] == [int(boxes[p, 0]), int(boxes[p, 1]), int(boxes[p, 2] - boxes[p, 0]), int(boxes[p, 3] - boxes[p, 1])]
        assert d["score"] == float(score[p]) and d["time"] >= 1.0 and decs[p]["template_id"] == [[10, 20, 30], [11, 21, 31]][obj[p]][tpl[p]]
    assert du.detections_to_list(dets)[0].keys() == {"scene_id", "image_id", "category_id", "bbox", "score", "time", "segmentation"}
