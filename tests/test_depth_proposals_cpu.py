"""CPU: the numpy restatement of the depth proposals (tests/depth_proposals_ref.py) on scenes whose answers are
known, the conditions every fixture of tests/test_gpu_depth_proposals.py relies on, the options' refusals and the header's symbols."""

import os

import numpy as np
import pytest

from foundpose_amd.infer_pose_util import rle_to_binary_mask
from tests import depth_proposals_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def e2e():
    D, plane, visible = ref.e2e_scene()
    return D, plane, visible, ref.propose_frame(D, ref.E2E_CAM, ref.E2E_KEY, ref.options(min_pixels=12))


def test_the_analytic_scene_gives_exactly_its_four_spheres(e2e):
    D, plane, visible, out = e2e
    lv = out["levels"][0]
    assert len(out["planes"]) == 1 and out["records"][0]["accepted"]
    angle, offset = ref.plane_difference(out["planes"][0], plane)
    assert angle < np.deg2rad(0.01) and offset < 0.05
    assert lv["counts"][2] == 4 and len(lv["table"]) == 4
    for m in visible:
        assert max(ref.iou(lv["rank_map"] == r, m) for r in range(4)) >= 0.99
    assert list(lv["table"][:, 1]) == sorted(lv["table"][:, 1], reverse=True)


def test_with_a_wall_two_planes_are_accepted_and_the_third_is_refused():
    D, _, visible = ref.e2e_scene(wall=True)
    out = ref.propose_frame(D, ref.E2E_CAM, ref.E2E_KEY, ref.options(min_pixels=12, num_planes=3))
    rec = out["records"]
    assert [r["accepted"] for r in rec] == [True, True, False]
    shares = [r["support"] / r["valid"] for r in rec]
    assert 0.7 < shares[0] < 0.8 and 0.2 < shares[1] < 0.3 and shares[2] < 0.05
    assert rec[1]["eligible"] < rec[0]["eligible"] and rec[0]["valid"] == rec[1]["valid"]
    lv = out["levels"][0]
    assert len(lv["table"]) == 4
    for m in visible:
        assert max(ref.iou(lv["rank_map"] == r, m) for r in range(4)) >= 0.99


def test_runs_round_trip_sum_to_the_image_and_start_with_a_zero_run(e2e):
    D, _, _, out = e2e
    lv = out["levels"][0]
    for r, counts in enumerate(lv["runs"]):
        assert sum(counts) == D.size
        assert np.array_equal(rle_to_binary_mask({"size": list(D.shape), "counts": counts}), lv["rank_map"] == r)
    # a component that holds pixel (0, 0) has an empty leading run; one that fills a column's end and the next column's start has one run there
    m = np.zeros((6, 5), np.int32) - 1
    m[4:, 1] = 0
    m[:2, 2] = 0
    m[0, 0] = 1
    assert ref.runs(m, 2) == [[10, 4, 16], [0, 1, 29]]


def test_levels_nest_and_duplicates_are_dropped():
    D, _, _ = ref.e2e_scene()
    D = D.copy()
    D[60:62, 70:90] = D[60:62, 70:90] + np.float32(40.0)      # a groove that the fine level cannot cross on the plane's side
    out = ref.propose_frame(D, ref.E2E_CAM, ref.E2E_KEY, ref.options(min_pixels=12, connect_mm=(2.0, 5.0, 60.0)))
    fine, mid, coarse = (lv["labels"] for lv in out["levels"])
    for a, b in ((fine, mid), (mid, coarse)):
        assert np.array_equal(a >= 0, b >= 0)
        pairs = np.unique(np.stack([a[a >= 0], b[a >= 0]]), axis=1)
        assert len(np.unique(pairs[0])) == pairs.shape[1]          # every finer component lies in one coarser component
        assert np.all(pairs[1] <= pairs[0])                        # ... whose label is not larger
    seen = set()
    for lv in out["levels"]:
        rows = {(int(r[0]), int(r[1])) for r in lv["table"]}
        assert not rows & seen
        seen |= rows
    assert sum(lv["counts"][3] for lv in out["levels"]) > 0          # something was in fact the same on two levels


def test_the_hand_made_frames_have_the_components_they_are_named_for():
    for H, W in ref.PATTERN_SIZES:
        m = ref.pattern_masks(H, W)
        D = {k: np.where(v, ref.Z0, np.float32(0)) for k, v in m.items()}
        count = lambda k: len(np.unique(ref.components(D[k], m[k], ref.PATTERN_CMM, ref.PATTERN_SLOPE_FX)[m[k]]))
        for k in ("serpentine", "comb", "spiral", "all", "ring", "holes", "last_row", "first_row"):
            assert count(k) == 1, k
        assert count("checkerboard") == (H * W + 1) // 2 and count("none") == 0 and count("wrap") == 2
        ring = ref.components(D["ring"], m["ring"], ref.PATTERN_CMM, ref.PATTERN_SLOPE_FX)
        assert ring[0, 0] == 0 and ring[-1, -1] == 0 and ring[H // 2, W // 2] == 0
        # the corridors cross tile borders: the serpentine's rows cross every vertical border, four times and more
        assert m["serpentine"][::2, 32].sum() >= 4 and m["comb"][32, ::2].sum() >= 4
        blocks = ref.table(ref.components(D["blocks"], m["blocks"], ref.PATTERN_CMM, ref.PATTERN_SLOPE_FX), 1, H * W, 64)
        assert blocks[1][0] > 64 and blocks[1][2] == 64 and set(blocks[0][:, 1]) <= {9, 12}    # more than max_proposals, ties in area
        assert np.all(np.diff(blocks[0][:, 1]) <= 0)
        assert np.all(np.diff(blocks[0][:, 0])[np.diff(blocks[0][:, 1]) == 0] > 0)              # ties: label ascending
        every = ref.table(ref.components(D["blocks"], m["blocks"], ref.PATTERN_CMM, ref.PATTERN_SLOPE_FX), 1, H * W, 1024)[0]
        assert set(every[:, 1]) == {9, 12} and np.all(np.diff(every[:, 1]) <= 0)
        for frame, want_components in ((ref.ulp_frame, 9), (ref.ulp_frame_slope, 6)):
            Du, s, expect = frame(H, W)
            lab = ref.components(Du, Du > 0, ref.PATTERN_CMM, s)
            assert len(np.unique(lab[lab >= 0])) == want_components
            for (y, x), joined in expect.items():
                assert (lab[y, x] == lab[y, x + 1]) == joined


def test_foreground_is_decided_at_the_margin_to_the_ulp():
    for D, planes, margin, max_depth, want in ref.foreground_frames():
        assert np.array_equal(ref.foreground(D, ref.E2E_CAM, planes, margin, max_depth), want)
        assert want.sum() > 0 and (~want & (D > 0)).sum() > 0
    D, _, _, _, want = ref.foreground_frames()[0]
    assert want[0, :8].tolist() == [False, True, False, False, False, False, True, False]


def test_options_refuse_bad_values_by_name():
    from foundpose_amd import depth_proposals as dp
    assert dp.load_opts(None) == dp.DepthProposalOpts()
    assert dp.load_opts({"depth_proposal_opts": {"connect_mm": [2.0, 5.0]}}).levels() == [2.0, 5.0]
    for key, bad in (("num_planes", 5), ("num_planes", -1), ("plane_hypotheses", 0), ("plane_hypotheses", 4097), ("plane_stride", 0),
                     ("plane_thresh_mm", 0.0), ("min_plane_share", 1.5), ("max_depth_mm", -1.0), ("object_margin_mm", float("nan")),
                     ("connect_mm", [5.0, 2.0]), ("connect_mm", [1.0, 2.0, 3.0, 4.0]), ("connect_mm", -1.0), ("connect_slope", -0.1),
                     ("min_pixels", 0), ("max_area_share", 0.0), ("max_proposals", 0), ("max_proposals", 1025), ("seed", -1), ("min_pixels", 2.5),
                     ("num_planes", True)):
        with pytest.raises(ValueError, match=key):
            dp.load_opts({key: bad})
    with pytest.raises(ValueError, match="unknown"):
        dp.load_opts({"depth_proposal_opts": {"conect_mm": 5.0}})
    assert dp.frame_key(3, 7) == 3 * 2**32 + 7


def test_the_header_declares_the_entry_points_and_the_binding_matches():
    text = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    for name in ("fp_depth_plane_fit", "fp_depth_components", "fp_component_table", "fp_component_runs", "FP_DEPTH_PLANE_SCRATCH_BYTES",
                 "FP_DEPTH_COMPONENTS_SCRATCH_BYTES", "FP_COMPONENT_TABLE_SCRATCH_BYTES", "FP_DEPTH_MAX_PLANES", "FP_DEPTH_MAX_HYPOTHESES",
                 "FP_DEPTH_MAX_PROPOSALS"):
        assert name in text
    from foundpose_amd import _lib
    assert {"fp_depth_plane_fit", "fp_depth_components", "fp_component_table", "fp_component_runs"} <= set(_lib.exported_symbols())
    assert f"#define FP_DEPTH_MAX_PLANES {_lib.DEPTH_MAX_PLANES}" in text and f"#define FP_DEPTH_PLANE_CHUNK {_lib.DEPTH_PLANE_CHUNK}" in text
    assert _lib.depth_plane_scratch_bytes(3, 4480, 256) == 256 * 3 + 16 * 840 + 8 * 384 + 64 * 3 * 2
    assert _lib.depth_components_scratch_bytes(3, 4480) == 64 * 3 + 4 * 3 * 4480 and _lib.component_table_scratch_bytes(3, 4480) == 16 * 3 + 28 * 3 * 4480
