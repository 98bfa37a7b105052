"""CPU: the numpy restatement of fp_gt_visibility (tests/gt_info_ref.py) on hand-made arrays whose answers are written out here, the
record assembly and its key order, the target counting, the overwrite refusal, and that gt_info imports without a device."""
import json
import os

import numpy as np
import pytest

from tests import gt_info_ref as ref

W, H = 12, 10                     # the image, in the middle of a 36 x 30 window
K = np.array([[100.0, 0, 5.5], [0, 100.0, 4.5], [0, 0, 1]])
EMPTY = ref.EMPTY_BOX
KEYS = ["bbox_obj", "bbox_visib", "px_count_all", "px_count_valid", "px_count_visib", "visib_fract"]


def _large(x0, y0, x1, y1, depth=1000.0):
    """A square of constant depth, given in IMAGE coordinates (inclusive), inside the window."""
    a = np.zeros((3 * H, 3 * W), np.float32)
    a[H + y0:H + y1 + 1, W + x0:W + x1 + 1] = depth
    return a


def _run(test, large, delta=15.0):
    return ref.gt_visibility(test, large, K, delta, W, H)


def test_fully_visible_square():
    test = np.full((H, W), 1500.0, np.float32)
    row, mask, vis = _run(test, _large(3, 2, 6, 5))
    assert row.tolist() == [16, 16, 16, 3, 2, 6, 5, 3, 2, 6, 5]
    want = np.zeros((H, W), np.uint8)
    want[2:6, 3:7] = 255
    assert np.array_equal(mask, want) and np.array_equal(vis, want) and mask.dtype == np.uint8
    assert ref.record(row) == {"bbox_obj": [3, 2, 3, 3], "bbox_visib": [3, 2, 3, 3], "px_count_all": 16, "px_count_valid": 16,
                               "px_count_visib": 16, "visib_fract": 1.0}


def test_square_half_behind_an_occluder():
    test = np.full((H, W), 1500.0, np.float32)
    test[:, :5] = 900.0            # columns 3 and 4 of the square lie 100 mm behind it
    row, mask, vis = _run(test, _large(3, 2, 6, 5))
    assert row.tolist() == [16, 16, 8, 3, 2, 6, 5, 5, 2, 6, 5]
    assert mask[2:6, 3:7].all() and mask.sum() == 16 * 255
    assert vis[2:6, 5:7].all() and vis.sum() == 8 * 255
    rec = ref.record(row)
    assert rec["visib_fract"] == 0.5 and rec["bbox_obj"] == [3, 2, 3, 3] and rec["bbox_visib"] == [5, 2, 1, 3]


def test_square_half_over_a_hole_is_visible_but_not_valid():
    test = np.full((H, W), 1500.0, np.float32)
    test[:, :5] = 0.0
    row, mask, vis = _run(test, _large(3, 2, 6, 5))
    assert row.tolist() == [16, 8, 16, 3, 2, 6, 5, 3, 2, 6, 5]
    assert np.array_equal(mask, vis)
    assert ref.record(row)["visib_fract"] == 1.0


def test_square_leaving_the_image_on_the_left():
    test = np.full((H, W), 1500.0, np.float32)
    row, mask, vis = _run(test, _large(-3, 2, 1, 4))     # columns -3 .. 1: two of five inside
    assert row.tolist() == [15, 6, 6, -3, 2, 1, 4, 0, 2, 1, 4]
    assert mask[2:5, 0:2].all() and mask.sum() == 6 * 255 and np.array_equal(mask, vis)
    rec = ref.record(row)
    assert rec["bbox_obj"] == [-3, 2, 4, 2] and rec["bbox_visib"] == [0, 2, 1, 2] and rec["visib_fract"] == 6 / 15.0


def test_square_wholly_outside_the_image():
    test = np.full((H, W), 1500.0, np.float32)
    row, mask, vis = _run(test, _large(W + 2, -6, W + 5, -4))
    assert row.tolist() == [12, 0, 0, W + 2, -6, W + 5, -4] + EMPTY
    assert not mask.any() and not vis.any()
    rec = ref.record(row)
    assert rec["px_count_all"] == 12 and rec["px_count_visib"] == 0 and rec["visib_fract"] == 0.0
    assert rec["bbox_obj"] == [-1, -1, -1, -1] and rec["bbox_visib"] == [-1, -1, -1, -1]


def test_empty_render_has_fraction_zero_not_nan():
    test = np.full((H, W), 1500.0, np.float32)
    row, mask, vis = _run(test, np.zeros((3 * H, 3 * W), np.float32))
    assert row.tolist() == [0, 0, 0] + EMPTY + EMPTY
    rec = ref.record(row)
    assert rec["visib_fract"] == 0.0 and isinstance(rec["visib_fract"], float) and rec["bbox_obj"] == [-1] * 4
    assert not mask.any() and not vis.any()


def test_delta_boundary_in_float32():
    """At an integer principal point dist = depth exactly: 1015 against 1000 is visible at delta 15, the next float32 is not."""
    Kc = np.array([[100.0, 0, 5.0], [0, 100.0, 4.0], [0, 0, 1]])
    test = np.full((H, W), 1000.0, np.float32)
    for depth, seen in ((np.float32(1015), 1), (np.nextafter(np.float32(1015), np.float32(2000)), 0)):
        large = np.zeros((3 * H, 3 * W), np.float32)
        large[H + 4, W + 5] = depth
        row, _, vis = ref.gt_visibility(test, large, Kc, 15.0, W, H)
        assert row[:3].tolist() == [1, 1, seen] and int(vis[4, 5]) == 255 * seen


def test_record_assembly_and_key_order():
    from foundpose_amd import gt_info
    rows = [[16, 8, 4, -3, 2, 6, 5, 0, 2, 5, 4], [12, 0, 0, 14, -6, 17, -4] + EMPTY, [0, 0, 0] + EMPTY + EMPTY]
    for row in rows:
        rec = gt_info.gt_record(np.array(row, np.int32))
        assert list(rec) == KEYS and rec == ref.record(row)
        assert list(json.loads(json.dumps(rec))) == KEYS
        assert all(type(v) is int for k in KEYS[:2] for v in rec[k]) and type(rec["visib_fract"]) is float
    assert gt_info.gt_record(rows[0]) == {"bbox_obj": [-3, 2, 9, 3], "bbox_visib": [0, 2, 5, 2], "px_count_all": 16, "px_count_valid": 8,
                                          "px_count_visib": 4, "visib_fract": 0.25}
    assert gt_info.scan_box([2**31 - 1, 2**31 - 1, -2**31, -2**31]) == (0, 0, -1, -1) and gt_info.scan_box([3, 4, 3, 4]) == (3, 4, 3, 4)
    assert gt_info.chunk_views(640, 480) == 32 and gt_info.chunk_views(4000, 3000) == 1 and gt_info.chunk_views(1920, 1080) == 11


def test_targets_threshold_is_inclusive_and_zero_counts_are_left_out():
    from foundpose_amd import gt_info
    inst = [(1, 0, 5, 0.1), (1, 0, 5, 0.0999), (1, 0, 5, 0.7), (1, 0, 6, 0.05), (1, 1, 6, 1.0), (2, 0, 5, 0.0), (2, 3, 7, 0.1)]
    want = [{"scene_id": 1, "im_id": 0, "obj_id": 5, "inst_count": 2}, {"scene_id": 1, "im_id": 1, "obj_id": 6, "inst_count": 1},
            {"scene_id": 2, "im_id": 3, "obj_id": 7, "inst_count": 1}]
    assert gt_info.count_targets(inst, "bop19") == want == ref.targets_bop19(inst)
    assert gt_info.count_targets(reversed(inst), "bop19") == want
    assert gt_info.count_targets(inst, "bop24") == [{"scene_id": 1, "im_id": 0}, {"scene_id": 1, "im_id": 1}, {"scene_id": 2, "im_id": 0},
                                                    {"scene_id": 2, "im_id": 3}]
    with pytest.raises(ValueError):
        gt_info.count_targets(inst, "bop23")


def _tree(tmp_path):
    """A split with one scene and one instance, without any pixels: enough for the refusals that come before the device."""
    sd = tmp_path / "ds" / "test" / "000003"
    sd.mkdir(parents=True)
    (sd / "scene_gt.json").write_text(json.dumps({"4": [{"cam_R_m2c": np.eye(3).ravel().tolist(), "cam_t_m2c": [0, 0, 800.0], "obj_id": 2}]}))
    (sd / "scene_camera.json").write_text(json.dumps({"4": {"cam_K": K.ravel().tolist(), "depth_scale": 1.0}}))
    return str(tmp_path / "ds" / "test"), sd


def test_existing_outputs_are_refused_before_anything_is_read_or_written(tmp_path):
    from foundpose_amd import gt_info
    split, sd = _tree(tmp_path)
    models = str(tmp_path / "ds" / "models")         # does not exist: the refusal comes first
    (sd / "scene_gt_info.json").write_text("{}")
    with pytest.raises(FileExistsError, match="scene_gt_info.json"):
        gt_info.write_gt_info(split, models)
    os.remove(sd / "scene_gt_info.json")
    (sd / "mask_visib").mkdir()
    (sd / "mask_visib" / "000004_000000.png").write_bytes(b"x")
    with pytest.raises(FileExistsError, match="000004_000000.png"):
        gt_info.write_gt_info(split, models)
    with pytest.raises(FileNotFoundError, match="obj_000002.ply"):      # masks not written: that file is not an output
        gt_info.write_gt_info(split, models, write_masks=False)
    (tmp_path / "ds" / "test_targets_bop24.json").write_text("[]")
    with pytest.raises(FileExistsError, match="test_targets_bop24.json"):
        gt_info.write_gt_info(split, models, write_masks=False, targets="bop24")
    other = tmp_path / "elsewhere" / "test"
    with pytest.raises(FileNotFoundError, match="obj_000002.ply"):      # a mirror directory holds none of them
        gt_info.write_gt_info(split, models, output_dir=str(other), targets="bop24")
    with pytest.raises(FileNotFoundError, match="obj_000002.ply"):      # overwrite lifts the refusal
        gt_info.write_gt_info(split, models, overwrite=True, targets="bop24")
    assert (sd / "mask_visib" / "000004_000000.png").read_bytes() == b"x" and not other.exists()
    assert sorted(os.listdir(sd)) == ["mask_visib", "scene_camera.json", "scene_gt.json"]
    gt_info.refuse_existing([str(sd / "nothing")], overwrite=False)
    with pytest.raises(ValueError, match="targets"):
        gt_info.write_gt_info(split, models, targets="bop23")
    with pytest.raises(FileNotFoundError, match="scene"):
        gt_info.write_gt_info(split, models, scenes=[9])


def test_module_imports_without_a_device_and_says_what_is_not_pinned():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; import foundpose_amd.gt_info as g; assert 'torch' not in sys.modules; print(g.NOT_PINNED)"
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert out.returncode == 0, out.stderr
    assert "not" in out.stdout and "bop_toolkit" in out.stdout
    from foundpose_amd import gt_info
    assert "PINNED AGAINST bop_toolkit" in gt_info.__doc__ and "bop_toolkit" in gt_info.write_gt_info.__doc__
