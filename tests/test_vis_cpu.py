"""CPU: the numpy restatement of the result-picture contract (tests/vis_ref.py) on cases worked by hand, and the driver
plumbing that needs no GPU (the --vis flag, the refusal of the unbuilt layout, the palette, the file names)."""
import os

import numpy as np
import pytest

from tests import vis_ref as vr


def test_edge_ring_and_dilation_of_a_square():
    m = np.zeros((9, 9), np.uint8)
    m[3:6, 3:6] = 1
    ring = np.zeros((9, 9), bool)
    ring[3:6, 3:6] = True
    ring[4, 4] = False                      # the centre has four set neighbours
    assert np.array_equal(vr.edge(m), ring)
    dil = np.zeros((9, 9), bool)
    dil[2:7, 2:7] = True                    # every pixel of the 5 x 5 block touches a ring pixel, the centre included
    assert np.array_equal(vr.dilate(ring, 1), dil)
    assert np.array_equal(vr.dilate(ring, 0), ring)
    img = np.zeros((9, 9, 3), np.uint8)
    out = vr.contour(img, m, (0, 255, 0))
    assert np.array_equal(out[..., 1] == 255, dil) and not out[..., 0].any()
    # a mask that fills the image has no edge: the border does not count
    assert not vr.edge(np.ones((4, 5), np.uint8)).any()
    full_but_one = np.ones((3, 3), np.uint8)
    full_but_one[0, 0] = 0
    want = np.zeros((3, 3), bool)
    want[0, 1] = want[1, 0] = True
    assert np.array_equal(vr.edge(full_but_one), want)


def test_segment_and_disc_coverage():
    seg = (2.0, 5.0, 12.0, 5.0)             # horizontal, lw = 1
    for d, cov in ((0.0, 1.0), (0.5, 0.5), (1.0, 0.0), (1.5, 0.0)):
        dist = vr.segment_distance(np.array([7.0]), np.array([5.0 + d]), seg)
        assert dist[0] == d and vr.segment_coverage(dist, 1.0)[0] == cov
    # beyond an end the distance is to the end point
    assert vr.segment_distance(np.array([15.0]), np.array([9.0]), seg)[0] == 5.0
    assert vr.segment_distance(np.array([3.0]), np.array([4.0]), (1.0, 1.0, 1.0, 1.0))[0] == np.hypot(2.0, 3.0)
    assert list(vr.disc_coverage(np.array([0.0, 2.5, 3.0, 3.5]), 2.5)) == [1.0, 0.5, 0.0, 0.0]
    # one vertical segment on a black tile: the pixel column whose centres lie on it is fully covered, its neighbours not at all
    t = vr.draw_matches(np.zeros((9, 9, 3), np.uint8), [[4.5, -10.0, 4.5, 20.0]], colour=(200, 100, 50), radius=0.0)
    assert np.array_equal(t[:, 4], np.tile(np.array([200, 100, 50], np.uint8), (9, 1))) and not t[:, 3].any() and not t[:, 5].any()
    # half coverage blends half way, rounded once
    t = vr.draw_matches(np.full((1, 3, 3), 100, np.uint8), [[-5.0, 1.0, 9.0, 1.0]], colour=(201, 201, 201), radius=0.0)
    assert t[0, 1, 0] == 150                                 # 150.5: round half to even


def test_area_resize():
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (6, 8, 3)).astype(np.uint8)
    want = np.floor(src.reshape(3, 2, 4, 2, 3).astype(np.float64).mean(axis=(1, 3)) + 0.5).astype(np.uint8)
    assert np.array_equal(vr.resize_area(src, 3, 4), want)
    assert np.array_equal(vr.resize_area(src, 6, 8), src)
    # 3 -> 2: the footprints are [0, 1.5) and [1.5, 3), weights (1, 1/2) / 1.5
    row = np.array([[[30, 30, 30], [60, 60, 60], [120, 120, 120]]], np.uint8)
    assert vr.resize_area(row, 1, 2)[0, :, 0].tolist() == [40, 100]
    with pytest.raises(ValueError):
        vr.resize_area(src, 7, 8)


def test_pca_colorize():
    assert not vr.pca_colorize(np.full((3, 4, 8), 2.5), 7, 9).any()
    m = np.zeros((1, 2, 5))
    m[0, 0, :3] = [0.0, 1.0, 2.0]
    m[0, 1, :3] = [4.0, 3.0, 0.5]
    m[..., 3:] = 99.0                                        # channels beyond the third do not enter the range
    out = vr.pca_colorize(m, 2, 4)
    assert out.shape == (2, 4, 3)
    assert out[0, 0].tolist() == [0, 63, 127] and out[1, 3].tolist() == [255, 191, 31]   # ONE range (0, 4) for the three channels
    assert np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, 2], out[:, 3])  # floor(x * 2 / 4)
    assert np.array_equal(vr.darken(np.array([255, 10, 9], np.uint8)), np.array([229, 9, 8], np.uint8))


def test_scene_composite_crossing_depths():
    d = np.zeros((2, 1, 4), np.float32)
    d[0, 0] = [500, 600, 0, 0]
    d[1, 0] = [600, 500, 700, 0]
    img = np.full((1, 4, 3), 100, np.uint8)
    out, ids = vr.scene_composite(img, d, [(255, 0, 0), (0, 0, 201)])
    assert ids.tolist() == [[0, 1, 1, -1]]
    assert out[0].tolist() == [[177, 50, 50], [50, 50, 150], [50, 50, 150], [100, 100, 100]]
    d[1, 0, 0] = 500                                         # a tie goes to the lowest layer
    assert vr.scene_composite(img, d, [(255, 0, 0), (0, 0, 201)])[1][0, 0] == 0


def test_mask_tint_and_match_selection():
    img = np.array([[[0, 1, 254], [10, 20, 30]]], np.uint8)
    assert vr.mask_tint(img, np.array([[7, 0]])).tolist() == [[[127, 128, 254], [10, 20, 30]]]
    conf = [0.5, 0.9, 0.9, np.nan, 0.1]
    left = np.arange(10.0).reshape(5, 2)
    right = np.array([[1, 1], [2, 2], [50, 2], [3, 3], [4, 4]], np.float64)
    segs = vr.select_matches(conf, left, right, 3, 10, 10)    # top 3: 1, 2 (tie: lower index first), 0; 2 falls outside; least confident first
    assert segs.tolist() == [[0.0, 1.0, 11.0, 1.0], [2.0, 3.0, 12.0, 2.0]]
    assert vr.strip_size(5, 224, 224, 224) == (89, 448)


# ---------------------------------------------------------------------------------------------------- driver plumbing
def test_infer_help_lists_vis(capsys):
    from foundpose_amd import infer
    with pytest.raises(SystemExit):
        infer.main(["--help"])
    assert "--vis" in capsys.readouterr().out


def test_unbuilt_layout_is_refused_before_device_work():
    from foundpose_amd import infer
    base = dict(version="v", repre_version="r", object_dataset="lmo")
    with pytest.raises(NotImplementedError, match="vis_for_paper"):
        infer.infer_object(infer.InferOpts(**base, vis_for_paper=False), 1, None, [], {}, renderer=object(), output_dir="unused")
    with pytest.raises(NotImplementedError, match="vis_for_paper"):
        infer.infer(infer.InferOpts(**base, vis_for_paper=False), lambda lid: iter([]), {}, {}, "unused", extractor=object(), renderer=object())
    with pytest.raises(ValueError, match="vis_corresp_top_n"):
        infer.infer_object(infer.InferOpts(**base, vis_corresp_top_n=5000), 1, None, [], {}, renderer=object(), output_dir="unused")


def test_palette_and_file_names():
    from foundpose_amd import vis_util
    assert len(vis_util.PALETTE) == 12 and len(set(vis_util.PALETTE)) == 12
    assert all(len(c) == 3 and all(0 <= v <= 255 for v in c) for c in vis_util.PALETTE)
    assert vis_util.palette_colour(13) == vis_util.PALETTE[1] and vis_util.palette_colour(12) == vis_util.PALETTE[0]
    assert vis_util.tile_path("out", 48, 1107, 5, 2) == os.path.join("out", "5", "48_1107_5_2_0.png")
    assert vis_util.summary_path("out", 48, 1107) == os.path.join("out", "vis", "48_1107.png")
    assert (vis_util.COLOUR_GT, vis_util.COLOUR_COARSE, vis_util.COLOUR_FINAL) == ((255, 0, 0), (0, 0, 255), (0, 255, 0))
    assert vis_util.MATCH_COLOUR == (230, 230, 230) and vis_util.MATCH_RADIUS == 2.5 and vis_util.MATCH_LW == 1.0
