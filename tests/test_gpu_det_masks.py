"""fp_detection_masks (ops.detection_masks) against the host path it replaces.  Every expected value is computed here by
infer_pose_util.rle_to_binary_mask, open_mask_3x3, the [dy : hc - dy, dx : wc - dx] slice and .sum() -- the functions select_instances runs,
pinned by tests/test_infer_pose_util.py -- and every comparison is an equality.  Canvases are at most 128 x 96."""
import numpy as np
import pytest
import torch

from foundpose_amd import _lib, infer_pose_util as ipu, ops

pytestmark = pytest.mark.gpu


def _expected(rle, image_hw, open3x3):
    m = ipu.rle_to_binary_mask(rle).astype(np.uint8)
    if open3x3:
        m = ipu.open_mask_3x3(m)
    (hc, wc), (H, W) = m.shape, image_hw
    dy, dx = (hc - H) // 2, (wc - W) // 2
    m = m[dy:hc - dy, dx:wc - dx]
    assert m.shape == (H, W)
    return torch.from_numpy(np.ascontiguousarray(m)), int(m.sum())


def _run(rles, image_hw, open3x3):
    counts, run_off, size = ipu.pack_rle(rles)
    masks, area = ops.detection_masks(torch.from_numpy(counts).cuda(), torch.from_numpy(run_off).cuda(), size, image_hw, open3x3=open3x3)
    assert masks.dtype == torch.uint8 and tuple(masks.shape) == (len(rles), *image_hw) and masks.is_cuda
    assert area.dtype == torch.int32 and tuple(area.shape) == (len(rles),)
    return masks.cpu(), area.cpu()


def _check(rles, image_hw, open3x3):
    masks, area = _run(rles, image_hw, open3x3)
    for i, rle in enumerate(rles):
        want, want_area = _expected(rle, image_hw, open3x3)
        assert torch.equal(masks[i], want), (i, rle["counts"][:8], int((masks[i] != want).sum()))
        assert int(area[i]) == want_area, (i, int(area[i]), want_area)
    return masks, area


def _rle(mask):
    return ipu.binary_mask_to_rle(np.asarray(mask, np.uint8))


def _run_lists(hc, wc):
    n = hc * wc
    lists = [[n], [0, n], [10], [0, 7, 5, 9], [5, 0, 0, 8, 0, 3, 20, 0, 0, 6], [100, 50], [30, n + 100], [n - 5, 50], [0, 0, 0, hc + 1, hc - 1, 2 * hc],
             [n - 1, 1], [n, 7], []]
    return [{"counts": c, "size": [hc, wc]} for c in lists]


def _blobs(hc, wc, seed):
    rng = np.random.default_rng(seed)
    out = [rng.random((hc, wc)) < 0.5, rng.random((hc, wc)) < 0.9]
    yy, xx = np.mgrid[:hc, :wc]
    out.append((yy - hc / 2) ** 2 + (xx - wc / 2) ** 2 <= (0.4 * min(hc, wc)) ** 2)
    out.append(((yy - 3) ** 2 + (xx - wc + 4) ** 2 <= 81) | (rng.random((hc, wc)) < 0.02))     # a disc over a corner, and specks
    return [_rle(m) for m in out]


@pytest.mark.parametrize("open3x3", [False, True])
@pytest.mark.parametrize("canvas,image", [((37, 53), (37, 53)), ((44, 60), (40, 52))])
def test_ragged_sizes_and_run_lists(canvas, image, open3x3):
    """Canvases that are no multiple of the 64 x 16 tile, without and with a crop (dy = 2, dx = 4); the run lists: empty and full masks,
    R = 1 short of the canvas, leading zero runs, zero runs in the middle, totals short of the canvas, beyond it and ending exactly on it,
    and no run at all."""
    _check(_run_lists(*canvas) + _blobs(*canvas, seed=canvas[0]), image, open3x3)


def _shapes(hc, wc):
    """name -> mask on the canvas."""
    z = lambda: np.zeros((hc, wc), np.uint8)
    s = {}
    for name, (y, x) in {"pixel_tl": (0, 0), "pixel_br": (hc - 1, wc - 1)}.items():
        s[name] = z()
        s[name][y, x] = 1
    s["line_h"], s["line_v"] = z(), z()
    s["line_h"][20, :] = 1
    s["line_v"][:, 30] = 1
    for name, sl in {"strip_top": np.s_[0:2, :], "strip_bottom": np.s_[hc - 2:hc, :], "strip_left": np.s_[:, 0:2], "strip_right": np.s_[:, wc - 2:wc],
                     "strip_inner_h": np.s_[21:23, :], "strip_inner_v": np.s_[:, 17:19], "strip_one_off_top": np.s_[1:3, :],
                     "block_inner": np.s_[10:13, 33:36], "block_tl": np.s_[0:3, 0:3], "block_tr": np.s_[0:3, wc - 3:wc],
                     "block_bl": np.s_[hc - 3:hc, 0:3], "block_br": np.s_[hc - 3:hc, wc - 3:wc],
                     "blob_over_crop_corner": np.s_[0:9, 0:13], "bar_over_crop_edge": np.s_[0:4, 20:40], "bar_inside_crop_edge": np.s_[2:4, 20:40]}.items():
        s[name] = z()
        s[name][sl] = 1
    return s


def test_opening_follows_the_canvas_border_rule_then_the_crop():
    """open_mask_3x3's rule: a neighbour outside the canvas neither vetoes an erosion nor wins a dilation.  So a 2-pixel strip along a canvas
    edge survives and the same strip in the interior (or one pixel off the edge) vanishes; a 3 x 3 block survives anywhere; and with a crop
    (dy = 2, dx = 4) the border that matters is the CANVAS's: a 2-pixel bar that starts at the crop window's first row vanishes although it
    would survive if the opening ran on the cropped image, a 4-pixel bar across the window's edge leaves its two rows inside."""
    hc, wc = 44, 60
    shapes = _shapes(hc, wc)
    names = list(shapes)
    rles = [_rle(shapes[k]) for k in names]
    full, full_area = _check(rles, (hc, wc), True)
    a = dict(zip(names, full_area.tolist()))
    assert a["pixel_tl"] == a["pixel_br"] == a["line_h"] == a["line_v"] == a["strip_inner_h"] == a["strip_inner_v"] == a["strip_one_off_top"] == 0
    assert a["strip_top"] == a["strip_bottom"] == 2 * wc and a["strip_left"] == a["strip_right"] == 2 * hc
    assert a["block_inner"] == a["block_tl"] == a["block_tr"] == a["block_bl"] == a["block_br"] == 9
    _check(rles, (hc, wc), False)
    crop, crop_area = _check(rles, (40, 52), True)
    c = dict(zip(names, crop_area.tolist()))
    assert c["strip_top"] == c["strip_left"] == 0 and c["blob_over_crop_corner"] == 7 * 9
    assert c["bar_over_crop_edge"] == 2 * 20 and c["bar_inside_crop_edge"] == 0
    # ... while the opening of the cropped image would have kept that bar: the order is opening, then crop
    assert int(ipu.open_mask_3x3(shapes["bar_inside_crop_edge"][2:42, 4:56]).sum()) == 2 * 20
    _check(rles, (40, 52), False)


def _checkerboard(hc, wc):
    yy, xx = np.mgrid[:hc, :wc]
    return ((yy + xx) % 2).astype(np.uint8)


def test_many_runs():
    """A 128 x 96 checkerboard: about 12 200 runs (one per pixel, less the runs that merge across the ends of the even columns).  The kernels
    stage no prefix sums in LDS -- a pixel's binary search reads the detection's sums in global memory, whatever their number -- so there is
    no staged count for this case to exceed; it is the longest search and the longest scan (48 chunks of 256 with a carry).  Raw it must be
    the host's mask; opened it is empty."""
    for hc, wc in ((96, 128), (128, 96)):
        rle = _rle(_checkerboard(hc, wc))
        assert len(rle["counts"]) > 12000
        raw, raw_area = _check([rle], (hc, wc), False)
        assert int(raw_area[0]) == hc * wc // 2
        opened, area = _check([rle], (hc, wc), True)
        assert int(area[0]) == 0 and not opened.any()


@pytest.mark.parametrize("open3x3", [False, True])
def test_run_counts_around_one_scan_chunk(open3x3):
    """The prefix sums are scanned in chunks of 256 runs with a carry: detections of exactly 255, 256 and 257 runs (one short of a chunk,
    a whole one, one entry in a second) on a 32 x 32 canvas, in one batch.  Run lengths are >= 1 and sum to 1024.  The reference is the
    decode rule as tests/test_det_masks_cpu.py restates it, then open_mask_3x3."""
    from tests.test_det_masks_cpu import _decode_rule
    rng = np.random.default_rng(255)
    lists = []
    for R in (255, 256, 257):
        p = np.full(R, 0.4 / R)
        p[[1, 60, 121, 180, 201, R - 2]] += 0.1              # a few long runs, set and unset: blocks that survive the opening
        lists.append((rng.multinomial(1024 - R, p) + 1).tolist())
    assert [len(c) for c in lists] == [255, 256, 257] and all(sum(c) == 1024 for c in lists)
    masks, area = _run([{"counts": c, "size": [32, 32]} for c in lists], (32, 32), open3x3)
    for i, c in enumerate(lists):
        want = _decode_rule(c, 32, 32).astype(np.uint8)
        if open3x3:
            want = ipu.open_mask_3x3(want)
        assert want.any() and np.array_equal(masks[i].numpy(), want) and int(area[i]) == int(want.sum()), len(c)


def test_a_detection_depends_on_its_own_runs_only():
    """Eight detections of very different run counts in one call: the same bits as each alone and as the reversed batch."""
    hc, wc, image = 96, 128, (90, 120)
    yy, xx = np.mgrid[:hc, :wc]
    disc = (yy - 50) ** 2 + (xx - 60) ** 2 <= 40 ** 2
    rles = [{"counts": [hc * wc], "size": [hc, wc]}, {"counts": [0, hc * wc], "size": [hc, wc]}, {"counts": [700, 4000, 100], "size": [hc, wc]},
            _rle(disc), _rle(_checkerboard(hc, wc)), _rle(_checkerboard(hc, wc) | disc), {"counts": [], "size": [hc, wc]},
            _rle(np.random.default_rng(5).random((hc, wc)) < 0.8)]
    assert [len(r["counts"]) for r in rles][:3] == [1, 2, 3] and len(rles[3]["counts"]) > 100 and len(rles[4]["counts"]) > 12000
    for open3x3 in (False, True):
        masks, area = _check(rles, image, open3x3)
        rev_masks, rev_area = _run(rles[::-1], image, open3x3)
        assert torch.equal(rev_masks.flip(0), masks) and torch.equal(rev_area.flip(0), area)
        for i, rle in enumerate(rles):
            m1, a1 = _run([rle], image, open3x3)
            assert torch.equal(m1[0], masks[i]) and int(a1[0]) == int(area[i]), i


def test_no_detection_no_launch():
    masks, area = ops.detection_masks(torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), (44, 60), (40, 52))
    assert tuple(masks.shape) == (0, 40, 52) and masks.dtype == torch.uint8 and tuple(area.shape) == (0,) and area.dtype == torch.int32


def test_bad_arguments_raise():
    counts, run_off = torch.tensor([5, 10], dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32)
    with pytest.raises(_lib.FoundPoseNativeError):
        ops.detection_masks(counts, run_off.cuda(), (6, 8), (6, 8))                    # a CPU tensor
    with pytest.raises(_lib.FoundPoseNativeError):
        ops.detection_masks(counts.cuda(), run_off, (6, 8), (6, 8))
    with pytest.raises(ValueError, match="int32"):
        ops.detection_masks(counts.long().cuda(), run_off.cuda(), (6, 8), (6, 8))      # not int32
    with pytest.raises(ValueError, match="int32"):
        ops.detection_masks(counts.cuda(), run_off.long().cuda(), (6, 8), (6, 8))
    for image in ((7, 8), (6, 9), (0, 8)):
        with pytest.raises(ValueError, match="out of a canvas"):
            ops.detection_masks(counts.cuda(), run_off.cuda(), (6, 8), image)
    # the library's own checks, past the wrapper's
    c, r = counts.cuda(), run_off.cuda()
    out, area, pre = torch.empty(1, 6, 8, dtype=torch.uint8, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"), torch.empty(2, dtype=torch.int32, device="cuda")
    for hc, wc, H, W, n in ((6, 8, 7, 8, 1), (6, 8, 6, 9, 1), (6, 8, 0, 8, 1), (1 << 15, (1 << 15) + 1, 6, 8, 1), (6, 8, 6, 8, -1)):
        with pytest.raises(_lib.FoundPoseNativeError, match="fp_detection_masks"):
            _lib.call("fp_detection_masks", _lib.ptr(c), _lib.ptr(r), 2, n, hc, wc, H, W, 1, _lib.ptr(pre), _lib.ptr(out), _lib.ptr(area), _lib.stream())
    with pytest.raises(_lib.FoundPoseNativeError, match="null pointer"):
        _lib.call("fp_detection_masks", _lib.ptr(c), _lib.ptr(None), 2, 1, 6, 8, 6, 8, 1, _lib.ptr(pre), _lib.ptr(out), _lib.ptr(area), _lib.stream())
