"""numpy restatement of fp_gt_visibility (csrc/gt_info.hip) and of gt_info's record assembly, in the operation order of bop_toolkit's
calc_gt_info.py / calc_gt_masks.py as published (the toolkit is not installed here): misc.depth_im_to_dist_im_fast,
visibility.estimate_visib_mask_gt in `bop19` mode, nonzero() min / max and misc.calc_2d_bbox."""
import numpy as np

from tests.vsd_ref import dist_im

INT_MAX, INT_MIN = 2**31 - 1, -2**31
EMPTY_BOX = [INT_MAX, INT_MAX, INT_MIN, INT_MIN]


def visib_mask_gt(d_test: np.ndarray, d_gt: np.ndarray, delta) -> np.ndarray:
    """visibility.estimate_visib_mask_gt -> _estimate_visib_mask, bop19 mode: fp64 distance images, astype(float32) before the
    difference, the comparison against a float32 delta."""
    d_diff = d_gt.astype(np.float32) - d_test.astype(np.float32)
    return np.logical_and(np.logical_or(d_diff <= np.float32(delta), d_test == 0), d_gt > 0)


def _extent(mask: np.ndarray, ox: int, oy: int):
    """(min x, min y, max x, max y) of the set pixels, shifted by the offset; the kernel's empty box when there is none."""
    ys, xs = mask.nonzero()
    if xs.size == 0:
        return list(EMPTY_BOX)
    xs, ys = xs - ox, ys - oy
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def gt_visibility(depth_test: np.ndarray, depth_obj_large: np.ndarray, K, delta, ox: int, oy: int):
    """One instance: depth_test [H, W] fp32, depth_obj_large [Hr, Wr] fp32 holding the image at (ox, oy), K of the image
    -> (row [11] int64, mask [H, W] uint8, mask_visib [H, W] uint8), the kernel's outputs."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    depth_test = np.asarray(depth_test, np.float32)
    large = np.asarray(depth_obj_large, np.float32)
    h, w = depth_test.shape
    depth_gt = large[oy:oy + h, ox:ox + w]
    dist_test = dist_im(depth_test, K)
    dist_gt = dist_im(depth_gt, K)
    visib_gt = visib_mask_gt(dist_test, dist_gt, delta)
    obj_mask_gt_large = large > 0
    obj_mask_gt = dist_gt > 0
    px_count_all = int(np.sum(obj_mask_gt_large))
    px_count_valid = int(np.sum(dist_test[obj_mask_gt] > 0))
    px_count_visib = int(visib_gt.sum())
    row = [px_count_all, px_count_valid, px_count_visib] + _extent(obj_mask_gt_large, ox, oy) + _extent(visib_gt, 0, 0)
    return np.array(row, np.int64), obj_mask_gt.astype(np.uint8) * 255, visib_gt.astype(np.uint8) * 255


def calc_2d_bbox(x0: int, y0: int, x1: int, y1: int):
    """misc.calc_2d_bbox on the extremes: [x, y, w, h] with w = max x - min x (no + 1)."""
    return [int(x0), int(y0), int(x1 - x0), int(y1 - y0)]


def record(row) -> dict:
    """calc_gt_info.py's per-instance entry from a kernel row, in the toolkit's key order."""
    px_all, px_valid, px_visib = (int(v) for v in row[:3])
    bbox_obj, bbox_visib = [-1, -1, -1, -1], [-1, -1, -1, -1]
    if px_visib > 0:
        bbox_obj = calc_2d_bbox(*row[3:7])
        bbox_visib = calc_2d_bbox(*row[7:11])
    visib_fract = px_visib / float(px_all) if px_all > 0 else 0.0
    rec = {}
    rec["bbox_obj"] = bbox_obj
    rec["bbox_visib"] = bbox_visib
    rec["px_count_all"] = px_all
    rec["px_count_valid"] = px_valid
    rec["px_count_visib"] = px_visib
    rec["visib_fract"] = visib_fract
    return rec


def targets_bop19(records) -> list:
    """records: [(scene_id, im_id, obj_id, visib_fract)] -> one {scene_id, im_id, obj_id, inst_count} per image and object, inst_count
    the instances with visib_fract >= 0.1, entries with 0 left out, sorted."""
    count = {}
    for s, im, lid, vf in records:
        count[(s, im, lid)] = count.get((s, im, lid), 0) + (1 if vf >= 0.1 else 0)
    return [{"scene_id": s, "im_id": im, "obj_id": lid, "inst_count": n} for (s, im, lid), n in sorted(count.items()) if n > 0]
