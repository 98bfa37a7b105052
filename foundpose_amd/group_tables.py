"""The host side of the group tables the two AP scorers share (eval_bop24, eval_coco; csrc/group_parts.hpp reads them on the device): the
kernels' limits, the checks of the tables and their upload."""

from typing import Optional, Sequence, Tuple

import numpy as np

MAX_THS = 16         # FP_DETECTION_MAX_THS of include/foundpose_amd.h: thresholds per error type (or IoU thresholds)
MAX_GROUP_GT = 256   # FP_DETECTION_MAX_GROUP_GT: GT instances of one (image, object) group
MAX_REC = 128        # FP_DETECTION_MAX_REC: recall thresholds


def int32_table(name: str, a, size: Optional[int] = None) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)) or (size is not None and a.size != size):
        raise ValueError(f"{name} must be a 1-D integer table" + (f" of {size} entries" if size is not None else "") + f", got {a.dtype} {a.shape}")
    a = a.astype(np.int64)
    if a.size and (int(a.min()) < -2**31 or int(a.max()) > 2**31 - 1):
        raise ValueError(f"{name} does not fit int32")
    return a


def offsets(name: str, a) -> np.ndarray:
    a = int32_table(name, a)
    if a.size < 1 or int(a[0]) < 0 or np.any(np.diff(a) < 0):
        raise ValueError(f"{name} must hold at least one entry, start at >= 0 and ascend")
    return a


def upload(tables: Sequence[np.ndarray], dtype, device):
    """Host tables of one dtype -> device views of ONE pinned upload."""
    import torch

    from . import _lib
    sizes = [int(t.size) for t in tables]
    flat = np.concatenate([np.asarray(t, dtype).reshape(-1) for t in tables]) if sum(sizes) else np.zeros(0, dtype)
    dev = _lib.upload_async(torch.from_numpy(flat), device)
    out, pos = [], 0
    for n in sizes:
        out.append(dev[pos:pos + n])
        pos += n
    return out


def check_groups(who: str, est_off, gt_off, pair_off, num_per_gt: int, num_rows: int, rows_name: str,
                 per_gt_name: str = "the per-GT table") -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """The three offset tables of NG groups, checked (ValueError): [NG + 1] each, ascending from >= 0 and within int32; group g owns E_g
    estimates, G_g <= MAX_GROUP_GT of the `num_per_gt` GT instances and the E_g G_g rows from pair_off[g] of the `num_rows` rows of
    `rows_name`.  -> (est_off, gt_off, pair_off) as int64, NG."""
    est_off, gt_off, pair_off = offsets("est_off", est_off), offsets("gt_off", gt_off), offsets("pair_off", pair_off)
    NG = est_off.size - 1
    if gt_off.size != NG + 1 or pair_off.size != NG + 1:
        raise ValueError(f"{who}: est_off, gt_off and pair_off must have the same length")
    E, G = np.diff(est_off), np.diff(gt_off)
    if NG and int(G.max()) > MAX_GROUP_GT:
        raise ValueError(f"{who}: group {int(np.argmax(G))} has {int(G.max())} GT instances (at most {MAX_GROUP_GT})")
    if int(gt_off[-1]) > num_per_gt:
        raise ValueError(f"{who}: gt_off reaches {int(gt_off[-1])}, {per_gt_name} has {num_per_gt} entries")
    if np.any(np.diff(pair_off) != E * G) or int(pair_off[-1]) > num_rows:
        raise ValueError(f"{who}: group g must own E_g x G_g rows of {rows_name} from pair_off[g]")
    return est_off, gt_off, pair_off, NG
