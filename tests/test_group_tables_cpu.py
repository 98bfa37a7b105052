"""CPU: foundpose_amd.group_tables -- the one check of the group tables that eval_bop24.match_groups and eval_coco.match_groups share, on
plain numpy, and the kernels' limits against the C header."""

import os
import re

import numpy as np
import pytest

from foundpose_amd import group_tables as gt

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "foundpose_amd.h")


def check(est_off, gt_off, pair_off, num_per_gt, num_rows):
    return gt.check_groups("match_groups", est_off, gt_off, pair_off, num_per_gt, num_rows, "err")


def test_the_limits_are_the_headers():
    with open(HEADER) as f:
        macros = {k: int(v) for k, v in re.findall(r"^#define\s+FP_DETECTION_(MAX_\w+)\s+(\d+)", f.read(), re.M)}
    assert macros == {"MAX_THS": gt.MAX_THS, "MAX_GROUP_GT": gt.MAX_GROUP_GT, "MAX_REC": gt.MAX_REC}


def test_every_header_of_csrc_is_a_build_dependency():
    """An edit of a shared header must rebuild the objects that include it: group_parts.hpp like every other."""
    from foundpose_amd import build
    csrc = os.path.join(os.path.dirname(HEADER), os.pardir, "foundpose_amd", "csrc")
    assert "group_parts.hpp" in build.HEADERS
    assert sorted(f for f in os.listdir(csrc) if f.endswith(".hpp")) == sorted(h for h in build.HEADERS if os.sep not in h)


def test_sound_tables_come_back_as_int64():
    est, g, pair, NG = check(np.array([0, 2, 2, 5], np.int32), [0, 3, 4, 4], [0, 6, 6, 6], 4, 6)
    assert NG == 3 and all(t.dtype == np.int64 for t in (est, g, pair))
    assert est.tolist() == [0, 2, 2, 5] and g.tolist() == [0, 3, 4, 4] and pair.tolist() == [0, 6, 6, 6]
    assert check([0, 1], [0, 4], [0, 4], 9, 7)[3] == 1          # more per-GT entries and rows than the tables reach: fine
    assert check([3, 4], [2, 4], [1, 3], 4, 3)[3] == 1          # tables need not start at 0


def test_a_group_of_256_instances_is_taken_and_257_is_not():
    assert check([0, 1, 2], [0, 1, 257], [0, 1, 257], 257, 257)[3] == 2
    with pytest.raises(ValueError, match=r"match_groups: group 1 has 257 GT instances \(at most 256\)"):
        check([0, 1, 2], [0, 1, 258], [0, 1, 258], 258, 258)


def test_no_group():
    est, g, pair, NG = check([0], [0], [0], 0, 0)
    assert NG == 0 and est.tolist() == [0]
    with pytest.raises(ValueError, match="at least one entry"):
        check([], [], [], 0, 0)


@pytest.mark.parametrize("tables, match", [
    (([0, 2], [0, 2, 2], [0, 4]), "same length"),                          # unequal lengths
    (([0, 2], [0, 2], [0, 4, 4]), "same length"),
    (([0, 2, 1], [0, 2, 2], [0, 4, 4]), "est_off must .* ascend"),         # descending offsets
    (([0, 2], [2, 0], [0, 4]), "gt_off must .* ascend"),
    (([0, 2], [0, 2], [4, 0]), "pair_off must .* ascend"),
    (([-1, 1], [0, 2], [0, 4]), "est_off must .* start at >= 0"),          # a first offset below 0
    (([0.0, 2.0], [0, 2], [0, 4]), "est_off must be a 1-D integer table"), # a non-integer table
    (([0, 2], [[0, 2]], [0, 4]), "gt_off must be a 1-D integer table"),
    (([0, 2], [0, 2], [0, 2**31]), "pair_off does not fit int32"),         # a value past int32
    (([0, 2], [0, 3], [0, 6]), "gt_off reaches 3, .* has 2 entries"),      # gt_off[-1] past the per-GT table
    (([0, 2], [0, 2], [0, 3]), "must own E_g x G_g rows of err"),          # pair_off that is not E * G
    (([0, 2, 3], [0, 1, 2], [0, 2, 4]), "must own E_g x G_g rows of err"),
    (([0, 3], [0, 2], [0, 6]), "must own E_g x G_g rows of err"),          # pair_off[-1] past the rows
])
def test_refusals(tables, match):
    with pytest.raises(ValueError, match=match):
        check(*tables, 2, 4)
