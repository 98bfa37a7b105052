"""GPU: fp_coco_match (csrc/coco_eval.hip) against the sequential loop of tests/coco_ref.py: flags and matched
indices by equality."""

import numpy as np
import pytest
import torch

from tests import coco_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda"
VALUES = np.array([0.0, 0.25, 0.5, np.nextafter(0.5, 0), 0.55, 0.6, 2.0 / 3.0, 0.75, 0.95, np.nextafter(0.95, 1), 1.0])


def run(groups, ths):
    """groups: [(overlap [E, G], ignore [G])] -> (flag, matched) of one fp_coco_match call, as numpy."""
    from foundpose_amd import eval_coco
    est_off = np.cumsum([0] + [np.asarray(o).shape[0] for o, _ in groups])
    gt_off = np.cumsum([0] + [len(i) for _, i in groups])
    pair_off = np.cumsum([0] + [np.asarray(o).shape[0] * len(i) for o, i in groups])
    flat = np.concatenate([np.asarray(o, np.float64).reshape(-1) for o, _ in groups]) if groups else np.zeros(0)
    ign = np.concatenate([np.asarray(i, np.int64).reshape(-1) for _, i in groups]) if groups else np.zeros(0, np.int64)
    flag, matched = eval_coco.match_groups(torch.from_numpy(flat).to(DEV), est_off, gt_off, pair_off, ign, ths)
    return flag.cpu().numpy(), matched.cpu().numpy(), est_off


def check(groups, ths):
    flag, matched, est_off = run(groups, ths)
    assert flag.shape == (est_off[-1], len(ths)) and flag.dtype == np.int8 and matched.dtype == np.int32
    for g, (ov, ign) in enumerate(groups):
        f, m = cr.match(np.asarray(ov, np.float64).reshape(-1, len(ign)) if len(ign) else np.zeros((np.asarray(ov).shape[0], 0)), [bool(v) for v in ign], ths)
        sl = slice(est_off[g], est_off[g + 1])
        assert np.array_equal(flag[sl], f) and np.array_equal(matched[sl], m), g
    return flag, matched, est_off


def test_hand_made_tables():
    below = np.nextafter(0.5, 0)
    groups = [
        (np.array([[0.5, below]]), [0, 0]),                 # 0: exactly at the threshold matches ...
        (np.array([[below]]), [0]),                          # 1: ... the next double below does not
        (np.array([[0.7, 0.7, 0.1]]), [0, 0, 0]),            # 2: equal overlaps go to the higher index
        (np.array([[0.6, 0.9]]), [0, 1]),                    # 3: a regular instance at 0.6 beats an ignored one at 0.9
        (np.array([[0.2, 0.9], [0.2, 0.9]]), [0, 1]),        # 4: only an ignored candidate: flag 2, and it is used up
        (np.zeros((3, 0)), []),                              # 5: G = 0
        (np.zeros((0, 2)), [0, 1]),                          # 6: E = 0
        (np.array([[0.8, 0.6], [0.8, 0.6]]), [0, 0]),        # 7: the second estimate takes what is left
    ]
    flag, matched, off = check(groups, [0.5])
    assert (flag[off[0], 0], matched[off[0], 0]) == (1, 0) and (flag[off[1], 0], matched[off[1], 0]) == (0, -1)
    assert matched[off[2], 0] == 1 and (flag[off[3], 0], matched[off[3], 0]) == (1, 0)
    assert flag[off[4]:off[5], 0].tolist() == [2, 0] and matched[off[4]:off[5], 0].tolist() == [1, -1]
    assert flag[off[5]:off[6], 0].tolist() == [0, 0, 0] and matched[off[7]:off[8], 0].tolist() == [0, 1]
    flag, matched, _ = check([(np.array([[1.0, np.nextafter(1.0, 0)]]), [0, 0])], [1.0])     # threshold 1 matches exactly 1, through 1 - 1e-10
    assert (flag[0, 0], matched[0, 0]) == (1, 0)
    check(groups, cr.IOU_THS)                                # T = 10
    check(groups, np.linspace(0.05, 1.0, 16))                # T = 16


def test_random_tables_with_ties():
    rng = np.random.default_rng(5)
    groups = []
    for _ in range(300):
        E, G = int(rng.integers(0, 9)), int(rng.integers(0, 9))
        groups.append((VALUES[rng.integers(0, len(VALUES), (E, G))], sorted(int(v) for v in rng.integers(0, 2, G))))
    flag, matched, off = check(groups, cr.IOU_THS)
    assert (flag == 1).any() and (flag == 2).any() and (flag == 0).any()
    for g in (3, 77, 150, 299):                              # a group alone gives the bytes it gave in the batch
        f1, m1, _ = run([groups[g]], cr.IOU_THS)
        assert np.array_equal(f1, flag[off[g]:off[g + 1]]) and np.array_equal(m1, matched[off[g]:off[g + 1]])


def test_a_group_of_256_by_256():
    rng = np.random.default_rng(6)
    ov = VALUES[rng.integers(0, len(VALUES), (256, 256))]
    ign = [0] * 200 + [1] * 56
    flag, matched, _ = check([(ov, ign), (ov[:5, :70], ign[:70])], [0.5, 0.75, 0.95])
    got = [int(v) for v in matched[:256, 0] if v >= 0]
    assert len(got) > 200 and len(set(got)) == len(got)                                      # no instance is used twice


@pytest.mark.parametrize("num_groups, empty_last", [(1, False), (5, False), (6, True)])
def test_waves_of_the_last_workgroup(num_groups, empty_last):
    """One wave per (group, threshold), four to a workgroup, T = 1: NG T = 1 leaves three idle waves in the only workgroup, 5 puts one
    live wave into a second one, and in 6 the last live wave's group has no estimate.  Every case holds a matched and an unmatched estimate."""
    rng = np.random.default_rng(40 + num_groups)
    groups = []
    for g in range(num_groups):
        E, G = int(rng.integers(2, 9)), int(rng.integers(1, 9))
        ov = VALUES[rng.integers(0, len(VALUES), (E, G))]
        ov[0, 0], ov[1, :] = 0.75, 0.25                      # estimate 0 finds an instance, estimate 1 none
        groups.append((ov, sorted(int(v) for v in rng.integers(0, 2, G))))
    if empty_last:
        groups[-1] = (np.zeros((0, 3)), [0, 0, 1])
    flag, matched, off = check(groups, [0.5])
    assert flag[0, 0] in (1, 2) and matched[0, 0] >= 0 and (flag[1, 0], matched[1, 0]) == (0, -1)
    assert off[-1] == flag.shape[0] and (not empty_last or off[-1] == off[-2])


def test_refused_before_any_launch():
    from foundpose_amd import eval_coco
    ov = torch.zeros(4, dtype=torch.float64, device=DEV)
    ok = ([0, 2], [0, 2], [0, 4], [0, 0])
    for ths in (np.linspace(0.05, 0.9, 17), [0.0], [0.5, 1.0001], [float("nan")], []):
        with pytest.raises(ValueError):
            eval_coco.match_groups(ov, *ok, ths)
    big = torch.zeros(257, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="256"):
        eval_coco.match_groups(big, [0, 1], [0, 257], [0, 257], [0] * 257)
    with pytest.raises(ValueError):
        eval_coco.match_groups(ov, [0, 2], [0, 2], [0, 3], [0, 0])          # the pairs are not E x G
    with pytest.raises(ValueError):
        eval_coco.match_groups(ov, [0, 2], [0, 2], [0, 4], [0])             # gt_off reaches beyond gt_ignore
    with pytest.raises(ValueError):
        eval_coco.match_groups(ov.float(), *ok)
    f, m = eval_coco.match_groups(ov, *ok, [0.5])
    assert f.cpu().numpy().tolist() == [[0], [0]] and m.cpu().numpy().tolist() == [[-1], [-1]]
