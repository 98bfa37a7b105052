"""CPU: the numpy restatement of fp_pose_add_errors (tests/pose_add_ref.py) against scipy's k-d tree, and eval_add's host protocol: the AUC's
hand values, the matching rules, the error-type rule and the refusals that need no device.  The device is compared with the restatement bit for
bit in tests/test_gpu_pose_add.py."""

import math

import numpy as np
import pytest

from foundpose_amd import eval_add
from tests import pose_add_ref as ref

SIZES = (1, 255, 256, 257, 1500)


def _rot(rng):
    w, x, y, z = (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _cases():
    rng = np.random.default_rng(0)
    out = []
    for M in SIZES:
        pts = rng.normal(size=(M, 3)) * 40.0
        Rg, tg = _rot(rng), np.array([30.0, -20.0, 900.0])
        for k in range(3):   # the GT pose shifted, another rotation shifted, another rotation in place
            Re = _rot(rng) if k else Rg
            te = tg + rng.normal(size=3) * (5.0 if k < 2 else 0.0)
            out.append((pts, np.concatenate([Re.ravel(), te]), np.concatenate([Rg.ravel(), tg])))
    return out


def test_restatement_agrees_with_the_kd_tree_and_adi_is_at_most_add():
    from scipy.spatial import cKDTree
    for pts, est, gt in _cases():
        add, adi = ref.pair_errors(pts, est, gt)
        E, G = ref.place(est, pts), ref.place(gt, pts)
        d, _ = cKDTree(E).query(G, k=1)                      # pose_error.adi: the tree on the estimate's points, queried with the GT's
        # 1e-9 relative: the bar DESIGN section 9 uses where the other side's summation order is not pinned (d.mean() is pairwise)
        assert abs(d.mean() - adi) <= 1e-9 * d.mean()
        assert abs(np.linalg.norm(G - E, axis=1).mean() - add) <= 1e-9 * add
        # every point's nearest neighbour is at most as far as its own counterpart, value by value, and the two sums share one order
        assert adi <= add
    err = ref.batch_errors(np.concatenate([c[0] for c in _cases()[:4]]), np.stack([c[1] for c in _cases()[:4]]), np.stack([c[2] for c in _cases()[:4]]),
                           [(0, 1), (1, 1), (2, 1), (3, 255)])
    assert err.shape == (4, 2) and np.array_equal(err[3], ref.pair_errors(*_cases()[3]))


def test_a_nan_never_wins_the_minimum():
    G = np.array([[0.0, 0.0, 0.0]])
    E = np.array([[np.nan, 0.0, 0.0], [3.0, 4.0, 0.0], [np.nan, np.nan, np.nan]])
    assert ref.nn_sq(G, E)[0] == 25.0
    assert ref.nn_sq(G, E[:1])[0] == np.inf


@pytest.mark.parametrize("fn", [eval_add.auc, ref.auc], ids=["eval_add", "restatement"])
def test_auc_hand_values(fn):
    assert fn([0, 0, 0], 100) == 1.0
    assert fn([50, 200], 100) == 0.5
    assert fn([150], 100) == 0.0
    assert fn([25, 25, 75, np.inf], 100) == 0.625
    assert fn([], 100) == 0.0 and fn([np.nan, np.inf], 100) == 0.0
    # one of two at 40: the step from 0 to 40 counts with the accuracy reached at 40 (VOCap's rectangles), so 0.5 over the whole range
    assert fn([np.inf, 40.0], 100) == 0.5
    # the threshold itself is kept (d <= auc_max): accuracy 0.5 at 50, 1 at 100 -> (50 x 0.5 + 50 x 1) / 100
    assert fn([100.0, 50.0], 100) == 0.75


def test_auc_of_random_errors_equals_the_restatement():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 50):
        d = rng.uniform(0, 150, n)
        d[rng.integers(0, n)] = np.inf
        d = np.concatenate([d, d[:2]])   # repeated values: mrec does not change there
        assert eval_add.auc(d, 100.0) == ref.auc(d, 100.0)


@pytest.mark.parametrize("fn", [lambda e: eval_add.match_target(np.asarray(e, float).reshape(len(e), -1)).tolist(), ref.match], ids=["eval_add", "restatement"])
def test_matching_rules(fn):
    # a tie goes to the lower GT id
    assert fn(np.array([[2.0, 1.0, 1.0]])) == [-1, 0, -1]
    # the better-scored estimate chooses first; the second takes what is left although the taken one is nearer to it
    assert fn(np.array([[1.0, 5.0], [0.5, 9.0]])) == [0, 1]
    # more estimates than GT instances: the last one gets nothing
    assert fn(np.array([[1.0], [0.1]])) == [0]
    # inf and NaN errors still match (there is no threshold): to the lowest free GT
    assert fn(np.array([[np.inf, np.nan]])) == [0, -1]


def _tables(err, valid, n_est, sym=False):
    return {"targets": [{"obj_id": 1, "n_est": n_est, "valid": np.array(valid, bool), "pair_off": 0}], "err": np.asarray(err, np.float64),
            "symmetric": {1: sym}, "diameters": {1: 100.0}}


def test_an_invalid_gt_is_consumed_and_an_unmatched_valid_gt_is_inf():
    # one estimate, two GT instances; the estimate is nearer to the invalid one and takes it: the valid one stays unmatched
    tb = _tables([[1.0, 0.5], [4.0, 3.0]], [False, True], 1)
    inst = eval_add.instance_errors(tb["targets"], tb["err"], tb["symmetric"])
    assert inst[1].tolist() == [[math.inf, math.inf, math.inf]]
    s = eval_add.summarize(inst, tb["diameters"], 0.1, 100.0)
    assert s["all"] == {"recall_add_s": 0.0, "auc_add": 0.0, "auc_adi": 0.0, "auc_add_s": 0.0} == ref.summarize(tb)["all"]
    # the other way round: the valid instance is matched with its own errors
    tb = _tables([[1.0, 0.5], [4.0, 3.0]], [True, False], 1)
    inst = eval_add.instance_errors(tb["targets"], tb["err"], tb["symmetric"])
    assert inst[1].tolist() == [[1.0, 0.5, 1.0]]
    assert eval_add.summarize(inst, tb["diameters"], 0.1, 100.0) == ref.summarize(tb)
    # no estimate at all
    tb = _tables(np.zeros((0, 2)), [True], 0)
    assert eval_add.instance_errors(tb["targets"], tb["err"], tb["symmetric"])[1].tolist() == [[math.inf] * 3]


def test_a_symmetric_object_is_matched_and_scored_by_adi():
    # by ADD the estimate prefers GT 0, by ADI GT 1
    err = [[1.0, 0.9], [2.0, 0.1]]
    for sym, want in ((False, [[1.0, 0.9, 1.0], [math.inf] * 3]), (True, [[math.inf] * 3, [2.0, 0.1, 0.1]])):
        tb = _tables(err, [True, True], 1, sym)
        inst = eval_add.instance_errors(tb["targets"], tb["err"], tb["symmetric"])
        assert inst[1].tolist() == want
        assert eval_add.summarize(inst, tb["diameters"], 0.1, 100.0) == ref.summarize(tb)
    # the recall compares strictly: an error of exactly recall_factor x diameter is not correct
    tb = _tables([[10.0, 10.0]], [True], 1)
    s = eval_add.summarize(eval_add.instance_errors(tb["targets"], tb["err"], tb["symmetric"]), tb["diameters"], 0.1, 100.0)
    assert s["all"]["recall_add_s"] == 0.0 and s["all"]["auc_add"] == 1.0


@pytest.mark.parametrize("fn", [eval_add.is_symmetric, ref.is_symmetric], ids=["eval_add", "restatement"])
def test_error_type_rule(fn):
    assert not fn({"diameter": 1.0}, 3)
    assert not fn({"diameter": 1.0, "symmetries_discrete": [], "symmetries_continuous": []}, 3)
    assert fn({"symmetries_discrete": [list(range(16))]}, 3)
    assert fn({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 3)
    assert fn({"diameter": 1.0}, 3, [1, 3]) and not fn({"diameter": 1.0}, 3, [1, 2]) and not fn({"diameter": 1.0}, 3, [])


def test_options_are_refused_before_anything_is_read(tmp_path):
    missing = str(tmp_path / "none.csv")
    for kw in (dict(recall_factor=0.0), dict(recall_factor=-0.1), dict(recall_factor=math.nan), dict(auc_max=0.0), dict(auc_max=math.inf),
               dict(recall_factor="0.1")):
        with pytest.raises(ValueError):
            eval_add.evaluate_add(missing, str(tmp_path), [], str(tmp_path), **kw)
    with pytest.raises(SystemExit):
        eval_add.main(["--result-csv", missing])   # --dataset-dir and --output are required


def test_tables_are_refused_without_a_device():
    import torch

    from foundpose_amd import ops
    pts, pose = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(1, 12, dtype=torch.float64)
    with pytest.raises(ValueError, match="device tensor"):
        ops.pose_add_errors(pts, pose, pose, [(0, 4)])
