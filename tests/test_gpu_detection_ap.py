"""GPU: fp_detection_match and fp_detection_ap (csrc/detection_ap.hip) against the numpy restatement of
tests/detection_ap_ref.py -- exactly: integer outputs with np.array_equal, fp64 outputs by their bit patterns.  The shapes are the ones
at which the kernels take another path: a lane's second GT instance (65) and the cap (256), no GT at all, more estimates than lanes;
objects of 255 / 256 / 257 estimates around the 256-wide chunk, several chunks (1000), none; recalls that land on a threshold."""

import numpy as np
import pytest
import torch

from foundpose_amd import eval_bop24
from tests import detection_ap_ref as ref

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _group(rng, E, G, ths_row, typ_scale=(1.0, 1.0)):
    """Errors of one group [E * G, 2] on a coarse lattice, so that equal errors in one row and errors EQUAL to a threshold are common, with
    NaN and +inf sprinkled in; validity from the seed."""
    err = np.stack([rng.integers(0, 24, size=E * G).astype(np.float64) * s for s in typ_scale], axis=1)
    if err.size:
        err[rng.random(E * G) < 0.03, 0] = NAN
        err[rng.random(E * G) < 0.03, 1] = INF
        err[rng.random(E * G) < 0.02] = NAN
    return err, (rng.random(G) < 0.7).astype(np.int64)


def _batch(groups):
    """[(err [E G, 2], valid [G], E, tab)] -> fp_detection_match's host tables."""
    est_off, gt_off, pair_off, errs, valid, tab = [0], [0], [0], [], [], []
    for err, v, E, t in groups:
        G = len(v)
        est_off.append(est_off[-1] + E)
        gt_off.append(gt_off[-1] + G)
        pair_off.append(pair_off[-1] + E * G)
        errs.append(err.reshape(-1, 2))
        valid.append(v)
        tab.append(t)
    return (np.array(est_off), np.array(gt_off), np.array(pair_off), np.concatenate(errs) if errs else np.zeros((0, 2)),
            np.concatenate(valid).astype(np.int64) if valid else np.zeros(0, np.int64), np.array(tab, np.int64))


def _match(tables, ths):
    est_off, gt_off, pair_off, err, valid, tab = tables
    flag, matched = eval_bop24.match_groups(torch.from_numpy(err).cuda(), est_off, gt_off, pair_off, valid, tab, ths)
    return flag.cpu().numpy(), matched.cpu().numpy()


SHAPES = [(E, G) for G in (0, 1, 64, 65, 256) for E in (1, 5, 300)]


@pytest.fixture(scope="module")
def match_case():
    """Every (E, G) shape as one group of ONE batch, T = 10; groups 0 and 1 share threshold row 0, the others alternate between the rows.
    Thresholds are lattice values, so an error equal to its threshold occurs in every column."""
    rng = np.random.default_rng(24)
    ths = np.stack([np.stack([np.arange(2, 22, 2, dtype=np.float64), np.arange(2, 22, 2, dtype=np.float64) * 0.5]),
                    np.stack([np.arange(1, 11, dtype=np.float64), np.arange(3, 23, 2, dtype=np.float64) * 0.5])])
    groups = []
    for n, (E, G) in enumerate(SHAPES):
        err, v = _group(rng, E, G, None, (1.0, 0.5))
        groups.append((err, v, E, 0 if n < 2 else n % 2))
    tables = _batch(groups)
    return groups, tables, ths, ref.match_batch(*tables, ths)


def test_match_equals_the_restatement_at_every_shape(match_case):
    groups, tables, ths, (want_flag, want_matched) = match_case
    flag, matched = _match(tables, ths)
    assert flag.dtype == np.int8 and matched.dtype == np.int32 and flag.shape == (tables[0][-1], 20)
    for n, (E, G) in enumerate(SHAPES):
        e0, e1 = tables[0][n], tables[0][n + 1]
        assert np.array_equal(matched[e0:e1], want_matched[e0:e1]), (E, G)
        assert np.array_equal(flag[e0:e1], want_flag[e0:e1]), (E, G)
    # the case holds what it is meant to hold: all three flags, an error equal to its threshold, NaN and +inf, a tie inside a row
    assert set(np.unique(flag)) == {0, 1, 2} and (matched >= 64).any() and (matched >= 192).any()
    err = tables[3]
    assert np.isnan(err).any() and np.isinf(err).any() and (err[:, 0] == ths[0, 0, 3]).any()


def test_match_with_one_threshold_and_the_named_contents():
    """T = 1 (two columns), and the contents the rule names, each in a group of its own."""
    ths = np.array([[[5.0], [5.0]]])
    two = lambda rows: np.repeat(np.asarray(rows, np.float64).reshape(-1, 1), 2, axis=1)
    groups = [(two([3.0, 1.0, 1.0, 0.5, 0.1, 2.0, 9.0, 9.0, 9.0]), np.array([1, 1, 1]), 3, 0),       # equal errors in one row -> the lower index
              (two([5.0, 7.0]), np.array([1, 1]), 1, 0),                                            # equal to the threshold: no match
              (two([np.nextafter(5.0, 0.0), 7.0]), np.array([1, 1]), 1, 0),
              (two([NAN, 4.0, NAN, INF]), np.array([1, 1]), 2, 0),
              (two([1.0, 2.0, 1.5, 9.0]), np.array([0, 1]), 2, 0),                                  # the best match is invalid: ignored, and used up
              (np.zeros((0, 2)), np.zeros(0, np.int64), 2, 0)]                                      # no GT
    tables = _batch(groups)
    flag, matched = _match(tables, ths)
    assert matched[:, 0].tolist() == [1, 0, -1, -1, 0, 1, -1, 0, -1, -1, -1] and np.array_equal(matched[:, 0], matched[:, 1])
    assert flag[:, 0].tolist() == [1, 1, 0, 0, 1, 1, 0, 2, 0, 0, 0]
    want = ref.match_batch(*tables, ths)
    assert np.array_equal(flag, want[0]) and np.array_equal(matched, want[1])


def test_a_group_alone_equals_the_group_in_a_shuffled_batch(match_case):
    groups, tables, ths, _ = match_case
    flag, matched = _match(tables, ths)
    perm = np.random.default_rng(5).permutation(len(groups))
    shuffled = _batch([groups[i] for i in perm])
    sflag, smatched = _match(shuffled, ths)
    for at, i in enumerate(perm):
        a0, a1, b0, b1 = tables[0][i], tables[0][i + 1], shuffled[0][at], shuffled[0][at + 1]
        assert np.array_equal(flag[a0:a1], sflag[b0:b1]) and np.array_equal(matched[a0:a1], smatched[b0:b1]), SHAPES[i]
    i = SHAPES.index((300, 65))
    alone = _match(_batch([groups[i]]), ths)
    assert np.array_equal(alone[0], flag[tables[0][i]:tables[0][i + 1]]) and np.array_equal(alone[1], matched[tables[0][i]:tables[0][i + 1]])


# ---------------------------------------------------------------------------------------------------- average precision
SIZES, VALIDS = (0, 1, 255, 256, 257, 1000), (0, 1, 4, 100)


@pytest.fixture(scope="module")
def ap_case():
    """One object per (number of estimates, n_valid), plus one whose estimates are all ignored and one that is all true positives; T = 1.
    The rows of an object are scattered over the flag table, so `order` is a real indirection.  Column 0: mostly true positives (the recalls
    pass every threshold), column 1: mostly false."""
    rng = np.random.default_rng(101)
    sizes = [n for n in SIZES for _ in VALIDS] + [300, 100]
    n_valid = [v for _ in SIZES for v in VALIDS] + [4, 100]
    N = sum(sizes)
    flag = np.stack([rng.choice([0, 1, 2], size=N, p=[0.25, 0.6, 0.15]), rng.choice([0, 1, 2], size=N, p=[0.7, 0.2, 0.1])], axis=1).astype(np.int8)
    rows = rng.permutation(N)
    obj_off = np.concatenate([[0], np.cumsum(sizes)])
    flag[rows[obj_off[-3]:obj_off[-2]]] = 2          # all ignored
    flag[rows[obj_off[-2]:obj_off[-1]]] = 1          # all true, n_valid = 100: r_k = k / 100 against linspace's rounded values
    return obj_off, rows, flag, np.array(n_valid)


@pytest.mark.parametrize("R", [101, 1])
def test_ap_equals_the_restatement_bit_for_bit(ap_case, R):
    obj_off, rows, flag, n_valid = ap_case
    rec_thr = ref.REC_THR if R == 101 else np.array([0.5])
    ap, q, totals = (x.cpu().numpy() for x in eval_bop24.ap_objects(torch.from_numpy(flag).cuda(), obj_off, rows, n_valid, rec_thr))
    want_ap, want_q, want_totals = ref.ap_batch(obj_off, rows, flag, n_valid, rec_thr)
    assert ap.shape == (len(n_valid), 2) and q.shape == (len(n_valid), 2, R) and totals.dtype == np.int32
    assert np.array_equal(totals, want_totals)
    for o in range(len(n_valid)):
        assert np.array_equal(_bits(q[o]), _bits(want_q[o])), (o, obj_off[o + 1] - obj_off[o], n_valid[o])
        assert np.array_equal(_bits(ap[o]), _bits(want_ap[o])), (o, obj_off[o + 1] - obj_off[o], n_valid[o])
    assert (ap[n_valid == 0] == -1.0).all() and (ap[(n_valid > 0) & (np.diff(obj_off) == 0)] == 0.0).all()
    assert (ap[-2] == 0.0).all() and totals[-2, :, 2].tolist() == [300, 300]      # all ignored
    if R == 101:
        assert (ap[-1] == 1.0).all()                                            # 100 true positives of 100: every threshold is reached
        assert len(np.unique(ap[n_valid > 0])) > 10                             # and the random objects give many different values


def test_ap_with_ten_thresholds_per_type():
    """C = 20 columns over one flag table: every workgroup reads its own column."""
    rng = np.random.default_rng(7)
    flag = rng.choice([0, 1, 2], size=(700, 20), p=[0.4, 0.5, 0.1]).astype(np.int8)
    obj_off, rows, n_valid = np.array([0, 300, 300, 700]), rng.permutation(700), np.array([100, 3, 4])
    ap, q, totals = (x.cpu().numpy() for x in eval_bop24.ap_objects(torch.from_numpy(flag).cuda(), obj_off, rows, n_valid))
    want = ref.ap_batch(obj_off, rows, flag, n_valid)
    assert np.array_equal(_bits(ap), _bits(want[0])) and np.array_equal(_bits(q), _bits(want[1])) and np.array_equal(totals, want[2])


# ---------------------------------------------------------------------------------------------------- refusals
def test_bad_tables_are_refused_before_any_launch():
    ths = np.ones((1, 2, 10))
    err = torch.zeros(257, 2, dtype=torch.float64, device="cuda")
    ok = dict(err=err, est_off=[0, 1], gt_off=[0, 256], pair_off=[0, 256], gt_valid=np.ones(257, np.int64), group_tab=[0], ths=ths)
    eval_bop24.match_groups(**ok)
    for bad in (dict(gt_off=[0, 257], pair_off=[0, 257]),                  # G_g = 257
                dict(ths=np.ones((1, 2, 17))),                              # T = 17
                dict(est_off=[1, 0]), dict(gt_off=[256, 0]), dict(pair_off=[256, 0]),   # offsets not ascending
                dict(err=err.cpu()),                                        # a CPU tensor
                dict(pair_off=[0, 255]), dict(group_tab=[1]), dict(err=err.float()), dict(gt_valid=np.ones(10, np.int64))):
        with pytest.raises(ValueError):
            eval_bop24.match_groups(**dict(ok, **bad))
    flag = torch.zeros(4, 2, dtype=torch.int8, device="cuda")
    ok = dict(flag=flag, obj_off=[0, 4], order=[0, 1, 2, 3], n_valid=[2])
    eval_bop24.ap_objects(**ok)
    for bad in (dict(flag=flag.cpu()), dict(obj_off=[4, 0]), dict(order=[0, 1, 2, 4]), dict(rec_thr=np.zeros(129)), dict(rec_thr=np.zeros(0)),
                dict(flag=torch.zeros(4, 34, dtype=torch.int8, device="cuda")), dict(n_valid=[2, 2]), dict(obj_off=[0, 5])):
        with pytest.raises(ValueError):
            eval_bop24.ap_objects(**dict(ok, **bad))
    from foundpose_amd import ops
    with pytest.raises(ValueError):
        ops.detection_ap(torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), flag.cpu(), torch.zeros(1, dtype=torch.int32),
                         torch.zeros(1, dtype=torch.float64))
