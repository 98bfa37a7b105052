"""tests/kmeans_ref.py held to its own definition, without a GPU: the summation order, the distance stage on exact data, the split rule
worked by hand, the scenarios the GPU datasets were chosen for, and proof that those datasets tell wrong variants of the rule apart."""
import numpy as np
import pytest
import torch

from oracle import clib
from oracle import match as om
from tests import kmeans_ref as kr

F32 = np.float32


# ------------------------------------------------------------------------------------------------ sum order
def _means_scalar_loop(x, ids, k):
    """The definition, one scalar at a time."""
    sums = [[F32(0)] * x.shape[1] for _ in range(k)]
    counts = [0] * k
    for i in range(x.shape[0]):
        c = int(ids[i])
        counts[c] += 1
        for j in range(x.shape[1]):
            sums[c][j] = F32(sums[c][j] + x[i, j])
    means = [[F32(s / F32(max(counts[c], 1))) for s in sums[c]] for c in range(k)]
    return np.array(means, F32), np.array(counts, np.int64), np.array(sums, F32)


def _pairwise_sum(members):
    """numpy's own sum along the contiguous axis: unrolled and pairwise, not sequential."""
    return np.ascontiguousarray(members.T).sum(axis=1, dtype=F32)


def test_cluster_means_is_the_sequential_fp32_sum():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((257, 7)) * rng.choice([1e4, 1.0, 1e-3], size=(257, 7))).astype(F32)
    ids = rng.integers(0, 6, 257)
    ids[ids == 4] = 3  # an empty cluster
    got = kr.cluster_means(x, ids, 6)
    want = _means_scalar_loop(x, ids, 6)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert got[1][4] == 0 and not got[0][4].any()  # empty: sum 0 over max(0, 1)
    x, ids, k = kr.update_stage_case()
    for g, w in zip(kr.cluster_means(x, ids, k), _means_scalar_loop(x, ids, k)):
        assert np.array_equal(g, w)


def test_sum_order_is_visible():
    """[1e8, 1, -1e8, 1]: in sequence 1e8 + 1 rounds back to 1e8, so the chain ends at 1; the exact sum is 2.  Ascending sample order is
    part of the value: the same members as [1, 1, 1e8, -1e8] give 0."""
    x = np.array([[1e8], [1.0], [-1e8], [1.0]], F32)
    means, counts, sums = kr.cluster_means(x, np.zeros(4, np.int64), 1)
    assert sums[0, 0] == F32(1.0) and counts[0] == 4 and means[0, 0] == F32(0.25)
    assert F32(x.astype(np.float64).sum()) == F32(2.0)
    _, _, other = kr.cluster_means(x[[1, 3, 0, 2]], np.zeros(4, np.int64), 1)
    assert other[0, 0] == F32(0.0)
    # two clusters interleaved: each chain sees only its own members, in their order
    ids = np.array([0, 1, 0, 1])
    _, _, s2 = kr.cluster_means(np.array([[1e8], [1.0], [1.0], [1e8]], F32), ids, 2)
    assert s2[0, 0] == F32(1e8) and s2[1, 0] == F32(1e8)
    # the update-stage case of the GPU test is order-sensitive too: a pairwise numpy sum gives other bits somewhere
    x, ids, k = kr.update_stage_case()
    _, counts, sums = kr.cluster_means(x, ids, k)
    assert counts[2] == 0 and counts[5] == 1 and counts[1] > 0.6 * len(ids)
    pairwise = np.stack([_pairwise_sum(x[ids == c]) for c in range(k)])
    assert not np.array_equal(pairwise, sums)
    exact = np.stack([x[ids == c].astype(np.float64).sum(0).astype(F32) for c in range(k)])
    assert not np.array_equal(exact, sums)


# ------------------------------------------------------------------------------------------------ distance stage
def test_assign_on_lattice_data_is_the_exact_argmin():
    """Small integers: every product, norm and distance is an integer below 2^24, so the fp32 chain is exact and the restated assignment
    must be the float64 brute-force arg-min with ties to the lowest index."""
    x, k, _ = kr.dataset("lattice")
    c = kr.init_centroids(x, k, 0)
    ids, d2 = kr.assign(x, c)
    full = ((x[:, None, :].astype(np.float64) - c[None].astype(np.float64)) ** 2).sum(-1)
    assert np.array_equal(ids, full.argmin(1))  # np.argmin: first minimum
    assert np.array_equal(d2.astype(np.float64), full.min(1))
    s = np.sort(full, 1)
    assert int((s[:, 0] == s[:, 1]).sum()) > 0  # and ties do occur here


def test_init_centroids_is_the_cpu_randperm():
    x = np.arange(40, dtype=F32).reshape(20, 2)
    perm = torch.randperm(20, generator=torch.Generator(device="cpu").manual_seed(5))[:6].numpy()
    assert np.array_equal(kr.init_centroids(x, 6, 5), x[perm])
    assert not np.array_equal(kr.init_centroids(x, 6, 5), kr.init_centroids(x, 6, 6))


# ------------------------------------------------------------------------------------------------ split rule
def test_split_empty_hand_worked():
    """counts [0, 5, 0, 9, 2].  Slot 0: sizes [0, 5, 0, 9, 2] -> big = 3; sizes[0] = 9 // 2 = 4, sizes[3] = 5.  Slot 2: sizes
    [4, 5, 0, 5, 2], clusters 1 and 3 tie at 5 and the lowest index wins -> big = 1; sizes[2] = 2, sizes[1] = 3."""
    up, dn = F32(1025.0 / 1024.0), F32(1023.0 / 1024.0)
    means = np.array([[0, 0, 0, 0],
                      [1024, -2048, 512, 1],
                      [0, 0, 0, 0],
                      [2048, 1024, -1024, 3],
                      [7, 7, 7, 7]], F32)
    c, sizes, splits = kr.split_empty(means, np.array([0, 5, 0, 9, 2]))
    assert splits == [(0, 3), (2, 1)]
    assert sizes.tolist() == [4, 3, 2, 5, 2]
    want = np.array([[2050, 1023, -1025, F32(3) * dn],   # cluster 3 times (1+e, 1-e, 1+e, 1-e)
                     [1023, -2050, 511.5, up],           # cluster 1 times (1-e, 1+e, 1-e, 1+e)
                     [1025, -2046, 512.5, dn],           # cluster 1 times (1+e, 1-e, 1+e, 1-e)
                     [2046, 1025, -1023, F32(3) * up],   # cluster 3 times (1-e, 1+e, 1-e, 1+e)
                     [7, 7, 7, 7]], F32)
    assert np.array_equal(c, want)
    assert np.array_equal(kr.split_alt(4), np.array([up, dn, up, dn], F32))
    # the inputs are left alone and nothing happens without an empty slot
    assert means[0].tolist() == [0, 0, 0, 0]
    c2, s2, sp2 = kr.split_empty(means, np.array([1, 5, 1, 9, 2]))
    assert np.array_equal(c2, means) and sp2 == [] and s2.tolist() == [1, 5, 1, 9, 2]


def test_split_twice_from_one_cluster_compounds_the_perturbation():
    """counts [0, 0, 21, 3]: both slots are refilled from cluster 2 (21 -> 11 -> 6), and the second copy is taken from the centroid the
    first split already scaled by (2 - alt).  With 20 members the halves tie at 10 and the refilled slot 0, the lowest index, is split."""
    up, dn = F32(1025.0 / 1024.0), F32(1023.0 / 1024.0)
    means = np.array([[0, 0], [0, 0], [1024, 1024], [1, 1]], F32)
    c, sizes, splits = kr.split_empty(means, np.array([0, 0, 21, 3]))
    assert splits == [(0, 2), (1, 2)] and sizes.tolist() == [10, 5, 6, 3]
    assert np.array_equal(c[0], np.array([1025, 1023], F32))
    assert np.array_equal(c[1], np.array([F32(1023) * up, F32(1025) * dn], F32))
    assert np.array_equal(c[2], np.array([F32(1023) * dn, F32(1025) * up], F32))
    c, sizes, splits = kr.split_empty(means, np.array([0, 0, 20, 3]))
    assert splits == [(0, 2), (1, 0)] and sizes.tolist() == [5, 5, 10, 3]
    assert np.array_equal(c[0], np.array([F32(1025) * dn, F32(1023) * up], F32))
    assert np.array_equal(c[1], np.array([F32(1025) * up, F32(1023) * dn], F32))
    assert np.array_equal(c[2], np.array([1023, 1025], F32))


# ------------------------------------------------------------------------------------------------ scenario guards
def test_datasets_cover_every_pad_width():
    assert {kr.dataset(n)[0].shape[0] % 4 for n in kr.DATASETS} == {0, 1, 2, 3}
    assert max(kr.dataset(n)[0].shape[0] for n in kr.DATASETS) == 1301
    assert any(kr.dataset(n)[0].shape[0] % 32 for n in kr.DATASETS)


def test_scenario_blobs_reaches_a_fixed_point():
    x, k, iters, trace, _ = kr.reference_run("blobs")
    cs = trace["centroids"]
    assert iters <= 12 and any(np.array_equal(cs[i], cs[i - 1]) for i in range(1, iters + 1))
    assert not any(trace["splits"])


def test_scenario_wide_splits_one_cluster_twice_and_reuses_a_refilled_slot():
    x, k, iters, trace, _ = kr.reference_run("wide")
    assert x.shape == (1301, 256) and k == 40
    splits = trace["splits"]
    assert any(len(s) >= 2 for s in splits)
    assert any(len({b for _, b in s}) < len(s) for s in splits)  # one cluster is `big` twice within an iteration
    refilled, reused = set(), False
    for s in splits:
        reused = reused or any(b in refilled for _, b in s)
        refilled.update(e for e, _ in s)
    assert reused


def test_scenario_cancelled_is_clamped_and_splits():
    x, k, iters, trace, assigned = kr.reference_run("cancelled")
    m = clib.l2_matrix(x, x)
    off = ~np.eye(x.shape[0], dtype=bool)
    assert len(np.unique(x, axis=0)) == x.shape[0]
    assert float((m[off] == 0).mean()) >= 0.10
    assert any(trace["splits"])
    objs = [float(a[1].astype(np.float64).sum()) for a in assigned]
    assert any(b > a for a, b in zip(objs, objs[1:]))  # not monotone: no property test could cover this regime


def test_scenario_lattice_has_exact_ties():
    x, k, iters, trace, _ = kr.reference_run("lattice")
    assert set(np.unique(x).tolist()) <= set(range(-3, 4))
    tied = 0
    for c in trace["centroids"]:
        s = np.sort(clib.l2_matrix(x, c), 1)
        tied += int((s[:, 0] == s[:, 1]).sum())
    assert tied > 0


def test_scenario_n_eq_k_refills_from_the_two_member_cluster():
    x, k, iters, trace, assigned = kr.reference_run("n_eq_k")
    assert x.shape[0] == k == 16
    for i, s in enumerate(trace["splits"]):
        assert len(s) == 1
        counts = np.bincount(assigned[i][0], minlength=k)
        assert counts[s[0][0]] == 0 and counts[s[0][1]] == 2 and counts.max() == 2


def test_scenario_k1_and_k200():
    x, k, iters, trace, assigned = kr.reference_run("k1")
    assert k == 1 and not assigned[1][0].any()
    assert np.array_equal(trace["centroids"][1], kr.cluster_means(x, np.zeros(len(x), np.int64), 1)[0])
    x, k, iters, trace, assigned = kr.reference_run("k200")
    assert k > 128  # more than one 128-column tile of centroids
    assert all((a[0] >= 128).any() and (a[0] < 128).any() for a in assigned)


@pytest.mark.parametrize("m,n", kr.KNN_CLAMP_SHAPES)
def test_scenario_knn_clamp_regime(m, n):
    q, db = kr.knn_clamp_case(m, n, planted=False)
    rows = np.concatenate([q, db])
    assert len(np.unique(rows, axis=0)) == len(rows)  # no two rows are equal, so every zero below is a clamped negative
    assert float((clib.l2_matrix(q, db) == 0).mean()) >= 0.10
    qp, dbp = kr.knn_clamp_case(m, n)
    assert np.array_equal(dbp[n // 2], dbp[0]) and np.array_equal(qp[0], dbp[0])
    for k in kr.KNN_CLAMP_K:  # the tie rule decides: a clamped zero at a lower index beats the planted copy
        d2, idx = clib.l2_knn(qp, dbp, k)
        assert (d2[:, 0] == 0).mean() > 0.5 and (np.diff(idx, axis=1)[np.diff(d2, axis=1) == 0] > 0).all()


def test_scenario_unpopulated_word():
    fv, f2t, words, T = kr.unpopulated_word_case()
    d2, ids = clib.l2_knn(fv, words, 3)
    assert not (ids[:, 0] == 7).any() and (ids[:, 1] == 7).any()
    idfs = om.calc_word_idfs(ids[:, 0], f2t, 8, T)
    assert np.isinf(idfs[7]) and np.isfinite(idfs[:7]).all()
    for soft in (False, True):
        with np.errstate(invalid="ignore"):  # 0 * inf
            descs, _ = om.calc_tfidf_descriptors(fv, ids[:, 0], f2t, words, T, 3, soft, 10.0)
        assert np.isfinite(descs[:, :7]).all() and (descs[:, :7] > 0).any()
        assert np.isinf(descs[:2, 7]).all() and descs[2, 7] == 0
        assert np.isnan(descs[3, 7]) if soft else np.isinf(descs[3, 7])  # inf + 0 * inf


# ------------------------------------------------------------------------------------------------ mutations
def _split_mutant(means, counts, mode):
    c = np.array(means, dtype=F32, copy=True)
    sizes = np.array(counts, dtype=np.int64, copy=True)
    alt = kr.split_alt(c.shape[1])
    if mode == "signs":
        alt = (F32(2) - alt).astype(F32)
    other = (F32(2) - alt).astype(F32)
    for e in np.flatnonzero(np.asarray(counts) == 0).tolist():
        big = int(np.argmax(counts if mode == "counts" else sizes))
        c[e] = c[big] * alt
        c[big] = c[big] * other
        if mode != "stale":
            sizes[e] = sizes[big] // 2
            sizes[big] -= sizes[e]
    return c


def _mutant_run(name, mode):
    """The restatement with one rule broken -> the centroids after every iteration."""
    x, k, iters = kr.dataset(name)
    c = kr.init_centroids(x, k, 0)
    out, prev_ids = [c], None
    for _ in range(iters):
        ids, _ = kr.assign(x, c)
        use = prev_ids if mode == "previous_ids" and prev_ids is not None else ids
        means, counts, _ = kr.cluster_means(x, use, k)
        c = kr.split_empty(means, counts)[0] if mode in ("previous_ids", "pairwise") else _split_mutant(means, counts, mode)
        if mode == "pairwise":
            sums = np.stack([_pairwise_sum(x[ids == j]) for j in range(k)])
            c = kr.split_empty((sums / np.maximum(counts, 1).astype(F32)[:, None]).astype(F32), counts)[0]
        prev_ids = ids
        out.append(c)
    return out


@pytest.mark.parametrize("mode,name", [("counts", "wide"), ("stale", "cancelled"), ("signs", "wide"), ("signs", "n_eq_k"),
                                       ("previous_ids", "blobs"), ("pairwise", "wide")])
def test_datasets_tell_wrong_variants_apart(mode, name):
    """argmax of the counts instead of the running sizes, sizes not updated after a split, the two signs of the perturbation swapped,
    the previous iteration's ids in the update, a pairwise instead of a sequential sum: each changes the centroids of a dataset."""
    want = kr.reference_run(name)[3]["centroids"]
    got = _mutant_run(name, mode)
    assert any(not np.array_equal(g, w) for g, w in zip(got, want))


def test_mutant_harness_is_the_restatement_when_nothing_is_broken():
    for name in ("wide", "cancelled"):
        want = kr.reference_run(name)[3]["centroids"]
        got = _mutant_run(name, "none")
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
