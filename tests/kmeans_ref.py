"""Lloyd's rule as foundpose_amd/cluster_util.py states it, restated in numpy one rule per function (TEST INFRASTRUCTURE ONLY).

Only the distance stage goes through oracle.clib (the pinned k-ascending fmaf chain with the clamp at zero); everything else is plain
numpy on fp32 scalars and rows.  Nothing here imports foundpose_amd.  The datasets of tests/test_gpu_kmeans.py are built here too, so
that tests/test_kmeans_cpu.py can assert, on the restatement alone, that each of them still reaches the scenario it was chosen for.
"""

from typing import Dict, List, Tuple

import numpy as np
import torch

from oracle import clib

F32 = np.float32
EPS_SPLIT = F32(1.0 / 1024.0)


# ------------------------------------------------------------------------------------------------ the rules
def init_centroids(x: np.ndarray, k: int, seed: int = 0) -> np.ndarray:
    """The first k rows of a CPU-seeded torch.randperm(n).  The CPU generator is part of the definition: the same seed on a device
    generator draws another permutation."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    perm = torch.randperm(x.shape[0], generator=g)[:k].numpy()
    return np.ascontiguousarray(x[perm], dtype=F32)


def assign(x: np.ndarray, c: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """-> (ids [n] i64, d2 [n] f32): the oracle's 1-NN, d2 = max(0, fma(-2, <x, c>, |x|^2 + |c|^2)), ties -> lowest index."""
    d2, ids = clib.l2_knn(x, c, 1)
    return ids[:, 0].copy(), d2[:, 0].copy()


def cluster_means(x: np.ndarray, ids: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (means [k, d] f32, counts [k] i64, sums [k, d] f32).

    sums[c] starts at 0 and takes its members one at a time in ascending sample order, rounded to fp32 after every addition; the mean is
    sums[c] / float32(max(count, 1)), one correctly rounded fp32 division.

    This is what the device's one-hot GEMM computes.  There sums[c][j] is the fp32 fma chain acc = fma(onehot[c][i], x[i][j], acc) over
    i ascending, and the one-hot entry is 1 or 0: fma(1, x, acc) = fl(1 * x + acc) = fl(acc + x) because the product is exact, and
    fma(0, x, acc) = fl(0 + acc) = acc for finite x (acc is never -0: it starts at +0 and +0 + -0 = +0).  So the samples of other
    clusters, and the zero pad columns, leave the accumulator as it is, and the chain is the sequential sum of the members.

    The loop runs over the samples, not over a numpy reduction: np.sum adds pairwise, in an order numpy does not promise."""
    x = np.ascontiguousarray(x, dtype=F32)
    sums = np.zeros((k, x.shape[1]), F32)
    counts = np.zeros(k, np.int64)
    for i in range(x.shape[0]):
        c = int(ids[i])
        sums[c] = sums[c] + x[i]  # elementwise fp32 add, each rounded once
        counts[c] += 1
    means = sums / np.maximum(counts, 1).astype(F32)[:, None]
    return means.astype(F32), counts, sums


def split_alt(d: int) -> np.ndarray:
    """1 + 1/1024 on the even dimensions, 1 - 1/1024 on the odd ones (both exact in fp32)."""
    return np.where(np.arange(d) % 2 == 0, F32(1) + EPS_SPLIT, F32(1) - EPS_SPLIT).astype(F32)


def split_empty(means: np.ndarray, counts: np.ndarray) -> Tuple[np.ndarray, np.ndarray, List[Tuple[int, int]]]:
    """-> (centroids [k, d] f32, sizes [k] i64, [(e, big), ...]).

    Every empty slot e, in ascending order, is refilled from `big`, the first argmax of the RUNNING sizes: means[e] = means[big] * alt,
    then means[big] *= (2 - alt), in fp32; sizes[e] = sizes[big] // 2, then sizes[big] -= sizes[e]."""
    c = np.array(means, dtype=F32, copy=True)
    sizes = np.array(counts, dtype=np.int64, copy=True)
    alt = split_alt(c.shape[1])
    other = (F32(2) - alt).astype(F32)
    splits = []
    for e in np.flatnonzero(np.asarray(counts) == 0).tolist():
        big = int(np.argmax(sizes))  # first maximum
        c[e] = c[big] * alt
        c[big] = c[big] * other
        sizes[e] = sizes[big] // 2
        sizes[big] -= sizes[e]
        splits.append((int(e), big))
    return c, sizes, splits


def lloyd_step(x: np.ndarray, c: np.ndarray):
    """One iteration from centroids c -> (new_c, ids of c, d2 of c, splits)."""
    ids, d2 = assign(x, c)
    means, counts, _ = cluster_means(x, ids, c.shape[0])
    new_c, _, splits = split_empty(means, counts)
    return new_c, ids, d2, splits


def kmeans(x: np.ndarray, k: int, num_iter: int, seed: int = 0):
    """-> (centroids, ids i64, d2, trace); trace["centroids"][i] are the centroids after i iterations (entry 0: the initial draw) and
    trace["splits"][i] the (e, big) pairs of iteration i + 1."""
    x = np.ascontiguousarray(x, dtype=F32)
    if x.shape[0] < k:
        raise ValueError(f"{x.shape[0]} samples cannot form {k} clusters")
    c = init_centroids(x, k, seed)
    trace = {"centroids": [c.copy()], "splits": []}
    for _ in range(num_iter):
        c, _, _, splits = lloyd_step(x, c)
        trace["centroids"].append(c.copy())
        trace["splits"].append(splits)
    ids, d2 = assign(x, c)
    return c, ids, d2, trace


# ------------------------------------------------------------------------------------------------ the datasets
def _blobs(n: int, d: int, k: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, d)) * 4.0
    lab = rng.integers(0, k, n)
    return (centres[lab] + rng.standard_normal((n, d))).astype(F32)


def _blobs_ds():
    return _blobs(1003, 20, 8, 1003)


def _wide_ds():
    return _blobs(1301, 256, 40, 1301)


def _cancelled_ds():
    rng = np.random.default_rng(7)
    return (30.0 + 1e-2 * rng.standard_normal((601, 64))).astype(F32)


def _lattice_ds():
    return np.random.default_rng(778).integers(-3, 4, (778, 12)).astype(F32)


def _n_eq_k_ds():
    x = np.random.default_rng(16).standard_normal((16, 8)).astype(F32)
    x[11] = x[4]
    return x


def _k1_ds():
    rng = np.random.default_rng(130)
    return (rng.standard_normal((130, 8)) * np.array([1e3, 1, 1e-3, 1, 30, 1, 1, 1e2])).astype(F32)


def _k200_ds():
    return _blobs(900, 32, 200, 900)


# name -> (builder, k, iterations I: the trajectory is compared after 0..I iterations).  n % 4 is 3, 1, 1, 2, 0, 2, 0.
DATASETS: Dict[str, tuple] = {
    "blobs": (_blobs_ds, 8, 12),
    "wide": (_wide_ds, 40, 4),
    "cancelled": (_cancelled_ds, 12, 6),
    "lattice": (_lattice_ds, 24, 5),
    "n_eq_k": (_n_eq_k_ds, 16, 3),
    "k1": (_k1_ds, 1, 2),
    "k200": (_k200_ds, 200, 3),
}

_RUNS: dict = {}


def dataset(name: str) -> Tuple[np.ndarray, int, int]:
    build, k, iters = DATASETS[name]
    return build(), k, iters


def reference_run(name: str):
    """(x, k, I, trace, per-iteration (ids, d2)) of the restatement: computed once, shared by the tests, never written."""
    if name not in _RUNS:
        x, k, iters = dataset(name)
        _, _, _, trace = kmeans(x, k, iters)
        assigned = [assign(x, c) for c in trace["centroids"]]
        for a in [x] + trace["centroids"] + [v for pair in assigned for v in pair]:
            a.setflags(write=False)
        _RUNS[name] = (x, k, iters, trace, assigned)
    return _RUNS[name]


def update_stage_case():
    """Hand-made ids for the update stage alone: cluster 2 is empty, cluster 5 has one member, cluster 1 owns most samples; magnitudes
    of 1e6 stand next to 1e-2, so any other summation order gives other bits.  n = 203 (n % 4 == 3) -> (x, ids i64, k)."""
    rng = np.random.default_rng(203)
    n, d, k = 203, 24, 7
    x = rng.standard_normal((n, d)) * rng.choice([1e6, 1.0, 1e-2], size=(n, d))
    ids = np.where(rng.random(n) < 0.7, 1, rng.choice([0, 3, 4, 6], size=n))
    ids[97] = 5
    return x.astype(F32), ids.astype(np.int64), k


# (m, n) of the k-NN's clamp regime; k in KNN_CLAMP_K are the three epilogues that clamp (arg-min, per-tile top-k, distance store)
KNN_CLAMP_SHAPES = [(133, 133), (37, 300), (300, 37)]
KNN_CLAMP_K = [1, 3, 12]


def knn_clamp_case(m: int, n: int, planted: bool = True):
    """Rows far from the origin and close to each other (offset 30, spread 1e-2, d = 64): |q|^2 + |d|^2 - 2<q, d> rounds below zero for a
    large share of the pairs.  planted=False gives the rows before any is duplicated (the guard's input) -> (q, db)."""
    rng = np.random.default_rng(m * 1000 + n)
    q = (30.0 + 1e-2 * rng.standard_normal((m, 64))).astype(F32)
    db = (30.0 + 1e-2 * rng.standard_normal((n, 64))).astype(F32)
    if planted:
        db[n // 2] = db[0]   # equal rows: an exact tie even without the clamp
        db[n - 1] = db[3]
        q[0] = db[0]
        q[m - 1] = db[n // 2]
    return q, db


def unpopulated_word_case():
    """Four templates, 8 words, d = 8: word 7 sits 6 away from word 0, so it is the 2nd-nearest word of every feature around word 0 and
    nobody's nearest.  Template 2 has no feature around word 0 and keeps word 7 out of its three nearest.  Template 3 also has one
    feature between word 1 and word 7 whose 2nd-nearest word is word 7 at a squared distance near 200: its soft weight
    exp(-200^2 / 20) is 0 in fp32, and 0 * inf is a NaN -> (feat_vectors, feat_to_template_ids i32, words, num_templates)."""
    rng = np.random.default_rng(8)
    words = np.zeros((8, 8), F32)
    for w in range(7):
        words[w, w] = 10.0
    words[7, 0], words[7, 7] = 10.0, 6.0
    feats, f2t = [], []
    for t in range(4):
        near = [1, 2, 3, 4, 5, 6, 1, 3] if t == 2 else [0, 1, 2, 0, 4, 5, 6, 0, 3]
        for w in near:
            feats.append(words[w] + 0.2 * rng.standard_normal(8))
            f2t.append(t)
    far = words[1].copy()
    far[7] = 5.0
    feats.append(far)
    f2t.append(3)
    return np.asarray(feats, F32), np.asarray(f2t, np.int32), words, 4
