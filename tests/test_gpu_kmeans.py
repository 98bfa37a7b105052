"""cluster_util.kmeans on the MI355X, step by step against tests/kmeans_ref.py, and three neighbours it leans on.

A  trajectories: for every dataset and every it in 0..I, kmeans(x, k, num_iter=it) equals the restatement after it iterations: centroids,
   ids and squared distances.  num_iter=0 is the initial draw.
B  one step: the device's own centroids of iteration i - 1 through the restated step equal the device's iteration i, at an iteration
   that splits, so a broken trajectory points at one step.
C  the update stage alone: the one-hot GEMM's sums, the means and the counts on hand-made ids.
D  the k-NN where the distance clamp decides: rows far from the origin, all three clamping epilogues.
E  the row-chunk loop of ops.knn_l2.
F  the descriptor builder when a word has no member (idf = inf).

Every comparison is on the bits unless a tolerance is named."""
import numpy as np
import pytest
import torch

from foundpose_amd import _lib, bank_builder, cluster_util, ops, repre_util
from oracle import clib
from oracle import match as om
from tests import kmeans_ref as kr

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))  # a copy: the shared references are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def _same(got: torch.Tensor, want: np.ndarray, what: str):
    got = got.detach().cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} entries differ, the first at {tuple(bad[0])}: "
                             f"{got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}")


def _poison_free_blocks(*shapes):
    """Leave NaNs behind in the allocator's free blocks of these sizes, so a buffer that kmeans takes with torch.empty and does not
    fully write (the pad columns of the transposed samples) shows up: fma(0, NaN, acc) is a NaN, fma(0, 0, acc) is acc."""
    blocks = [torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for s in shapes for _ in range(2)]
    torch.cuda.synchronize()
    del blocks


def _device_kmeans(x_dev, k, it):
    n, d = x_dev.shape
    pad = (n + 3) // 4 * 4
    _poison_free_blocks((d, pad), (k, pad), (k, d), (n,))
    c, ids, d2 = cluster_util.kmeans(x_dev, k, num_iter=it, verbose=False)
    assert ids.dtype == torch.int32 and c.dtype == torch.float32 and d2.dtype == torch.float32
    return c, ids, d2


# ------------------------------------------------------------------------------------------------ A: trajectories
@pytest.mark.parametrize("name", list(kr.DATASETS))
def test_kmeans_trajectory(name):
    x, k, iters, trace, assigned = kr.reference_run(name)
    x_dev = _dev(x)
    for it in range(iters + 1):
        c, ids, d2 = _device_kmeans(x_dev, k, it)
        _same(c, trace["centroids"][it], f"{name}: centroids after {it} iterations")
        _same(ids, assigned[it][0].astype(np.int32), f"{name}: ids after {it} iterations")
        _same(d2, assigned[it][1], f"{name}: squared distances after {it} iterations")


def test_kmeans_seed_is_part_of_the_draw():
    x, k, _ = kr.dataset("lattice")
    for seed in (0, 1, 12345):
        c, _, _ = cluster_util.kmeans(_dev(x), k, num_iter=0, verbose=False, seed=seed)
        _same(c, kr.init_centroids(x, k, seed), f"initial draw of seed {seed}")


# ------------------------------------------------------------------------------------------------ B: one step
@pytest.mark.parametrize("name,step", [("wide", 2), ("wide", 3), ("cancelled", 4), ("n_eq_k", 2), ("k200", 2)])
def test_kmeans_one_step_from_the_device_centroids(name, step):
    x, k, iters, trace, _ = kr.reference_run(name)
    assert step <= iters and trace["splits"][step - 1], "this iteration was chosen because it splits"
    x_dev = _dev(x)
    c_prev, ids_prev, d2_prev = _device_kmeans(x_dev, k, step - 1)
    c_next, _, _ = _device_kmeans(x_dev, k, step)
    new_c, ids, d2, splits = kr.lloyd_step(x, c_prev.cpu().numpy())
    assert splits == trace["splits"][step - 1]
    _same(ids_prev, ids.astype(np.int32), f"{name}: ids entering iteration {step}")
    _same(d2_prev, d2, f"{name}: squared distances entering iteration {step}")
    _same(c_next, new_c, f"{name}: centroids of iteration {step} from the device's iteration {step - 1}")


# ------------------------------------------------------------------------------------------------ C: the update stage
def _transposed_padded(x_dev):
    n, d = x_dev.shape
    x_t = torch.zeros(d, (n + 3) // 4 * 4, dtype=torch.float32, device="cuda")
    x_t[:, :n] = x_dev.t()
    return x_t


def test_update_stage_sums_means_and_counts():
    x, ids, k = kr.update_stage_case()
    means, counts, sums = kr.cluster_means(x, ids, k)
    x_dev, ids_dev = _dev(x), _dev(ids, torch.int32)
    x_t = _transposed_padded(x_dev)
    onehot = torch.zeros(k, x_t.shape[1], dtype=torch.float32, device="cuda")
    onehot[ids_dev.long(), torch.arange(len(ids), device="cuda")] = 1.0
    _same(ops.gemm_f32(onehot, x_t), sums, "one-hot GEMM sums")
    got_means, got_counts = cluster_util._update(x_t, ids_dev, k)
    _same(got_counts, counts, "counts")
    _same(got_means, means, "means")
    assert counts[2] == 0 and not got_means[2].any()


@pytest.mark.parametrize("name", ["wide", "k1", "cancelled"])
def test_update_stage_on_the_datasets(name):
    """The restatement's own ids of the first iteration: sums, means and counts of the device at the datasets' sizes (n % 4 = 1, 2, 1;
    a K of 1304 / 132 / 604 in the GEMM, none a multiple of 32)."""
    x, k, _, _, assigned = kr.reference_run(name)
    ids = assigned[0][0]
    means, counts, sums = kr.cluster_means(x, ids, k)
    x_t = _transposed_padded(_dev(x))
    got_means, got_counts = cluster_util._update(x_t, _dev(ids, torch.int32), k)
    _same(got_counts, counts, f"{name}: counts")
    _same(got_means, means, f"{name}: means")


def test_device_division_is_correctly_rounded():
    """The means are sums / float32(count) by torch on the device; the restatement divides in numpy.  Both are the correctly rounded fp32
    quotient: across 60 decades of normal numbers and for every count up to 4096."""
    rng = np.random.default_rng(5)
    num = (rng.standard_normal((64, 4096)) * 10.0 ** rng.integers(-30, 30, (64, 4096))).astype(np.float32)
    num[0, :5] = [0.0, 3e38, -3e38, 1.0, -1.0]
    den = np.arange(1, 4097, dtype=np.float32)[None, :]
    _same(_dev(num) / _dev(den), (num / den).astype(np.float32), "fp32 division")


# ------------------------------------------------------------------------------------------------ D: the clamp regime of the k-NN
@pytest.mark.parametrize("k", kr.KNN_CLAMP_K)
@pytest.mark.parametrize("m,n", kr.KNN_CLAMP_SHAPES)
def test_knn_l2_where_the_clamp_decides(m, n, k):
    q, db = kr.knn_clamp_case(m, n)
    d2, idx = ops.knn_l2(_dev(q), _dev(db), k)
    o_d2, o_idx = clib.l2_knn(q, db, k)
    assert float((o_d2 == 0).mean()) > 0.10  # the clamp, then "ties -> lowest index", decides these
    _same(idx, o_idx.astype(np.int32), "indices")
    _same(d2, o_d2, "squared distances")


# ------------------------------------------------------------------------------------------------ E: row chunks
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("chunk", [50, 37])
def test_knn_l2_row_chunks(monkeypatch, k, chunk):
    """133 rows in chunks of 50 (50 + 50 + 33) and of 37 (the sliced norms and outputs then start at offsets that are no multiple of 16
    bytes): the same bits as the single launch and as the oracle, on clamped and on standard-normal rows."""
    rng = np.random.default_rng(chunk)
    for q, db in (kr.knn_clamp_case(133, 133), (rng.standard_normal((133, 64)).astype(np.float32),
                                                rng.standard_normal((300, 64)).astype(np.float32))):
        q_dev, db_dev = _dev(q), _dev(db)
        whole_d2, whole_idx = ops.knn_l2(q_dev, db_dev, k)
        per_row = _lib.knn_scratch_bytes(1, db.shape[0], k)
        assert ops._KNN_SCRATCH_BYTES // per_row >= 133  # the call above was one launch
        with monkeypatch.context() as mp:
            mp.setattr(ops, "_KNN_SCRATCH_BYTES", chunk * per_row)
            d2, idx = ops.knn_l2(q_dev, db_dev, k)
        o_d2, o_idx = clib.l2_knn(q, db, k)
        assert torch.equal(d2, whole_d2) and torch.equal(idx, whole_idx)
        _same(idx, o_idx.astype(np.int32), "indices")
        _same(d2, o_d2, "squared distances")


# ------------------------------------------------------------------------------------------------ F: a word without members
@pytest.mark.parametrize("soft", [False, True])
def test_tfidf_descriptors_with_an_unpopulated_word(soft):
    """Word 7 is nobody's nearest word, so its idf is log(T / 0) = inf as in the reference, yet it is the 2nd-nearest word of some
    features: the descriptor entry is inf (tf * inf), a NaN where a soft weight of 0 meets it, 0 where no feature lists it.  Same kind
    at the same positions as the oracle; every finite entry as in test_bank_builder_vs_reference_fixture."""
    fv, f2t, words, T = kr.unpopulated_word_case()
    _, o_ids = clib.l2_knn(fv, words, 3)
    with np.errstate(invalid="ignore"):  # 0 * inf
        want, want_idfs = om.calc_tfidf_descriptors(fv, o_ids[:, 0], f2t, words, T, 3, soft, 10.0)
    opts = repre_util.TemplateDescOpts(tfidf_soft_assign=soft)
    descs, idfs, f2c = bank_builder.calc_tfidf_descriptors(_dev(fv), _dev(f2t), _dev(words), T, opts)
    descs, idfs = descs.cpu().numpy(), idfs.cpu().numpy()
    _same(f2c, o_ids[:, 0].astype(np.int32), "feat_to_cluster_ids")
    assert np.isposinf(want_idfs[7]) and np.isposinf(idfs[7])
    np.testing.assert_allclose(idfs[:7], want_idfs[:7], rtol=3e-7, atol=0)
    assert not np.isfinite(want[:, 7]).all() and np.isfinite(want[:, :7]).all()
    assert np.array_equal(np.isnan(descs), np.isnan(want)) and np.array_equal(np.isposinf(descs), np.isposinf(want))
    assert not np.isneginf(descs).any()
    fin = np.isfinite(want)
    np.testing.assert_allclose(descs[fin], want[fin], rtol=5e-5, atol=1e-8)
