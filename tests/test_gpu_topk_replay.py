"""GPU: the wave-parallel replay of torch.topk's tie order (csrc/stl_wave.hpp inside cyclic_select_kernel) at every branch and size.

Each case of tests/topk_replay_cases.py is a sequence v of cycle distances and a k.  The planted (crop, one-patch template)
pair hands exactly v to the selection (tests/test_topk_replay_cpu.py checks that on the oracle), so the device's output order
is compared with `torch.topk(-v, k, sorted=True)` on a CPU tensor -- the thing replayed -- for Q up to the kernel's limit of
2048, on both sides of the partial_sort / nth_element seam (k = floor(n / 64), + 1), on both sides of the register / two-pass
placement seam (k - 1 = 512, 513) and on the four killer sequences that drive libstdc++ into its heap fallbacks.  The
canonical order (distance, then index: the 2048-slot bitonic sort) is checked at the same sizes.  Every comparison is bit exact.

Branches per case, counted on the CPU by the instrumented walk of csrc/stl_order.hpp (tests/csrc/stl_trace.cpp; part_le64 /
part_gt64: partitions whose scanned part fits one 64-lane chunk -- the register-only partition -- or needs the stopper tables):

case                                     n     k     partial_sort       part_le64       part_gt64 select_fallback   sort_fallback        two_pass
n64_k1_random_distinct                  64     1                1               0               0               0               0               0
n64_k7_grid14                           64     7                0               5               0               0               0               0
n64_k2_all_zero                         64     2                0               5               0               0               0               0
n64_k63_two_values_runs37               64    63                0               9               0               0               0               0
n64_k64_ascending                       64    64                0               9               0               0               0               0
n65_k1_two_values_runs37                65     1                1               0               0               0               0               0
n65_k7_ascending                        65     7                0               8               0               0               0               0
n65_k2_descending                       65     2                0               3               0               0               0               0
n65_k64_organ_pipe                      65    64                0              12               0               0               0               0
n65_k65_levels11_runs37                 65    65                0               9               0               0               0               0
n66_k1_organ_pipe                       66     1                1               0               0               0               0               0
n66_k7_levels11_runs37                  66     7                0               3               1               0               0               0
n66_k2_random_distinct                  66     2                0               3               1               0               0               0
n66_k65_grid14                          66    65                0               8               1               0               0               0
n66_k66_all_zero                        66    66                0               8               1               0               0               0
n129_k1_grid14                         129     1                1               0               0               0               0               0
n129_k7_all_zero                       129     7                0               5               1               0               0               0
n129_k2_two_values_runs37              129     2                1               0               0               0               0               0
n129_k3_ascending                      129     3                0               3               1               0               0               0
n129_k128_descending                   129   128                0              13               2               0               0               0
n129_k129_organ_pipe                   129   129                0              12               7               0               0               0
n517_k1_ascending                      517     1                1               0               0               0               0               0
n517_k7_descending                     517     7                1               0               0               0               0               0
n517_k8_organ_pipe                     517     8                1               0               0               0               0               0
n517_k9_levels11_runs37                517     9                0               4               2               0               0               0
n517_k300_random_distinct              517   300                0              25              13               0               0               0
n517_k513_grid14                       517   513                0              37              16               0               0               0
n517_k514_all_zero                     517   514                0              30              10               0               0               1
n517_k516_two_values_runs37            517   516                0              37              13               0               0               1
n517_k517_ascending                    517   517                0              47              14               0               0               1
n1369_k1_levels11_runs37              1369     1                1               0               0               0               0               0
n1369_k7_random_distinct              1369     7                1               0               0               0               0               0
n1369_k21_grid14                      1369    21                1               0               0               0               0               0
n1369_k22_all_zero                    1369    22                0               5               5               0               0               0
n1369_k300_two_values_runs37          1369   300                0              29              11               0               0               0
n1369_k513_ascending                  1369   513                0              40              17               0               0               0
n1369_k514_descending                 1369   514                0              40              16               0               0               1
n1369_k1368_organ_pipe                1369  1368                0             132              52               0               0               1
n1369_k1369_levels11_runs37           1369  1369                0              96              39               0               0               1
n2047_k1_all_zero                     2047     1                1               0               0               0               0               0
n2047_k7_two_values_runs37            2047     7                1               0               0               0               0               0
n2047_k31_ascending                   2047    31                1               0               0               0               0               0
n2047_k32_descending                  2047    32                0               9               8               0               0               0
n2047_k300_organ_pipe                 2047   300                0              34              24               1               0               0
n2047_k513_levels11_runs37            2047   513                0              35              16               0               0               0
n2047_k514_random_distinct            2047   514                0              46              18               0               0               1
n2047_k2046_grid14                    2047  2046                0             133              57               0               0               1
n2047_k2047_all_zero                  2047  2047                0             100              36               0               0               1
n2048_k1_descending                   2048     1                1               0               0               0               0               0
n2048_k7_organ_pipe                   2048     7                1               0               0               0               0               0
n2048_k32_levels11_runs37             2048    32                1               0               0               0               0               0
n2048_k33_random_distinct             2048    33                0               7               3               0               0               0
n2048_k300_grid14                     2048   300                0              27              14               0               0               0
n2048_k513_all_zero                   2048   513                0              29              12               0               0               0
n2048_k514_two_values_runs37          2048   514                0              29              13               0               0               1
n2048_k2047_ascending                 2048  2047                0             148              51               0               0               1
n2048_k2048_descending                2048  2048                0             154              54               0               0               1
select_killer_n1369_k300              1369   300                0               4              36               1               1               0
select_killer_n2048_k2040             2048  2040                0               4              42               1               1               1
sort_killer_m64_n564                   564    65                0              17               5               0               1               0
sort_killer_m1200_n1217               1217  1201                0              82              55               0               1               1
total                                                          17            1495             667               3               4              14
"""

import numpy as np
import pytest
import torch

from oracle import match as om
from tests import topk_replay_cases as cases

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in cases.all_cases()}
PAD = 5           # slots of a record past top_k: the kernel owns them too
SENTINEL_I, SENTINEL_F = -7, -123.5


def _scores(d):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.float32(1.0) - d / d.max()).astype(np.float32)   # oracle/match.py:140


def _torch_order(v, k):
    return torch.topk(torch.from_numpy(-v), k, sorted=True)[1].numpy()


def _canonical_order(v, k):
    return np.argsort(v, kind="stable")[:k]   # distance, then index


class Launch:
    """One fp_cyclic_buddies call on planted detections: detection b has the cycle distances seqs[b]; slot j of every detection
    is matched against template j (each template is the one shared patch), so pair (b, j) must select from seqs[b]."""

    def __init__(self, seqs, top_k, tie_mode, n_slots=1):
        from foundpose_amd import ops
        from foundpose_amd._lib import FoundPoseNativeError, call, cyclic_scratch_bytes, ptr, stream
        dev = "cuda"
        planted = [cases.planted_inputs(v) for v in seqs]
        self.pts = [p[0] for p in planted]
        self.vertices = (np.arange(3 * n_slots, dtype=np.float32).reshape(n_slots, 3) + 1) * np.float32(0.5)
        B, K = len(seqs), top_k + PAD
        q_off = np.concatenate([[0], np.cumsum([len(v) for v in seqs])]).astype(np.int32)
        q_max = max(len(v) for v in seqs)
        qf = torch.from_numpy(np.concatenate([p[1] for p in planted])).to(dev)
        qp = torch.from_numpy(np.concatenate(self.pts)).to(dev)
        feats = torch.from_numpy(np.repeat(planted[0][2], n_slots, 0)).to(dev)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        tabs = dict(q_off=t(q_off), tpl_off=t(np.arange(n_slots + 1, dtype=np.int32)), tpl_ids=t(np.tile(np.arange(n_slots, dtype=np.int32), B)),
                    base=t(np.zeros(B, np.int32)), vertices=t(self.vertices))
        q_sqn, f_sqn = ops.sqnorm_rows(qf), ops.sqnorm_rows(feats)
        scratch = torch.empty(cyclic_scratch_bytes(B * n_slots, q_max, 1) // 8 + 1, dtype=torch.int64, device=dev)
        full = lambda shape, dtype, val: torch.full(shape, val, dtype=dtype, device=dev)
        self.out = dict(count=full((B, n_slots), torch.int32, SENTINEL_I), q_ids=full((B, n_slots, K), torch.int32, SENTINEL_I),
                        feat_ids=full((B, n_slots, K), torch.int32, SENTINEL_I), dists=full((B, n_slots, K), torch.float32, SENTINEL_F),
                        conf=full((B, n_slots, K), torch.float32, SENTINEL_F), c2d=full((B, n_slots, K, 2), torch.float32, SENTINEL_F),
                        c3d=full((B, n_slots, K, 3), torch.float32, SENTINEL_F))
        o = self.out
        self.error = None
        try:
            call("fp_cyclic_buddies", ptr(qf), ptr(q_sqn), ptr(qp), ptr(tabs["q_off"]), B, q_max, ptr(feats), ptr(f_sqn), ptr(tabs["tpl_off"]), 1,
                 ptr(tabs["vertices"]), ptr(tabs["tpl_ids"]), ptr(tabs["base"]), ptr(tabs["base"]), n_slots, qf.shape[1], top_k, K, ptr(scratch),
                 ptr(o["count"]), ptr(o["q_ids"]), ptr(o["feat_ids"]), ptr(o["dists"]), ptr(o["conf"]), ptr(o["c2d"]), ptr(o["c3d"]), tie_mode, stream())
        except FoundPoseNativeError as e:   # kept for the refusal test; every other caller asserts error is None
            self.error = e
        torch.cuda.synchronize()
        self.np = {k: v.cpu().numpy() for k, v in o.items()}


def _check_pair(run, b, j, v, k, order, what):
    """Pair (b, j) of a launch holds exactly the record the replayed order defines: ids, distances, patch ids, scores,
    coordinates, and the padded tail."""
    r = run.np
    assert r["count"][b, j] == k, what
    assert np.array_equal(r["q_ids"][b, j, :k], order), what
    d = v[order]
    assert np.array_equal(r["dists"][b, j, :k].view(np.uint32), d.view(np.uint32)), what
    assert np.all(r["feat_ids"][b, j, :k] == j), what            # object ids: patch 0 of template j (all 0 with one slot)
    assert np.array_equal(r["conf"][b, j, :k], _scores(d), equal_nan=True), what
    assert np.array_equal(r["c2d"][b, j, :k], run.pts[b][order]), what
    assert np.array_equal(r["c3d"][b, j, :k], np.repeat(run.vertices[j][None], k, 0)), what
    assert np.all(r["q_ids"][b, j, k:] == -1) and np.all(r["feat_ids"][b, j, k:] == -1), what
    for name in ("dists", "conf", "c2d", "c3d"):
        assert np.all(r[name][b, j, k:].view(np.uint32) == 0), (what, name)


@pytest.mark.parametrize("name", list(CASES))
def test_planted_sequence_replays_torch_topk_and_canonical_order(name):
    c = CASES[name]
    v, k = c.v, c.k
    for tie_mode, order in ((1, _torch_order(v, k)), (0, _canonical_order(v, k))):
        run = Launch([v], k, tie_mode)
        assert run.error is None
        _check_pair(run, 0, 0, v, k, order, (name, tie_mode))
    # second witness: the oracle's restatement of cyclic_buddies on the same planted pair
    pts, qf, obj = cases.planted_inputs(v)
    o_q, o_o, o_d, o_s, _ = om.cyclic_buddies(pts, qf, obj, k, topk_mode="torch")
    run = Launch([v], k, 1)
    assert np.array_equal(run.np["q_ids"][0, 0, :k], o_q) and np.array_equal(run.np["feat_ids"][0, 0, :k], o_o)
    assert np.array_equal(run.np["dists"][0, 0, :k], o_d) and np.array_equal(run.np["conf"][0, 0, :k], o_s, equal_nan=True)


@pytest.mark.parametrize("name", list(cases.KILLERS))
def test_killers_through_the_drop_in_entry(name):
    """cyclic_buddies_matching (the reference's signature, torch order) on the killer sequences."""
    from foundpose_amd import corresp_util
    c = CASES[name]
    pts, qf, obj = (torch.from_numpy(x).cuda() for x in cases.planted_inputs(c.v))
    q_ids, o_ids, dists, scores = (t.cpu().numpy() for t in corresp_util.cyclic_buddies_matching(pts, qf, None, obj, None, c.k))
    order = _torch_order(c.v, c.k)
    assert np.array_equal(q_ids, order) and np.all(o_ids == 0)
    assert np.array_equal(dists.view(np.uint32), c.v[order].view(np.uint32))
    assert np.array_equal(scores, _scores(c.v[order]), equal_nan=True)


@pytest.mark.parametrize("top_k,names", [(300, ("select_killer_n1369_k300", "sort_killer_m64_n564")),
                                         (1201, ("sort_killer_m1200_n1217", "select_killer_n2048_k2040"))])
def test_one_launch_of_mixed_pairs_equals_each_alone(top_k, names):
    """Several (detection, slot) pairs of different Q and sequence in one launch -- a killer at its own k, another killer, an
    all-zero row and a Q = 1 row, two slots each: every pair gives the bits it gives alone, in both tie orders."""
    seqs = [CASES[names[0]].v, np.zeros(700, np.float32), CASES[names[1]].v, np.zeros(1, np.float32)]
    for tie_mode in (1, 0):
        both = Launch(seqs, top_k, tie_mode, n_slots=2)
        assert both.error is None
        for b, v in enumerate(seqs):
            k = min(top_k, len(v))
            alone = Launch([v], top_k, tie_mode)
            order = _torch_order(v, k) if tie_mode == 1 else _canonical_order(v, k)
            for j in range(2):
                _check_pair(both, b, j, v, k, order, (names, tie_mode, b, j))
                for key in ("q_ids", "dists", "conf", "c2d"):
                    assert np.array_equal(both.np[key][b, j].view(np.uint32), alone.np[key][0, 0].view(np.uint32)), (key, tie_mode, b, j)


def test_more_than_2048_query_points_are_refused():
    from foundpose_amd._lib import FoundPoseNativeError
    for tie_mode in (1, 0):
        run = Launch([cases.family_values("grid14", 2049)], 300, tie_mode)
        assert isinstance(run.error, FoundPoseNativeError) and "2048 query points" in str(run.error) and "2049" in str(run.error)
        for key, arr in run.np.items():   # nothing was selected, nothing was written
            assert np.all(arr == (SENTINEL_I if arr.dtype == np.int32 else SENTINEL_F)), key
    ok = Launch([cases.family_values("grid14", 2048)], 300, 1)   # the limit itself is served
    assert ok.error is None and ok.np["count"][0, 0] == 300


@pytest.fixture(scope="module")
def crop518():
    """The 37 x 37 patch grid of a 518-pixel crop (1369 query points, cell 14) against templates of 1369 and 1300 patches, dim 64:
    planted exact buddies, one duplicated query patch and one duplicated template patch, as in test_cyclic_buddies_pair_edge_tiles."""
    rng = np.random.default_rng(518)
    Q, sizes, dim, W = 1369, (1369, 1300), 64, 16
    feats = rng.standard_normal((sum(sizes), dim)).astype(np.float32)
    feats[sizes[0] - 1] = feats[1]                                   # duplicated template patch: exact ties on the row side
    qf = rng.standard_normal((Q, dim)).astype(np.float32)
    n_copy = Q // 2
    qf[:n_copy] = feats[rng.permutation(sizes[0])[:n_copy]]         # exact buddies in template 0
    qf[Q - 1] = qf[0]                                                # duplicated query patch: exact ties on the column side
    g = np.arange(37, dtype=np.float32) * 14 + 7
    pts = np.stack(np.meshgrid(g, g, indexing="xy"), -1).reshape(Q, 2).astype(np.float32)
    bank = {"vertices": rng.standard_normal((sum(sizes), 3)).astype(np.float32), "feat_vectors": feats,
            "feat_to_vertex_ids": np.arange(sum(sizes), dtype=np.int32), "feat_to_template_ids": np.repeat(np.arange(2, dtype=np.int32), sizes)}
    repre = om.build_synthetic_repre(bank, feats[rng.permutation(sum(sizes))[:W]].copy())
    oracle = {(order, top_k): om.establish_correspondences(pts, qf, repre, 2, top_k, topk_mode=order)
              for order in ("torch", "canonical") for top_k in (300, 1369)}
    return repre, pts, qf, oracle


@pytest.mark.parametrize("top_k", [300, 1369])
@pytest.mark.parametrize("order", ["torch", "canonical"])
def test_production_size_crop_vs_oracle(crop518, order, top_k):
    from tests.test_gpu_matching import _gpu_corresp
    repre, pts, qf, oracle = crop518
    got, ora = _gpu_corresp(repre, pts, qf, 2, top_k, tie_order=order), oracle[(order, top_k)]
    assert [int(x["template_id"]) for x in got] == [o["template_id"] for o in ora]
    for a, o in zip(got, ora):
        assert len(o["coord_2d_ids"]) == top_k
        for key in ("coord_2d_ids", "nn_vertex_ids", "nn_dists", "coord_2d", "coord_3d"):
            assert np.array_equal(a[key].cpu().numpy(), o[key]), (order, top_k, key)
        assert np.array_equal(a["coord_conf"].cpu().numpy(), o["coord_conf"], equal_nan=True)
