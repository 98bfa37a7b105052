"""CPU: the case list of the torch.topk replay (tests/topk_replay_cases.py) is what it claims to be.

The device test (tests/test_gpu_topk_replay.py) runs these cases through the wave-parallel replay (csrc/stl_wave.hpp).  Here,
without a GPU: the committed killer sequences are the ones this machine's libstdc++ produces, every case takes the branch it
is named for (counted by an instrumented walk of csrc/stl_order.hpp, tests/csrc/stl_trace.cpp), the sequential restatement
agrees with torch.topk on each of them, and the planted (crop, template) pair really hands the chosen sequence to the
selection.  Run with `-s` to see the table of case -> counters.
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import match as om
from tests import topk_replay_cases as cases


@pytest.fixture(scope="module")
def trace_lib(tmp_path_factory):
    return cases.build_trace_lib(tmp_path_factory.mktemp("stl_trace"))


@pytest.fixture(scope="module")
def order_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stl_order") / "libstl_order_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(cases.ROOT, "tests", "csrc", "stl_order_check.cpp")])
    return ctypes.CDLL(so)


def stl_order_topk(lib, x, k):
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(k, np.int64)
    lib.stl_order_topk(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(x)), ctypes.c_int64(k), out.ctypes.data_as(ctypes.c_void_p))
    return out


def test_case_list_covers_every_length_k_and_family():
    grid = cases.grid_cases()
    assert len({c.name for c in cases.all_cases()}) == len(grid) + len(cases.KILLERS)
    seen = {(len(c.v), c.k) for c in grid}
    for n in cases.LENGTHS:
        for k in cases.ks_for(n):
            assert (n, k) in seen
        # both sides of the partial_sort / nth_element seam
        assert (n // 64) * 64 <= n < (n // 64 + 1) * 64 and {n // 64, n // 64 + 1} <= set(cases.ks_for(n))
    for n in (1369, 2048):
        assert {c.name.split("_", 2)[2] for c in grid if len(c.v) == n} == set(cases.FAMILIES)
    for c in cases.all_cases():
        assert c.v.dtype == np.float32 and c.v.min() == 0 and c.v.max() < 1e18 and 1 <= c.k <= len(c.v) <= 2048
    for c in grid:
        assert c.v[0] == 0


def test_committed_killers_are_what_libstdcxx_gives(trace_lib):
    """(a) Regenerated here, the adversary's sequences equal tests/golden/topk_killers.npz."""
    fresh, committed = cases.make_killers(trace_lib), cases.load_killers()
    assert sorted(fresh) == sorted(committed)
    for name in fresh:
        assert fresh[name].dtype == committed[name].dtype and np.array_equal(fresh[name], committed[name]), name


def test_every_case_takes_the_branch_it_is_named_for(trace_lib, order_lib):
    """(b) + (c): counters of the instrumented walk per case; the walk, stl_order.hpp and torch.topk give the same ids."""
    total = dict.fromkeys(cases.COUNTERS, 0)
    print("\n%-36s %5s %5s  %s" % ("case", "n", "k", " ".join("%15s" % c for c in cases.COUNTERS)))
    for c in cases.all_cases():
        n = len(c.v)
        ids, cnt = cases.trace(trace_lib, c.v, c.k)
        print("%-36s %5d %5d  %s" % (c.name, n, c.k, " ".join("%15d" % cnt[x] for x in cases.COUNTERS)))
        for x in cases.COUNTERS:
            total[x] += cnt[x]
        want = cases.expected_branches(n, c.k)
        assert (cnt["partial_sort"] == 1) == want["partial_sort"], c.name
        assert (cnt["two_pass"] == 1) == want["two_pass"], c.name
        if want["partial_sort"]:
            assert cnt["part_le64"] == cnt["part_gt64"] == cnt["select_fallback"] == cnt["sort_fallback"] == 0, c.name
        if c.name.startswith("select_killer"):
            assert cnt["select_fallback"] == 1 and cnt["sort_fallback"] >= 1 and cnt["part_gt64"] >= 20, c.name
        if c.name.startswith("sort_killer"):
            assert cnt["select_fallback"] == 0 and cnt["sort_fallback"] >= 1 and cnt["part_le64"] >= 1 and cnt["part_gt64"] >= 1, c.name
        x = -c.v
        assert np.array_equal(ids, stl_order_topk(order_lib, x, c.k)), c.name      # the walk mirrors the shipped loops
        assert np.array_equal(ids, torch.topk(torch.from_numpy(x), c.k, sorted=True)[1].numpy()), c.name
    print("%-36s %5s %5s  %s" % ("total", "", "", " ".join("%15d" % total[x] for x in cases.COUNTERS)))
    assert all(total[x] > 0 for x in cases.COUNTERS), total
    # the two-pass placement is also reached by a killer (the fallbacks and the large placement in one run)
    assert cases.trace(trace_lib, cases.load_killers()["sort_killer_m1200_n1217"], 1201)[1]["two_pass"] == 1


def test_planted_pair_hands_the_sequence_to_the_selection():
    """(d) Under the oracle the planted pair's cycle distances are the chosen values bit for bit, every query maps to patch 0,
    and the ids are torch.topk's -- for every case, the killers (whose zero is not at index 0) included."""
    for c in cases.all_cases():
        pts, qf, obj = cases.planted_inputs(c.v)
        q_ids, o_ids, dists, _, dbg = om.cyclic_buddies(pts, qf, obj, c.k, topk_mode="torch")
        assert np.array_equal(dbg["cycle_dists"].view(np.uint32), c.v.view(np.uint32)), c.name
        assert np.all(o_ids == 0), c.name
        assert np.array_equal(q_ids, torch.topk(torch.from_numpy(-c.v), c.k, sorted=True)[1].numpy()), c.name
        assert np.array_equal(dists, c.v[q_ids]), c.name
