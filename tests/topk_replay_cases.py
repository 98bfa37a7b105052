"""Named (values, k) cases for the replay of torch.topk's tie order, shared by tests/test_topk_replay_cpu.py,
tests/test_gpu_topk_replay.py and tools/make_golden_topk_killers.py.

A case is a sequence v of non-negative fp32 cycle distances that holds a zero, and a k; the thing replayed is
`torch.topk(-v, k, sorted=True)` on a CPU tensor.  `planted_inputs` turns v into a (query crop, one-patch template) pair
whose cycle distances are exactly v, so the device selects from a sequence the test chose:

  * the template is one patch and all Q query features equal it: every query's nearest template patch is patch 0, and
    patch 0's nearest query is query 0 (all feature distances tie, the lowest index wins);
  * query 0 sits at (0, 0) and query i at (v[i], 0): cycle_dists[i] = sqrt(v[i]^2 + 0) = v[i] exactly.

Query 0 is its own cycle partner there, so v[0] must be 0: every value family is built that way.  The adversary decides
where its zeros fall (rank 0 and 1), and forcing v[0] = 0 on a killer loses the fallbacks it exists for.  For a sequence
with v[0] != 0 the anchor is the first query a with v[a] == 0: it alone carries the template's feature, every other query
one shared feature a step away, so patch 0's nearest query is query a without a tie and the same identity holds.

The grid of cases crosses every length with every k (k = floor(n / 64) and + 1 is the partial_sort / nth_element seam,
k - 1 = 512 / 513 the seam between the register placement and the two-pass placement of stl_wave::sort) and rotates the
value families so that each one meets n = 1369 and n = 2048.  The four killers come from McIlroy's adversary run against
libstdc++ (tests/csrc/stl_trace.cpp) and are committed as tests/golden/topk_killers.npz, so the GPU test needs no compiler.
"""

import ctypes
import os
import subprocess
from typing import Dict, List, NamedTuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "topk_killers.npz")

LENGTHS = (64, 65, 66, 129, 517, 1369, 2047, 2048)
FAMILIES = ("random_distinct", "grid14", "all_zero", "two_values_runs37", "ascending", "descending", "organ_pipe", "levels11_runs37")
COUNTERS = ("partial_sort", "part_le64", "part_gt64", "select_fallback", "sort_fallback", "two_pass")

# name -> (kind, n, k, m): "select": the adversary against nth_element(k - 1) + sort(k - 1) on n items; "sort": against
# std::sort of m items, placed first and followed by n - m strictly worse values, k = m + 1
KILLERS = {
    "select_killer_n1369_k300": ("select", 1369, 300, 0),
    "select_killer_n2048_k2040": ("select", 2048, 2040, 0),
    "sort_killer_m64_n564": ("sort", 564, 65, 64),
    "sort_killer_m1200_n1217": ("sort", 1217, 1201, 1200),
}


class Case(NamedTuple):
    name: str
    v: np.ndarray   # [n] f32, min 0 (v[0] == 0 in the grid cases)
    k: int


def ks_for(n: int) -> List[int]:
    ks = []
    for k in (1, 7, n // 64, n // 64 + 1, 300, 513, 514, n - 1, n):
        if 1 <= k <= n and k not in ks:
            ks.append(k)
    return ks


def family_values(family: str, n: int) -> np.ndarray:
    i = np.arange(n)
    if family == "random_distinct":
        v = np.concatenate([[0], np.random.default_rng(n).permutation(np.arange(1, n))]) * 0.37
    elif family == "grid14":     # the production tie pattern: distances between points of the 14-px patch grid
        g = np.random.default_rng(1000 + n).integers(0, 6, (n, 2))
        v = 14.0 * np.sqrt((g[:, 0] ** 2 + g[:, 1] ** 2).astype(np.float64))
    elif family == "all_zero":
        v = np.zeros(n)
    elif family == "two_values_runs37":
        v = 14.0 * ((i // 37) % 2)
    elif family == "ascending":
        v = i.astype(np.float64)
    elif family == "descending":
        v = np.concatenate([[0], np.arange(n - 1, 0, -1)]).astype(np.float64)
    elif family == "organ_pipe":
        v = np.minimum(i, n - 1 - i).astype(np.float64)
    elif family == "levels11_runs37":
        v = 14.0 * ((i // 37) % 11)
    else:
        raise ValueError(family)
    v = np.asarray(v, np.float32)
    v[0] = 0.0
    return v


def grid_cases() -> List[Case]:
    out = []
    for a, n in enumerate(LENGTHS):
        for b, k in enumerate(ks_for(n)):
            fam = FAMILIES[(3 * a + b) % len(FAMILIES)]
            out.append(Case(f"n{n}_k{k}_{fam}", family_values(fam, n), k))
    return out


def expected_branches(n: int, k: int) -> Dict[str, bool]:
    """What (n, k) alone decides: the partial_sort branch and the two-pass placement."""
    partial = k * 64 <= n
    return {"partial_sort": partial, "two_pass": (not partial) and k - 1 > 512}


# ------------------------------------------------------------------ the host harness (adversary + instrumented walk)
def build_trace_lib(out_dir: str) -> ctypes.CDLL:
    so = os.path.join(str(out_dir), "libstl_trace.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "csrc", "stl_trace.cpp")])
    return ctypes.CDLL(so)


def adversary_ranks(lib: ctypes.CDLL, n: int, k: int) -> np.ndarray:
    ranks = np.empty(n, np.int64)
    lib.stl_trace_adversary(ctypes.c_int64(n), ctypes.c_int64(k), ranks.ctypes.data_as(ctypes.c_void_p))
    return ranks


def make_killers(lib: ctypes.CDLL) -> Dict[str, np.ndarray]:
    """The four killer sequences from this machine's libstdc++.  A frozen rank r is planted as the distance r // 2, so the
    sequence carries its ties in pairs."""
    out = {}
    for name, (kind, n, k, m) in KILLERS.items():
        if kind == "select":
            v = adversary_ranks(lib, n, k) // 2
        else:
            head = adversary_ranks(lib, m, 0) // 2
            v = np.concatenate([head, head.max() + 1 + np.arange(n - m)])
        assert v.min() == 0 and v.shape == (n,)
        out[name] = v.astype(np.float32)
    return out


def trace(lib: ctypes.CDLL, v: np.ndarray, k: int):
    """-> (ids of stl_order.hpp's topk_torch_largest(-v, k) [k] i64, {counter: count})."""
    x = np.ascontiguousarray(-np.asarray(v, np.float32))
    ids, cnt = np.empty(k, np.int64), np.zeros(len(COUNTERS), np.int64)
    lib.stl_trace_topk(x.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(x)), ctypes.c_int64(k), ids.ctypes.data_as(ctypes.c_void_p),
                       cnt.ctypes.data_as(ctypes.c_void_p))
    return ids, dict(zip(COUNTERS, (int(c) for c in cnt)))


# ------------------------------------------------------------------ committed killers, the full list, the planted inputs
def load_killers() -> Dict[str, np.ndarray]:
    with np.load(GOLDEN) as z:
        return {name: z[name] for name in KILLERS}


def killer_cases() -> List[Case]:
    g = load_killers()
    return [Case(name, g[name], KILLERS[name][2]) for name in KILLERS]


def all_cases() -> List[Case]:
    return grid_cases() + killer_cases()


def planted_inputs(v: np.ndarray, dim: int = 32):
    """-> (query points [Q, 2], query features [Q, dim], template features [1, dim]), all f32."""
    v = np.asarray(v, np.float32)
    assert np.all(v >= 0) and np.all(v < 1e18) and np.any(v == 0)
    anchor = int(np.flatnonzero(v == 0)[0])
    pts = np.stack([v, np.zeros_like(v)], 1)
    obj = (np.arange(dim, dtype=np.float32)[None] % 7 - 3) * np.float32(0.25)
    qf = np.repeat(obj, len(v), 0)
    if anchor != 0:
        qf[:, 0] += np.float32(0.5)
        qf[anchor] = obj[0]
    return pts, qf, obj
