"""Writes tests/golden/topk_killers.npz: the four sequences on which libstdc++'s median-of-3 quicksort runs out of its depth
limit inside torch.topk's CPU kernel (McIlroy's adversary, tests/csrc/stl_trace.cpp; the cases are named in
tests/topk_replay_cases.py).  Needs g++ only; tests/test_topk_replay_cpu.py regenerates them and compares.

    python tools/make_golden_topk_killers.py
"""

import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import topk_replay_cases as cases  # noqa: E402


def main() -> None:
    with tempfile.TemporaryDirectory() as tmp:
        lib = cases.build_trace_lib(tmp)
        killers = cases.make_killers(lib)
        for name, v in killers.items():
            _, counters = cases.trace(lib, v, cases.KILLERS[name][2])
            print(name, len(v), counters)
    os.makedirs(os.path.dirname(cases.GOLDEN), exist_ok=True)
    np.savez_compressed(cases.GOLDEN, **killers)
    print(f"wrote {cases.GOLDEN} ({os.path.getsize(cases.GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
