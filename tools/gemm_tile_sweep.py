"""qkv / fc1 GEMM (folded-LayerNorm form) at 18 batch sizes with 256-, 320- and 352-row block tiles: the data the launcher's tile chooser
(csrc/gemm_kernel.hpp::wide_tile_rows, XCD rounds) is calibrated and validated on.  HIP events around 20 launches, three repetitions per tile, the tiles
taking turns; per tile the fastest repetition and the spread of the three.   python tools/gemm_tile_sweep.py > profiles/rN_gemm_tile_sweep.txt"""
import torch, sys
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from foundpose_amd import _lib, ops
from tools.bench_kernels import timeit
dev = 'cuda'; K = 1024
TILES = (256, 320, 352)
cus = torch.cuda.get_device_properties(0).multi_processor_count
for name, n, epi in (("qkv", 3072, 0), ("fc1", 4096, 1)):
    w = (torch.randn(n, K, device=dev) * 0.02).to(torch.bfloat16); bias = torch.randn(n, device=dev)
    cs, = (torch.zeros(n, device=dev),)
    for B in (8, 12, 16, 20, 24, 28, 30, 32, 33, 34, 35, 36, 38, 40, 44, 48, 56, 64):
        mv = B * 1374
        M = (mv + 1279) // 1280 * 1280
        a = torch.randn(M, K, device=dev).to(torch.bfloat16)
        out = torch.zeros(M, n, dtype=torch.bfloat16, device=dev)
        ln_row = torch.ones(M, 2, device=dev)
        r = {t: [] for t in TILES}
        for rep in range(3):
            for tile in TILES:
                ms = timeit(lambda: ops.gemm_bf16_ln(a, w, bias, cs, ln_row, epilogue=epi, out=out, tile=tile, m_valid=mv), iters=20)
                r[tile].append(ms * 1e3)
        tl = {t: ((mv + t - 1) // t) * (n // 256) for t in TILES}
        t = {k: min(v) for k, v in r.items()}
        sp = {k: max(v) - min(v) for k, v in r.items()}
        pick = _lib.lib().fp_gemm_wide_tile_rows(M, mv, n, cus)
        print(f"{name} B={B} mv={mv} r256={tl[256]/256:.2f} r320={tl[320]/256:.2f} r352={tl[352]/256:.2f} t256={t[256]:.1f} t320={t[320]:.1f} t352={t[352]:.1f} "
              f"spread={sp[256]:.1f}/{sp[320]:.1f}/{sp[352]:.1f} 352/320={t[352]/t[320]:.3f} fastest={min(t, key=t.get)} pick={pick}", flush=True)
