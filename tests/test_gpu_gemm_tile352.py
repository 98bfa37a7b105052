"""The 352 x 256 block tile of the residual GEMMs on the (hi, lo) stream (epilogue 8: attn.proj and mlp.fc2 of a ViT block, csrc/gemm_kernel.hpp).

The taller tile exists to turn the 2.69 rounds of 256-row tiles of the bench batch into two full ones; it must compute what the 256-row tile computes, bit for
bit: the K order of every accumulator, the hi / lo split and the 128-column LayerNorm partial sums are per-row arithmetic that does not know the tile.  So the
bar is equality -- of the hi array, the lo array and the partial sums -- between a launch forced to 352 rows and one forced to 256 rows on the same operands,
and every byte a launch must not write (rows past M_valid, the padding columns of the rows it does write) has to keep its value.
The launcher's pick is host arithmetic on (live rows, columns, compute units) and is checked without a device.
"""

import numpy as np
import pytest
import torch

from foundpose_amd import _lib

EPI_RESID_HILO = 8
N = 1024          # ViT-L width: 4 n-tiles, the launches the tile was built for
LD_PAD = 8        # padding columns of the stream's rows (16 bytes, the alignment the epilogue asks for)


def pick(m_valid, n, cus):
    import os
    if not os.path.exists(_lib.LIB_PATH):
        from foundpose_amd import build
        build.build(verbose=False)
    return _lib.lib().fp_gemm_resid_tile_rows(m_valid, n, cus)


def rounds(bm, m_valid, n, cus):
    """XCD rounds of a launch without raster (N = 4 n-tiles): the tiles are cut into one chunk per XCD, an XCD runs cus / 8 of them at a time."""
    tiles = -(-m_valid // bm) * (n // 256)
    return -(-(-(-tiles // 8)) // (cus // 8))


def test_pick_is_352_only_where_it_saves_rounds_and_rows():
    # the bench batch, 32 crops x 1374 tokens: 688 tiles of 256 rows = 3 rounds (768 tile rows per CU), 500 of 352 = 2 rounds (704)
    assert (rounds(256, 43968, N, 256), rounds(352, 43968, N, 256)) == (3, 2)
    assert pick(43968, N, 256) == 352
    # 256 crops: 22 rounds of 256 rows against 16 of 352 -- the same 5632 tile rows per CU: nothing to gain, today's pick stays
    assert (rounds(256, 351744, N, 256), rounds(352, 351744, N, 256)) == (22, 16)
    assert 22 * 256 == 16 * 352
    assert pick(351744, N, 256) == 256
    # one crop: one round either way
    assert (rounds(256, 1374, N, 256), rounds(352, 1374, N, 256)) == (1, 1)
    assert pick(1374, N, 256) == 256
    # degenerate arguments keep the default
    assert pick(0, N, 256) == 256 and pick(43968, 1000, 256) == 256 and pick(43968, N, 0) == 256


def test_pick_never_takes_352_for_more_tile_rows():
    for cus in (256, 304, 64):
        for m in list(range(1, 6000, 37)) + [43968, 44000, 87936, 351744]:
            r256, r352 = rounds(256, m, N, cus), rounds(352, m, N, cus)
            want = 352 if (r352 < r256 and r352 * 352 < r256 * 256) else 256
            assert pick(m, N, cus) == want, (m, cus)


def _launch(tile, f16, a, w, bias, xb, xl, stats, m_valid):
    M, K = a.shape
    bits = EPI_RESID_HILO | (tile << 8) | (_lib.GEMM_F16 if f16 else 0)
    _lib.call("fp_gemm_bf16_ln", _lib.ptr(a), a.stride(0), _lib.ptr(w), w.stride(0), M, N, K, m_valid, _lib.ptr(bias), _lib.ptr(xl), xl.stride(0), bits,
              None, None, _lib.ptr(xb), xb.stride(0), _lib.ptr(stats), _lib.stream())
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
@pytest.mark.parametrize("K", [1024, 4096])
@pytest.mark.parametrize("m_valid", [43968, 352, 353, 1374, 44000 - 1])
def test_tile352_equals_tile256_bit_for_bit(m_valid, K, f16):
    dev = torch.device("cuda")
    dt = torch.float16 if f16 else torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(352 + m_valid + K)
    M = -(-m_valid // 256) * 256 + 256    # whole 256-row tiles and one more of rows nothing may touch
    a = torch.randn(M, K, device=dev, generator=g).to(dt)
    w = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(dt)
    bias = torch.randn(N, device=dev, generator=g) * 0.1
    x = torch.randn(M, N + LD_PAD, device=dev, generator=g) * 3.0
    hi0 = x.to(dt)
    lo0 = (x - hi0.float()).to(dt)
    stats0 = torch.full((N // 128, M, 2), -7.25, device=dev)
    outs = {}
    for tile in (256, 352):
        xb, xl, stats = hi0.clone(), lo0.clone(), stats0.clone()
        _launch(tile, f16, a, w, bias, xb, xl, stats, m_valid)
        outs[tile] = tuple(t.view(torch.int16).cpu().numpy() if t.dtype == dt else t.cpu().numpy() for t in (xb, xl, stats))
    hi_i, lo_i, st_i = hi0.view(torch.int16).cpu().numpy(), lo0.view(torch.int16).cpu().numpy(), stats0.cpu().numpy()
    (h256, l256, s256), (h352, l352, s352) = outs[256], outs[352]
    # the launch did something, and finite
    assert not np.array_equal(h352[:m_valid, :N], hi_i[:m_valid, :N])
    assert np.isfinite(s352[:, :m_valid]).all() and (s352[:, :m_valid, 1] > 0).all()
    # the same bits from both tiles
    assert np.array_equal(h352, h256)
    assert np.array_equal(l352, l256)
    assert np.array_equal(s352, s256)
    # rows past M_valid and the padding columns keep their bytes
    for got, init in ((h352, hi_i), (l352, lo_i)):
        assert np.array_equal(got[m_valid:], init[m_valid:])
        assert np.array_equal(got[:, N:], init[:, N:])
    assert np.array_equal(s352[:, m_valid:], st_i[:, m_valid:])
