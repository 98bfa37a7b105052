"""The 352 x 256 block tile of the wide GEMMs (epilogues 0 and 1: qkv and fc1 of a ViT block, csrc/gemm_kernel.hpp), plain and with the folded LayerNorm.

The taller tile exists to turn the bench batch's 125 m-tiles into whole XCD rounds; it must compute what the 320- and 256-row tiles compute, bit for bit: the K
order of an accumulator, the folded-LayerNorm correction, the bias and the GELU polynomial are per-element arithmetic that does not know the tile.  So the bar is
`torch.equal` between a launch forced to 352 rows and launches forced to 320 rows (where M is a whole number of them) and 256 rows on the same operands, and every element a launch must not write (rows
past m_valid, the padding columns of a row stride wider than N) keeps the sentinel the output was filled with.

352 divides no padded M: the last m-tile of a launch passes m_valid and can pass M.  The folded form's `ln_row` has exactly M rows, so the row guard of that
table is the code that runs here; a read past it is not something this test can see (tests/test_gpu_gemm_guard.py puts NaN behind every operand for that).
The launcher's pick is host arithmetic on (padded rows, live rows, columns, compute units) and is checked without a device.
"""

import pytest
import torch

from foundpose_amd import _lib, ops

LD_PAD = 8          # padding columns of the output rows (16 bytes, the alignment the epilogue asks for)
SENTINEL = -7.25    # exact in bf16 and fp16

# cost = rounds x height x factor (csrc/gemm_kernel.hpp: WIDE_FACTOR_320 and, measured per raster, WIDE_FACTOR_352_R8X4 (qkv's) and WIDE_FACTOR_352_R4X8 (fc1's):
# profiles/EXPERIMENTS.md section 0.8)
F320, F352_R8X4, F352_R4X8 = 0.97, 1.02, 1.05

# (M, N, K, m_valid)
SHAPES = {
    # no raster (fewer than 512 tiles)
    "one-tile": (512, 512, 64, 352),              # one full tile, one K-tile
    "row-353": (512, 512, 128, 353),              # a one-row second tile whose rows pass M
    "one-crop": (1536, 3072, 1024, 1374),
    # raster 8 x 4 (qkv's): 43 m-tiles + 1 row = 44, a ragged last super-row (4 of 8), a grid of 6 x 3 x 32 = 576
    "raster-8x4": (15360, 3072, 128, 15137),
    # raster 4 x 8 (fc1's): 33 m-tiles, the last super-row holds one m-tile of four, a grid of 9 x 2 x 32 = 576
    "raster-4x8": (11520, 4096, 128, 11265),
}


def pick(m, m_valid, n, cus):
    import os
    if not os.path.exists(_lib.LIB_PATH):
        from foundpose_amd import build
        build.build(verbose=False)
    return _lib.lib().fp_gemm_wide_tile_rows(m, m_valid, n, cus)


def rounds(bm, m_valid, n, cus):
    """XCD rounds of a launch: with the super-tile raster (more than 4 n-tiles, at least 512 tiles) an XCD takes one super-tile of 32 tiles per round, else
    the tiles are cut into one chunk per XCD and an XCD runs cus / 8 of them at a time."""
    m_tiles, n_tiles = -(-m_valid // bm), n // 256
    r, gn = (4, 8) if n_tiles % 8 == 0 else (8, 4)
    if n_tiles % gn == 0 and n_tiles > 4 and m_tiles * n_tiles >= 512:
        return -(-(-(-m_tiles // r) * (n_tiles // gn)) // 8)
    return -(-(-(-m_tiles * n_tiles // 8)) // (cus // 8))


def want(m, m_valid, n, cus):
    tiles_big = (m // 256) * (n // 256)   # a launch that does not fill the device with 256^2 tiles never takes a taller one
    if tiles_big < cus or cus < tiles_big < cus + cus // 2:
        return 256
    best, cost = 256, rounds(256, m_valid, n, cus) * 256
    if m % 320 == 0:
        c320 = rounds(320, m_valid, n, cus) * 320 * F320
        if c320 < cost:
            best, cost = 320, c320
    # 352 rows only for a launch on the super-tile raster, where its factor was measured
    n_tiles = n // 256
    rastered = n_tiles > 4 and n_tiles % 4 == 0 and -(-m_valid // 352) * n_tiles >= 512
    if rastered and rounds(352, m_valid, n, cus) * 352 * (F352_R4X8 if n_tiles % 8 == 0 else F352_R8X4) < cost:
        best = 352
    return best


def test_pick_follows_rounds_times_height_times_factor():
    # the bench batch, 32 crops x 1374 tokens in 44 800 padded rows: 138 m-tiles of 320 rows, 125 of 352
    for cus in (64, 256, 304):
        # qkv, raster 8 x 4: 18 super-rows x 3 = 54 super-tiles = 7 rounds of 320 rows; 16 x 3 = 48 = 6 whole rounds of 352
        assert (rounds(256, 43968, 3072, cus), rounds(320, 43968, 3072, cus), rounds(352, 43968, 3072, cus)) == (9, 7, 6)
        # fc1, raster 4 x 8: 35 x 2 = 70 = 9 rounds of 320 rows; 32 x 2 = 64 = 8 whole rounds of 352
        assert (rounds(256, 43968, 4096, cus), rounds(320, 43968, 4096, cus), rounds(352, 43968, 4096, cus)) == (11, 9, 8)
        for n in (3072, 4096):
            assert pick(44800, 43968, n, cus) == want(44800, 43968, n, cus), (n, cus)
        # one crop: 48 or 64 tiles of 352 rows, far from a raster launch -- never 352
        assert want(1536, 1374, 3072, cus) == 256 and want(1536, 1374, 4096, cus) == 256
        assert pick(1536, 1374, 3072, cus) == 256 and pick(1536, 1374, 4096, cus) == 256
        # a sweep of batch sizes, padded as the extractor pads them
        for b in (8, 12, 16, 20, 24, 28, 30, 32, 33, 34, 35, 36, 38, 40, 44, 48, 56, 64):
            mv = b * 1374
            m = -(-mv // 1280) * 1280
            for n in (3072, 4096):
                assert pick(m, mv, n, cus) == want(m, mv, n, cus), (b, n, cus)
    # the measured factors: qkv takes 352 rows at the bench batch (6 x 352 x 1.02 = 2154 against 7 x 320 x 0.97 = 2173), fc1 keeps 320 (8 x 352 x 1.05 = 2957 against 9 x 320 x 0.97 = 2794)
    assert 6 * 352 * F352_R8X4 < 7 * 320 * F320 and 8 * 352 * F352_R4X8 > 9 * 320 * F320
    for cus in (64, 256, 304):
        assert pick(44800, 43968, 3072, cus) == 352 and pick(44800, 43968, 4096, cus) == 320
    # degenerate arguments keep the default
    assert pick(0, 0, 3072, 256) == 256 and pick(44800, 0, 3072, 256) == 256 and pick(44800, 44801, 3072, 256) == 256
    assert pick(44800, 43968, 3000, 256) == 256 and pick(44800, 43968, 3072, 0) == 256 and pick(44801, 43968, 3072, 256) == 256


_operands = {}


def operands(shape, f16):
    """One set of operands per (shape, format), shared by the epilogues and forms; never modified."""
    key = (shape, f16)
    if key not in _operands:
        if any(k[0] != shape for k in _operands):
            _operands.clear()   # (one shape's operands at a time)
        M, N, K, m_valid = SHAPES[shape]
        dev = torch.device("cuda")
        dt = torch.float16 if f16 else torch.bfloat16
        g = torch.Generator(device=dev).manual_seed(352 + M + N)
        a = (torch.randn(M, K, device=dev, generator=g) * 2.0 + 0.5).to(dt)
        w = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(dt)
        bias = torch.randn(N, device=dev, generator=g) * 0.1
        colsum = w.float().sum(dim=1).contiguous()
        af = a.float()
        mean = af.mean(dim=1)
        rstd = torch.rsqrt(af.var(dim=1, unbiased=False) + 1e-6)
        ln_row = torch.stack([rstd, mean * rstd], dim=1).contiguous()   # exactly M rows
        assert ln_row.shape == (M, 2)
        _operands[key] = (a, w, bias, colsum, ln_row)
    return _operands[key]


def launch(tile, shape, f16, epilogue, folded):
    M, N, K, m_valid = SHAPES[shape]
    a, w, bias, colsum, ln_row = operands(shape, f16)
    buf = torch.full((M, N + LD_PAD), SENTINEL, dtype=a.dtype, device=a.device)
    out = buf[:, :N]   # row stride N + LD_PAD
    if folded:
        ops.gemm_bf16_ln(a, w, bias, colsum, ln_row, epilogue=epilogue, out=out, tile=tile, m_valid=m_valid)
    else:
        ops.gemm_bf16(a, w, bias, out=out, epilogue=epilogue, m_valid=m_valid, tile=tile)
    torch.cuda.synchronize()
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("folded", [False, True], ids=["plain", "folded"])
@pytest.mark.parametrize("epilogue", [0, 1], ids=["bias", "gelu"])
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_tile352_equals_tile320_and_tile256_bit_for_bit(shape, epilogue, folded, f16):
    M, N, K, m_valid = SHAPES[shape]
    assert M % 256 == 0 and N % 256 == 0
    b352 = launch(352, shape, f16, epilogue, folded)
    # the launch did something, and finite
    live = b352[:m_valid, :N].float()
    assert torch.isfinite(live).all() and not (live == SENTINEL).all(dim=1).any()
    # the same bits from every tile
    # (the 320-row tile needs M to be a whole number of its tiles: the two raster shapes; the small shapes are compared with the 128-row tile in its place)
    for tile in (320 if M % 320 == 0 else 128, 256):
        other = launch(tile, shape, f16, epilogue, folded)
        assert torch.equal(b352.view(torch.int16), other.view(torch.int16)), tile
    # rows past m_valid and the padding columns keep the sentinel
    assert (b352[m_valid:] == SENTINEL).all()
    assert (b352[:, N:] == SENTINEL).all()
