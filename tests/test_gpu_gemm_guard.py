"""What the 352-row GEMM tiles (csrc/gemm_kernel.hpp) do with the rows behind their operands, and one comparison with fp64.

352 rows divide no padded M: the last m-tile of a launch passes M_valid and can pass M, the end of A and of the folded form's `ln_row` table.  The tile tests
(test_gpu_gemm_tile352.py, test_gpu_gemm_tile352_wide.py) compare tiles with tiles on exact-size operands, so a read past an operand is nothing they can see.
Here every operand is the leading part of a larger tensor of the test's own -- A with 352 guard rows, `ln_row` with 352 guard entries, `bias` and `colsum` with
256, W with 256 guard rows --, so a read past an operand stays inside memory this test allocated, and the guards (and the rows of A in [M_valid, M), which
no stored output row depends on) are filled once with zeros and once with NaN.  The 352-row and the 256-row launch must give identical bits under both fills,
and leave every byte they must not write.  The shapes are the smallest that hold a tile which passes M: (512, 512, 128, 353) -- a one-row second tile --
and (512, 512, 64, 352) for epilogues 0 and 1, N = 1024 with M_valid = 352 / 353 for the (hi, lo) residual epilogue.

The zero-guard 352-row output of the first shape is also held against the fp64 product of the same rounded operands under the bars of the 128- and 256-row
tiles' own fp64 tests (test_gemm_bf16_epilogues, test_gemm_f16_epilogues_vs_fp64): the one comparison that leaves the tile-against-tile chain.
"""

import pytest
import torch

from foundpose_amd import _lib, ops

pytestmark = pytest.mark.gpu

A_GUARD, W_GUARD, VEC_GUARD = 352, 256, 256
LD_PAD = 8          # padding columns of the output rows
SENTINEL = -7.25    # exact in bf16 and fp16
NAN = float("nan")


def guarded(t, extra, fill):
    """t [rows, ...] -> (buffer with `extra` more leading-dimension entries holding `fill`, view of its first rows)."""
    buf = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


_base = {}


def base_operands(M, N, K, f16):
    key = (M, N, K, f16)
    if key not in _base:
        dev = torch.device("cuda")
        dt = torch.float16 if f16 else torch.bfloat16
        g = torch.Generator(device=dev).manual_seed(352 + M + N + K)
        a = (torch.randn(M, K, device=dev, generator=g) * 2.0 + 0.5).to(dt)
        w = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(dt)
        bias = torch.randn(N, device=dev, generator=g) * 0.1
        colsum = w.float().sum(dim=1).contiguous()
        af = a.float()
        rstd = torch.rsqrt(af.var(dim=1, unbiased=False) + 1e-6)
        ln_row = torch.stack([rstd, af.mean(dim=1) * rstd], dim=1).contiguous()
        _base[key] = (a, w, bias, colsum, ln_row)
    return _base[key]


def filled_operands(M, N, K, m_valid, f16, fill):
    a, w, bias, colsum, ln_row = base_operands(M, N, K, f16)
    a = a.clone()
    a[m_valid:] = fill
    return guarded(a, A_GUARD, fill), guarded(w, W_GUARD, fill), guarded(bias, VEC_GUARD, fill), guarded(colsum, VEC_GUARD, fill), guarded(ln_row, A_GUARD, fill)


def launch_wide(tile, shape, f16, epilogue, folded, fill):
    M, N, K, m_valid = shape
    a, w, bias, colsum, ln_row = filled_operands(M, N, K, m_valid, f16, fill)
    buf = torch.full((M, N + LD_PAD), SENTINEL, dtype=a.dtype, device=a.device)
    out = buf[:, :N]
    if folded:
        ops.gemm_bf16_ln(a, w, bias, colsum, ln_row, epilogue=epilogue, out=out, tile=tile, m_valid=m_valid)
    else:
        ops.gemm_bf16(a, w, bias, out=out, epilogue=epilogue, m_valid=m_valid, tile=tile)
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("folded", [False, True], ids=["plain", "folded"])
@pytest.mark.parametrize("epilogue", [0, 1], ids=["bias", "gelu"])
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", [(512, 512, 128, 353), (512, 512, 64, 352)], ids=["row-353", "one-tile"])
def test_wide_tiles_ignore_what_lies_behind_their_operands(shape, f16, epilogue, folded):
    M, N, K, m_valid = shape
    outs = {(tile, name): launch_wide(tile, shape, f16, epilogue, folded, fill) for tile in (352, 256) for name, fill in (("zero", 0.0), ("nan", NAN))}
    first = outs[(352, "zero")]
    live = first[:m_valid, :N].float()
    assert torch.isfinite(live).all() and not (live == SENTINEL).all(dim=1).any()
    for key, other in outs.items():
        assert torch.equal(first.view(torch.int16), other.view(torch.int16)), key
    assert (first[m_valid:] == SENTINEL).all() and (first[:, N:] == SENTINEL).all()
    if shape != (512, 512, 128, 353):
        return
    # ---- against fp64 on the same rounded operands
    a, w, bias, colsum, ln_row = (t.double() for t in base_operands(M, N, K, f16))
    lin = a @ w.T
    if folded:   # the folded form's arithmetic: rstd (a w^T) - mean rstd colsum + bias
        lin = ln_row[:, :1] * lin - ln_row[:, 1:] * colsum
    ref = (lin + bias)[:m_valid]
    scale = float(ref.abs().max())
    if epilogue == 1:
        ref = torch.nn.functional.gelu(ref)
    err = float((live.double() - ref).abs().max())
    # one rounding of the result to the 16-bit format (+ the GELU polynomial's 4e-5 in fp16): the bars of test_gemm_bf16_epilogues / test_gemm_f16_epilogues_vs_fp64
    bar = (1.01 * 2.0 ** -11 * scale + (4e-5 if epilogue == 1 else 0.0)) if f16 else 2.0 ** -8 * scale
    print(f"tile 352 vs fp64: {err:.3e} (bar {bar:.3e})")
    assert err < bar, (err, bar)


EPI_RESID_HILO = 8
N_RESID = 1024


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "f16"])
@pytest.mark.parametrize("m_valid", [352, 353])
def test_residual_tiles_ignore_what_lies_behind_their_operands(m_valid, f16):
    dev = torch.device("cuda")
    dt = torch.float16 if f16 else torch.bfloat16
    N, K = N_RESID, 128
    M = -(-m_valid // 256) * 256 + 256    # as test_gpu_gemm_tile352.py: whole 256-row tiles and one more of rows nothing may touch
    g = torch.Generator(device=dev).manual_seed(352 + m_valid + K)
    a0 = torch.randn(M, K, device=dev, generator=g).to(dt)
    w0 = (torch.randn(N, K, device=dev, generator=g) * 0.02).to(dt)
    bias0 = torch.randn(N, device=dev, generator=g) * 0.1
    x = torch.randn(M, N + LD_PAD, device=dev, generator=g) * 3.0
    hi0 = x.to(dt)
    lo0 = (x - hi0.float()).to(dt)
    stats0 = torch.full((N // 128, M, 2), SENTINEL, device=dev)
    outs = {}
    for tile in (352, 256):
        for name, fill in (("zero", 0.0), ("nan", NAN)):
            a = a0.clone()
            a[m_valid:] = fill
            a, w, bias = guarded(a, A_GUARD, fill), guarded(w0, W_GUARD, fill), guarded(bias0, VEC_GUARD, fill)
            xb, xl, stats = hi0.clone(), lo0.clone(), stats0.clone()
            _lib.call("fp_gemm_bf16_ln", _lib.ptr(a), a.stride(0), _lib.ptr(w), w.stride(0), M, N, K, m_valid, _lib.ptr(bias), _lib.ptr(xl), xl.stride(0),
                      EPI_RESID_HILO | (tile << 8) | (_lib.GEMM_F16 if f16 else 0), None, None, _lib.ptr(xb), xb.stride(0), _lib.ptr(stats), _lib.stream())
            torch.cuda.synchronize()
            outs[(tile, name)] = (xb.view(torch.int16), xl.view(torch.int16), stats)
    h, l, s = outs[(352, "zero")]
    assert not torch.equal(h[:m_valid, :N], hi0.view(torch.int16)[:m_valid, :N])
    assert torch.isfinite(s[:, :m_valid]).all() and (s[:, :m_valid, 1] > 0).all()
    for key, (h2, l2, s2) in outs.items():
        assert torch.equal(h, h2) and torch.equal(l, l2) and torch.equal(s, s2), key
    # rows past M_valid and the padding columns keep their bytes
    for got, init in ((h, hi0.view(torch.int16)), (l, lo0.view(torch.int16))):
        assert torch.equal(got[m_valid:], init[m_valid:]) and torch.equal(got[:, N:], init[:, N:])
    assert torch.equal(s[:, m_valid:], stats0[:, m_valid:])
