"""The ViT's pointwise arithmetic on the GPU, element by element against exact fp64 functions of pre-activations that are known exactly.

How a chosen pre-activation reaches an epilogue (tests/pointwise_ref.py, preact_grid): W is a 0/1 selection matrix and every value sits in
a row of A as a few pieces the operand format represents, so the fp32 accumulator is an exact short sum and the epilogue's own fp32 bias
add lands on a known fp32 number.  No GEMM rounding enters any bar.  Every bar is a source-stated bound (confirmed on the CPU by
tests/test_pointwise_cpu.py) or a multiple of the numpy restatement's own error on the same inputs; the checks live in pointwise_ref so
that the CPU test can feed them deliberately wrong arithmetic and see each of them fail.  Each assertion prints measured against bar.
"""

import functools
import math

import numpy as np
import pytest
import torch

from tests import pointwise_ref as R

pytestmark = pytest.mark.gpu

OUT_SCALE = 16.0        # split-row outputs: 3.5 x 1000 x 16 = 56000 stays inside both formats' range (65504 and 57344)
SA, SW = 1024.0, 128.0  # split-row operand scales: |a| <= 12 -> 12288; w = 1 -> 128 (its e4m3 copy, 128 x 2^-7, is exactly 1)


@functools.lru_cache(maxsize=None)
def _grid(fmt, swiglu=False):
    return R.preact_grid(fmt, swiglu)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(dtype).cuda()


def _unpack_split16(o, scale):
    g = o.reshape(o.shape[0], -1, 2, 32).double()
    return ((g[:, :, 0] + g[:, :, 1]) / scale).reshape(o.shape[0], -1).cpu().numpy()


def _unpack_splitx(o, scale):
    by = o.contiguous().view(torch.uint8).unflatten(1, (-1, 256))
    hi = by[:, :, :128].contiguous().view(torch.float16).double()
    lo = by[:, :, 192:256].contiguous().view(torch.float8_e4m3fn).double() * 2.0 ** -4
    return ((hi + lo) / scale).reshape(o.shape[0], -1).cpu().numpy()


def _launch(fmt, epi, tile=0, swiglu=False, fold=False):
    """-> (x [256, L] fp32 pre-activations, x2 or None, stored result as fp64 values [256, L], stored format, scale)."""
    from foundpose_amd import ops
    g = _grid(fmt, swiglu)
    bias = _t(g["bias"])
    if fmt in ("bf16", "f16"):
        dt = torch.bfloat16 if fmt == "bf16" else torch.float16
        a, w = _t(g["a"], dt), _t(g["w"], dt)
        assert np.array_equal(a.double().cpu().numpy(), g["a"]) and np.array_equal(w.double().cpu().numpy(), g["w"])   # the operands hold the pieces exactly
        if fold:     # the folded-LayerNorm consumer with (rstd, mean rstd) = (1, 0): the plain op
            ln_row = torch.tensor([[1.0, 0.0]]).repeat(256, 1).cuda()
            out = ops.gemm_bf16_ln(a, w, bias, torch.linspace(-3.0, 3.0, 256).cuda(), ln_row, epilogue=epi, tile=tile)
        else:
            out = ops.gemm_bf16(a, w, bias, epilogue=epi, tile=tile)
        return g["x"], g["x2"], out.double().cpu().numpy(), fmt, 1.0, out
    if fmt == "fp8":
        a, w = _t(g["a"], torch.float8_e4m3fn), _t(g["w"], torch.float8_e4m3fn)
        assert np.array_equal(a.double().cpu().numpy(), g["a"]) and np.array_equal(w.double().cpu().numpy(), g["w"])
        out = ops.gemm_fp8(a, w, bias, _t(g["col_scale"]), epilogue=epi | (tile << 8))
        return g["x"], g["x2"], out.double().cpu().numpy(), "bf16", 1.0, out
    if fmt in ("split16", "splitx"):
        sx = fmt == "splitx"
        pack, unpack = (ops.splitx_pack, _unpack_splitx) if sx else (ops.split16_pack, _unpack_split16)
        A, W = pack(_t(g["a"]), SA), pack(_t(g["w"]), SW)
        assert np.array_equal(unpack(A, SA), g["a"]) and np.array_equal(unpack(W, SW), g["w"])      # hi + lo holds every value exactly
        out = ops.gemm_split(A, W, bias, 1.0 / (SA * SW), epilogue=epi, out_scale=OUT_SCALE, tile=tile, f16f8=sx)
        if epi == 0 and sx:
            return g["x"], g["x2"], _unpack_split16(out, OUT_SCALE), "split16", OUT_SCALE, out    # the f16f8 BIAS output stays a split-fp16 row
        return g["x"], g["x2"], unpack(out, OUT_SCALE), fmt, OUT_SCALE, out
    assert fmt == "f32"
    out = ops.gemm_f32(_t(g["a"]), _t(g["w"]), bias, epilogue={1: 5, 6: 8, 0: 4}[epi])
    out = out[:, :g["x"].shape[1]]
    return g["x"], g["x2"], out.double().cpu().numpy(), "f32", 1.0, out


def _report(res):
    ok, measured, bar, text = res
    print(f"[pointwise] {text}")
    assert ok, text


GELU_CASES = [("pk", "bf16", 128), ("pk", "bf16", 256), ("pk", "fp8", 0), ("pk9", "f16", 128), ("pk9", "f16", 256),
              ("erf_pk", "split16", 128), ("erf_pk", "split16", 256), ("erf_pk", "splitx", 128), ("erf_pk", "splitx", 256), ("erff", "f32", 0)]


@pytest.mark.parametrize("form,fmt,tile", GELU_CASES)
def test_gelu_against_exact_function(form, fmt, tile):
    """Element by element: |stored - gelu(x)| <= the form's approximation bound at x + one rounding of the stored format.  Then the
    tails (sign and magnitude at x = -8 ... -1000: the seven-coefficient form's POSITIVE tail is pinned, not hidden), gelu(+0) = +0
    (and gelu(-0) = -0 where a -0 pre-activation can be made: the fp8 epilogue), the sign of tiny negative inputs, and finiteness."""
    x, _, out, ofmt, scale, _raw = _launch(fmt, 1, tile)
    keep = np.abs(x.astype(np.float64)) <= (65000.0 if ofmt == "f16" else 1e39)     # beyond: the stored format overflows (the saturation tests own that)
    assert np.isfinite(out[keep]).all(), "non-finite output for a finite pre-activation"
    _report(R.check_gelu(form, ofmt, x[keep], out[keep], scale))
    _report(R.check_gelu_tails(form, ofmt, x, out, scale))
    z = x == 0
    assert z.any() and np.all(out[z] == 0) and np.array_equal(np.signbit(out[z]), np.signbit(x[z])), "gelu(+-0) must be +-0 with the sign of the input"
    if fmt == "fp8":
        assert np.signbit(x[z]).any(), "the fp8 grid reaches -0"
    tiny = (x < 0) & (x > -1e-5) & (x < -1e-35)      # (below that the result is a denormal of the stored format, or nothing)
    if ofmt in ("bf16", "f32"):      # (the narrower formats flush these to a zero)
        assert tiny.any() and np.all(out[tiny] < 0), "a tiny negative input keeps its sign"
    print(f"[pointwise] gelu {form}/{fmt} tile {tile}: +-0 and tiny negatives keep their sign, {int(keep.sum())} finite outputs")


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("epi", [0, 1])
def test_folded_consumer_with_unit_statistics_gives_the_plain_ops_bits(fmt, epi):
    plain = _launch(fmt, epi, 128)[5]
    fold = _launch(fmt, epi, 128, fold=True)[5]
    assert torch.equal(plain.view(torch.int16), fold.view(torch.int16))


SILU_CASES = [("exp2", "bf16", 128), ("exp2", "bf16", 256), ("exp2", "f16", 128), ("exp2", "fp8", 0), ("expf", "split16", 128), ("expf", "split16", 256),
              ("expf", "splitx", 128), ("expf", "f32", 0)]


@pytest.mark.parametrize("form,fmt,tile", SILU_CASES)
def test_silu_gate_against_exact_function(form, fmt, tile):
    """silu(x1) x2 with x2 in {1, -1, 3.5} on the same grid of x1, x1 <= -90 included (exp overflows to inf: the quotient must be a zero,
    not NaN).  Bar: pointwise_ref.silu_bar_rel -- 2 fp32 ulps for the expf form, 2 + 0.75 |x1| for the exp2 form -- plus one output rounding."""
    x1, x2, out, ofmt, scale, _raw = _launch(fmt, 6, tile, swiglu=True)
    keep = np.abs(x1.astype(np.float64) * 3.5) <= (65000.0 if ofmt == "f16" else 1e38)
    assert np.isfinite(out[keep]).all(), "non-finite output for a finite pre-activation"
    _report(R.check_silu(form, ofmt, x1[keep], x2[keep], out[keep], scale))


@pytest.mark.parametrize("fmt,tile", [("bf16", 128), ("bf16", 256), ("f16", 128), ("f16", 256)])
def test_16_bit_store_is_one_correct_rounding(fmt, tile):
    """Epilogue 0 (bias only): the stored bf16 / fp16 equals torch's round-to-nearest-even cast of the exact fp32 value, bit for bit."""
    x, _, _, _, _, raw = _launch(fmt, 0, tile)
    want = torch.from_numpy(x).to(raw.dtype)
    assert torch.equal(raw.cpu().view(torch.int16), want.view(torch.int16))
    # the grid holds what decides: ties, and values that round up to a power of two
    b = x.view(np.uint32)
    low = b & (0xFFFF if fmt == "bf16" else 0x1FFF)
    assert (low == (0x8000 if fmt == "bf16" else 0x1000)).any(), "no tie in the grid"
    got = raw.float().cpu().numpy()
    up = (np.abs(got) > np.abs(x)) & (np.frexp(got)[0] == np.copysign(0.5, got)) & np.isfinite(got)
    assert up.any(), "no value that rounds up to a power of two"
    print(f"[pointwise] 16-bit store {fmt} tile {tile}: {x.size} values bit-equal to the cast; {int(up.sum())} round up to a power of two")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_layernorm_16_bit_output_is_the_cast_of_the_fp32_output(dtype):
    from foundpose_amd import ops
    for D in (384, 1024):
        x, _ = R.ln_rows(D)
        g = torch.Generator().manual_seed(D)
        w, b = torch.randn(D, generator=g).cuda(), torch.randn(D, generator=g).cuda()
        y32 = ops.layernorm(torch.from_numpy(x).cuda(), w, b, torch.float32)
        y16 = ops.layernorm(torch.from_numpy(x).cuda(), w, b, dtype)
        assert torch.equal(y16.view(torch.int16), y32.to(dtype).view(torch.int16))


@pytest.mark.parametrize("affine", ["unit", "random"])
@pytest.mark.parametrize("D", [384, 1024, 1536])
def test_layernorm_two_pass_on_the_rows_that_decide(D, affine):
    """ops.layernorm (VEC = 2, VEC = 4 and the six-vector instantiation) on 67 rows -- not a multiple of the 4 rows per workgroup --
    against the fp64 LayerNorm per element, in units of the row's std."""
    from foundpose_amd import ops
    x, _ = R.ln_rows(D)
    g = torch.Generator().manual_seed(D)
    w = torch.ones(D) if affine == "unit" else torch.randn(D, generator=g)
    b = torch.zeros(D) if affine == "unit" else torch.randn(D, generator=g)
    y = ops.layernorm(torch.from_numpy(x).cuda(), w.cuda(), b.cuda(), torch.float32).cpu().numpy()
    _report(R.check_layernorm_two_pass(x, w.numpy(), b.numpy(), y))


def _consumer_operands(D, N2=256):
    """A 0/1 (signed) selection of N2 of the D columns: the consumer's accumulator is then one bf16 element, exact."""
    rng = np.random.default_rng(D)
    cols = rng.permutation(D)[:N2]
    w = np.zeros((N2, D))
    w[np.arange(N2), cols] = np.where(np.arange(N2) % 3 == 0, -1.0, 1.0)
    bias = rng.standard_normal(N2).astype(np.float32)
    return w, bias


@pytest.mark.parametrize("chain", ["fp32-stream", "hi-lo"])
@pytest.mark.parametrize("D", [384, 1024])
def test_folded_layernorm_chain_on_the_rows_that_decide(D, chain):
    """The chain a block runs -- residual GEMM (epilogue 7, or 8 on the (hi, lo) stream), ln_finalize, consumer GEMM -- with a zero `a`
    operand, so the stream that is normalised is known exactly.  M = 128, m_valid = 67."""
    from foundpose_amd import ops
    M, mv = 128, 67
    rows, cls = R.ln_rows(D)
    x = np.zeros((M, D), np.float32)
    x[:mv] = rows
    a = torch.zeros(M, 64, dtype=torch.bfloat16).cuda()
    w0, b0 = torch.zeros(D, 64, dtype=torch.bfloat16).cuda(), torch.zeros(D).cuda()
    if chain == "fp32-stream":
        xs = torch.from_numpy(x).cuda()
        xb, stats = ops.gemm_bf16_resid_ln(a, w0, b0, xs, m_valid=mv)
        stream = x[:mv]
        assert torch.equal(xs.cpu(), torch.from_numpy(x)) and torch.equal(xb[:mv].cpu(), torch.from_numpy(stream).to(torch.bfloat16))
    else:
        hi = torch.from_numpy(x).to(torch.bfloat16)
        lo = (torch.from_numpy(x) - hi.float()).to(torch.bfloat16)
        stream = (hi.float() + lo.float()).numpy()[:mv]                 # what the pair represents: exact in fp32
        xb, xl = hi.clone().cuda(), lo.clone().cuda()
        stats = ops.gemm_bf16_resid_hilo(a, w0, b0, xb, xl, m_valid=mv)
        assert np.array_equal((xb.float() + xl.float()).cpu().numpy()[:mv], stream)
    _report(R.check_fold_partials(stream, stats[:, :mv].cpu().numpy()))
    ln_row = ops.ln_finalize(stats, D)
    lr = ln_row[:mv].cpu().numpy()
    _report(R.check_fold_rstd(stream, lr))
    w, bias = _consumer_operands(D)
    wt = _t(w, torch.bfloat16)
    out = ops.gemm_bf16_ln(xb, wt, _t(bias), wt.float().sum(1), ln_row, epilogue=0, m_valid=mv)[:mv].double().cpu().numpy()
    _report(R.check_fold_consumer(xb[:mv].double().cpu().numpy(), stream, w, bias, out))
    # how far the folded output is from the two-pass one, per class, and where the folded mode stops being a LayerNorm
    y2 = ops.layernorm(torch.from_numpy(stream).cuda(), torch.ones(D).cuda(), torch.zeros(D).cuda(), torch.float32).double().cpu().numpy()
    two = y2 @ w.T + bias[None, :].astype(np.float64)
    e_rs, e_mrs, kap = R.fold_rstd_errors(stream, lr)
    for c in R.LN_CLASSES:
        m = cls == c
        print(f"[pointwise] folded {chain} D={D} {c:12s}: kappa {kap[m].max():9.3g}  rstd err {e_rs[m].max():.2e}  mean*rstd err {e_mrs[m].max():.2e}  "
              f"|folded - two-pass| {np.abs(out - two)[m].max():.3e} (outputs of magnitude {np.abs(two)[m].max():.3g})")
    live = (kap > 1.5) & (kap < 1e9)
    c_meas = float(np.max(np.maximum(e_rs, e_mrs)[live] / (kap[live] * R.U24)))
    k_star = 2.0 ** 15 / c_meas
    print(f"[pointwise] folded {chain} D={D}: measured constant {c_meas:.2f} -> the rstd error reaches a bf16 half-ulp (2^-9) at kappa = {k_star:.3g}, "
          f"|mean| / std = {math.sqrt(k_star - 1):.0f}")
