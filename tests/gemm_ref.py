"""Exact references of the ViT GEMMs (csrc/gemm_kernel.hpp: gemm_bf16_kernel, launch, launch_fp8, gemm_launch_fmt) -- torch CPU / numpy, no GPU.

* LAUNCHES: every (format, tile, epilogue, folded-or-plain, e4m3-output) the library can run, and resolve_tile: the tile a FORCED tile
  really runs at a shape, restated from launch / launch_fp8 (a forced tile the shape does not admit falls through to another without an
  error, so every case asserts resolve_tile(...) == its own tile before it launches);
* tile_order: xcd_remap, the super-tile raster with its ragged last super-row and the cut of m_tiles at M_valid, as a list of tiles;
* build: operands in their stored format whose products and partial sums are exact in fp32 in ANY order -- small integers, powers of two
  for every scale -- so the result of a linear epilogue (0, 3, 5, 7, 8, folded 0) is one known bit pattern and needs no tolerance; the
  pre-activation of epilogues 1 / 6 is exact too, and their outputs are held per element to tests/pointwise_ref.py's bounds for the form
  the format uses.  build asserts (it does not assume) that every stored operand decodes to the value meant, that the sum of the
  magnitudes of the products, in units of their common last place, is below 2^24, and that what leaves through a 16-bit or split store
  is representable there;
* place: the operands as the leading corner of larger buffers (A: 352 more rows, W: 256, both 16 more columns; bias / gamma / colsum:
  256 more entries; ln_row: 352) whose guards -- and A's rows in [M_valid, M) -- hold zeros, NaN (in the operand's own format) or a
  large finite value, and every output as the leading corner of a buffer filled with the byte 0x35;
* emulate: the reference written as tiles over those buffers (what the CPU test runs the checkers on), with FAULTS: imitated defects of
  the kind a performance change to the kernel produces, each of which must fail check();
* check: bits of the live elements (or the per-element bound), and every byte the launch must not write.  A mismatch names the format, tile,
  epilogue, shape, M_valid, the first differing (row, column) with its m-tile, n-tile and 32-row band, and the two values;
* real_case / real_check: randn and nearly cancelling ("offset") operands with the per-element bound of vit_front_ref.token_bound.

Used by tests/test_gemm_ref_cpu.py (no GPU) and tests/test_gpu_gemm_edges.py."""

from collections import namedtuple

import numpy as np
import torch

from foundpose_amd import ops
from tests import pointwise_ref as pr
from tests import vit_front_ref as fr

F32 = np.float32
EPI_BIAS, EPI_GELU, EPI_LS_RESID, EPI_BIAS_F32, EPI_SWIGLU, EPI_RESID_F32, EPI_RESID_HILO = 0, 1, 3, 5, 6, 7, 8
LINEAR = (EPI_BIAS, EPI_LS_RESID, EPI_BIAS_F32, EPI_RESID_F32, EPI_RESID_HILO)
RMW = (EPI_LS_RESID, EPI_RESID_F32, EPI_RESID_HILO)       # read-modify-write epilogues: a tile run twice shows
FORMATS = ("bf16", "f16", "fp8", "f16x3", "f16f8")
SPLIT = ("f16x3", "f16f8")
GEOM = {64: (64, 128), 128: (128, 128), 256: (256, 256), 320: (320, 256), 352: (352, 256)}   # tile -> (BM, BN)
A_GUARD, W_GUARD, VEC_GUARD, LD_EXTRA = 352, 256, 256, 16
OUT_ROWS_EXTRA, OUT_COLS_EXTRA = 64, 8
SENTINEL = 0x35            # byte: a finite number in every output format
FILLS = ("zero", "nan", "big")
GELU_FORM = {"bf16": "pk", "fp8": "pk", "f16": "pk9", "f16x3": "erf_pk", "f16f8": "erf_pk"}
SILU_FORM = {"bf16": "exp2", "fp8": "exp2", "f16": "exp2", "f16x3": "expf", "f16f8": "expf"}

Launch = namedtuple("Launch", "fmt tile epi folded f8out")


def _launches():
    rows = []
    for fmt in ("bf16", "f16"):
        for tile in (128, 256):
            rows += [Launch(fmt, tile, e, False, False) for e in (0, 1, 6, 3, 5, 7, 8)] + [Launch(fmt, tile, e, True, False) for e in (0, 1, 6)]
        rows += [Launch(fmt, 64, e, False, False) for e in (3, 7, 8)]
        for tile in (320, 352):
            rows += [Launch(fmt, tile, e, False, False) for e in (0, 1, 8)] + [Launch(fmt, tile, e, True, False) for e in (0, 1)]
    rows += [Launch("fp8", 256, e, False, False) for e in (0, 1, 3, 6)] + [Launch("fp8", 256, e, False, True) for e in (1, 6)]
    rows += [Launch("fp8", 320, e, False, False) for e in (0, 1, 6)] + [Launch("fp8", 320, e, False, True) for e in (1, 6)]
    for fmt in SPLIT:
        for tile in (128, 256):
            rows += [Launch(fmt, tile, e, False, False) for e in (0, 1, 6, 3, 5)]
    return rows


LAUNCHES = _launches()


def launch_id(l):
    return f"{l.fmt}-t{l.tile}-e{l.epi}" + ("-folded" if l.folded else "") + ("-e4m3" if l.f8out else "")


def stored_k(fmt, K):
    """Stored elements of a row of K logical ones (split rows: 2K halves; fp8: K bytes)."""
    return 2 * K if fmt in SPLIT else K


# ------------------------------------------------------------------------------------------------ the launch logic, restated
def resolve_tile(l, M, N, K, m_valid, lda, ldw):
    """The block-tile height that `tile` forced through the C ABI really runs (launch / launch_fp8 / gemm_launch_fmt); ValueError where the
    library refuses.  lda / ldw in stored elements."""
    fmt, force, epi = l.fmt, l.tile, l.epi

    def need(cond, why):
        if not cond:
            raise ValueError(f"{launch_id(l)} M {M} N {N} K {K} M_valid {m_valid}: {why}")

    if fmt == "fp8":
        need(force in (256, 320), "tile override")
        need(M > 0 and M % 256 == 0 and N > 0 and N % 256 == 0, "M and N multiples of 256")
        need(K > 0 and K % 128 == 0, "K a multiple of 128")
        need(lda % 16 == 0 and ldw % 16 == 0, "16-byte rows")
        need(epi in (0, 1, 3, 6) and (not l.f8out or epi in (1, 6)), "epilogue")
        return 320 if epi != EPI_LS_RESID and force == 320 and M % 320 == 0 else 256
    if fmt in SPLIT:
        need(force in (128, 256), "tile override")
        need(M > 0 and M % 128 == 0 and N > 0 and N % 128 == 0, "M and N multiples of 128")
        need(K > 0 and K % (64 if fmt == "f16f8" else 32) == 0, "K a multiple of 32 (f16f8: 64)")
        need(lda % 8 == 0 and ldw % 8 == 0 and lda >= 2 * K and ldw >= 2 * K, "rows of 2K halves, 16-byte aligned")
        need(epi in (0, 1, 3, 5, 6), "epilogue")
        return 256 if force == 256 and M % 256 == 0 and N % 256 == 0 else 128
    need(force in (64, 128, 256, 320) or (force == 352 and epi in (0, 1, 8)), "tile override")
    need(M > 0 and M % 128 == 0 and N > 0 and N % 128 == 0 and K > 0 and K % 64 == 0, "M, N multiples of 128, K of 64")
    need(lda % 8 == 0 and ldw % 8 == 0, "16-byte rows")
    need(not l.folded or epi in (0, 1, 6), "folded form")
    use_big = M % 256 == 0 and N % 256 == 0 and force == 256
    ok352 = N % 256 == 0 and 0 < m_valid <= M
    ok320 = force == 320 and M % 320 == 0 and N % 256 == 0
    if epi in (0, 1):
        if force == 352:
            need(ok352, "352 rows need N % 256 == 0 and 0 < M_valid <= M")
            return 352
        if ok320:
            return 320
    if epi == EPI_RESID_HILO:
        if ok320:
            return 320
        if force == 352:
            need(ok352, "352 rows need N % 256 == 0 and 0 < M_valid <= M")
            return 352
    if use_big:
        return 256
    if epi in RMW and force == 64 and M % 64 == 0:
        return 64
    return 128


def xcd_remap(bid, nwg):
    q, r = divmod(nwg, 8)
    xcd, idx = bid % 8, bid // 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def pick_raster(bm, n_tiles, grid):
    rr, gn = (4, 8) if n_tiles % 8 == 0 else (8, 4)
    return (rr, gn) if bm >= 256 and n_tiles % gn == 0 and n_tiles > 4 and grid >= 512 else (0, 0)


def tile_order(tile, M, N, m_valid):
    """-> (grid, [(block id, m0, n0)]): what launch_cfg launches and where each workgroup that does not exit at once works."""
    BM, BN = GEOM[tile]
    m_tiles = -(-M // BM)
    if m_valid > 0 and -(-m_valid // BM) < m_tiles:
        m_tiles = -(-m_valid // BM)
    n_tiles = N // BN
    grid = m_tiles * n_tiles
    r, gn = pick_raster(BM, n_tiles, grid)
    if r:
        grid = -(-m_tiles // r) * (n_tiles // gn) * 32
    tiles = []
    for bid in range(grid):
        lid = xcd_remap(bid, grid)
        if r:
            per = r * gn
            st, rem = divmod(lid, per)
            sn, sm = divmod(st, -(-m_tiles // r))
            tm, tn = sm * r + rem % r, sn * gn + rem // r
            if tm >= m_tiles:
                continue
        else:
            tm, tn = divmod(lid, n_tiles)
        tiles.append((bid, tm * BM, tn * BN))
    return grid, tiles


# ------------------------------------------------------------------------------------------------ stored formats
E4M3 = torch.float8_e4m3fn


def _t16(fmt):
    return torch.bfloat16 if fmt == "bf16" else torch.float16


def store(fmt, vals):
    """fp32 values [rows, K] -> the stored row image (tight).  Split rows are packed at scale 1."""
    v = torch.as_tensor(np.asarray(vals, F32))
    if fmt == "f16x3":
        return ops.split16_pack(v, 1.0)
    if fmt == "f16f8":
        return ops.splitx_pack(v, 1.0)
    if fmt == "fp8":
        return v.to(E4M3).view(torch.uint8)      # (fp8 rows are kept as their bytes: torch indexes uint8, not float8)
    return v.to(_t16(fmt))


def parts(fmt, stored):
    """The factors a stored row enters the MFMAs with, fp64 [rows, K] each, READ BACK from the stored bytes.
    16-bit / fp8: (value,).  f16x3: (hi, lo).  f16f8: (hi, e4m3 copy of hi x 2^7, e4m3 lo x 2^-4)."""
    if fmt == "f16x3":
        g = stored.reshape(stored.shape[0], -1, 2, 32).double()
        return g[:, :, 0].reshape(stored.shape[0], -1).numpy(), g[:, :, 1].reshape(stored.shape[0], -1).numpy()
    if fmt == "f16f8":
        by = stored.contiguous().view(torch.uint8).unflatten(1, (-1, 256))
        n = stored.shape[0]
        hi = by[:, :, :128].contiguous().view(torch.float16).double().reshape(n, -1).numpy()
        hi8 = by[:, :, 128:192].contiguous().view(E4M3).double().reshape(n, -1).numpy() * 2.0 ** 7
        lo8 = by[:, :, 192:256].contiguous().view(E4M3).double().reshape(n, -1).numpy() * 2.0 ** -4
        return hi, hi8, lo8
    if fmt == "fp8":
        return (stored.contiguous().view(E4M3).double().numpy(),)
    return (stored.double().numpy(),)


def products(fmt, pa, pw, drop_lo_hi=False):
    """The (a factor, w factor) pairs whose products the format sums: one for the plain formats, hi*hi + hi_a*lo_w + lo_a*hi_w for the split
    ones (lo*lo is dropped by design; f16f8 takes the cross terms' hi from its e4m3 copy).  drop_lo_hi: the imitated fault."""
    if fmt == "f16x3":
        pairs = [(pa[0], pw[0]), (pa[0], pw[1]), (pa[1], pw[0])]
    elif fmt == "f16f8":
        pairs = [(pa[0], pw[0]), (pa[1], pw[2]), (pa[2], pw[1])]
    else:
        return [(pa[0], pw[0])]
    return pairs[:2] if drop_lo_hi else pairs


def fill_pattern(fmt, fill, n):
    """n stored elements of the guard fill in the operand's own format (f16f8 rows: per 128 halves, 64 fp16 then 128 e4m3 bytes)."""
    if fmt == "fp8":
        b = {"zero": torch.zeros((), dtype=torch.uint8), "nan": torch.tensor(0x7F, dtype=torch.uint8),
             "big": torch.tensor(240.0).to(E4M3).view(torch.uint8)}[fill]
        return b.expand(n).clone()
    val = {"zero": 0.0, "nan": float("nan"), "big": 1.0e4}[fill]
    row = torch.full((n,), val, dtype=_t16(fmt))
    if fmt == "f16f8":
        b8 = fill_pattern("fp8", fill, 2 * n).view(torch.uint8).view(torch.float16)
        idx = torch.arange(n)
        row = torch.where(idx % 128 >= 64, b8, row)
    return row


# ------------------------------------------------------------------------------------------------ cases
class Case:
    pass


_operand_cache = {}


def _int_operands(fmt, M, N, K, kind, seed, sparse):
    """Integer operands: A in {-1, 0, 1}, W in {-2 .. 2}; kind "lo" (split formats): i + j 2^-12 with i != 0 so that hi = i, lo = j 2^-12."""
    key = (fmt, M, N, K, kind, seed, sparse)
    if key in _operand_cache:
        return _operand_cache[key]
    rng = np.random.default_rng([seed, M, N, K, FORMATS.index(fmt)])
    a = rng.integers(-1, 2, size=(M, K)).astype(np.float64)
    w = rng.integers(-2, 3, size=(N, K)).astype(np.float64)
    if sparse:    # non-linear epilogues: pre-activations near zero, where GELU and SiLU are not yet the identity or zero
        a *= rng.random((M, K)) < 0.125
    if kind == "lo":
        assert fmt in SPLIT
        a = np.where(a == 0, 1.0, a) * (rng.random((M, K)) < 0.75)
        w = np.where(w == 0, -1.0, w)
        a = a + (a != 0) * rng.integers(-1, 2, size=(M, K)) * 2.0 ** -12
        w = w + rng.integers(-1, 2, size=(N, K)) * 2.0 ** -12
    sa, sw = store(fmt, a), store(fmt, w)
    pa, pw = parts(fmt, sa), parts(fmt, sw)
    # every stored operand decodes to its value
    if fmt == "f16x3":
        assert np.array_equal(pa[0] + pa[1], a) and np.array_equal(pw[0] + pw[1], w)
    elif fmt == "f16f8":
        assert np.array_equal(pa[0] + pa[2], a) and np.array_equal(pw[0] + pw[2], w) and np.array_equal(pa[0], pa[1]) and np.array_equal(pw[0], pw[1])
    else:
        assert np.array_equal(pa[0], a) and np.array_equal(pw[0], w)
    if kind == "lo":
        assert np.array_equal(pa[0], np.rint(a)) and (pa[-1] != 0).any() and (pw[-1] != 0).any()
    acc, mag = np.zeros((M, N)), np.zeros((M, N))
    for fa, fw in products(fmt, pa, pw):
        acc += fa @ fw.T
        mag += np.abs(fa) @ np.abs(fw).T
    # every product is a multiple of q, and the magnitudes sum to less than 2^24 q: every partial sum, in any order, is exact in fp32
    q = 2.0 ** -12 if kind == "lo" else 1.0
    assert np.array_equal(np.rint(acc / q) * q, acc) and mag.max() / q < 2.0 ** 24
    _operand_cache[key] = (sa, sw, acc, mag)
    return _operand_cache[key]


def _exact32(x):
    y = np.asarray(x, np.float64).astype(F32)
    assert np.array_equal(y.astype(np.float64), x), "not exact in fp32"
    return y


def _pow2(rng, n, exps):
    return (2.0 ** rng.choice(np.asarray(exps, np.float64), size=n)).astype(F32)


def build(l, M, N, K, m_valid, kind="int", seed=0):
    """One launch at one shape with exact operands.  kind: "int"; "lo" (split formats: non-zero low parts); "big" (epilogue 8: a stream of
    integers up to +-30000, so the new lo half is non-zero)."""
    c = Case()
    c.l, c.M, c.N, c.K, c.m_valid, c.kind, c.exact = l, M, N, K, m_valid, kind, True
    fmt, epi = l.fmt, l.epi
    nonlin = epi in (EPI_GELU, EPI_SWIGLU)
    c.a, c.w, acc, c.mag = _int_operands(fmt, M, N, K, "lo" if kind == "lo" else "int", seed, nonlin)
    rng = np.random.default_rng([seed, N, epi, int(l.folded)])
    rrow = np.random.default_rng([seed, M, 7])
    c.bias = rng.integers(-8, 9, size=N).astype(F32)
    c.gamma = c.colsum = c.ln_row = None
    c.acc_scale, c.out_scale = 0.0, 0.0
    lin = acc.copy()
    if fmt in SPLIT:
        c.acc_scale = 2.0 ** -3 if nonlin else 0.5
        lin = lin * c.acc_scale
    if l.folded:
        rstd = _pow2(rrow, M, [-3, -2] if nonlin else [0, 1])
        mrs = rrow.integers(-2, 3, size=M).astype(F32)
        c.ln_row = np.stack([rstd, mrs], 1)
        c.colsum = rng.integers(-4, 5, size=N).astype(F32)
        lin = rstd[:, None].astype(np.float64) * lin - mrs[:, None].astype(np.float64) * c.colsum[None]
    lin = lin + c.bias[None]
    if fmt == "fp8":
        c.gamma = _pow2(rng, N, [-4, -3] if nonlin else [-1, 0, 1])
        lin = lin * c.gamma[None]
    elif epi == EPI_LS_RESID:
        c.gamma = _pow2(rng, N, [-1, 0, 1])
        lin = lin * c.gamma[None]
    c.pre = _exact32(lin)
    _finish(c, rng)
    return c


def _store16(fmt16, x):
    return torch.as_tensor(np.asarray(x, F32)).to(_t16(fmt16))


def _finish(c, rng):
    """Streams, output geometry and the expected outputs from c.pre (the fp32 value in front of the store / non-linearity / residual add)."""
    l, M, N = c.l, c.M, c.N
    fmt, epi = l.fmt, l.epi
    t16 = "f16" if fmt == "f16" else "bf16"
    c.stream, c.want = {}, {}
    c.out_cols = N // 2 if epi == EPI_SWIGLU else N
    if epi in (EPI_LS_RESID, EPI_RESID_F32):
        x = rng.integers(-64, 65, size=(M, N)).astype(np.float64)
        c.stream["out"] = torch.as_tensor(x.astype(F32))
        c.x_new = _exact32(x + c.pre) if c.exact else (x + c.pre.astype(np.float64)).astype(F32)
        c.want["out"] = torch.as_tensor(c.x_new)
    if epi == EPI_RESID_HILO:
        lim = 30000 if c.kind == "big" else 64
        x = rng.integers(-lim, lim + 1, size=(M, N)).astype(F32)
        hi = _store16(t16, x)
        lo = _store16(t16, x - hi.float().numpy())
        assert np.array_equal(hi.double().numpy() + lo.double().numpy(), x)
        c.stream["xb"], c.stream["xl"] = hi, lo
        c.x_new = _exact32(x.astype(np.float64) + c.pre) if c.exact else (x.astype(np.float64) + c.pre.astype(np.float64)).astype(F32)
        nh = _store16(t16, c.x_new)
        nl = _store16(t16, c.x_new - nh.float().numpy())
        if c.exact:
            assert np.array_equal(nh.double().numpy() + nl.double().numpy(), c.x_new.astype(np.float64))   # hi' + lo' = x', exactly
            assert c.kind != "big" or bool((nl != 0).any())
        c.want["xb"], c.want["xl"] = nh, nl
    if epi == EPI_RESID_F32:
        c.want["xb"] = _store16(t16, c.x_new)
    if epi in (EPI_RESID_F32, EPI_RESID_HILO):
        xd = c.x_new.astype(np.float64).reshape(M, N // 128, 128)
        s = np.stack([xd.sum(2).T, (xd * xd).sum(2).T], 2)                 # [N / 128, M, 2]
        c.stats64 = s
        c.stats_abs = np.stack([np.abs(xd).sum(2).T, (xd * xd).sum(2).T], 2)
        c.stats_exact = bool(c.exact and c.stats_abs.max() < 2.0 ** 24)
        assert c.kind == "big" or not c.exact or c.stats_exact
        if c.stats_exact:
            c.want["stats"] = torch.as_tensor(s.astype(F32))
    # the main output of the store epilogues
    if epi == EPI_BIAS_F32:
        c.want["out"] = torch.as_tensor(c.pre)
    if epi == EPI_BIAS:
        if fmt in SPLIT:
            c.out_scale = 2.0
            c.want["out"] = ops.split16_pack(torch.as_tensor(c.pre), c.out_scale)
            if c.exact:
                assert np.array_equal(ops.split16_unpack(c.want["out"], c.out_scale).double().numpy(), c.pre.astype(np.float64))
        else:
            c.want["out"] = _store16(t16, c.pre)
            if c.exact:
                assert np.array_equal(c.want["out"].double().numpy(), c.pre.astype(np.float64)), "not representable in the 16-bit output"
    if epi in (EPI_GELU, EPI_SWIGLU):
        c.out_scale = 4.0 if (fmt in SPLIT or l.f8out) else 0.0
        if epi == EPI_GELU:
            c.y = pr.gelu(c.pre)
        else:
            c.y = pr.silu(c.pre[:, 0::2]) * c.pre[:, 1::2].astype(np.float64)
        if l.f8out:
            assert np.abs(c.y).max() * c.out_scale * 1.01 <= 448.0, "the e4m3 output would clamp"
    # stored elements per output row and the output's dtype
    if epi in (EPI_LS_RESID, EPI_BIAS_F32, EPI_RESID_F32):
        c.out_dtype, c.out_width = torch.float32, N
    elif epi == EPI_RESID_HILO:
        c.out_dtype, c.out_width = None, 0
    elif l.f8out:
        c.out_dtype, c.out_width = torch.uint8, c.out_cols
    elif fmt in SPLIT:
        c.out_dtype, c.out_width = torch.float16, 2 * c.out_cols
    else:
        c.out_dtype, c.out_width = _t16(t16), c.out_cols
    c.t16 = t16


def describe(c):
    return f"{launch_id(c.l)} {c.kind} M {c.M} N {c.N} K {c.K} M_valid {c.m_valid}"


# ------------------------------------------------------------------------------------------------ buffers
def _guarded(t, extra_rows, extra_cols, fill_row):
    """t [rows, cols] -> the leading corner of a [rows + extra_rows, cols + extra_cols] buffer whose other elements repeat fill_row."""
    rows, cols = t.shape
    buf = fill_row[:cols + extra_cols].repeat(rows + extra_rows, 1).contiguous()
    buf[:rows, :cols] = t
    return buf


def _vec(v, extra, fill):
    val = {"zero": 0.0, "nan": float("nan"), "big": 1.0e4}[fill]
    t = torch.as_tensor(np.asarray(v, F32))
    buf = torch.full((t.shape[0] + extra,) + tuple(t.shape[1:]), val, dtype=torch.float32)
    buf[:t.shape[0]] = t
    return buf


def _sentinel(rows, cols, dtype):
    t = torch.empty(rows, cols, dtype=dtype)
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def place(c, fill):
    """-> dict of CPU buffers: operands with their guards (and A's rows from M_valid on) holding `fill`, outputs preset.  The views a launch is
    given are the leading corners: buf[:rows, :cols]."""
    fmt, M, N = c.l.fmt, c.M, c.N
    kst = stored_k(fmt, c.K)
    pat = fill_pattern(fmt, fill, kst + LD_EXTRA)
    b = {"a": _guarded(c.a, A_GUARD, LD_EXTRA, pat), "w": _guarded(c.w, W_GUARD, LD_EXTRA, pat), "bias": _vec(c.bias, VEC_GUARD, fill)}
    b["a"][c.m_valid:M] = pat
    for name in ("gamma", "colsum"):
        if getattr(c, name) is not None:
            b[name] = _vec(getattr(c, name), VEC_GUARD, fill)
    if c.ln_row is not None:
        b["ln_row"] = _vec(c.ln_row, A_GUARD, fill)
    pad = 16 if c.l.f8out else OUT_COLS_EXTRA
    if c.out_dtype is not None:
        o = _sentinel(M + OUT_ROWS_EXTRA, c.out_width + pad, c.out_dtype)
        if "out" in c.stream:
            o[:c.m_valid, :N] = c.stream["out"][:c.m_valid]
        b["out"] = o
    if c.l.epi in (EPI_RESID_F32, EPI_RESID_HILO):
        for name in ("xb", "xl") if c.l.epi == EPI_RESID_HILO else ("xb",):
            o = _sentinel(M + OUT_ROWS_EXTRA, N + OUT_COLS_EXTRA, _t16(c.t16))
            if name in c.stream:
                o[:c.m_valid, :N] = c.stream[name][:c.m_valid]
            b[name] = o
        b["stats"] = _sentinel(N // 128, M * 2, torch.float32).reshape(N // 128, M, 2)
    return b


OUTPUTS = ("out", "xb", "xl", "stats")


# ------------------------------------------------------------------------------------------------ the emulated kernel
FAULTS = ["store_le", "drop_ktile", "bias_shift4", "skip_tile", "tile_twice", "k_plus8", "drop_lo_hi", "lda_is_k", "guard_row"]


def fault_applies(fault, c):
    """Whether the imitated fault can change what this case stores (tile_twice: read-modify-write epilogues; drop_lo_hi: non-zero low parts)."""
    if fault == "tile_twice":
        return c.l.epi in RMW
    if fault == "drop_lo_hi":
        return c.l.fmt in SPLIT and c.kind == "lo"
    if fault == "drop_ktile":
        return c.m_valid > GEOM[c.l.tile][0]      # the second m-tile loses its first K-tile
    return True


def _f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(F32)


def _round_store(c, v, scale):
    """fp32 values -> the stored output rows [rows, width] (torch), the arithmetic of the epilogue's store."""
    l = c.l
    t = torch.as_tensor(np.ascontiguousarray(v, dtype=F32))
    if l.f8out:
        return (t * scale).clamp(-448.0, 448.0).to(E4M3).view(torch.uint8)
    if l.fmt == "f16f8" and l.epi != EPI_BIAS:
        return ops.splitx_pack(t, scale)
    if l.fmt in SPLIT:
        return ops.split16_pack(t, scale)
    return t.to(_t16(c.t16))


def emulate(c, b, fault=None):
    """The kernel as tiles over the buffers of place(): tile_order, per K-tile products read from the guarded buffers with their row
    strides, the epilogue in fp32, stores under `row < M_valid`.  Writes into b's outputs (clones first) and returns them."""
    l, M, N, K, mv = c.l, c.M, c.N, c.K, c.m_valid
    fmt, epi = l.fmt, l.epi
    BM, BN = GEOM[l.tile]
    kst = stored_k(fmt, K)
    out = {k: b[k].clone() for k in OUTPUTS if k in b}

    def operand(buf, rows):
        if fault == "lda_is_k":     # the row stride taken as the row length
            flat = buf.reshape(-1)
            return parts(fmt, torch.stack([flat[r * kst:(r + 1) * kst] for r in rows]))
        return parts(fmt, buf[rows, :kst])

    kt = 64 if fmt == "f16f8" else (32 if fmt == "f16x3" else (128 if fmt == "fp8" else 64))   # logical k per K-tile (f16f8: per pair of tiles)
    _, tiles = tile_order(l.tile, M, N, mv)
    last_m0 = max(m0 for _, m0, _ in tiles)
    if fault == "skip_tile":
        tiles = tiles[:len(tiles) // 2] + tiles[len(tiles) // 2 + 1:]
    if fault == "tile_twice":
        tiles = tiles + [tiles[len(tiles) // 3]]
    for _, m0, n0 in tiles:
        rows = np.arange(BM)
        if l.tile == 352:           # a row group past the end of A is fetched from A's last row group
            last_grp = min(M - m0, BM) - 8
            rows = np.minimum(rows // 8 * 8, last_grp) + rows % 8
        rows = m0 + rows
        if fault == "guard_row" and m0 == last_m0:      # the last live row of the last tile comes from the row behind it
            rows = np.where(m0 + np.arange(BM) == mv - 1, M if mv == M else mv, rows)
        pa, pw = operand(b["a"], rows.tolist()), operand(b["w"], list(range(n0, n0 + BN)))
        acc = np.zeros((BM, BN))
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(K // kt):
                if fault == "drop_ktile" and t == 0 and m0 == BM:
                    continue
                ks = slice(t * kt, (t + 1) * kt)
                for fa, fw in products(fmt, pa, pw, drop_lo_hi=fault == "drop_lo_hi"):
                    fw = fw[:, ks]
                    if fault == "k_plus8":
                        fw = np.roll(fw, -8, axis=1)
                    acc += fa[:, ks] @ fw.T
            cols = n0 + np.arange(BN)
            bias = b["bias"].numpy()[n0 + (np.arange(BN) + 4) % BN if fault == "bias_shift4" else cols].astype(np.float64)
            grow = m0 + np.arange(BM)                 # the output rows of the tile
            acc32 = _f32(acc).astype(np.float64)
            if l.folded:
                ln = np.tile(np.asarray([[1.0, 0.0]]), (BM, 1))
                ok = grow < (mv if l.tile == 352 else M + A_GUARD)
                ln[ok] = b["ln_row"].numpy()[grow[ok]]
                t0 = _f32(-ln[:, 1:2] * b["colsum"].numpy()[cols][None].astype(np.float64) + bias[None]).astype(np.float64)
                v = _f32(ln[:, 0:1] * acc32 + t0)
            elif fmt in SPLIT:
                v = _f32(acc32 * c.acc_scale + bias[None])
            else:
                v = _f32(acc32 + bias[None])
            if fmt == "fp8" or epi == EPI_LS_RESID:
                v = _f32(v.astype(np.float64) * b["gamma"].numpy()[cols][None].astype(np.float64))
            live = grow < (mv + 1 if fault == "store_le" else mv)
            r = torch.as_tensor(grow[live])
            v = v[live]
            if epi == EPI_GELU:
                v = pr.GELU_FORMS[GELU_FORM[fmt]](v)
            if epi == EPI_SWIGLU:
                v = (pr.silu_gate_exp2 if SILU_FORM[fmt] == "exp2" else pr.silu_gate_expf)(v[:, 0::2], v[:, 1::2])
            oc = n0 // 2 if epi == EPI_SWIGLU else n0
            ow = v.shape[1]
            if epi in (EPI_BIAS, EPI_GELU, EPI_SWIGLU):
                per = c.out_width // c.out_cols          # stored elements per output column
                out["out"][r, oc * per:(oc + ow) * per] = _round_store(c, v, c.out_scale)
                continue
            if epi == EPI_BIAS_F32:
                out["out"][r, n0:n0 + BN] = torch.as_tensor(v)
                continue
            if epi == EPI_RESID_HILO:
                x = _f32(out["xb"][r, n0:n0 + BN].double().numpy() + out["xl"][r, n0:n0 + BN].double().numpy())
            else:
                x = out["out"][r, n0:n0 + BN].numpy()
            xn = _f32(v.astype(np.float64) + x.astype(np.float64))
            if epi != EPI_RESID_HILO:
                out["out"][r, n0:n0 + BN] = torch.as_tensor(xn)
            if epi == EPI_LS_RESID:
                continue
            hi = _store16(c.t16, xn)
            out["xb"][r, n0:n0 + BN] = hi
            if epi == EPI_RESID_HILO:
                out["xl"][r, n0:n0 + BN] = _store16(c.t16, _f32(xn.astype(np.float64) - hi.double().numpy()))
            xd = xn.astype(np.float64).reshape(len(r), BN // 128, 128)
            for g in range(BN // 128):
                out["stats"][n0 // 128 + g, r, 0] = torch.as_tensor(_f32(xd[:, g].sum(1)))
                out["stats"][n0 // 128 + g, r, 1] = torch.as_tensor(_f32((xd[:, g] ** 2).sum(1)))
    return out


# ------------------------------------------------------------------------------------------------ checks
def _bytes2d(t):
    t = t.contiguous()
    return t.view(torch.uint8).reshape(t.shape[0], -1)


def _where(c, row, col_elem, per):
    BM, BN = GEOM[c.l.tile]
    col = col_elem // per
    ncol = col * 2 if c.l.epi == EPI_SWIGLU else col
    return f"row {row}, column {col} (m-tile {row // BM}, n-tile {ncol // BN}, band {row % BM // 32})"


def _first_diff(c, name, got, want, per):
    d = (_bytes2d(got) != _bytes2d(want))
    if not bool(d.any()):
        return None
    esz = got.element_size()
    r, cb = (int(v) for v in d.nonzero()[0])
    e = cb // esz
    g, w = got[r, e], want[r, e]
    gv, wv = (float(t.float()) for t in (g, w))
    return (f"{describe(c)}: {name} differs in {int(d.any(1).sum())} rows, first at {_where(c, r, e, per)}: "
            f"got {gv!r} want {wv!r} (difference {gv - wv!r})")


def out_values(c, stored):
    """The fp64 values the stored rows of the main output stand for."""
    l = c.l
    if l.f8out:
        return stored.contiguous().view(E4M3).double().numpy() / c.out_scale
    if l.fmt == "f16f8" and l.epi != EPI_BIAS:
        return ops.splitx_unpack(stored.contiguous(), c.out_scale).double().numpy()
    if l.fmt in SPLIT and l.epi in (EPI_BIAS, EPI_GELU, EPI_SWIGLU):
        return ops.split16_unpack(stored.contiguous(), c.out_scale).double().numpy()
    return stored.double().numpy()


def store_bar(c, y):
    """One rounding of the stored output format at |y| (fp64 array of the unscaled values)."""
    l = c.l
    if l.f8out:    # half an e4m3 step at the scaled value
        s = np.abs(y) * c.out_scale
        e = np.floor(np.log2(np.maximum(s, 2.0 ** -9)))
        return 2.0 ** (np.maximum(e, -6.0) - 4.0) / c.out_scale
    if l.fmt == "f16f8" and l.epi != EPI_BIAS:
        r, t = fr.REPR["f16f8"]
        return r * np.abs(y) + t / c.out_scale
    if l.fmt in SPLIT:
        return pr._half_ulp("split16", y, c.out_scale)
    return pr._half_ulp(c.t16, y)


def check_nonlinear(c, got_rows):
    """Epilogues 1 / 6 on the exactly known pre-activation: per element, the form's approximation bound + one rounding of the stored format."""
    mv = c.m_valid
    got = out_values(c, got_rows[:mv])
    y = c.y[:mv]
    if c.l.epi == EPI_GELU:
        form = GELU_FORM[c.l.fmt]
        ab = pr.gelu_approx_bound(form, c.pre[:mv].astype(np.float64))
    else:
        form = SILU_FORM[c.l.fmt]
        x1, x2 = c.pre[:mv, 0::2].astype(np.float64), c.pre[:mv, 1::2].astype(np.float64)
        ab = pr.silu_bar_rel(form, x1) * np.abs(y) + 89.0 * 2.0 ** -128 * np.abs(x2)
    bar = ab + store_bar(c, np.abs(y) + ab)
    err = np.where(np.isfinite(got), np.abs(got - y), np.inf)
    ratio = err / bar
    if bool((ratio <= 1.0).all()):
        return None, float(ratio.max()) if ratio.size else 0.0
    r, col = (int(v) for v in np.argwhere(ratio > 1.0)[0])
    return (f"{describe(c)}: {form} output beyond its bound in {int((ratio > 1.0).any(1).sum())} rows, first at {_where(c, r, col, 1)}: "
            f"got {got[r, col]!r} want {y[r, col]!r} (error {err[r, col]:.3e}, bound {bar[r, col]:.3e})"), float(ratio.max())


def check(c, b, outs):
    """outs: the output buffers after the launch (CPU tensors shaped like place()'s).  -> list of messages, empty when all is well."""
    msgs = []
    mv, N = c.m_valid, c.N
    for name in OUTPUTS:
        if name not in b:
            continue
        got, init = outs[name], b[name]
        if name == "stats":
            if not torch.equal(_bytes2d(got[:, mv:].reshape(got.shape[0], -1)), _bytes2d(init[:, mv:].reshape(got.shape[0], -1))):
                msgs.append(f"{describe(c)}: stats rows from M_valid on were written")
            live = got[:, :mv]
            if c.stats_exact:
                m = _first_diff(c, "stats[group, row]", live.reshape(live.shape[0], -1), c.want["stats"][:, :mv].reshape(live.shape[0], -1), 2)
                if m:
                    msgs.append(m)
            else:   # 128 terms summed in fp32 in some order: |error| <= 127 x 2^-24 x sum of the magnitudes (K-free), + the rounding of each square
                err = np.abs(live.double().numpy() - c.stats64[:, :mv])
                bar = 128 * pr.U24 * c.stats_abs[:, :mv] * (1 + 2 * pr.U24)
                if not bool((err <= bar).all()):
                    g, r, k = (int(v) for v in np.argwhere(err > bar)[0])
                    msgs.append(f"{describe(c)}: stats group {g} row {r} sum {k}: error {err[g, r, k]:.3e} beyond {bar[g, r, k]:.3e}")
            continue
        width = c.out_width if name == "out" else N
        per = c.out_width // c.out_cols if name == "out" and c.out_width else 1
        if not torch.equal(_bytes2d(got[mv:]), _bytes2d(init[mv:])):
            r = int((_bytes2d(got[mv:]) != _bytes2d(init[mv:])).any(1).nonzero()[0]) + mv
            msgs.append(f"{describe(c)}: {name} row {r} (>= M_valid) was written")
        if not torch.equal(_bytes2d(got[:, width:]), _bytes2d(init[:, width:])):
            msgs.append(f"{describe(c)}: {name}: the padding columns were written")
        live = got[:mv, :width]
        if name in c.want:
            m = _first_diff(c, name, live, c.want[name][:mv], per)
            if m:
                msgs.append(m)
        else:
            m, _ = check_nonlinear(c, live)
            if m:
                msgs.append(m)
            if bool((_bytes2d(live) == SENTINEL).all(1).any()):
                msgs.append(f"{describe(c)}: a live row of {name} was not written")
    return msgs


def same_outputs(c, first, other, what):
    """Two launches that differ only in what lies behind the operands must agree in every byte."""
    for name in OUTPUTS:
        if name in first and not torch.equal(_bytes2d(first[name].reshape(first[name].shape[0], -1)), _bytes2d(other[name].reshape(other[name].shape[0], -1))):
            return [f"{describe(c)}: {name} depends on what lies behind the operands ({what})"]
    return []


# ------------------------------------------------------------------------------------------------ shapes
def tile_ks(fmt, tile):
    if fmt == "fp8":
        return (128, 256)
    if fmt == "f16x3":
        return (32, 64, 128)
    if fmt == "f16f8":
        return (64, 128)
    return (64, 128, 192, 320) if tile == 64 else (64, 128, 320)


def tile_shapes(l):
    """[(M, N, M_valid)]: two tiles of rows (what the format admits), two n-tiles; M_valid = M, h + 1, h, 1; 352 rows also at M = 768."""
    h, BN = GEOM[l.tile]
    M = {64: 128, 128: 256, 256: 512, 320: 1280 if l.fmt == "fp8" else 640, 352: 512}[l.tile]
    N = 1024 if (l.tile == 352 and l.epi == EPI_RESID_HILO) else 2 * BN
    shapes = [(M, N, mv) for mv in (M, h + 1, h, 1)]
    if l.tile == 352:
        shapes.append((768, N, 768))
    return shapes


def first_k(l):
    return tile_ks(l.fmt, l.tile)[0]


# ------------------------------------------------------------------------------------------------ real-valued operands
def real_case(l, M, N, K, m_valid, kind, seed=0):
    """randn operands ("randn") or rows that nearly cancel ("offset": every row of A is a constant + a small randn and every row of W sums to
    about zero, so |a w^T| << sum |a w|), in the stored format; the reference is the fp64 sum of the products of the stored factors."""
    assert l.epi in LINEAR
    c = Case()
    c.l, c.M, c.N, c.K, c.m_valid, c.kind, c.exact = l, M, N, K, m_valid, kind, False
    fmt, epi = l.fmt, l.epi
    rng = np.random.default_rng([seed, M, N, K, FORMATS.index(fmt), epi, int(l.folded), int(kind == "offset")])
    a = rng.standard_normal((M, K))
    w = rng.standard_normal((N, K)) * 0.05
    if kind == "offset":
        a = 3.0 + 0.01 * a
        w = w - w.mean(1, keepdims=True)
    split = fmt in SPLIT
    s_a, s_w = (16.0, 256.0) if split or fmt == "fp8" else (1.0, 1.0)     # powers of two: the scaling itself is exact
    a32, w32 = a.astype(F32), w.astype(F32)
    c.a, c.w = store(fmt, a32 * F32(s_a)), store(fmt, w32 * F32(s_w))
    pa, pw = parts(fmt, c.a), parts(fmt, c.w)
    if split:     # the operands are the fp32 values BEFORE packing, as token_bound takes them; the kernel undoes the scales with acc_scale
        a_v, w_v, unscale = a32.astype(np.float64), w32.astype(np.float64), 1.0 / (s_a * s_w)
    else:         # plain formats: the stored values, taken exactly (fp8: in the units of the stored bytes, dequantised by gamma)
        a_v, w_v, unscale, s_a, s_w = pa[0], pw[0], 1.0, 1.0, 1.0
    acc = a_v @ w_v.T
    c.mag = np.abs(a_v) @ np.abs(w_v).T
    # K 2^-24 sum |a w| + 2^-23 |acc| (+ the split formats' per-product term): vit_front_ref.token_bound without bias and position row,
    # with the number of products an accumulator really sums (three per k in the split formats)
    zero = np.zeros((M, N))
    acc_err = fr.token_bound(fmt if split else "bf16", a_v, w_v, np.zeros(N), zero, (3 if split else 1) * K, 1, s_a, s_w).numpy()
    if fmt == "fp8":
        # the fp8 MFMA aligns the 64 products of an instruction to the largest and cuts each off below 2^-13 of that one's binade (DESIGN.md
        # section 33): at most 64 x 2^-13 x the largest |product| per instruction.  (f16f8: its cross terms only, inside token_bound's 2 r |a w|.)
        for k0 in range(0, K, 64):
            acc_err = acc_err + 64 * 2.0 ** -13 * np.abs(a_v[:, k0:k0 + 64]).max(1)[:, None] * np.abs(w_v[:, k0:k0 + 64]).max(1)[None]
    bscale = 100.0 if fmt == "fp8" else 0.1
    c.bias = (rng.standard_normal(N) * bscale).astype(F32)
    c.gamma = c.colsum = c.ln_row = None
    c.acc_scale, c.out_scale = 0.0, 0.0
    lin, err = acc, acc_err
    ops_mag = np.zeros((M, N))                                # magnitudes of the results of the epilogue's fp32 operations: 2^-23 of each
    if split:
        c.acc_scale = unscale        # (acc in true units already: the reference multiplies the unscaled values)
    if l.folded:
        rstd = (0.5 + rng.random(M)).astype(F32)
        mrs = (rng.standard_normal(M) * 0.5).astype(F32)
        c.ln_row = np.stack([rstd, mrs], 1)
        c.colsum = (rng.standard_normal(N) * 0.2).astype(F32)
        t0 = -mrs[:, None].astype(np.float64) * c.colsum[None] + c.bias[None]
        lin, err = rstd[:, None] * lin + t0, rstd[:, None] * err
        ops_mag += np.abs(t0) + np.abs(lin)
    else:
        lin = lin + c.bias[None]
        ops_mag += np.abs(lin)
    if fmt == "fp8" or epi == EPI_LS_RESID:
        g = (0.5 + rng.random(N)).astype(F32)
        if fmt == "fp8":
            g = (g.astype(np.float64) * 2.0 ** -12).astype(F32)
        c.gamma = g
        lin, err, ops_mag = lin * g[None], err * g[None], ops_mag * g[None]
        ops_mag += np.abs(lin)
    c.pre = lin.astype(F32)
    c.lin64, c.err = lin, err
    c.ops_mag = ops_mag
    _finish(c, rng)
    if epi in RMW:
        x = (c.stream["out"].double().numpy() if "out" in c.stream else c.stream["xb"].double().numpy() + c.stream["xl"].double().numpy())
        c.lin64 = lin + x
        c.ops_mag = ops_mag + np.abs(c.lin64)
    return c


def real_check(c, outs):
    """Per element |out - fp64| <= accumulation + epilogue roundings + one rounding of the stored format.  -> (message or None, max err / bound)."""
    mv, N = c.m_valid, c.N
    epi = c.l.epi
    bound = c.err + fr.U24 * 2 * c.ops_mag          # each fp32 operation of the epilogue: half an ulp of its result, taken twice over
    if epi == EPI_RESID_HILO:
        got = outs["xb"][:mv, :N].double().numpy() + outs["xl"][:mv, :N].double().numpy()
        bound = bound + pr._half_ulp(c.t16, pr._half_ulp(c.t16, np.abs(c.lin64) + bound))   # hi' + lo' = x' up to lo's rounding: half an ulp at |lo'| <= half an ulp of x'
        bound = bound[:mv]
    elif epi in (EPI_LS_RESID, EPI_BIAS_F32, EPI_RESID_F32):
        got = outs["out"][:mv, :N].double().numpy()
    else:
        got = out_values(c, outs["out"][:mv, :c.out_width])
        bound = bound + store_bar(c, np.abs(c.lin64) + bound)
    ratio = np.abs(got - c.lin64[:mv]) / bound[:mv]    # (rows up to M_valid)
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    worst = float(ratio.max())
    if worst <= 1.0:
        return None, worst
    r, col = (int(v) for v in np.argwhere(ratio > 1.0)[0])
    return (f"{describe(c)}: {_where(c, r, col, 1)}: got {got[r, col]!r} want {c.lin64[r, col]!r}, "
            f"error {abs(got[r, col] - c.lin64[r, col]):.3e} beyond {bound[r, col]:.3e}"), worst
