"""gemm_bf16_kernel (csrc/gemm_kernel.hpp) against tests/gemm_ref.py: every row of the launch table -- five operand formats, five tile heights,
eight epilogues, plain and folded -- bit for bit on operands whose products and partial sums are exact in fp32 in any order.

A   per (format, tile): every epilogue of the table at K = one, two and more K-tiles, M = two tiles (352 rows: also three), M_valid = M, h + 1,
    h and 1.  Never an exact-size operand: A and W are the leading corners of buffers with 352 / 256 more rows and 16 more columns (lda = ldw =
    K + 16), the vectors have 256 (ln_row: 352) more entries, and those guards and A's rows in [M_valid, M) hold zeros, NaN and a large finite
    value in turn: the three launches must agree in every byte, the live elements must be the reference's bits (epilogues 1 / 6: within the
    per-element bound of their form on the exactly known pre-activation), and every byte outside them -- rows from M_valid on, 64 rows and 8 (e4m3:
    16) columns of padding, xb / xl / stats past M_valid -- must keep the 0x35 it was given.  Each case first asserts that the tile it forces
    is the tile the library runs (a forced tile the shape does not admit falls through to another one without an error).
B   per (format, tile): the linear epilogues on randn operands and on operands whose products nearly cancel, every element within the derived
    bound of vit_front_ref.token_bound; max err / bound is printed (DESIGN.md section 36 records it), nothing is tuned.
C   the tile map: three launches on the super-tile raster (>= 512 workgroups; a ragged last super-row, the cut at M_valid) with epilogue 0 into a
    sentinel-filled output (a tile never visited shows) and a read-modify-write epilogue on an integer stream (a tile visited twice shows)."""
import pytest
import torch

from foundpose_amd import _lib
from foundpose_amd._lib import ptr, stream
from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu

FMT_TILES = sorted({(l.fmt, l.tile) for l in gr.LAUNCHES}, key=lambda ft: (gr.FORMATS.index(ft[0]), ft[1]))
FT_IDS = [f"{f}-t{t}" for f, t in FMT_TILES]


def launch(c, dev):
    """One launch on the device buffers `dev` (place()'s, uploaded); the operands are the leading corners."""
    l, M, N, K, mv = c.l, c.M, c.N, c.K, c.m_valid
    kst = gr.stored_k(l.fmt, K)
    a, w = dev["a"][:M, :kst], dev["w"][:N, :kst]
    assert a.stride(0) == kst + gr.LD_EXTRA and w.stride(0) == kst + gr.LD_EXTRA
    assert gr.resolve_tile(l, M, N, K, mv, a.stride(0), w.stride(0)) == l.tile, f"{gr.describe(c)}: the shape does not admit the forced tile"
    out = dev.get("out")
    flags = l.epi | (l.tile << 8)
    if l.fmt == "fp8":
        _lib.call("fp_gemm_fp8", ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, mv, ptr(dev["bias"]), ptr(dev["gamma"]), ptr(out), out.stride(0),
                  flags, float(c.out_scale if l.f8out else 0.0), stream())
    elif l.fmt in gr.SPLIT:
        _lib.call("fp_gemm_split", ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, mv, ptr(dev["bias"]), ptr(dev.get("gamma")), ptr(out), out.stride(0),
                  flags | (_lib.GEMM_SPLIT_F16F8 if l.fmt == "f16f8" else 0), float(c.acc_scale), float(c.out_scale or 1.0), stream())
    else:
        flags |= _lib.GEMM_F16 if l.fmt == "f16" else 0
        head = (ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, mv, ptr(dev["bias"]))
        if l.folded:
            _lib.call("fp_gemm_bf16_ln", *head, ptr(out), out.stride(0), flags, ptr(dev["colsum"]), ptr(dev["ln_row"]), None, 0, None, stream())
        elif l.epi == gr.EPI_RESID_HILO:
            xb, xl = dev["xb"], dev["xl"]
            _lib.call("fp_gemm_bf16_ln", *head, ptr(xl), xl.stride(0), flags, None, None, ptr(xb), xb.stride(0), ptr(dev["stats"]), stream())
        elif l.epi == gr.EPI_RESID_F32:
            xb = dev["xb"]
            _lib.call("fp_gemm_bf16_ln", *head, ptr(out), out.stride(0), flags, None, None, ptr(xb), xb.stride(0), ptr(dev["stats"]), stream())
        else:
            _lib.call("fp_gemm_bf16", *head, ptr(dev.get("gamma")), ptr(out), out.stride(0), flags, stream())
    return {k: dev[k] for k in gr.OUTPUTS if k in dev}


def run_fill(c, fill):
    b = gr.place(c, fill)
    return b, launch(c, {k: t.cuda() for k, t in b.items()})


def _same(x, y):
    return torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8))


def exact_case(c):
    """Three fills, one answer; the answer is the reference's."""
    b, first = run_fill(c, "zero")
    for fill in ("nan", "big"):
        _, other = run_fill(c, fill)
        for name in first:
            assert _same(first[name], other[name]), f"{gr.describe(c)}: {name} depends on what lies behind the operands ({fill})"
    if all(name in c.want for name in first):
        # every output has exact bits: the expected bytes of a buffer are what it was given, with the reference's bits in the live corner
        ok = True
        for name, got in first.items():
            want = b[name].clone()
            if name == "stats":
                want[:, :c.m_valid] = c.want[name][:, :c.m_valid]
            else:
                want[:c.m_valid, :c.want[name].shape[1]] = c.want[name][:c.m_valid]
            ok = ok and _same(got, want.cuda())
        if ok:
            return
    # a non-linear epilogue, the fp32-summed stats of the large stream -- or a mismatch, for its message
    torch.cuda.synchronize()
    msgs = gr.check(c, b, {k: t.cpu() for k, t in first.items()})
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("fmt,tile", FMT_TILES, ids=FT_IDS)
def test_every_epilogue_bit_for_bit_whatever_lies_behind_the_operands(fmt, tile):
    rows = [l for l in gr.LAUNCHES if (l.fmt, l.tile) == (fmt, tile)]
    n = 0
    for l in rows:
        for K in gr.tile_ks(fmt, tile):
            for i, (M, N, mv) in enumerate(gr.tile_shapes(l)):
                kinds = ["int"] + (["lo"] if fmt in gr.SPLIT else []) + (["big"] if l.epi == gr.EPI_RESID_HILO and i == 1 else [])
                for kind in kinds:
                    exact_case(gr.build(l, M, N, K, mv, kind))
                    n += 1
    torch.cuda.synchronize()
    gr._operand_cache.clear()
    print(f"gemm_edges/exact {fmt} tile {tile}: {len(rows)} rows of the launch table, {n} cases x 3 fills")


@pytest.mark.parametrize("fmt,tile", FMT_TILES, ids=FT_IDS)
def test_real_operands_within_the_derived_bound_per_element(fmt, tile):
    """Measured on the MI355X: DESIGN.md section 36."""
    rows = [l for l in gr.LAUNCHES if (l.fmt, l.tile) == (fmt, tile) and l.epi in gr.LINEAR]
    K = gr.tile_ks(fmt, tile)[-1]
    worst = {}
    for l in rows:
        M, N, mv = gr.tile_shapes(l)[0]
        for kind in ("randn", "offset"):
            c = gr.real_case(l, M, N, K, mv, kind)
            _, outs = run_fill(c, "nan")
            torch.cuda.synchronize()
            msg, ratio = gr.real_check(c, {k: t.cpu() for k, t in outs.items()})
            print(f"gemm_edges/real {gr.describe(c)}: max err / bound = {ratio:.4f}")
            assert msg is None, msg
            worst[kind] = max(worst.get(kind, 0.0), ratio)
    print(f"gemm_edges/real {fmt} tile {tile} K {K}: max err / bound randn {worst['randn']:.4f} offset {worst['offset']:.4f}")


RASTERS = [(256, 16640, 2048, 16640), (256, 11264, 3072, 11009), (352, 22272, 2048, 22177)]


@pytest.mark.parametrize("tile,M,N,mv", RASTERS, ids=[f"t{t}-{m}x{n}-valid{v}" for t, m, n, v in RASTERS])
def test_tile_map_visits_every_tile_once(tile, M, N, mv):
    K, dev = 64, torch.device("cuda")
    BM, BN = gr.GEOM[tile]
    grid, tiles = gr.tile_order(tile, M, N, mv)
    assert grid >= 512 and gr.pick_raster(BM, N // BN, -(-mv // BM) * (N // BN))[0], "the launch is not on the super-tile raster"
    g = torch.Generator(device=dev).manual_seed(tile + M)
    A = torch.full((M + gr.A_GUARD, K + gr.LD_EXTRA), float("nan"), dtype=torch.bfloat16, device=dev)
    W = torch.full((N + gr.W_GUARD, K + gr.LD_EXTRA), float("nan"), dtype=torch.bfloat16, device=dev)
    A[:mv, :K] = torch.randint(-1, 2, (mv, K), device=dev, generator=g).to(torch.bfloat16)
    W[:N, :K] = torch.randint(-2, 3, (N, K), device=dev, generator=g).to(torch.bfloat16)
    bias = torch.full((N + gr.VEC_GUARD,), float("nan"), device=dev)
    bias[:N] = torch.randint(-8, 9, (N,), device=dev, generator=g).float()
    gamma = torch.full((N + gr.VEC_GUARD,), float("nan"), device=dev)
    gamma[:N] = 2.0 ** torch.randint(-1, 2, (N,), device=dev, generator=g).float()
    a, w = A[:M, :K], W[:N, :K]
    ref = (A[:mv, :K].double() @ W[:N, :K].double().T + bias[:N].double())     # integers: exact in fp64 and, below 2^24, in fp32 in any order
    assert float(ref.abs().max()) <= 256
    head = (ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, mv, ptr(bias))

    def sentinel(rows, cols, dtype):
        t = torch.empty(rows, cols, dtype=dtype, device=dev)
        t.view(torch.uint8).fill_(gr.SENTINEL)
        return t

    def where(diff):
        r, c = (int(v) for v in diff.nonzero()[0])
        return f"tile {tile} M {M} N {N} M_valid {mv}: first at row {r}, column {c} (m-tile {r // BM}, n-tile {c // BN}, band {r % BM // 32}); {int(diff.any(1).sum())} rows differ"

    # epilogue 0 into a sentinel-filled output: a tile that is never visited keeps its sentinel
    out = sentinel(M + gr.OUT_ROWS_EXTRA, N + gr.OUT_COLS_EXTRA, torch.bfloat16)
    want = out.clone()
    want[:mv, :N] = ref.to(torch.bfloat16)
    assert torch.equal(want[:mv, :N].double(), ref)
    _lib.call("fp_gemm_bf16", *head, None, ptr(out), out.stride(0), 0 | (tile << 8), stream())
    diff = out.view(torch.int16) != want.view(torch.int16)
    assert not bool(diff.any()), "epilogue 0: " + where(diff)
    # a read-modify-write epilogue on an integer stream: a tile visited twice adds twice
    x = torch.randint(-64, 65, (mv, N), device=dev, generator=g).float()
    if tile == 352:     # (epilogue 3 has no 352-row tile: the (hi, lo) stream instead)
        xb, xl = sentinel(M + gr.OUT_ROWS_EXTRA, N + gr.OUT_COLS_EXTRA, torch.bfloat16), sentinel(M + gr.OUT_ROWS_EXTRA, N + gr.OUT_COLS_EXTRA, torch.bfloat16)
        stats = sentinel(N // 128, M * 2, torch.float32).reshape(N // 128, M, 2)
        want_b, want_l, want_s = xb.clone(), xl.clone(), stats.clone()
        xb[:mv, :N], xl[:mv, :N] = x.to(torch.bfloat16), 0.0
        xn = x.double() + ref
        want_b[:mv, :N], want_l[:mv, :N] = xn.to(torch.bfloat16), 0.0
        assert torch.equal(want_b[:mv, :N].double(), xn)
        want_s[:, :mv, 0] = xn.reshape(mv, N // 128, 128).sum(2).T.float()
        want_s[:, :mv, 1] = (xn * xn).reshape(mv, N // 128, 128).sum(2).T.float()
        assert float((xn * xn).reshape(mv, N // 128, 128).sum(2).max()) < 2.0 ** 24
        _lib.call("fp_gemm_bf16_ln", *head, ptr(xl), xl.stride(0), 8 | (tile << 8), None, None, ptr(xb), xb.stride(0), ptr(stats), stream())
        for name, got, wnt in (("xb", xb, want_b), ("xl", xl, want_l)):
            diff = got.view(torch.int16) != wnt.view(torch.int16)
            assert not bool(diff.any()), f"epilogue 8 {name}: " + where(diff)
        assert torch.equal(stats.view(torch.int32), want_s.view(torch.int32)), "epilogue 8: stats"
    else:
        o32 = sentinel(M + gr.OUT_ROWS_EXTRA, N + gr.OUT_COLS_EXTRA, torch.float32)
        want32 = o32.clone()
        o32[:mv, :N] = x
        want32[:mv, :N] = (x.double() + ref * gamma[:N].double()).float()
        _lib.call("fp_gemm_bf16", *head, ptr(gamma), ptr(o32), o32.stride(0), 3 | (tile << 8), stream())
        diff = o32.view(torch.int32) != want32.view(torch.int32)
        assert not bool(diff.any()), "epilogue 3: " + where(diff)
    torch.cuda.synchronize()
