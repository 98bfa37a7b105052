"""tests/gemm_ref.py against itself (no GPU): the exactness conditions of its builders, the reference against plain torch fp64, the restated
launch logic, and -- what shows that tests/test_gpu_gemm_edges.py has teeth -- the emulated kernel under every checker: the faithful
emulation passes on every row of the launch table, and every imitated fault fails."""
import numpy as np
import pytest
import torch

from tests import gemm_ref as gr

IDS = [gr.launch_id(l) for l in gr.LAUNCHES]


def _cpu_shape(l):
    """One live row in the second tile: the shape at which a store guard, a dropped K-tile and a row read from behind A all show."""
    M, N, mv = gr.tile_shapes(l)[1]
    return M, gr.GEOM[l.tile][1], gr.tile_ks(l.fmt, l.tile)[1], mv      # (one n-tile: the emulation is paid for per element)


def _kind(l):
    return "lo" if l.fmt in gr.SPLIT else "int"


def test_launch_table_is_the_issue_s():
    assert len(gr.LAUNCHES) == len(set(gr.LAUNCHES)) == 97
    per = {}
    for l in gr.LAUNCHES:
        per.setdefault((l.fmt, l.tile), []).append((l.epi, l.folded, l.f8out))
    assert sorted(per) == sorted([(f, t) for f in ("bf16", "f16") for t in (64, 128, 256, 320, 352)] + [("fp8", 256), ("fp8", 320)]
                                 + [(f, t) for f in gr.SPLIT for t in (128, 256)])
    assert per[("bf16", 64)] == [(3, False, False), (7, False, False), (8, False, False)]
    assert len(per[("f16", 256)]) == 10 and len(per[("bf16", 352)]) == 5 and len(per[("fp8", 256)]) == 6 and len(per[("fp8", 320)]) == 5


@pytest.mark.parametrize("l", gr.LAUNCHES, ids=IDS)
def test_every_shape_is_admitted_by_its_tile(l):
    for M, N, mv in gr.tile_shapes(l):
        for K in gr.tile_ks(l.fmt, l.tile):
            ld = gr.stored_k(l.fmt, K) + gr.LD_EXTRA
            assert gr.resolve_tile(l, M, N, K, mv, ld, ld) == l.tile


def test_forced_tiles_fall_through_silently():
    L = gr.Launch
    assert gr.resolve_tile(L("bf16", 320, 0, False, False), 512, 512, 64, 512, 80, 80) == 128          # M % 320 != 0
    assert gr.resolve_tile(L("bf16", 64, 0, False, False), 128, 256, 64, 128, 80, 80) == 128           # 64 rows: residual epilogues only
    assert gr.resolve_tile(L("bf16", 256, 0, False, False), 384, 512, 64, 384, 80, 80) == 128
    assert gr.resolve_tile(L("bf16", 320, 6, False, False), 640, 512, 64, 640, 80, 80) == 128          # SwiGLU has no 320-row tile
    assert gr.resolve_tile(L("fp8", 320, 3, False, False), 1280, 512, 128, 1280, 144, 144) == 256      # the fp8 residual epilogue keeps 256 rows
    assert gr.resolve_tile(L("fp8", 320, 0, False, False), 512, 512, 128, 512, 144, 144) == 256
    assert gr.resolve_tile(L("f16x3", 256, 0, False, False), 384, 512, 32, 384, 80, 80) == 128
    with pytest.raises(ValueError):
        gr.resolve_tile(L("bf16", 352, 0, False, False), 512, 384, 64, 512, 80, 80)                    # 352 rows without N % 256 == 0: refused
    with pytest.raises(ValueError):
        gr.resolve_tile(L("f16x3", 128, 0, False, False), 256, 256, 64, 256, 120, 144)                 # lda < 2K


RASTERS = [(256, 16640, 2048, 16640, (4, 8), 65), (256, 11264, 3072, 11009, (8, 4), 44), (352, 22272, 2048, 22177, (4, 8), 64)]


@pytest.mark.parametrize("tile,M,N,mv,raster,m_tiles", RASTERS)
def test_tile_order_visits_every_tile_once(tile, M, N, mv, raster, m_tiles):
    BM, BN = gr.GEOM[tile]
    grid, tiles = gr.tile_order(tile, M, N, mv)
    assert gr.pick_raster(BM, N // BN, m_tiles * (N // BN)) == raster and grid >= 512
    assert -(-m_tiles // raster[0]) * raster[0] > m_tiles or tile == 352, "the last super-row is ragged"
    seen = sorted((m0, n0) for _, m0, n0 in tiles)
    assert seen == [(i * BM, j * BN) for i in range(m_tiles) for j in range(N // BN)]
    assert len(set(b for b, _, _ in tiles)) == len(tiles) and grid - len(tiles) == (-(-m_tiles // raster[0]) * raster[0] - m_tiles) * (N // BN)


def test_tile_order_small_launches_and_the_cut_at_m_valid():
    for tile, M, N, mv, want in [(128, 256, 256, 129, 2), (128, 256, 256, 128, 1), (352, 512, 512, 512, 2), (352, 768, 512, 768, 3), (64, 128, 256, 1, 1)]:
        BM, BN = gr.GEOM[tile]
        grid, tiles = gr.tile_order(tile, M, N, mv)
        assert grid == len(tiles) == want * (N // BN)
        assert sorted((m0, n0) for _, m0, n0 in tiles) == [(i * BM, j * BN) for i in range(want) for j in range(N // BN)]


def test_small_integers_survive_every_stored_format():
    ints = np.arange(-16, 17, dtype=np.float32).reshape(1, -1)
    row = np.zeros((1, 64), np.float32)
    row[:, :33] = ints
    for fmt in gr.FORMATS:
        st = gr.store(fmt, row)
        p = gr.parts(fmt, st)
        assert np.array_equal(p[0], row), fmt
        if fmt == "f16f8":
            assert np.array_equal(p[1], row) and not p[2].any()       # the e4m3 copy of hi holds integers up to 16 exactly
        if fmt == "f16x3":
            assert not p[1].any()
    lo = (row + (row != 0) * 2.0 ** -12).astype(np.float32)           # i + 2^-12: hi = i, lo = 2^-12, in both split packings
    for fmt in gr.SPLIT:
        p = gr.parts(fmt, gr.store(fmt, lo))
        assert np.array_equal(p[0], row) and np.array_equal(p[-1], (row != 0) * 2.0 ** -12), fmt


def test_accumulator_range_of_the_integer_operands():
    """max |acc + bias| at 704 x 512 over five seeds stays inside bf16's exact integers (256) up to K = 512."""
    for K, limit in ((64, 80), (128, 100), (256, 140), (512, 190)):
        worst = 0.0
        for seed in range(5):
            rng = np.random.default_rng([seed, K])
            a = rng.integers(-1, 2, size=(704, K)).astype(np.float64)
            w = rng.integers(-2, 3, size=(512, K)).astype(np.float64)
            worst = max(worst, float(np.abs(a @ w.T + rng.integers(-8, 9, size=512)[None]).max()))
        print(f"K {K}: max |acc + bias| {worst:g}")
        assert worst < limit < 256


@pytest.mark.parametrize("l", gr.LAUNCHES, ids=IDS)
def test_reference_is_the_fp64_product(l):
    """The exact reference against plain torch fp64 on the decoded operands (and the builders' own assertions, which run inside build)."""
    M, N, K, mv = _cpu_shape(l)
    c = gr.build(l, M, N, K, mv, _kind(l), seed=1)
    pa, pw = gr.parts(l.fmt, c.a), gr.parts(l.fmt, c.w)
    if l.fmt == "f16x3":
        a, w = pa[0] + pa[1], pw[0] + pw[1]
        lolo = pa[1] @ pw[1].T
    elif l.fmt == "f16f8":
        a, w = pa[0] + pa[2], pw[0] + pw[2]
        lolo = pa[2] @ pw[2].T
    else:
        a, w, lolo = pa[0], pw[0], 0.0
    acc = (torch.from_numpy(a) @ torch.from_numpy(w).T).numpy() - lolo        # the split modes drop lo * lo by design
    lin = acc * (c.acc_scale if l.fmt in gr.SPLIT else 1.0)
    if l.folded:
        lin = c.ln_row[:, :1].astype(np.float64) * lin - c.ln_row[:, 1:].astype(np.float64) * c.colsum[None]
    lin = lin + c.bias[None]
    if c.gamma is not None:
        lin = lin * c.gamma[None]
    assert np.array_equal(lin, c.pre.astype(np.float64))
    if l.epi in gr.RMW:
        x = c.stream["out"].double().numpy() if "out" in c.stream else c.stream["xb"].double().numpy() + c.stream["xl"].double().numpy()
        assert np.array_equal(x + lin, c.x_new.astype(np.float64))


@pytest.mark.parametrize("l", gr.LAUNCHES, ids=IDS)
def test_clean_emulation_passes_and_every_fault_fails(l):
    M, N, K, mv = _cpu_shape(l)
    c = gr.build(l, M, N, K, mv, _kind(l), seed=2)
    ld = gr.stored_k(l.fmt, K) + gr.LD_EXTRA
    assert gr.resolve_tile(l, M, N, K, mv, ld, ld) == l.tile
    bufs = {f: gr.place(c, f) for f in gr.FILLS}
    outs = {f: gr.emulate(c, bufs[f]) for f in gr.FILLS}
    msgs = gr.check(c, bufs["zero"], outs["zero"])
    for f in ("nan", "big"):
        msgs += gr.same_outputs(c, outs["zero"], outs[f], f)
    assert not msgs, "\n".join(msgs)
    for i, fault in enumerate(gr.FAULTS):
        # each row of the table takes a third of the faults in turn, and always the two that only some rows can show
        if not gr.fault_applies(fault, c) or ((i + gr.LAUNCHES.index(l)) % 3 and fault not in ("tile_twice", "drop_lo_hi")):
            continue
        bad = {f: gr.emulate(c, bufs[f], fault) for f in ("zero", "nan")}
        caught = gr.check(c, bufs["zero"], bad["zero"]) + gr.same_outputs(c, bad["zero"], bad["nan"], "nan")
        assert caught, f"{gr.describe(c)}: the imitated fault {fault} passes every checker"


def test_every_fault_is_exercised():
    """Each imitated fault applies to (and so, by the test above, is caught on) at least one row of the launch table."""
    for fault in gr.FAULTS:
        n = 0
        for l in gr.LAUNCHES:
            M, N, K, mv = _cpu_shape(l)
            c = gr.Case()
            c.l, c.kind, c.m_valid = l, _kind(l), mv
            n += gr.fault_applies(fault, c) and ((gr.FAULTS.index(fault) + gr.LAUNCHES.index(l)) % 3 == 0 or fault in ("tile_twice", "drop_lo_hi"))
        assert n >= 12, fault


@pytest.mark.parametrize("l", [l for l in gr.LAUNCHES if l.epi == 8 and l.tile in (64, 352)], ids=lambda l: gr.launch_id(l))
def test_big_stream_has_a_new_low_half(l):
    M, N, mv = gr.tile_shapes(l)[1]
    c = gr.build(l, M, N, 64, mv, "big", seed=3)
    assert not c.stats_exact and bool((c.want["xl"] != 0).any())
    b = gr.place(c, "nan")
    assert not gr.check(c, b, gr.emulate(c, b))
    assert gr.check(c, b, gr.emulate(c, b, "tile_twice")) and gr.check(c, b, gr.emulate(c, b, "drop_ktile"))


def test_mismatch_message_names_the_place():
    l = gr.Launch("bf16", 352, 8, False, False)
    c = gr.build(l, 512, 1024, 128, 353, "int", seed=4)
    b = gr.place(c, "zero")
    msgs = gr.check(c, b, gr.emulate(c, b, "drop_ktile"))
    assert msgs and "bf16-t352-e8" in msgs[0] and "M 512 N 1024 K 128 M_valid 353" in msgs[0]
    assert "row 352, column 0 (m-tile 1, n-tile 0, band 0)" in msgs[0] and "got" in msgs[0] and "want" in msgs[0]


@pytest.mark.parametrize("l", [gr.Launch("bf16", 128, 0, False, False), gr.Launch("f16", 256, 8, False, False), gr.Launch("fp8", 256, 3, False, False),
                               gr.Launch("f16x3", 128, 0, False, False), gr.Launch("f16f8", 128, 5, False, False), gr.Launch("bf16", 128, 0, True, False)],
                         ids=lambda l: gr.launch_id(l))
@pytest.mark.parametrize("kind", ["randn", "offset"])
def test_real_bound_holds_for_fp32_accumulation_and_catches_a_lost_product(l, kind):
    """The per-element bound on the fp32 restatement of the accumulation (sequential fp32 sums: the worst order) and on one with a product lost."""
    M, N, mv = gr.tile_shapes(l)[0]
    K = gr.tile_ks(l.fmt, l.tile)[-1]
    c = gr.real_case(l, M, N, K, mv, kind)
    b = gr.place(c, "zero")
    pa, pw = gr.parts(l.fmt, c.a), gr.parts(l.fmt, c.w)

    def run(drop):
        acc = np.zeros((M, N), np.float32)
        for fa, fw in gr.products(l.fmt, pa, pw):
            for k in range(K):
                if drop and k == K // 2 and fa is pa[0] and fw is pw[0]:
                    continue
                acc = (acc + np.outer(fa[:, k], fw[:, k]).astype(np.float32)).astype(np.float32)
        return acc

    for drop in (False, True):
        acc = run(drop)
        # the epilogue in fp32 on that accumulator
        v = acc.astype(np.float64)
        if l.fmt in gr.SPLIT:
            v = np.float32(v * c.acc_scale).astype(np.float64)
        if l.folded:
            t0 = np.float32(-c.ln_row[:, 1:].astype(np.float64) * c.colsum[None] + c.bias[None]).astype(np.float64)
            v = np.float32(c.ln_row[:, :1].astype(np.float64) * v + t0)
        else:
            v = np.float32(v + c.bias[None])
        if c.gamma is not None:
            v = np.float32(v.astype(np.float64) * c.gamma[None])
        outs = {k: t.clone() for k, t in b.items() if k in gr.OUTPUTS}
        if l.epi == 8:
            x = np.float32(outs["xb"][:M, :N].double().numpy() + outs["xl"][:M, :N].double().numpy())
            xn = np.float32(v.astype(np.float64) + x)
            hi = torch.as_tensor(xn).to(outs["xb"].dtype)
            outs["xb"][:M, :N] = hi
            outs["xl"][:M, :N] = torch.as_tensor(xn - hi.float().numpy()).to(hi.dtype)
        elif l.epi == 3:
            outs["out"][:M, :N] = torch.as_tensor(np.float32(v.astype(np.float64) + outs["out"][:M, :N].double().numpy()))
        elif l.epi == 5:
            outs["out"][:M, :N] = torch.as_tensor(np.float32(v))
        else:
            outs["out"][:M, :c.out_width] = gr._round_store(c, np.float32(v), c.out_scale)
        msg, worst = gr.real_check(c, outs)
        print(f"{gr.describe(c)} {'one product lost' if drop else 'fp32 restatement'}: max err / bound {worst:.3f}")
        assert (msg is None) == (not drop), msg
