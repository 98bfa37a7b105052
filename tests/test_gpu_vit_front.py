"""The ViT's token-embedding front, kernel by kernel, against tests/vit_front_ref.py: what builds the input of block 0.

A / B  fp_patchify (patchify_kernel<T, SPLIT>, the LDS kernel): the five operand formats bit for bit, the wide-row loop (W > 576), padding
       columns, guard rows, and the launcher's refusals.
C      the embedding alone through the extractor (fp_vit_forward, layer = -1) on a workspace pre-filled with a sentinel: the patch rows of
       both patchify kernels bit for bit, the stored patch matrix, prefix_tokens_kernel bit for bit, and the TOKENS epilogue (row b Np + p ->
       b Ntok + skip + p, + pos[p]) within a derived bound (vit_front_ref.token_bound) of the fp64 token sequence.
D      rowstats_cast_kernel (fp_vit_forward_prefix, layer = 0): the (hi, lo) pair bit for bit, the row sums, the zeroed slots.
E      fp_convert_f32_to_bf16 against torch's cast, specials and the odd tail included.

Every buffer a kernel writes is first filled with the byte 0x35 (a finite number in every format involved); what the kernel must not touch must
still hold it afterwards."""
import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops, synthetic
from foundpose_amd._lib import ptr, stream
from foundpose_amd.dinov2_utils import DinoFeatureExtractor
from foundpose_amd.vit_config import VitArch
from oracle import vit as ov
from tests import vit_front_ref as fr

pytestmark = pytest.mark.gpu

TINY = VitArch("tiny-reg", dim=128, depth=3, heads=2, ffn="mlp", hidden=512, registers=4, pretrain_grid=4, interp_antialias=True, interp_offset=0.0)
TINY_NOREG = VitArch("tiny", dim=128, depth=3, heads=2, ffn="mlp", hidden=512, registers=0, pretrain_grid=4, interp_antialias=False, interp_offset=0.1)
SMALL1 = VitArch("small1-reg", dim=384, depth=1, heads=6, ffn="mlp", hidden=1536, registers=4, pretrain_grid=4, interp_antialias=True, interp_offset=0.0)
PRECISION = {"f32": "fp32", "bf16": "bf16", "f16": "f16", "f16x3": "f16x3", "f16f8": "f16f8"}
P, K, KPAD = 14, 588, 640
SENTINEL = 0x35


def _fill(t):
    t.view(torch.uint8).fill_(SENTINEL)
    return t


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == SENTINEL).all())


def _images(B, H, W, seed=0):
    """rng.random in fp32 with exact 0 and 1 planted: corners, the seam between the 576-pixel passes, one interior pixel per channel."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, 3, H, W), dtype=np.float32)
    x[:, :, 0, 0], x[:, :, -1, -1], x[:, :, 0, -1], x[:, :, -1, 0] = 0.0, 1.0, 1.0, 0.0
    x[:, 0, H // 2, W // 2], x[:, 1, H // 3, W // 3], x[:, 2, H - 2, W // 5] = 1.0, 0.0, 1.0
    if W > 576:
        x[:, :, :, 575], x[:, :, :, 576] = 0.0, 1.0
    return x


def _assert_bits(got, want, what):
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} against {want.dtype} {tuple(want.shape)}"
    diff = (got.view(torch.uint8) != want.view(torch.uint8)).reshape(got.shape[0], -1)
    if bool(diff.any()):
        r, c = (int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.sum())} bytes differ, the first in row {r} at byte {c}")


# ------------------------------------------------------------------------------------------------ A: fp_patchify, bit for bit
PATCHIFY_SHAPES = [(1, 14, 14), (3, 28, 70), (2, 42, 588), (2, 28, 630), (1, 14, 1162)]
PATCHIFY_CASES = [(f, s) for s in PATCHIFY_SHAPES for f in fr.FORMATS if s[2] < 882 or f in ("bf16", "f16")]   # fp32 / split rows of W >= 882 exceed LDS


@pytest.mark.parametrize("fmt,shape", PATCHIFY_CASES, ids=[f"{f}-{s[0]}x{s[1]}x{s[2]}" for f, s in PATCHIFY_CASES])
def test_patchify_rows_bit_for_bit(fmt, shape):
    B, H, W = shape
    x = _images(B, H, W, seed=H + W)
    rows = fr.patch_rows(x, P)
    n = rows.shape[0]
    xd = torch.from_numpy(x).cuda()
    em = 2 if fmt in ("f16x3", "f16f8") else 1
    for ld in (em * 640, em * 704):
        buf = _fill(torch.empty(n + 2, ld, dtype=fr.FMT_DTYPE[fmt], device="cuda"))      # a guard row before and one behind
        _lib.call("fp_patchify", ptr(xd), B, H, W, P, ptr(buf[1:]), ld, fr.FMT_ABI[fmt], stream())
        torch.cuda.synchronize()
        want = fr.pack(fmt, rows, ld)                    # padding columns (hi and lo halves, e4m3 copies) are zero in it
        _assert_bits(buf[1:n + 1], want, f"patchify {fmt} {shape} ld {ld}")
        assert _untouched(buf[0]) and _untouched(buf[n + 1]), f"patchify {fmt} {shape} ld {ld}: a guard row was written"


# ------------------------------------------------------------------------------------------------ B: refusals
REFUSALS = [
    ("H not a multiple of the patch", "f32", 1, 15, 14, 640),
    ("W not a multiple of the patch", "bf16", 1, 14, 21, 640),
    ("ld_out below 588", "bf16", 1, 14, 14, 584),
    ("fp32 rows of 642 floats are not 16-byte rows", "f32", 1, 14, 14, 642),
    ("bf16 rows of 644 elements are not 16-byte rows", "bf16", 1, 14, 14, 644),
    ("split ld_out not a multiple of 64", "f16x3", 1, 14, 14, 1312),
    ("split ld_out below 2 x the padded columns", "f16x3", 1, 14, 14, 1152),
    ("f16f8 ld_out below 1280", "f16f8", 1, 14, 14, 1152),
    ("f16f8 ld_out not a multiple of 128", "f16f8", 1, 14, 14, 1344),
    ("fp32 rows of W = 882 need 164052 B of LDS", "f32", 1, 14, 882, 640),
    ("null images", "f32", 1, 14, 14, 640),
    ("null output", "f32", 1, 14, 14, 640),
]


@pytest.mark.parametrize("why,fmt,B,H,W,ld", REFUSALS, ids=[r[0].replace(" ", "_") for r in REFUSALS])
def test_patchify_refuses(why, fmt, B, H, W, ld):
    xd = torch.rand(B, 3, H + P, W + P, device="cuda")                       # (room for what a launch that is NOT refused would read and write)
    buf = _fill(torch.empty(B * (H // P + 1) * (W // P + 1) + 2, max(ld, 1408), dtype=fr.FMT_DTYPE[fmt], device="cuda"))
    img = None if why == "null images" else xd
    out = None if why == "null output" else buf[1:]
    rc = _lib.lib().fp_patchify(ptr(img), B, H, W, P, ptr(out), ld, fr.FMT_ABI[fmt], stream())
    torch.cuda.synchronize()
    assert rc != 0, f"{why}: accepted"
    assert "patchify" in _lib.lib().fp_last_error().decode()
    assert _untouched(buf), f"{why}: refused, yet the output was written"


def test_patchify_empty_batch_writes_nothing():
    xd = torch.rand(1, 3, 28, 28, device="cuda")
    buf = _fill(torch.empty(6, 640, dtype=torch.float32, device="cuda"))
    _lib.call("fp_patchify", ptr(xd), 0, 28, 28, P, ptr(buf[1:]), 640, _lib.FP_F32, stream())
    torch.cuda.synchronize()
    assert _untouched(buf)


# ------------------------------------------------------------------------------------------------ C: the embedding alone, through the extractor
_EXTRACTORS = {}


def _extractor(arch, fmt, stride):
    key = (arch.name, fmt, stride)
    if key not in _EXTRACTORS:
        sd = synthetic.make_vit_state_dict(arch, seed=1)
        name = f"dinov2_version={arch.name}_stride={stride}_facet=token_layer=0_norm=1"
        _EXTRACTORS[key] = (DinoFeatureExtractor(name, state_dict=sd, arch=arch, precision=PRECISION[fmt]).to("cuda"), sd)
    return _EXTRACTORS[key]


def _pos_table(sd, arch, stride, H, W):
    gh, gw = fr.grid(H, W, P, stride)
    if stride == P:
        return ov.interpolate_pos_embed(sd["pos_embed"], arch, gh, gw)[0]
    return ov.interpolate_pos_embed_strided(sd["pos_embed"], P, stride, H, W)[0]     # the reference's _fix_pos_enc


EMBED_SHAPES = [(14, (3, 28, 70)), (14, (3, 140, 140)), (14, (2, 42, 588)), (7, (2, 28, 49)), (7, (3, 70, 77))]
EMBED_CASES = ([(TINY, f, s, shp) for s, shp in EMBED_SHAPES for f in fr.FORMATS]
               + [(TINY_NOREG, f, s, shp) for s, shp in (EMBED_SHAPES[0], EMBED_SHAPES[3]) for f in fr.FORMATS])


@pytest.mark.parametrize("arch,fmt,stride,shape", EMBED_CASES,
                         ids=[f"{a.name}-{f}-s{s}-{shp[0]}x{shp[1]}x{shp[2]}" for a, f, s, shp in EMBED_CASES])
def test_embedding_rows_prefix_and_tokens(arch, fmt, stride, shape):
    """The bound of the patch-token rows is vit_front_ref.token_bound: derived, nothing in it is tuned to the kernels.  Measured on the MI355X,
    max(err / bound) over the cases of a format: f32 0.0068, bf16 0.0026, f16 0.0023, f16x3 0.0039, f16f8 0.0104 (a worst-case bound over 640
    products against rounding errors that mostly cancel; a wrong position row or a lost lo half is 10 to 1000 x the bound)."""
    B, H, W = shape
    ex, sd = _extractor(arch, fmt, stride)
    x = _images(B, H, W, seed=stride + H + W)
    gh, gw = fr.grid(H, W, P, stride)
    n_p, R, D = gh * gw, arch.registers, arch.dim
    ntok = 1 + R + n_p
    live = ex.embed_tokens(torch.from_numpy(x).cuda(), prefill=lambda t: [_fill(v) for v in t.values()])
    torch.cuda.synchronize()
    em = 2 if fmt in ("f16x3", "f16f8") else 1
    what = f"{arch.name} {fmt} stride {stride} {shape}"

    # the patch rows: the kernel of this stride in this format, bit for bit; the rows behind them untouched
    rows = fr.patch_rows(x, P, stride)
    patches = live["patches"]
    assert patches.shape[1] == em * KPAD and patches.shape[0] >= B * n_p
    _assert_bits(patches[:B * n_p], fr.pack(fmt, rows, em * KPAD), f"patch rows, {what}")
    assert _untouched(patches[B * n_p:]), f"{what}: patch rows beyond the batch were written"

    # the stored patch matrix: the checkpoint's conv weight flattened (c, py, px), columns >= 588 zero
    w32 = sd["patch_embed.proj.weight"].reshape(D, K)
    s_w = ops.pow2_scale(w32) if em == 2 else 1.0
    w_stored = fr.pack(fmt, w32.numpy(), em * KPAD, scale=s_w)
    _assert_bits(ex._w["patch_w"], w_stored, f"patch_w, {what}")

    # cls + pos[0] and the register tokens, bit for bit; the rows behind the batch untouched
    pos = _pos_table(sd, arch, stride, H, W)
    assert pos.shape == (1 + n_p, D)
    xt = live["x"]
    tok = xt[:B * ntok].cpu().reshape(B, ntok, D)
    cls_row = (sd["cls_token"].reshape(1, D).float() + pos[:1].float())              # one fp32 add, on the host
    _assert_bits(tok[:, 0], cls_row.expand(B, D), f"cls row, {what}")
    if R:
        _assert_bits(tok[:, 1:1 + R].reshape(B * R, D), sd["register_tokens"].float().expand(B, R, D).reshape(B * R, D), f"register rows, {what}")
    assert _untouched(xt[B * ntok:]), f"{what}: token rows beyond the batch were written"
    for name in ("xb", "xl", "stats"):                  # (a folded model: the embedding alone leaves the chain's buffers alone)
        assert name not in live or _untouched(live[name]), f"{what}: {name} was written by an embedding-only run"

    # the patch tokens against the fp64 sequence, within the derived bound
    if em == 2:      # split formats: the operands are the fp32 values before packing
        a_op, w_op = torch.from_numpy(rows), w32
    else:            # plain formats: the stored values, taken exactly
        a_op, w_op = fr.pack(fmt, rows, KPAD)[:, :K], w_stored[:, :K]
    bias = sd["patch_embed.proj.bias"]
    ref = fr.tokens_ref(a_op, w_op, bias, pos, sd["cls_token"], sd["register_tokens"][0] if R else None, B)
    assert ref.shape == (B, ntok, D)
    bound = fr.token_bound(fmt, a_op, w_op, bias, pos[1:], KPAD, B, s_w=s_w).reshape(B, n_p, D)
    err = (tok[:, 1 + R:].double() - ref[:, 1 + R:]).abs()
    ratio = float((err / bound).max())
    print(f"vit_front/tokens {what}: max err / bound = {ratio:.4f} (max err {float(err.max()):.3e})")
    assert ratio <= 1.0, f"{what}: a patch token is {ratio:.3f} x its bound away from the fp64 sequence"


# ------------------------------------------------------------------------------------------------ D: rowstats_cast
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_rowstats_cast_pair_and_sums(fmt):
    """dim 384: three stat groups; lanes 32..63 of a wave do one pass fewer than lanes 0..31."""
    B, H, W = 2, 28, 70
    ex, _ = _extractor(SMALL1, fmt, P)
    x = _images(B, H, W, seed=11)
    live = ex.embed_tokens(torch.from_numpy(x).cuda(), prefill=lambda t: [_fill(v) for v in t.values()], row_stats=True)
    torch.cuda.synchronize()
    D, rows = SMALL1.dim, B * (1 + SMALL1.registers + 2 * 5)
    xt = live["x"][:rows].cpu()
    xb_ref, xl_ref, s1, s2 = fr.rowstats_ref(xt, fmt)
    for name, want in (("xb", xb_ref), ("xl", xl_ref)):
        t = live[name]
        assert t.dtype == want.dtype and t.shape[1] > D
        _assert_bits(t[:rows, :D], want, f"{name} {fmt}")
        assert _untouched(t[:rows, D:]) and _untouched(t[rows:]), f"{name} {fmt}: padding columns or rows beyond the batch were written"
    stats = live["stats"]                               # [D / 128 partial-sum slots + the row constants, m_pad, (sum x, sum x^2)]
    assert stats.shape[0] == D // 128 + 1
    got = stats[:, :rows].cpu().double()
    b1, b2 = D * fr.U24 * xt.double().abs().sum(1), D * fr.U24 * (xt.double() ** 2).sum(1)
    r1, r2 = float(((got[0, :, 0] - s1).abs() / b1).max()), float(((got[0, :, 1] - s2).abs() / b2).max())
    print(f"vit_front/rowstats {fmt}: max err / bound = {r1:.4f} (sum x), {r2:.4f} (sum x^2)")
    assert r1 <= 1.0 and r2 <= 1.0
    assert not bool(stats[1:3, :rows].cpu().view(torch.int32).any()), "slots 1 and 2 of a live row must be exactly +0"
    assert _untouched(stats[:3, rows:]), "stat rows beyond the batch were written"
    assert _untouched(stats[3]), "the row constants were written although no block ran"


# ------------------------------------------------------------------------------------------------ E: fp_convert_f32_to_bf16
def _bits(v):
    return np.array(v, dtype=np.uint32).view(np.float32)


SPECIALS = np.concatenate([
    np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32),
    _bits([0x00000001, 0x807FFFFF, 0x00008000, 0x00018000]),      # subnormals, two of them ties
    _bits([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000]),      # exact ties: to the even neighbour below, and above
    _bits([0x3F808001, 0x3F807FFF]),                              # just off a tie
    _bits([0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF]),                  # the largest finite fp32 (rounds to inf), and the largest that stays finite
    _bits([0x7F800001, 0x7FC00000]),                              # a signalling and a quiet NaN
])


@pytest.mark.parametrize("n", [1, 2, 511, 512, 513, 65537])
def test_convert_f32_to_bf16_bits(n):
    rng = np.random.default_rng(n)
    x = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()   # every exponent, NaNs and infs among them
    m = min(n, SPECIALS.size)
    x[:m] = SPECIALS[:m]
    if n & 1:
        x[n - 1] = _bits([0x3F818000 if n > 1 else 0x3F808000])[0]  # a tie as the last, odd element: the scalar path
    xt = torch.from_numpy(x)
    out = _fill(torch.empty(n + 8, dtype=torch.bfloat16, device="cuda"))
    _lib.call("fp_convert_f32_to_bf16", ptr(xt.cuda()), ptr(out), n, stream())
    torch.cuda.synchronize()
    got, want = out[:n].cpu(), xt.to(torch.bfloat16)
    nan = torch.isnan(xt)
    assert bool(torch.isnan(got.float())[nan].all()), "a NaN did not stay a NaN"
    gi, wi = got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]
    bad = (gi != wi).nonzero()
    assert bad.numel() == 0, f"{bad.numel()} of {n} differ from torch's cast, the first: {float(xt[~nan][int(bad[0])])!r}"
    assert _untouched(out[n:]), "elements behind n were written"
