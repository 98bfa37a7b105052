"""tests/vit_front_ref.py against torch's own arithmetic (CPU only): the restatement the GPU tests of the token-embedding front compare
the kernels with must itself be the reference's operation -- T.Normalize followed by the patch-embedding conv, the token order of the
backbone (cls, registers, patches), and operand rows that stand for the values they were packed from."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from foundpose_amd import _lib, synthetic
from foundpose_amd.vit_config import VitArch
from oracle import vit as ov
from tests import vit_front_ref as fr

TINY = VitArch("tiny-reg", dim=128, depth=3, heads=2, ffn="mlp", hidden=512, registers=4, pretrain_grid=4, interp_antialias=True, interp_offset=0.0)
SHAPES = [(2, 28, 70, 14), (3, 42, 28, 14), (2, 28, 49, 7), (1, 35, 21, 7)]   # (B, H, W, stride): non-square, both strides


def _images(B, H, W, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.random((B, 3, H, W), dtype=np.float32)
    x[:, :, 0, 0], x[:, :, -1, -1], x[:, 1, H // 2, W // 2] = 0.0, 1.0, 1.0
    return x


@pytest.mark.parametrize("B,H,W,stride", SHAPES)
def test_patch_rows_are_the_unfold_of_the_normalised_image(B, H, W, stride):
    x = _images(B, H, W)
    rows = fr.patch_rows(x, 14, stride)
    gh, gw = fr.grid(H, W, 14, stride)
    norm = ov.normalize_images(torch.from_numpy(x))                     # (x - mean) / std in fp32, torch's own two operations
    want = F.unfold(norm, kernel_size=14, stride=stride)                 # [B, 3 P P, gh gw]: channel order (c, py, px), positions (gy, gx)
    assert want.shape == (B, 588, gh * gw)
    want = want.transpose(1, 2).reshape(B * gh * gw, 588)
    assert rows.dtype == np.float32 and fr.same_bits(torch.from_numpy(rows), want.contiguous())
    assert float(np.abs(rows).max()) < 2.65


@pytest.mark.parametrize("B,H,W,stride", SHAPES)
def test_patch_rows_times_the_flattened_weight_is_the_conv(B, H, W, stride):
    x = _images(B, H, W, seed=1)
    g = torch.Generator().manual_seed(2)
    D = 24
    weight = torch.randn(D, 3, 14, 14, generator=g, dtype=torch.float64) * 0.02
    rows = torch.from_numpy(fr.patch_rows(x, 14, stride)).double()
    got = rows @ weight.reshape(D, -1).T
    xn = ((torch.from_numpy(x) - torch.tensor(fr.IMNET_MEAN).view(1, 3, 1, 1)) / torch.tensor(fr.IMNET_STD).view(1, 3, 1, 1)).double()
    want = F.conv2d(xn, weight, stride=stride).flatten(2).transpose(1, 2).reshape(-1, D)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()) * 588


@pytest.mark.parametrize("stride,H,W", [(14, 28, 70), (7, 28, 49)])
def test_tokens_ref_is_the_oracles_token_sequence(stride, H, W):
    sd = synthetic.make_vit_state_dict(TINY, seed=1)
    x = _images(2, H, W, seed=3)
    gh, gw = fr.grid(H, W, 14, stride)
    pos = (ov.interpolate_pos_embed(sd["pos_embed"], TINY, gh, gw) if stride == 14 else
           ov.interpolate_pos_embed_strided(sd["pos_embed"], 14, stride, H, W))[0]
    got = fr.tokens_ref(fr.patch_rows(x, 14, stride), sd["patch_embed.proj.weight"].reshape(TINY.dim, -1), sd["patch_embed.proj.bias"], pos,
                        sd["cls_token"], sd["register_tokens"][0], 2)
    want = ov.embed_tokens(sd, TINY, ov.normalize_images(torch.from_numpy(x)), stride=None if stride == 14 else stride)
    assert got.shape == want.shape == (2, 1 + 4 + gh * gw, TINY.dim)
    assert float((got - want.double()).abs().max()) < 1e-5               # fp32 conv against fp64: a wrong row or position would be ~0.05
    assert torch.equal(got[:, 1:5].float(), sd["register_tokens"].expand(2, -1, -1))
    assert torch.equal(got[:, 0].float(), (sd["cls_token"][0] + pos[:1]).expand(2, -1))


@pytest.mark.parametrize("fmt", fr.FORMATS)
@pytest.mark.parametrize("ld_cols", [640, 704])
def test_pack_stands_for_the_row_and_pads_with_zeros(fmt, ld_cols):
    x = _images(2, 28, 42, seed=4)
    x[0, 0, 3, 3] = np.float32(0.485) + np.float32(2.0 ** -20)          # a normalised value of ~4e-6: below the formats' normal ranges
    rows = fr.patch_rows(x)
    split = fmt in ("f16x3", "f16f8")
    ld = 2 * ld_cols if split else ld_cols
    p = fr.pack(fmt, rows, ld)
    assert p.shape == (rows.shape[0], ld) and p.dtype == fr.FMT_DTYPE[fmt]
    back = fr.unpack(fmt, p)
    v = torch.from_numpy(rows).double()
    assert back.shape == (rows.shape[0], ld_cols) and not bool(back[:, 588:].any())
    err, s = (back[:, :588] - v).abs(), _lib.SPLIT_SCALE_ACT
    if fmt == "f32":
        assert not bool(err.any())
        assert not bool(p[:, 588:].any())
    elif fmt == "bf16":
        assert bool((err <= 2.0 ** -8 * v.abs()).all()) and not bool(p[:, 588:].view(torch.int16).any())
    elif fmt == "f16":
        assert bool((err <= torch.maximum(2.0 ** -11 * v.abs(), torch.tensor(2.0 ** -25, dtype=torch.float64))).all())
        assert not bool(p[:, 588:].view(torch.int16).any())
    elif fmt == "f16x3":       # the bounds tests/test_gpu_split.py asserts of split16_pack
        big = v.abs() * s > 0.25
        assert float((err / v.abs())[big].max()) < 2.0 ** -21 and float(err[~big].max() if bool((~big).any()) else 0.0) * s <= 2.0 ** -24
        g = p.view(torch.int16).reshape(rows.shape[0], ld_cols // 32, 2, 32)   # groups of 32 columns: [hi 32 | lo 32]
        assert not bool(g.permute(0, 1, 3, 2).reshape(rows.shape[0], ld_cols, 2)[:, 588:].any())
        assert torch.equal(g[:, :, 0].reshape(rows.shape[0], ld_cols)[:, :588].view(torch.float16), (torch.from_numpy(rows) * s).half())
    else:                      # ... and tests/test_gpu_f16f8.py of splitx_pack
        big = v.abs() * s > 1.0
        assert float((err / v.abs())[big].max()) < 2.0 ** -14 and float(err[~big].max() if bool((~big).any()) else 0.0) * s <= 2.0 ** -13
        by = p.view(torch.uint8).reshape(rows.shape[0], ld_cols // 64, 256)    # groups of 64 columns: [hi 128 B | e4m3(hi) 64 B | e4m3(lo) 64 B]
        col = torch.arange(ld_cols).reshape(ld_cols // 64, 64) >= 588
        assert not bool(by[:, :, :128].reshape(rows.shape[0], ld_cols // 64, 64, 2)[:, col].any())
        assert not bool(by[:, :, 128:192][:, col].any()) and not bool(by[:, :, 192:][:, col].any())
    if split:                  # the lo halves carry information: dropping them is 2^-11 of the value, not 2^-21
        hi_only = (torch.from_numpy(rows) * s).half().double() / s
        assert float(((hi_only - v).abs() / v.abs()).max()) > 2.0 ** -13


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_rowstats_ref_pair_rebuilds_the_row(fmt):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(7, 384, generator=g) * 3.0
    xb, xl, s1, s2 = fr.rowstats_ref(x, fmt)
    assert xb.dtype == xl.dtype == fr.FMT_DTYPE[fmt]
    assert torch.equal(xb, x.to(fr.FMT_DTYPE[fmt]))
    bits = 8 if fmt == "bf16" else 11
    back = xb.double() + xl.double()
    floor = 0.0 if fmt == "bf16" else 2.0 ** -25            # fp16: a lo half below 2^-14 is subnormal (spacing 2^-24)
    err = (back - x.double()).abs()
    assert bool((err <= torch.clamp(2.0 ** (-2 * bits) * x.double().abs(), min=floor)).all())   # two roundings of `bits` significant bits each
    assert torch.allclose(s1, x.double().sum(1)) and torch.allclose(s2, (x.double() ** 2).sum(1))
