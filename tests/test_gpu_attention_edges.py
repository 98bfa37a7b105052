"""Attention kernels (csrc/attn.hip) at the ragged key tiles, against fp64 per element, and what they do with the rows behind their operands.

Shapes (tests/attention_ref.py TOKENS x PAIRS): the three forms of the last key tile -- full, at most 32 live keys (second key half skipped), 33 - 63
live keys (N = 33, 63, 97, 127, 161, 319: the form no older test reaches in the 16-bit and split-fp16 kernels) --, a short second query tile (N = 300: 44
queries, the one-block-per-wave path, at the end of the launch when the (image, head) pairs divide by 8), a short tail of exactly 128 (N = 384), 129 remaining
queries with one live key (N = 385); 1, 6, 8 and 8 (image, head) pairs for both block mappings.

Checks, per kernel and operand builder, every token count inside one test:
  1. accuracy against fp64 on the rounded operands: per element under the derived bound for bf16 / fp16 (attention_ref.bound), per row in units of the row's
     scale for the fp32 and split-fp16 kernels (helpers.check_bar); `planted` operands also name the key each output row came from.
  2. guard fills: the operand is the leading corner of a tensor with 128 more rows and 16 more columns, so no launch here reads memory the test did not
     allocate -- never pass an exact-size operand in this file.  The guard rows and columns are filled with zeros, with NaN and with an "attractor" (K = 8 x
     the mean query, V = 1000); the three outputs must be bit-identical.  A padded key's score is overwritten with -inf, so its K cannot matter; its V row
     meets P = 0 in the P V product, and 0 x NaN = NaN: a kernel that fetches rows past the last token must fetch something finite.  With three images each
     image alone must give the bits of its rows in the batched launch (image b's padded keys are image b + 1's first rows, whose V is set to 1000).
  3. output footprint: the output is the leading corner of a sentinel-filled tensor with 64 more rows and 8 more columns; the guards keep the sentinel and
     every live element was written.
"""

import pytest
import torch

from foundpose_amd import _lib, ops
from foundpose_amd._lib import call, ptr, stream
from tests import attention_ref as ar
from tests.helpers import check_bar

pytestmark = pytest.mark.gpu

GUARD_ROWS, GUARD_COLS = 128, 16     # behind / beside the qkv operand
OUT_ROWS, OUT_COLS = 64, 8           # behind / beside the output
SENTINEL = -7.25                     # exact in bf16, fp16 and fp32
IN_SCALE, OUT_SCALE = 64.0, 128.0    # split-fp16 operand and output scales (tests/test_gpu_split.py)

# kernel -> (operand format, variant, f16f8 output)
KERNELS = {
    "bf16_v0": ("bf16", 0, False),       # attn_bf16_w64_kernel<false>: what the pipeline runs
    "bf16_v1": ("bf16", 1, False),       # attn_bf16_kernel: the register-staged cross-check
    "f16": ("f16", 0, False),            # attn_bf16_w64_kernel<true>
    "fp32_mfma": ("fp32", 0, False),     # attn_f32_mfma_kernel
    "fp32_valu": ("fp32", 1, False),     # attn_f32_kernel
    "split": ("split", 0, False),        # attn_split_kernel, split-fp16 output rows
    "split_f16f8": ("split", 0, True),   # attn_split_kernel, f16f8 output rows
}
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "fp32": torch.float32, "split": torch.float16}
# while a key has no record in tests/golden/measured_bars.json: the existing relative bars of these kernels (tests/test_gpu_vit.py 2e-5, tests/test_gpu_split.py
# 5e-6), applied to the row's scale instead of the global maximum
FALLBACK = {"fp32": 2e-5, "split": 5e-6}
# Recorded on the MI355X (tests/golden/measured_bars.json, attention_edges/*): fp32 kernels 1.7e-7 - 9.8e-6, split-fp16 output 1.8e-7 - 8.2e-6, f16f8 output
# 3.1e-6 - 1.5e-5.  `offset` is the largest of each: its scores are -256 + noise before the 1/8, so every fp32 accumulation step rounds at 2^-16 and the
# probabilities carry ~1e-5 -- the split kernel (8.2e-6) sits at the fp32 kernels' own level there (9.7e-6), above its 5e-6 fallback.  The f16f8 output row keeps
# ~16 bits of an element (fp16 hi + a 4-bit e4m3 lo), 1.5e-5, which the fallback of the split-fp16 row does not fit either; tests/test_gpu_f16f8.py holds that
# row format to 2^-13 of the split-fp16 output.


def encode(x, fmt):
    """fp32 logical rows [rows, 3 D] -> the kernel's operand rows [rows, 3 D em]."""
    if fmt == "split":
        D = x.shape[1] // 3
        return torch.cat([ops.split16_pack(x[:, i * D:(i + 1) * D].contiguous(), IN_SCALE) for i in range(3)], dim=1)
    return x.to(DTYPES[fmt])


def decode_operand(rows, fmt):
    """operand rows -> the values they stand for, fp64 [rows, 3 D]."""
    if fmt == "split":
        g = rows.reshape(rows.shape[0], rows.shape[1] // 64, 2, 32).double()
        return ((g[:, :, 0] + g[:, :, 1]) / IN_SCALE).reshape(rows.shape[0], rows.shape[1] // 2)
    return rows.double()


def decode_output(live, fmt, f16f8):
    """live output rows -> fp64 [rows, D]."""
    if fmt != "split":
        return live.double()
    live = live.contiguous()
    if f16f8:
        return ops.splitx_unpack(live, OUT_SCALE).double()
    g = live.reshape(live.shape[0], live.shape[1] // 64, 2, 32).double()
    return ((g[:, :, 0] + g[:, :, 1]) / OUT_SCALE).reshape(live.shape[0], live.shape[1] // 2)


def guarded_operand(logical, fmt, fill):
    """logical fp32 [rows, 3 D] (the operand's rows) -> (buffer [rows + GUARD_ROWS, 3 D em + GUARD_COLS], operand view = its leading corner).
    fill: what the guard rows and columns hold -- "zero", "nan" (in the operand's format; both halves of a split pair) or "attractor"."""
    rows, D3 = logical.shape
    D = D3 // 3
    guard = torch.zeros(GUARD_ROWS, D3, device=logical.device)
    if fill == "attractor":
        guard[:, D:2 * D] = 8.0 * logical[:, :D].mean(dim=0)
        guard[:, 2 * D:] = 1000.0
    enc = encode(torch.cat([logical, guard]), fmt)
    pad = {"zero": 0.0, "nan": float("nan"), "attractor": 1000.0}[fill]
    buf = torch.full((rows + GUARD_ROWS, enc.shape[1] + GUARD_COLS), pad, dtype=enc.dtype, device=logical.device)
    buf[:, :enc.shape[1]] = enc
    if fill == "nan":
        buf[rows:] = float("nan")
    return buf, buf[:rows, :enc.shape[1]]


def launch(kernel, operand, B, N, heads):
    """operand: a [B N, 3 D em] view of a guarded buffer -> (sentinel-filled output buffer, its live corner)."""
    fmt, variant, f16f8 = KERNELS[kernel]
    D = heads * 64
    em = 2 if fmt == "split" else 1
    assert operand.shape == (B * N, 3 * D * em) and operand.stride(1) == 1 and operand.storage_offset() == 0
    # the rows behind and the columns beside the operand belong to the test's own allocation
    assert operand.stride(0) == 3 * D * em + GUARD_COLS and operand.untyped_storage().nbytes() >= (B * N + GUARD_ROWS) * operand.stride(0) * operand.element_size()
    obuf = torch.full((B * N + OUT_ROWS, D * em + OUT_COLS), SENTINEL, dtype=operand.dtype, device=operand.device)
    if fmt == "split":
        call("fp_attention_split", ptr(operand), operand.stride(0), ptr(obuf), obuf.stride(0), B, N, D, heads, IN_SCALE, OUT_SCALE,
             (_lib.FP_F16F8 if f16f8 else _lib.FP_F16X3) | (variant << 8), stream())
    else:
        dt = {"bf16": _lib.FP_BF16, "f16": _lib.FP_F16, "fp32": _lib.FP_F32}[fmt]
        call("fp_attention", ptr(operand), operand.stride(0), ptr(obuf), obuf.stride(0), B, N, D, heads, dt | (variant << 8), stream())
    return obuf, obuf[:B * N, :D * em]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


_sweeps = {}


def sweep(kernel, kind):
    """Every launch of one (kernel, builder), once -> {"accuracy": [...], "guards": [...], "footprint": [...], "planted": [...]} failure lists and
    "row_error", the worst row error of the fp32 / split-fp16 kernels."""
    if (kernel, kind) in _sweeps:
        return _sweeps[(kernel, kind)]
    fmt, variant, f16f8 = KERNELS[kernel]
    res = {"accuracy": [], "guards": [], "footprint": [], "planted": [], "variants": [], "row_error": 0.0, "bound_ratio": 0.0}
    dev = torch.device("cuda")
    for B, heads in ar.PAIRS:
        D = heads * 64
        for N in ar.TOKENS:
            tag = f"B={B} heads={heads} N={N}"
            logical = ar.build(kind, B, N, heads).reshape(B * N, 3 * D).to(dev)
            outs = {}
            for fill in ("zero", "nan", "attractor"):
                buf, operand = guarded_operand(logical, fmt, fill)
                outs[fill] = launch(kernel, operand, B, N, heads)
            torch.cuda.synchronize()
            obuf, live = outs["zero"]
            # ---- 1. accuracy, on the operand the kernel read
            x = decode_operand(operand, fmt).reshape(B, N, 3, heads, 64)
            ref, S = ar.reference(x)
            got = decode_output(live, fmt, f16f8).reshape(B, N, heads, 64)
            if not torch.isfinite(got).all():
                res["accuracy"].append(f"{tag}: non-finite output with zero guards")
            elif fmt in ("bf16", "f16"):
                ratio = float(((got - ref).abs() / ar.bound(S, x[:, :, 2], fmt)).max())
                res["bound_ratio"] = max(res["bound_ratio"], ratio)
                if ratio > 1.0:
                    res["accuracy"].append(f"{tag}: |out - ref| / bound = {ratio:.3f}")
            else:
                res["row_error"] = max(res["row_error"], ar.row_error(got, ref, S))
                if kind == "planted":
                    want = (ar.planted_key(N, dev) % 64)[None, :, None].expand(B, N, heads)
                    bad = int((got.argmax(dim=-1) != want).sum())
                    if bad:
                        res["planted"].append(f"{tag}: {bad} output rows name another key than t(q)")
            if kernel == "bf16_v1":   # the two work splits stay bit-identical
                o0 = launch("bf16_v0", operand, B, N, heads)[1]
                if not same_bits(o0, live):
                    res["variants"].append(tag)
            # ---- 2. guard fills
            for fill in ("nan", "attractor"):
                if not same_bits(outs[fill][1], live):
                    o = decode_output(outs[fill][1], fmt, f16f8)
                    res["guards"].append(f"{tag}: {fill} guards change the output ({int((~torch.isfinite(o)).sum())} non-finite elements, "
                                         f"{int((o != decode_output(live, fmt, f16f8)).sum())} differ)")
            if B == 3:   # each image alone against its rows of the batched launch; V of the rows behind an image = 1000
                lg = logical.clone()
                for b in range(1, B):
                    lg[b * N:b * N + min(N, 63), 2 * D:] = 1000.0
                batched = launch(kernel, guarded_operand(lg, fmt, "zero")[1], B, N, heads)[1]
                for b in range(B):
                    alone = launch(kernel, guarded_operand(lg[b * N:(b + 1) * N], fmt, "zero")[1], 1, N, heads)[1]
                    if not same_bits(alone, batched[b * N:(b + 1) * N]):
                        res["guards"].append(f"{tag}: image {b} alone differs from its rows in the batch")
            # ---- 3. output footprint
            if not bool((obuf[B * N:] == SENTINEL).all()) or not bool((obuf[:, live.shape[1]:] == SENTINEL).all()):
                res["footprint"].append(f"{tag}: a guard row or pad column of the output lost the sentinel")
            if fmt == "split" and not f16f8:
                # an unwritten element keeps the sentinel in BOTH halves (a written pair cannot: |lo| <= half an ulp of hi)
                pair = live.reshape(B * N, -1, 2, 32)
                unwritten = int(((pair[:, :, 0] == SENTINEL) & (pair[:, :, 1] == SENTINEL)).sum())
            elif fmt == "split":
                # f16f8 row: per 64 columns 128 B of fp16 hi halves, 64 B e4m3(hi 2^-7), 64 B e4m3 lo.  Unwritten: the hi half and its e4m3 copy both hold the
                # sentinel's bytes (0x40, 0xC7: as e4m3, 2.0 and -3.75, neither of them e4m3(-7.25 x 2^-7))
                by = live.contiguous().view(torch.uint8).reshape(B * N, -1, 256)
                hi = by[:, :, :128].contiguous().view(torch.float16)
                pattern = torch.tensor([0x40, 0xC7], dtype=torch.uint8, device=dev).repeat(32)
                unwritten = int(((hi == SENTINEL) & (by[:, :, 128:192] == pattern)).sum())
            else:
                unwritten = int(((live == SENTINEL) & (ref.reshape(B * N, D).to(live.dtype) != SENTINEL)).sum())
            if unwritten:
                res["footprint"].append(f"{tag}: {unwritten} live elements still hold the sentinel")
    _sweeps[(kernel, kind)] = res
    return res


@pytest.mark.parametrize("kind", ar.BUILDERS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_accuracy_against_fp64(kernel, kind):
    res = sweep(kernel, kind)
    fmt = KERNELS[kernel][0]
    print(f"{kernel} {kind}: worst error / bound {res['bound_ratio']:.3f}, worst row error {res['row_error']:.3e}")
    assert not res["accuracy"], "\n".join(res["accuracy"])
    assert not res["planted"], "\n".join(res["planted"])
    assert not res["variants"], "bf16 variants 0 and 1 differ at " + "; ".join(res["variants"])
    if fmt in ("fp32", "split"):
        check_bar(f"attention_edges/{kernel}/{kind}", res["row_error"], FALLBACK[fmt])


@pytest.mark.parametrize("kind", ar.BUILDERS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_rows_behind_the_operand_do_not_reach_the_output(kernel, kind):
    res = sweep(kernel, kind)
    assert not res["guards"], f"{len(res['guards'])} cases, first ones:\n" + "\n".join(res["guards"][:12])


def test_a_nan_value_row_under_zero_probability_reaches_the_output():
    """The positive control of the guard fills: what they would see if a kernel did fetch the rows behind its operand.  fp16 kernel, `planted` operands, 33 keys:
    with K[5] = 0 key 5 scores 0 against the ~54 of a query's planted key, so its probability (e^-30 or less, times at most 2^8 of lazy rescale) rounds to an fp16
    zero for every query but the one it was planted for; with V[5] = NaN the P V MFMA multiplies 0 x NaN and every output row of the head turns NaN."""
    B, N, heads = 1, 33, 1
    logical = ar.build("planted", B, N, heads).reshape(B * N, 3 * 64).to("cuda")
    clean = launch("f16", guarded_operand(logical, "f16", "zero")[1], B, N, heads)[1]
    assert torch.isfinite(clean.float()).all()
    logical[5, 64:2 * 64] = 0.0
    logical[5, 2 * 64:] = float("nan")
    poisoned = launch("f16", guarded_operand(logical, "f16", "zero")[1], B, N, heads)[1]
    assert torch.isnan(poisoned.float()).all()


@pytest.mark.parametrize("kind", ar.BUILDERS)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_output_footprint(kernel, kind):
    res = sweep(kernel, kind)
    assert not res["footprint"], "\n".join(res["footprint"][:12])


# ---------------------------------------------------------------------------------------------------- the 33 - 63-key tile inside a whole forward
# TINY at 84 x 84: 36 patches + 1 + 4 registers = 41 tokens; ViT-S/14-reg at 140 x 140: 100 + 5 = 105 tokens = one full key tile + 41 live keys
EXTRACTOR_CASES = {"tiny_84": ("tiny-reg", 84, 2, 3e-5, 6e-2), "vits14reg_140": ("vits14-reg", 140, 9, 5e-5, 8e-2)}


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "bf16", "f16"])
@pytest.mark.parametrize("case", list(EXTRACTOR_CASES))
def test_extractor_with_41_live_keys_in_the_last_tile(case, precision):
    """Against the fp32 CPU oracle (oracle.vit.extractor_forward), under the bars these modes have at the other crop sizes: the exact modes' tolerance
    (tests/test_gpu_vit.py), the recorded-bar rule for bf16 (fallback: its tolerance there) and f16 (fallback 2e-3, tests/test_gpu_f16.py)."""
    import numpy as np
    from foundpose_amd import feature_util, synthetic
    from foundpose_amd.vit_config import ARCHS
    from oracle import vit as ov
    from tests.helpers import TINY, assert_features_close
    version, size, layer, tol_exact, tol_bf16 = EXTRACTOR_CASES[case]
    arch = TINY if version == "tiny-reg" else ARCHS[version]
    assert (1 + arch.registers + (size // 14) ** 2) % 64 == 41
    sd = synthetic.make_vit_state_dict(arch, seed=1234)
    imgs = synthetic.make_crops(2, size, seed=5)
    key = (case, "ref")
    if key not in _sweeps:
        _sweeps[key] = ov.extractor_forward(sd, arch, imgs, layer, True)
    ref = _sweeps[key]
    name = f"dinov2_version={version}_stride=14_facet=token_layer={layer}_logbin=0_norm=1"
    ex = feature_util.make_feature_extractor(name, state_dict=sd, precision=precision, arch=arch if arch is TINY else None).to("cuda")
    o = ex(imgs.cuda())
    fm, rf = o["feature_maps"].cpu().numpy(), ref["feature_maps"].numpy()
    assert fm.shape == rf.shape and np.isfinite(fm).all()
    scale = np.abs(rf).max()
    lossy = precision in ("bf16", "f16")
    tol = {"fp32": tol_exact, "f16x3": tol_exact, "bf16": tol_bf16, "f16": 2e-3}[precision]
    e = assert_features_close(f"attention_edges/{case}/{precision}/fmap", fm, rf, scale, tol, lossy)
    assert_features_close(f"attention_edges/{case}/{precision}/cls", o["cls_tokens"].cpu().numpy(), ref["cls_tokens"].numpy(), scale, tol, lossy)
    print(f"{case} {precision}: {e:.3e} of the feature scale")
