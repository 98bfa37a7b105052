"""Plain restatement of the ViT's token-embedding front (numpy / torch CPU, no GPU): what sits between the image and block 0.

* patch_rows: T.Normalize + the unfold of the patch-embedding conv -> the fp32 rows of the patch GEMM (csrc/vit.hip: patchify_kernel,
  patchify_strided_kernel);
* pack: the stored image of such a row in each of the five operand formats (fp32, bf16, fp16, split-fp16 "f16x3", "f16f8");
* tokens_ref: the token sequence [cls + pos0 | registers | A W^T + bias + pos] in fp64 (prefix_tokens_kernel, the TOKENS epilogues of
  csrc/gemm_kernel.hpp and csrc/f32_tile.hip), and token_bound: the error a correct fp32-accumulating kernel may show against it;
* rowstats_ref: the entry of the folded-LayerNorm chain (rowstats_cast_kernel): the (hi, lo) 16-bit pair of a row and its two sums.

Used by tests/test_vit_front_cpu.py (the restatement against torch's own unfold / conv2d) and tests/test_gpu_vit_front.py (the kernels
against the restatement)."""

import numpy as np
import torch

from foundpose_amd import _lib, ops

IMNET_MEAN = (0.485, 0.456, 0.406)    # the constants of csrc/vit.hip (T.Normalize of the reference's extractor)
IMNET_STD = (0.229, 0.224, 0.225)
FORMATS = ("f32", "bf16", "f16", "f16x3", "f16f8")
FMT_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16, "f16x3": torch.float16, "f16f8": torch.float16}
FMT_ABI = {"f32": _lib.FP_F32, "bf16": _lib.FP_BF16, "f16": _lib.FP_F16, "f16x3": _lib.FP_F16X3, "f16f8": _lib.FP_F16F8}
U24, U23 = 2.0 ** -24, 2.0 ** -23
# what a packed row represents, as tests/test_gpu_split.py and tests/test_gpu_f16f8.py assert it of the two packers: (relative, absolute x scale)
REPR = {"f16x3": (2.0 ** -21, 2.0 ** -24), "f16f8": (2.0 ** -13, 2.0 ** -13)}


def grid(H, W, patch, stride=None):
    """Patch tokens per axis: 1 + (size - patch) // stride."""
    stride = patch if stride is None else stride
    return 1 + (H - patch) // stride, 1 + (W - patch) // stride


def patch_rows(images, patch=14, stride=None):
    """images fp32 [B, 3, H, W] -> fp32 [B * gh * gw, 3 * P * P]: row b * gh * gw + gy * gw + gx, column c * P * P + py * P + px holds
    (x - mean_c) / std_c of pixel (gy * stride + py, gx * stride + px): two individually rounded fp32 operations, T.Normalize's order."""
    x = np.ascontiguousarray(np.asarray(images, dtype=np.float32))
    B, C, H, W = x.shape
    assert C == 3
    stride = patch if stride is None else stride
    gh, gw = grid(H, W, patch, stride)
    mean = np.asarray(IMNET_MEAN, np.float32).reshape(1, 3, 1, 1)
    std = np.asarray(IMNET_STD, np.float32).reshape(1, 3, 1, 1)
    v = ((x - mean).astype(np.float32) / std).astype(np.float32)
    rows = np.empty((B, gh, gw, 3, patch, patch), np.float32)
    for gy in range(gh):
        for gx in range(gw):
            rows[:, gy, gx] = v[:, :, gy * stride:gy * stride + patch, gx * stride:gx * stride + patch]
    return rows.reshape(B * gh * gw, 3 * patch * patch)


def pack(fmt, rows, ld, scale=_lib.SPLIT_SCALE_ACT):
    """The stored image of fp32 rows [n, K] in format fmt with a row of `ld` stored elements (split formats: halves, two per column):
    torch tensor [n, ld] of FMT_DTYPE[fmt]; columns from K up to the padded width are zero.  The 16-bit formats are one round-to-nearest-even
    cast; the split formats are ops.split16_pack / ops.splitx_pack of scale * rows (the patch rows use FP_SPLIT_SCALE_ACT).  Nothing is
    clamped here (a normalised pixel is below 2.65 in magnitude)."""
    rows = torch.as_tensor(np.asarray(rows, dtype=np.float32))
    n, K = rows.shape
    split = fmt in ("f16x3", "f16f8")
    cols = ld // 2 if split else ld
    assert cols >= K and (not split or ld % (128 if fmt == "f16f8" else 64) == 0)
    padded = torch.zeros(n, cols, dtype=torch.float32)
    padded[:, :K] = rows
    if fmt == "f16x3":
        return ops.split16_pack(padded, scale)
    if fmt == "f16f8":
        return ops.splitx_pack(padded, scale)
    return padded.to(FMT_DTYPE[fmt])


def unpack(fmt, stored, scale=_lib.SPLIT_SCALE_ACT):
    """The fp64 values a stored row stands for in the products it enters (the inverse of pack up to its rounding)."""
    if fmt == "f16x3":
        return ops.split16_unpack(stored, scale).double()
    if fmt == "f16f8":
        return ops.splitx_unpack(stored, scale).double()
    return stored.double()


def same_bits(a, b):
    """Bit-for-bit equality of two tensors of the same dtype and shape (NaN-safe, -0 != +0)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def tokens_ref(a, w, bias, pos, cls_token, registers, batch):
    """fp64 token sequence [batch, 1 + R + Np, D].  a [batch * Np, K] patch-row operands, w [D, K], bias [D], pos [1 + Np, D], cls_token [D],
    registers [R, D] or None.  Per image: row 0 = cls + pos[0]; rows 1..R the register tokens (no position); then a w^T + bias + pos[1 + p]."""
    a, w = torch.as_tensor(a).double(), torch.as_tensor(w).double()
    bias, pos = torch.as_tensor(bias).double().reshape(-1), torch.as_tensor(pos).double()
    D, n_p = w.shape[0], a.shape[0] // batch
    assert a.shape[0] == batch * n_p and pos.shape == (1 + n_p, D)
    patch = (a @ w.T + bias).reshape(batch, n_p, D) + pos[1:][None]
    head = [(torch.as_tensor(cls_token).double().reshape(1, D) + pos[:1]).expand(batch, 1, D)]
    if registers is not None and registers.numel():
        head.append(torch.as_tensor(registers).double().reshape(1, -1, D).expand(batch, -1, D))
    return torch.cat(head + [patch], dim=1)


def token_bound(fmt, a, w, bias, pos_patch, k_pad, batch, s_a=_lib.SPLIT_SCALE_ACT, s_w=1.0):
    """What |kernel - tokens_ref| of a patch-token element may be, [batch * Np, D] fp64, derived and not tuned:

      k_pad 2^-24 sum_k |a_k w_k|          fp32 accumulation of k_pad products, in any order
    + 2^-23 (|acc| + |bias| + |pos|)       the two fp32 additions of the epilogue (an fma with the power-of-two operand scale rounds once)
    + the per-product term of the split formats, where a and w are the fp32 values BEFORE packing: a stored operand stands for
      a (1 + d) + e with |d| <= r, |e| <= t / scale (REPR: what the packers are held to), so a product is off by at most
      |a w| (2 r + r^2) + (|a| e_w + |w| e_a)(1 + r) + e_a e_w.  The dropped lo * lo term of the three-MFMA product (2^-22 |a w|) and the
      e4m3 copies of the hi halves in the f16f8 cross terms (2 x 2^-4 x 2^-11 |a w|) sit inside 2 r |a w| for both formats.
    For f32 / bf16 / f16 the operands are the stored values, taken exactly: no per-product term."""
    a, w = torch.as_tensor(a).double(), torch.as_tensor(w).double()
    bias = torch.as_tensor(bias).double().reshape(1, -1)
    n_p = a.shape[0] // batch
    pos = torch.as_tensor(pos_patch).double().repeat(batch, 1)
    assert pos.shape[0] == batch * n_p
    mag = a.abs() @ w.abs().T
    acc = a @ w.T
    bound = k_pad * U24 * mag + U23 * (acc.abs() + bias.abs() + pos.abs())
    if fmt in REPR:
        r, t = REPR[fmt]
        e_a, e_w = t / s_a, t / s_w
        sum_a = a.abs().sum(1, keepdim=True)            # sum_k |a_k| over the live columns; padding columns are exact zeros on both sides
        sum_w = w.abs().sum(1, keepdim=True).T
        bound = bound + mag * (2 * r + r * r) + (sum_a * e_w + sum_w * e_a) * (1 + r) + a.shape[1] * e_a * e_w
    return bound


def rne16(x, fmt):
    return x.to(FMT_DTYPE[fmt])


def rowstats_ref(x, fmt):
    """x fp32 [rows, D] -> (xb, xl, s1, s2): xb = RNE16(x), xl = RNE16(x - float(xb)) (the difference is exact in fp32), and the row sums
    (sum x, sum x^2) in fp64.  fmt: "bf16" or "f16"."""
    x = torch.as_tensor(x, dtype=torch.float32)
    xb = rne16(x, fmt)
    xl = rne16(x - xb.float(), fmt)
    xd = x.double()
    return xb, xl, xd.sum(1), (xd * xd).sum(1)
