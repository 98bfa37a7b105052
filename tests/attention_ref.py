"""Operands, fp64 reference and derived error bound for the attention edge tests (tests/test_attention_ref_cpu.py, tests/test_gpu_attention_edges.py).

Plain torch on whatever device the tensors live on; nothing here touches the native library.

Operand builders return fp32 [B, N, 3, heads, 64] (q | k | v of every token, head-major like a row of the qkv buffer); the caller rounds them to the
kernel's operand format and hands the ROUNDED values to `reference`, so the reference and the kernel see the same numbers.

  random    randn x 1.5, what the older attention tests use.
  planted   query q of every (image, head) is 3 x key t(q) = (N - 1 - q) mod N: every key -- key N - 1, key 0, both sides of every 64-key tile boundary --
            is the dominant key of exactly one query (score 3 |k|^2 / 8 ~ 54 against a spread of ~7 for the others).  V[j] = (1 + j // 64) e_{j mod 64}:
            an output row names the key that produced it (column = j mod 64, value = 1 + tile).  A mask that drops key N - 1, a tail query block that
            reads another head's rows or a P.V step that pairs P with the wrong V rows all show as a wrong column or a wrong value of order 1.
  offset    random with q[..., 0] = -16 and k[..., 0] = +16: every real score is about -32.  A padded all-zero key that slipped through the mask would score 0
            and take the whole softmax (e^32 against the real keys).

Bound (16-bit kernels), per output element, with S = P |V| the element's scale:
  * P and the output are each rounded to nearest even (v_cvt_pk_*): two half-ulps, 2^-7 S for bf16 (8 significant bits), 2^-10 S for fp16 (11).
  * fp16 only: a probability below the subnormal step 2^-24 loses up to 2^-25 absolutely; the kernel normalises by l >= 1 (the reference of the exponent is
    never above the row maximum), so this adds at most 2^-25 sum_j |V_j[d]|.
  * both: 2^-20 max_d S[q, :] for the fp32 summation order and the hardware exp2 / rcp.
"""

import torch

HEAD_DIM = 64

# token counts of the edge tests and what each reaches (tests/test_gpu_attention_edges.py)
TOKENS = (1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 161, 300, 319, 384, 385)
# (images, heads): 1, 6, 8 and 8 (image, head) pairs -- both block mappings of the kernels
PAIRS = ((1, 1), (3, 2), (2, 4), (1, 8))
BUILDERS = ("random", "planted", "offset")


def planted_key(N, device=None):
    """t(q) = (N - 1 - q) mod N for q = 0 .. N - 1."""
    return (N - 1 - torch.arange(N, device=device)) % N


def build(kind, B, N, heads, seed=0):
    """-> fp32 [B, N, 3, heads, 64] on the CPU (seeded)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * N + 31 * B + heads)
    x = torch.randn(B, N, 3, heads, HEAD_DIM, generator=g) * 1.5
    if kind == "random":
        return x
    if kind == "planted":
        x[:, :, 0] = 3.0 * x[:, planted_key(N), 1]
        j = torch.arange(N)
        v = torch.zeros(N, HEAD_DIM)
        v[j, j % 64] = (1 + j // 64).float()
        x[:, :, 2] = v[None, :, None, :]
        return x
    if kind == "offset":
        x[:, :, 0, :, 0] = -16.0
        x[:, :, 1, :, 0] = 16.0
        return x
    raise ValueError(kind)


def round_to(x, fmt):
    """fp32 -> the values a 16-bit kernel sees, as fp32."""
    return x.to({"bf16": torch.bfloat16, "f16": torch.float16}[fmt]).float()


def reference(qkv):
    """qkv [B, N, 3, heads, 64] (already rounded to the operand format; any float dtype) -> (out, S), fp64 [B, N, heads, 64] each:
    out = softmax(q k^T / 8) v and S = softmax(q k^T / 8) |v|."""
    q, k, v = qkv.double().permute(2, 0, 3, 1, 4)   # [B, heads, N, 64] each
    p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
    return (p @ v).permute(0, 2, 1, 3).contiguous(), (p @ v.abs()).permute(0, 2, 1, 3).contiguous()


def bound(S, V, fmt):
    """Per-element bar of a 16-bit kernel (module docstring).  S [B, N, heads, 64] from `reference`, V [B, N, heads, 64] the rounded values."""
    S, V = S.double(), V.double()
    rowmax = S.amax(dim=-1, keepdim=True)
    if fmt == "bf16":
        return 2.0 ** -7 * S + 2.0 ** -20 * rowmax
    if fmt == "f16":
        return 2.0 ** -10 * S + 2.0 ** -25 * V.abs().sum(dim=1, keepdim=True) + 2.0 ** -20 * rowmax
    raise ValueError(fmt)


def row_error(out, ref, S):
    """Worst row of max_d |out - ref| / max_d S[q, :] (the measure of the fp32 and split-fp16 kernels)."""
    err = (out.double() - ref).abs().amax(dim=-1)
    return float((err / S.amax(dim=-1)).max())


def emulate(qkv, fmt):
    """The 16-bit kernels' arithmetic in torch: fp32 scores, fp32 p = exp2((s - max) c), l from the unrounded p, P rounded to the format, fp32 P V, the
    normalised output rounded to the format.  qkv: rounded operands, fp32 [B, N, 3, heads, 64] -> fp32 [B, N, heads, 64]."""
    q, k, v = qkv.float().permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2)
    c = 0.125 * 1.44269504088896340736
    p = torch.exp2((s - s.amax(dim=-1, keepdim=True)) * c)
    l = p.sum(dim=-1, keepdim=True)
    o = (round_to(p, fmt) @ v) / l
    return round_to(o, fmt).permute(0, 2, 1, 3).contiguous()
