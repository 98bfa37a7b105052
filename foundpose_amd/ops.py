"""Tensor-level wrappers over the C ABI: allocate outputs/scratch with torch, pass raw pointers.

torch is plumbing here (device memory + the current HIP stream); every computation is a
hand-written gfx950 kernel behind include/foundpose_amd.h.
"""

from typing import Dict, Optional, Tuple

import torch

from . import _lib
from ._lib import call, knn_scratch_bytes, ptr, stream, require_cuda
from .group_tables import MAX_REC, MAX_THS


def _f32c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def sqnorm_rows(x: torch.Tensor) -> torch.Tensor:
    require_cuda(x)
    x = _f32c(x)
    out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    call("fp_sqnorm_rows", ptr(x), x.shape[0], x.shape[1], ptr(out), stream())
    return out


def normalize_rows(x: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    require_cuda(x)
    x = _f32c(x)
    out = torch.empty_like(x)
    call("fp_normalize_rows", ptr(x), x.shape[0], x.shape[1], eps, ptr(out), stream())
    return out


_KNN_SCRATCH_BYTES = 1 << 29  # rows are processed in chunks so the [m, n] distance scratch stays <= 512 MiB


def knn_l2(q: torch.Tensor, db: torch.Tensor, k: int, q_sqnorm: Optional[torch.Tensor] = None,
           db_sqnorm: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (squared distances [m,k] f32, indices [m,k] int32), ascending, ties -> lowest index."""
    require_cuda(q, db)
    q, db = _f32c(q), _f32c(db)
    m, d = q.shape
    n = db.shape[0]
    if db.shape[1] != d:
        raise ValueError(f"dimension mismatch: queries {d} vs database {db.shape[1]}")
    if n == 0:
        raise ValueError("empty database")
    k_eff = min(k, n)
    qn = sqnorm_rows(q) if q_sqnorm is None else q_sqnorm
    dn = sqnorm_rows(db) if db_sqnorm is None else db_sqnorm
    d2 = torch.empty(m, k_eff, dtype=torch.float32, device=q.device)
    idx = torch.empty(m, k_eff, dtype=torch.int32, device=q.device)
    if m > 0:
        per_row = knn_scratch_bytes(1, n, k_eff)
        chunk = max(1, min(m, _KNN_SCRATCH_BYTES // per_row))
        scratch = torch.empty(chunk * per_row, dtype=torch.uint8, device=q.device)
        for r0 in range(0, m, chunk):
            r1 = min(m, r0 + chunk)
            call("fp_knn_l2", ptr(q[r0:r1]), ptr(qn[r0:r1]), r1 - r0, ptr(db), ptr(dn), n, d, k_eff,
                 ptr(scratch), ptr(d2[r0:r1]), ptr(idx[r0:r1]), stream())
    if k_eff < k:  # faiss pads missing neighbours with (inf, -1)
        pad_d = torch.full((m, k - k_eff), float("inf"), dtype=torch.float32, device=q.device)
        pad_i = torch.full((m, k - k_eff), -1, dtype=torch.int32, device=q.device)
        d2, idx = torch.cat([d2, pad_d], 1), torch.cat([idx, pad_i], 1)
    return d2, idx


def tfidf_build(word_ids: torch.Tensor, word_d2: torch.Tensor, seg_off: torch.Tensor, idf: torch.Tensor,
                soft_assign: bool, soft_sigma_squared: float, sqrt_dists: bool, eps: float = 1e-8, out=None):
    """-> (desc [S, W], desc_n [S, W]) for S = len(seg_off) - 1 point sets (written into `out` = (desc, desc_n) if given:
    contiguous row slices of larger buffers)."""
    require_cuda(word_ids, word_d2, seg_off, idf)
    num_segs = seg_off.shape[0] - 1
    W = idf.shape[0]
    if out is not None:
        desc, desc_n = out
        if desc.shape != (num_segs, W) or desc_n.shape != (num_segs, W) or not desc.is_contiguous() or not desc_n.is_contiguous():
            raise ValueError("tfidf_build: `out` must be two contiguous [num_segs, num_words] fp32 tensors")
    else:
        desc = torch.empty(num_segs, W, dtype=torch.float32, device=idf.device)
        desc_n = torch.empty_like(desc)
    call("fp_tfidf_build", ptr(word_ids), ptr(word_d2), word_ids.shape[1], ptr(seg_off), num_segs, ptr(idf), W,
         int(soft_assign), float(soft_sigma_squared), int(sqrt_dists), ptr(desc), ptr(desc_n), eps, stream())
    return desc, desc_n


def sample_bilinear(fmap_bchw: torch.Tensor, points: torch.Tensor, point_img: Optional[torch.Tensor],
                    image_size: Tuple[int, int]) -> torch.Tensor:
    """fmap_bchw: [B,C,H,W] fp32 with arbitrary strides (no copy); points [P,2] in image coords."""
    require_cuda(fmap_bchw, points)
    if fmap_bchw.dtype != torch.float32:
        fmap_bchw = fmap_bchw.float()
    points = _f32c(points)
    B, Cc, H, W = fmap_bchw.shape
    sb, sc, sh, sw = fmap_bchw.stride()
    out = torch.empty(points.shape[0], Cc, dtype=torch.float32, device=points.device)
    call("fp_sample_bilinear", ptr(fmap_bchw), sb, sc, sh, sw, Cc, H, W, int(image_size[0]), int(image_size[1]),
         ptr(points), ptr(point_img), points.shape[0], ptr(out), stream())
    return out


def pca_project(x: torch.Tensor, components: torch.Tensor, mean_proj: Optional[torch.Tensor]) -> torch.Tensor:
    require_cuda(x, components)
    x, components = _f32c(x), _f32c(components)
    out = torch.empty(x.shape[0], components.shape[0], dtype=torch.float32, device=x.device)
    call("fp_pca_project", ptr(x), x.shape[0], x.shape[1], ptr(components), components.shape[0], ptr(mean_proj),
         ptr(out), stream())
    return out


def gemm_f32(a: torch.Tensor, w: torch.Tensor, bias=None, gamma=None, out=None, epilogue: int = 0) -> torch.Tensor:
    require_cuda(a, w)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    call("fp_gemm_f32", ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, ptr(bias), ptr(gamma), ptr(out),
         out.stride(0), epilogue, stream())
    return out


def _h16_bit(a: torch.Tensor, w: torch.Tensor) -> int:
    """FP_GEMM_F16 when the operands are IEEE fp16 (the "f16" mode's kernels), 0 for bf16; both operands must agree."""
    if a.dtype != w.dtype or a.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("the 16-bit GEMMs take two bf16 or two fp16 operands")
    return _lib.GEMM_F16 if a.dtype == torch.float16 else 0


def gemm_bf16(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, gamma=None, out=None, epilogue: int = 0,
              m_valid: Optional[int] = None, tile: int = 0) -> torch.Tensor:
    """bf16 operands, or fp16 ones (the "f16" mode: same kernels on v_mfma_f32_32x32x16_f16; 16-bit outputs are then fp16)."""
    require_cuda(a, w, bias)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        dt = torch.float32 if (epilogue & 0xff) in (3, 5) else a.dtype
        out = torch.zeros(M, N // 2 if (epilogue & 0xff) == 6 else N, dtype=dt, device=a.device)
    call("fp_gemm_bf16", ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, M if m_valid is None else m_valid,
         ptr(bias), ptr(gamma), ptr(out), out.stride(0), epilogue | (tile << 8) | _h16_bit(a, w), stream())
    return out


def gemm_bf16_resid_ln(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, x: torch.Tensor, emit: bool = True, tile: int = 0, m_valid: Optional[int] = None):
    """Producer of the folded-LayerNorm chain (epilogue 7): x (fp32, in place) += a @ w.T + bias; with emit also
    -> (xb = bf16(x) [M, N], stats [N / 128, M, 2] partial (sum, sum of squares) per 128-column group)."""
    require_cuda(a, w, bias, x)
    M, K = a.shape
    N = w.shape[0]
    xb = torch.zeros(M, N, dtype=a.dtype, device=a.device) if emit else None
    stats = torch.zeros(N // 128, M, 2, dtype=torch.float32, device=a.device) if emit else None
    call("fp_gemm_bf16_ln", ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, M if m_valid is None else m_valid, ptr(bias), ptr(x), x.stride(0),
         7 | (tile << 8) | _h16_bit(a, w), None, None, ptr(xb), N, ptr(stats), stream())
    return xb, stats


def gemm_bf16_resid_hilo(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, xb: torch.Tensor, xl: torch.Tensor, tile: int = 0, m_valid: Optional[int] = None):
    """Producer of the folded-LayerNorm chain on the (hi, lo) residual stream (epilogue 8): x = xb + xl (bf16 [M, N] each, updated in place) += a @ w.T + bias,
    xb = bf16(x), xl = bf16(x - xb).  -> stats [N / 128, M, 2]."""
    require_cuda(a, w, bias, xb, xl)
    M, K = a.shape
    N = w.shape[0]
    if xb.dtype != a.dtype or xl.dtype != a.dtype or xb.stride(0) != xl.stride(0):
        raise ValueError("xb / xl are arrays of the operands' 16-bit type with one row stride")
    if xb.stride(0) % 8 or xb.data_ptr() % 16 or xl.data_ptr() % 16 or xb.stride(1) != 1 or xl.stride(1) != 1:
        raise ValueError("xb / xl: 16-byte aligned rows (row stride a multiple of 8 elements, unit column stride) -- the epilogue moves 8 bf16 per access")
    stats = torch.zeros(N // 128, M, 2, dtype=torch.float32, device=a.device)
    call("fp_gemm_bf16_ln", ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, M if m_valid is None else m_valid, ptr(bias), ptr(xl), xl.stride(0),
         8 | (tile << 8) | _h16_bit(a, w), None, None, ptr(xb), xb.stride(0), ptr(stats), stream())
    return stats


def ln_finalize(stats: torch.Tensor, dim: int, eps: float = 1e-6) -> torch.Tensor:
    """stats [parts, M, 2] -> ln_row [M, 2] = (rstd, mean * rstd)."""
    require_cuda(stats)
    parts, M = stats.shape[0], stats.shape[1]
    out = torch.empty(M, 2, dtype=torch.float32, device=stats.device)
    call("fp_ln_finalize", ptr(stats), parts, M, M, dim, eps, ptr(out), stream())
    return out


def gemm_bf16_ln(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, colsum: torch.Tensor, ln_row: torch.Tensor, epilogue: int = 0, out=None,
                 tile: int = 0, m_valid: Optional[int] = None) -> torch.Tensor:
    """Consumer of the folded-LayerNorm chain: out(bf16) = epi(rstd * (a @ w.T) - mean * rstd * colsum + bias), epilogue 0 / 1 (GELU) / 6 (SwiGLU)."""
    require_cuda(a, w, bias, colsum, ln_row)
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        out = torch.zeros(M, N // 2 if epilogue == 6 else N, dtype=a.dtype, device=a.device)
    call("fp_gemm_bf16_ln", ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, M if m_valid is None else m_valid, ptr(bias), ptr(out), out.stride(0),
         epilogue | (tile << 8) | _h16_bit(a, w), ptr(colsum), ptr(ln_row), None, 0, None, stream())
    return out


def quantize_fp8(x: torch.Tensor, scale: float) -> torch.Tensor:
    """e4m3(clamp(x * scale, +-448)) -> torch.float8_e4m3fn tensor of x's shape (x fp32 or bf16, contiguous)."""
    require_cuda(x)
    if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous():
        raise ValueError("quantize_fp8 takes a contiguous fp32 or bf16 tensor")
    out = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
    call("fp_quantize_fp8", ptr(x), _lib.FP_BF16 if x.dtype == torch.bfloat16 else _lib.FP_F32, x.numel(), float(scale), ptr(out), stream())
    return out


def gemm_fp8(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, col_scale: torch.Tensor, out=None, epilogue: int = 0,
             m_valid: Optional[int] = None, out_scale: float = 0.0) -> torch.Tensor:
    """fp8 x fp8 -> fp32-accumulated GEMM: out = epilogue((a @ w.T + bias) * col_scale), a [M, K] and w [N, K] in
    torch.float8_e4m3fn; bias is the true bias divided by col_scale (see include/foundpose_amd.h)."""
    require_cuda(a, w, bias, col_scale)
    if a.dtype != torch.float8_e4m3fn or w.dtype != torch.float8_e4m3fn:
        raise ValueError("gemm_fp8 operands must be torch.float8_e4m3fn")
    M, K = a.shape
    N = w.shape[0]
    if out is None:
        epi = epilogue & 0xff   # (bits 8+: the block-tile override of benchmarks and tests)
        odt = torch.float8_e4m3fn if out_scale > 0 else (torch.float32 if epi == 3 else torch.bfloat16)
        out = torch.zeros(M, N // 2 if epi == 6 else N, dtype=odt, device=a.device)  # out_scale > 0: e4m3(result * out_scale)
    call("fp_gemm_fp8", ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, M if m_valid is None else m_valid,
         ptr(bias), ptr(col_scale), ptr(out), out.stride(0), epilogue, float(out_scale), stream())
    return out


def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, out_dtype: torch.dtype, eps: float = 1e-6):
    require_cuda(x, weight, bias)
    rows, D = x.shape
    out = torch.empty(rows, D, dtype=out_dtype, device=x.device)
    call("fp_layernorm", ptr(x), x.stride(0), ptr(weight), ptr(bias), eps, ptr(out), D,
         {torch.bfloat16: _lib.FP_BF16, torch.float16: _lib.FP_F16, torch.float32: _lib.FP_F32}[out_dtype], D, rows, rows, rows, 0, stream())
    return out


def attention(qkv: torch.Tensor, batch: int, n_tok: int, dim: int, heads: int, variant: int = 0):
    """variant: bf16 work split (FP_ATTN_VARIANT in the header; all bit-identical) -- 0 is what the pipeline runs."""
    require_cuda(qkv)
    dt = {torch.bfloat16: _lib.FP_BF16, torch.float16: _lib.FP_F16, torch.float32: _lib.FP_F32}[qkv.dtype]   # fp16: the "f16" mode's kernel (variant 0 only)
    out = torch.zeros(qkv.shape[0], dim, dtype=qkv.dtype, device=qkv.device)
    call("fp_attention", ptr(qkv), qkv.stride(0), ptr(out), dim,
         batch, n_tok, dim, heads, dt | (int(variant) << 8), stream())
    return out


# ---------------------------------------------------------------- split-fp16 rows (the f16x3 near-exact mode, include/foundpose_amd.h)
def pow2_scale(t: torch.Tensor, target: float = 16384.0) -> float:
    """Largest power of two s with max|t| * s <= target (16384 leaves a factor 4 of head room below the fp16 maximum)."""
    import math
    amax = float(t.abs().max())
    if not math.isfinite(amax) or amax <= 0.0:
        return 1.0
    return float(2.0 ** math.floor(math.log2(target / amax)))


def split16_pack(x: torch.Tensor, scale: float = 1.0, pad: int = 0) -> torch.Tensor:
    """fp32 [rows, K] (K % 32 == 0) -> fp16 [rows, 2K] split rows (groups of 32: [hi 32 | lo 32]) of scale * x; `pad` extra halves of row
    stride (the returned tensor is then a view of a wider buffer).  Host-side preparation of weights and test operands; inside the
    pipeline the producing kernels write this layout themselves."""
    rows, K = x.shape
    if K % 32:
        raise ValueError("split16_pack: the row length must be a multiple of 32")
    xs = (x.float() * scale).clamp(-65504.0, 65504.0)
    hi = xs.half()
    lo = (xs - hi.float()).half()
    out = torch.stack([hi.reshape(rows, K // 32, 32), lo.reshape(rows, K // 32, 32)], 2).reshape(rows, 2 * K)
    if pad == 0:
        return out.contiguous()
    buf = torch.zeros(rows, 2 * K + pad, dtype=torch.float16, device=x.device)
    buf[:, :2 * K] = out
    return buf[:, :2 * K]


def splitx_pack(x: torch.Tensor, scale: float = 1.0, pad: int = 0) -> torch.Tensor:
    """fp32 [rows, K] (K % 64 == 0) -> fp16-typed [rows, 2K] f16f8 rows of scale * x (include/foundpose_amd.h "f16f8 rows"): per 64 columns the
    fp16 high halves (128 B), e4m3(hi 2^-7) (64 B) and e4m3((s x - hi) 2^4) (64 B).  Host-side preparation of weights and test operands, the
    same arithmetic as the device's splitx_pack2 (common.hpp)."""
    rows, K = x.shape
    if K % 64:
        raise ValueError("splitx_pack: the row length must be a multiple of 64")
    xs = (x.float() * scale).clamp(-65504.0, 65504.0)
    hi = xs.half()
    hi8 = (hi.float() * 2.0 ** -7).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    lo8 = ((xs - hi.float()) * 2.0 ** 4).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    buf = torch.zeros(rows, 2 * K + pad, dtype=torch.float16, device=x.device)
    by = buf.view(torch.uint8)[:, :4 * K].unflatten(1, (K // 64, 256))
    by[:, :, :128] = hi.contiguous().view(torch.uint8).unflatten(1, (K // 64, 128))
    by[:, :, 128:192] = hi8.unflatten(1, (K // 64, 64))
    by[:, :, 192:256] = lo8.unflatten(1, (K // 64, 64))
    return buf[:, :2 * K] if pad else buf


def splitx_unpack(xs: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """What an f16f8 row represents in the products it enters: fp16 [rows, 2K] -> fp32 [rows, K] = (hi + e4m3-lo 2^-4) / scale (summed in fp64)."""
    rows, K2 = xs.shape
    by = xs.contiguous().view(torch.uint8).unflatten(1, (K2 // 128, 256))
    hi = by[:, :, :128].contiguous().view(torch.float16).double()
    lo = by[:, :, 192:256].contiguous().view(torch.float8_e4m3fn).double() * 2.0 ** -4
    return ((hi + lo) / scale).reshape(rows, K2 // 2).float()


def split16_unpack(xs: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """Inverse of split16_pack (up to its 2^-22 rounding): fp16 [rows, 2K] -> fp32 [rows, K] = (hi + lo) / scale (summed in fp64)."""
    rows, K2 = xs.shape
    g = xs.reshape(rows, K2 // 64, 2, 32).double()
    return ((g[:, :, 0] + g[:, :, 1]) / scale).reshape(rows, K2 // 2).float()


def gemm_split(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, acc_scale: float, gamma=None, out=None, epilogue: int = 0,
               out_scale: float = 1.0, m_valid: Optional[int] = None, tile: int = 0, f16f8: bool = False) -> torch.Tensor:
    """a [M, 2K], w [N, 2K] split rows (fp16); -> epilogue 0 / 1 / 6: split rows [M, 2N] (6: [M, N]) scaled by out_scale; 3 / 5: fp32 [M, N].
    f16f8: a and w (and the output of epilogues 1 / 6) are f16f8 rows (splitx_pack); the output of epilogue 0 stays a split-fp16 row."""
    require_cuda(a, w, bias)
    if a.dtype != torch.float16 or w.dtype != torch.float16:
        raise ValueError("gemm_split operands are fp16 split rows")
    M, K = a.shape[0], a.shape[1] // 2
    N = w.shape[0]
    if out is None:
        if epilogue in (3, 5):
            out = torch.zeros(M, N, dtype=torch.float32, device=a.device)
        else:
            out = torch.zeros(M, N if epilogue == 6 else 2 * N, dtype=torch.float16, device=a.device)
    call("fp_gemm_split", ptr(a), a.stride(0), ptr(w), w.stride(0), M, N, K, M if m_valid is None else m_valid, ptr(bias), ptr(gamma),
         ptr(out), out.stride(0), epilogue | (tile << 8) | (_lib.GEMM_SPLIT_F16F8 if f16f8 else 0), float(acc_scale), float(out_scale), stream())
    return out


def attention_split(qkv: torch.Tensor, batch: int, n_tok: int, dim: int, heads: int, in_scale: float, out_scale: float, f16f8_out: bool = False,
                    variant: int = 0) -> torch.Tensor:
    """qkv [B*N, 6D] split rows (q | k | v) -> [B*N, 2D] split rows (f16f8_out: f16f8 rows).  variant 0 and 1 both run the lock-step kernel
    (2 is refused: FP_ATTN_VARIANT in the header)."""
    require_cuda(qkv)
    out = torch.zeros(qkv.shape[0], 2 * dim, dtype=torch.float16, device=qkv.device)
    call("fp_attention_split", ptr(qkv), qkv.stride(0), ptr(out), 2 * dim, batch, n_tok, dim, heads, float(in_scale), float(out_scale),
         (_lib.FP_F16F8 if f16f8_out else _lib.FP_F16X3) | (int(variant) << 8), stream())
    return out


def layernorm_split(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, out_scale: float, eps: float = 1e-6, f16f8: bool = False) -> torch.Tensor:
    require_cuda(x, weight, bias)
    rows, D = x.shape
    out = torch.empty(rows, 2 * D, dtype=torch.float16, device=x.device)
    call("fp_layernorm_scaled", ptr(x), x.stride(0), ptr(weight), ptr(bias), eps, ptr(out), 2 * D, _lib.FP_F16F8 if f16f8 else _lib.FP_F16X3, float(out_scale), D, rows, stream())
    return out


def pose_errors(pts: torch.Tensor, est: torch.Tensor, p_est: torch.Tensor, gt_sym: torch.Tensor, p_gt: torch.Tensor,
                ranges) -> Tuple[torch.Tensor, torch.Tensor]:
    """Symmetry-aware MSSD / MSPD of a ragged batch (fp_pose_errors): pts [V, 3], est / p_est [H, 12], gt_sym / p_gt [S, 12]
    (fp64, on the device); ranges [H, 4] int (host) = (pt_off, pt_cnt, sym_off, sym_cnt) per hypothesis.
    -> (err [H, 2] fp64 = (mssd, mspd), idx [H, 4] int32 = (mssd vertex, mssd symmetry, mspd vertex, mspd symmetry))."""
    import numpy as np
    require_cuda(pts, est, p_est, gt_sym, p_gt)
    if isinstance(ranges, torch.Tensor):
        if ranges.is_cuda:
            raise ValueError("pose_errors: ranges is a host table (it is validated and sized on the host)")
        ranges = ranges.numpy()
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 4))
    if np.any(np.abs(r) > 2**31 - 1):
        raise ValueError("pose_errors: range entries must fit int32")
    r = r.astype(np.int32)
    pts, est, p_est, gt_sym, p_gt = (t.to(torch.float64).contiguous() for t in (pts, est, p_est, gt_sym, p_gt))
    h = r.shape[0]
    if est.shape != (h, 12) or p_est.shape != (h, 12) or pts.dim() != 2 or pts.shape[1] != 3 or gt_sym.dim() != 2 or gt_sym.shape[1] != 12 \
            or p_gt.shape != gt_sym.shape:
        raise ValueError("pose_errors: shapes must be pts [V, 3], est / p_est [H, 12], gt_sym / p_gt [S, 12], ranges [H, 4]")
    err = torch.empty(h, 2, dtype=torch.float64, device=pts.device)
    idx = torch.empty(h, 4, dtype=torch.int32, device=pts.device)
    nbytes = _lib.pose_err_scratch_bytes(h, int(r[:, 1].max()) if h else 0, int(r[:, 3].max()) if h else 0)
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=pts.device)
    call("fp_pose_errors", ptr(pts), pts.shape[0], ptr(est), ptr(p_est), ptr(gt_sym), ptr(p_gt), gt_sym.shape[0],
         r.ctypes.data_as(_lib.vp), h, ptr(scratch), nbytes, ptr(err), ptr(idx), stream())
    return err, idx


def pose_add_errors(pts: torch.Tensor, est: torch.Tensor, gt: torch.Tensor, ranges) -> torch.Tensor:
    """ADD / ADI of a ragged batch of (estimate, GT) pairs (fp_pose_add_errors): pts [V, 3], est / gt [H, 12] = R row-major | t (fp64, on the
    device); ranges [H, 2] int (host) = (pt_off, pt_cnt) per pair.  -> err [H, 2] fp64 = (add, adi).  The table is checked here, before any
    launch: ValueError, nothing written."""
    import numpy as np
    for name, t in (("pts", pts), ("est", est), ("gt", gt)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"pose_add_errors: {name} is a device tensor; there is no CPU path")
    if isinstance(ranges, torch.Tensor):
        if ranges.is_cuda:
            raise ValueError("pose_add_errors: ranges is a host table (it is validated and sized on the host)")
        ranges = ranges.numpy()
    r = np.asarray(ranges)
    if r.ndim != 2 or r.shape[1] != 2 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"pose_add_errors: ranges must be an integer [H, 2] table, got {r.dtype} {r.shape}")
    r = np.ascontiguousarray(r.astype(np.int64))
    h = r.shape[0]
    if h < 1 or h > 65535:
        raise ValueError(f"pose_add_errors: {h} pairs, 1 .. 65535 per call")
    if np.any(np.abs(r) > 2**31 - 1) or pts.shape[0] > 2**31 - 1:
        raise ValueError("pose_add_errors: range entries must fit int32")
    if pts.dim() != 2 or pts.shape[1] != 3 or est.shape != (h, 12) or gt.shape != (h, 12):
        raise ValueError("pose_add_errors: shapes must be pts [V, 3], est / gt [H, 12], ranges [H, 2]")
    if int(r[:, 1].min()) < 1:
        raise ValueError(f"pose_add_errors: pair {int(np.argmin(r[:, 1]))} has an empty point range")
    bad = np.nonzero((r[:, 0] < 0) | (r[:, 0] + r[:, 1] > pts.shape[0]))[0]
    if bad.size:
        raise ValueError(f"pose_add_errors: pair {int(bad[0])}: points [{int(r[bad[0], 0])}, +{int(r[bad[0], 1])}) outside [0, {pts.shape[0]})")
    r = r.astype(np.int32)
    pts, est, gt = (t.to(torch.float64).contiguous() for t in (pts, est, gt))
    err = torch.empty(h, 2, dtype=torch.float64, device=pts.device)
    nbytes = _lib.pose_add_scratch_bytes(h, int(r[:, 1].max()))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
    call("fp_pose_add_errors", ptr(pts), pts.shape[0], ptr(est), ptr(gt), r.ctypes.data_as(_lib.vp), h, ptr(scratch), nbytes, ptr(err), stream())
    return err


def _pts_f64(fn: str, name: str, t, cols: int) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{fn}: {name} is a device tensor; there is no CPU path")
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"{fn}: {name} must be float64 [N, {cols}], got {t.dtype} {tuple(t.shape)}")


def pts_diameter(pts: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The largest distance between two points of pts [V, 3] (fp64, on the device; fp_pts_diameter) -> (d [1] fp64, pair [2] int32 = the
    lexicographically lowest (i, j), i < j, that attains it; V = 1: 0.0 and (0, 0)).  Checked here, before any launch: ValueError."""
    _pts_f64("pts_diameter", "pts", pts, 3)
    v = pts.shape[0]
    if v < 1 or v > _lib.PTS_DIAMETER_MAX_V:
        raise ValueError(f"pts_diameter: {v} points, 1 .. {_lib.PTS_DIAMETER_MAX_V} per call")
    pts = pts.contiguous()
    d = torch.empty(1, dtype=torch.float64, device=pts.device)
    pair = torch.empty(2, dtype=torch.int32, device=pts.device)
    nbytes = _lib.pts_diameter_scratch_bytes(v)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
    call("fp_pts_diameter", ptr(pts), v, ptr(scratch), nbytes, ptr(d), ptr(pair), stream())
    return d, pair


def directed_hausdorff(pts: torch.Tensor, transforms: torch.Tensor, query_stride: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per transform k of transforms [K, 12] = R row-major | t, the directed Hausdorff distance from the transformed points
    v = 0, s, 2 s, ... (s = query_stride) of pts [V, 3] to ALL untransformed points (fp64, on the device; fp_directed_hausdorff)
    -> (h [K] fp64, arg [K] int32 = the lowest v that attains it).  Checked here, before any launch: ValueError."""
    _pts_f64("directed_hausdorff", "pts", pts, 3)
    _pts_f64("directed_hausdorff", "transforms", transforms, 12)
    if isinstance(query_stride, bool) or not hasattr(query_stride, "__index__"):
        raise ValueError(f"directed_hausdorff: query_stride must be an integer, got {query_stride!r}")
    v, k, s = pts.shape[0], transforms.shape[0], int(query_stride)
    if v < 1 or v > 2**31 - 1:
        raise ValueError(f"directed_hausdorff: {v} points, 1 .. 2^31 - 1 per call")
    if k < 1 or k > 65535:
        raise ValueError(f"directed_hausdorff: {k} transforms, 1 .. 65535 per call")
    if s < 1 or s > 2**31 - 1:
        raise ValueError(f"directed_hausdorff: query_stride {s} outside [1, 2^31 - 1]")
    pts, transforms = pts.contiguous(), transforms.contiguous()
    h = torch.empty(k, dtype=torch.float64, device=pts.device)
    arg = torch.empty(k, dtype=torch.int32, device=pts.device)
    nbytes = _lib.pts_hausdorff_scratch_bytes(v, s, k)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
    call("fp_directed_hausdorff", ptr(pts), v, s, ptr(transforms), k, ptr(scratch), nbytes, ptr(h), ptr(arg), stream())
    return h, arg


def vsd_counts(depth_test: torch.Tensor, depth_est: torch.Tensor, depth_gt: torch.Tensor, pairs, params, taus) -> torch.Tensor:
    """VSD counts of a batch of (estimate, GT) pairs (fp_vsd_counts): depth_test [N_test, H, W], depth_est [N_est, H, W],
    depth_gt [N_gt, H, W] fp32 mm (on the device); pairs [P, 7] int (host) = (test, est, gt, x0, y0, x1, y1) with the inclusive
    box of the two renders (x1 = x0 - 1: empty); params [P, 6] (host) = (fx, fy, cx, cy, delta, diameter); taus [T] (host).
    -> counts [P, 2 + T] int64 = (|union|, |intersection|, intersection pixels with dist >= tau for each tau)."""
    import numpy as np
    require_cuda(depth_test, depth_est, depth_gt)
    host = []
    for name, a in (("pairs", pairs), ("params", params), ("taus", taus)):
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                raise ValueError(f"vsd_counts: {name} is a host table (it is validated on the host)")
            a = a.numpy()
        host.append(a)
    p = np.asarray(host[0], dtype=np.int64).reshape(-1, 7)
    if np.any(np.abs(p) > 2**31 - 1):
        raise ValueError("vsd_counts: pair entries must fit int32")
    p = np.ascontiguousarray(p, np.int32)
    q = np.ascontiguousarray(np.asarray(host[1], dtype=np.float64).reshape(-1, 6))
    t = np.ascontiguousarray(np.asarray(host[2], dtype=np.float64).reshape(-1))
    dt, de, dg = (x.to(torch.float32).contiguous() for x in (depth_test, depth_est, depth_gt))
    if dt.dim() != 3 or de.dim() != 3 or dg.dim() != 3 or not (dt.shape[1:] == de.shape[1:] == dg.shape[1:]) or q.shape[0] != p.shape[0]:
        raise ValueError("vsd_counts: shapes must be depth_test / depth_est / depth_gt [N, H, W] of one H x W, pairs [P, 7], params [P, 6]")
    n = p.shape[0]
    counts = torch.empty(max(n, 1), 2 + len(t), dtype=torch.int64, device=dt.device)[:n]
    scratch = torch.empty(max(_lib.vsd_scratch_bytes(n), 1), dtype=torch.uint8, device=dt.device)
    call("fp_vsd_counts", ptr(dt), dt.shape[0], ptr(de), de.shape[0], ptr(dg), dg.shape[0], dt.shape[1], dt.shape[2],
         p.ctypes.data_as(_lib.vp), q.ctypes.data_as(_lib.vp), n, t.ctypes.data_as(_lib.vp), len(t), ptr(scratch),
         _lib.vsd_scratch_bytes(n), ptr(counts), stream())
    return counts


def gt_visibility(depth_test: torch.Tensor, depth_obj: torch.Tensor, inst, params) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Pixel counts, boxes and masks of a batch of GT instances (fp_gt_visibility): depth_test [N, H, W] and
    depth_obj [P, Hr, Wr] fp32 mm (on the device), instance p rendered alone into a window that holds the image at (ox, oy); inst [P, 7]
    int (host) = (test, x0, y0, x1, y1, ox, oy) with the inclusive scan box in render coordinates (x1 = x0 - 1: empty); params [P, 5]
    (host) = (fx, fy, cx, cy, delta) of the image.  -> (out [P, 11] int32 = px_count_all, px_count_valid, px_count_visib, the silhouette
    box and the visible box as (min x, min y, max x, max y) in image coordinates, INT_MAX / INT_MIN when empty; mask, mask_visib [P, H, W]
    uint8 255 / 0).  A refused call raises ValueError and writes nothing."""
    import numpy as np
    host = []
    for name, a in (("inst", inst), ("params", params)):
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                raise ValueError(f"gt_visibility: {name} is a host table (it is validated on the host)")
            a = a.numpy()
        host.append(a)
    for name, t in (("depth_test", depth_test), ("depth_obj", depth_obj)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"gt_visibility: {name} must be a tensor on the device (there is no CPU path)")
        if t.dim() != 3 or t.dtype != torch.float32:
            raise ValueError(f"gt_visibility: {name} must be float32 [N, H, W]")
    r = np.asarray(host[0], dtype=np.int64).reshape(-1, 7)
    if np.any(np.abs(r) > 2**31 - 1):
        raise ValueError("gt_visibility: inst entries must fit int32")
    r = np.ascontiguousarray(r, np.int32)
    q = np.ascontiguousarray(np.asarray(host[1], dtype=np.float64).reshape(-1, 5))
    n = r.shape[0]
    if q.shape[0] != n or depth_obj.shape[0] != n:
        raise ValueError(f"gt_visibility: {n} instance records, {q.shape[0]} parameter rows, {depth_obj.shape[0]} renders")
    dt, do = depth_test.contiguous(), depth_obj.contiguous()
    (h, w), (hr, wr) = dt.shape[1:], do.shape[1:]
    out = torch.empty(max(n, 1), 11, dtype=torch.int32, device=dt.device)[:n]
    mask = torch.empty(max(n, 1), h, w, dtype=torch.uint8, device=dt.device)[:n]
    mask_visib = torch.empty_like(mask)
    nbytes = _lib.gt_vis_scratch_bytes(n)
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dt.device)
    call("fp_gt_visibility", ptr(dt), dt.shape[0], h, w, ptr(do), hr, wr, r.ctypes.data_as(_lib.vp), q.ctypes.data_as(_lib.vp), n,
         ptr(scratch), nbytes, ptr(out), ptr(mask), ptr(mask_visib), stream(), invalid=ValueError)
    return out, mask, mask_visib


TSDF_PLANES = ("sdf_sum", "sdf_cnt", "rgb_sum", "rgb_cnt")


def _tsdf_box(fn: str, origin, voxel_mm, dims):
    """The checks the three TSDF wrappers share -> (box fp64 [4] on the host, (nx, ny, nz))."""
    import numpy as np
    try:
        box = np.ascontiguousarray(np.concatenate([np.asarray(origin, np.float64).reshape(3), [float(voxel_mm)]]))
        nx, ny, nz = (int(d) for d in dims)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{fn}: origin is three numbers, voxel_mm one, dims three integers ({e})")
    if not np.all(np.isfinite(box)) or not box[3] > 0:
        raise ValueError(f"{fn}: the origin must be finite and the voxel size finite and > 0")
    if min(nx, ny, nz) < 1 or max(nx, ny, nz) > _lib.TSDF_MAX_DIM:
        raise ValueError(f"{fn}: dimensions {nx} x {ny} x {nz} outside [1, {_lib.TSDF_MAX_DIM}]")
    if nx * ny * nz > _lib.TSDF_MAX_VOXELS:
        raise ValueError(f"{fn}: {nx} x {ny} x {nz} = {nx * ny * nz} voxels exceed {_lib.TSDF_MAX_VOXELS}")
    return box, (nx, ny, nz)


def _tsdf_state(fn: str, volume, dims) -> None:
    nx, ny, nz = dims
    for name in TSDF_PLANES:
        t = volume.get(name) if isinstance(volume, dict) else None
        want = (3, nz, ny, nx) if name == "rgb_sum" else (nz, ny, nx)
        dt = torch.float32 if name.endswith("sum") else torch.int32
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{fn}: {name} must be a tensor on the device (there is no CPU path)")
        if t.dtype != dt or tuple(t.shape) != want or not t.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous {dt} {want}, got {t.dtype} {tuple(t.shape)}")


def tsdf_new_volume(origin, voxel_mm: float, dims, device="cuda") -> dict:
    """An empty TSDF volume: a box in the model frame (mm) from `origin`, dims = (nx, ny, nz) voxels of
    voxel_mm, x fastest, voxel centres at origin + (index + 0.5) voxel_mm.  -> dict(origin, voxel_mm, dims, sdf_sum fp32 [nz, ny, nx],
    sdf_cnt int32, rgb_sum fp32 [3, nz, ny, nx], rgb_cnt int32), all zeros."""
    box, (nx, ny, nz) = _tsdf_box("tsdf_new_volume", origin, voxel_mm, dims)
    z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=device)   # noqa: E731
    return {"origin": tuple(float(v) for v in box[:3]), "voxel_mm": float(box[3]), "dims": (nx, ny, nz),
            "sdf_sum": z(nz, ny, nx, dt=torch.float32), "sdf_cnt": z(nz, ny, nx, dt=torch.int32),
            "rgb_sum": z(3, nz, ny, nx, dt=torch.float32), "rgb_cnt": z(nz, ny, nx, dt=torch.int32)}


def tsdf_integrate(volume: dict, depth: torch.Tensor, mask: torch.Tensor, rgb: torch.Tensor, cams, poses, trunc_mm: float) -> None:
    """Adds F frames, in order, to `volume` in place (fp_tsdf_integrate): depth fp32 [F, H, W] mm (0 = no measurement), mask uint8
    [F, H, W], rgb uint8 [F, H, W, 3] on the device; cams [F, 4] = (fx, fy, cx, cy) and poses [F, 12] = model -> camera R row-major | t
    on the host.  Checked here, before any launch: ValueError, nothing written."""
    import numpy as np
    fn = "tsdf_integrate"
    box, dims = _tsdf_box(fn, volume.get("origin") if isinstance(volume, dict) else None, volume.get("voxel_mm") if isinstance(volume, dict) else None,
                          volume.get("dims", ()) if isinstance(volume, dict) else ())
    _tsdf_state(fn, volume, dims)
    for name, t, dt, nd in (("depth", depth, torch.float32, 3), ("mask", mask, torch.uint8, 3), ("rgb", rgb, torch.uint8, 4)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{fn}: {name} must be a tensor on the device (there is no CPU path)")
        if t.dtype != dt or t.dim() != nd:
            raise ValueError(f"{fn}: {name} must be {dt} with {nd} dimensions, got {t.dtype} {tuple(t.shape)}")
    f, h, w = depth.shape
    if tuple(mask.shape) != (f, h, w) or tuple(rgb.shape) != (f, h, w, 3):
        raise ValueError(f"{fn}: depth {tuple(depth.shape)}, mask {tuple(mask.shape)} and rgb {tuple(rgb.shape)} are not one stack of frames")
    if f < 1 or f > _lib.TSDF_MAX_FRAMES or h < 1 or w < 1 or h * w > 2**31 - 1:
        raise ValueError(f"{fn}: {f} frames of {w} x {h}; 1 .. {_lib.TSDF_MAX_FRAMES} frames of at most 2^31 - 1 pixels per call")
    host = []
    for name, a, cols in (("cams", cams, 4), ("poses", poses, 12)):
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                raise ValueError(f"{fn}: {name} is a host table (it is validated on the host)")
            a = a.numpy()
        a = np.asarray(a, np.float64)
        if a.shape != (f, cols) or not np.all(np.isfinite(a)):
            raise ValueError(f"{fn}: {name} must be finite [{f}, {cols}], got {a.shape}")
        host.append(a)
    if not np.all(host[0][:, :2] > 0):
        raise ValueError(f"{fn}: fx and fy must be > 0")
    tau = float(trunc_mm)
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError(f"{fn}: trunc_mm must be finite and > 0, got {trunc_mm!r}")
    frames = np.ascontiguousarray(np.concatenate(host, 1))
    depth, mask, rgb = depth.contiguous(), mask.contiguous(), rgb.contiguous()
    nbytes = _lib.tsdf_scratch_bytes(f)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=depth.device)
    call("fp_tsdf_integrate", ptr(depth), ptr(mask), ptr(rgb), f, h, w, frames.ctypes.data_as(_lib.vp), box.ctypes.data_as(_lib.vp), *dims, tau,
         ptr(scratch), nbytes, ptr(volume["sdf_sum"]), ptr(volume["sdf_cnt"]), ptr(volume["rgb_sum"]), ptr(volume["rgb_cnt"]), stream())


def tsdf_extract(volume: dict, min_count: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Marching tetrahedra over `volume` (fp_tsdf_count_triangles, an exclusive scan by torch.cumsum, fp_tsdf_emit_triangles) -> (counts
    int32 [nz - 1, ny - 1, nx - 1] triangles per cell, keys int64 [3 T], positions fp32 [3 T, 3], colors fp32 [3 T, 3]): per triangle
    corner the grid edge it lies on, unwelded.  Checked here, before any launch: ValueError."""
    fn = "tsdf_extract"
    box, dims = _tsdf_box(fn, volume.get("origin") if isinstance(volume, dict) else None, volume.get("voxel_mm") if isinstance(volume, dict) else None,
                          volume.get("dims", ()) if isinstance(volume, dict) else ())
    _tsdf_state(fn, volume, dims)
    if min(dims) < 2:
        raise ValueError(f"{fn}: dimensions {dims} leave no cell between voxel centres")
    if isinstance(min_count, bool) or not hasattr(min_count, "__index__") or int(min_count) < 1 or int(min_count) > 2**31 - 1:
        raise ValueError(f"{fn}: min_count must be an integer >= 1, got {min_count!r}")
    nx, ny, nz = dims
    dev = volume["sdf_sum"].device
    counts = torch.empty(nz - 1, ny - 1, nx - 1, dtype=torch.int32, device=dev)
    call("fp_tsdf_count_triangles", ptr(volume["sdf_sum"]), ptr(volume["sdf_cnt"]), nx, ny, nz, int(min_count), ptr(counts), stream())
    ends = torch.cumsum(counts.reshape(-1), 0, dtype=torch.int64)
    total = int(ends[-1])
    offsets = (ends - counts.reshape(-1)).contiguous()
    keys = torch.empty(3 * total, dtype=torch.int64, device=dev)
    pos = torch.empty(3 * total, 3, dtype=torch.float32, device=dev)
    col = torch.empty(3 * total, 3, dtype=torch.float32, device=dev)
    call("fp_tsdf_emit_triangles", ptr(volume["sdf_sum"]), ptr(volume["sdf_cnt"]), ptr(volume["rgb_sum"]), ptr(volume["rgb_cnt"]),
         box.ctypes.data_as(_lib.vp), nx, ny, nz, int(min_count), ptr(offsets), total, ptr(keys) if total else None, ptr(pos) if total else None,
         ptr(col) if total else None, stream())
    return counts, keys, pos, col


def tsdf_diffuse(val: torch.Tensor, state: torch.Tensor, iters: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """`iters` Jacobi iterations of fp_tsdf_diffuse on val fp32 [C, nz, ny, nx], C 1 or 3, and state uint8
    [nz, ny, nx] (0 UNKNOWN, 1 FIXED, 2 FREE) -> (val', state'), new tensors; the arguments are left as they are.  CPU tensors, other
    dtypes or shapes, a state value above 2 (one read-back) and iters outside 0 .. 4096 are refused here, before any launch: ValueError."""
    fn = "tsdf_diffuse"
    for name, t, dt, nd in (("val", val, torch.float32, 4), ("state", state, torch.uint8, 3)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"{fn}: {name} must be a tensor on the device (there is no CPU path)")
        if t.dtype != dt or t.dim() != nd:
            raise ValueError(f"{fn}: {name} must be {dt} with {nd} dimensions, got {t.dtype} {tuple(t.shape)}")
    c, nz, ny, nx = (int(d) for d in val.shape)
    if c not in (1, 3) or tuple(state.shape) != (nz, ny, nx):
        raise ValueError(f"{fn}: val {tuple(val.shape)} must be [1 or 3, nz, ny, nx] and state {tuple(state.shape)} its [nz, ny, nx]")
    if min(nx, ny, nz) < 1 or max(nx, ny, nz) > _lib.TSDF_MAX_DIM or nx * ny * nz > _lib.TSDF_MAX_VOXELS:
        raise ValueError(f"{fn}: dimensions {nx} x {ny} x {nz} outside [1, {_lib.TSDF_MAX_DIM}] or beyond {_lib.TSDF_MAX_VOXELS} voxels")
    if isinstance(iters, bool) or not hasattr(iters, "__index__") or not 0 <= int(iters) <= _lib.TSDF_DIFFUSE_MAX_ITERS:
        raise ValueError(f"{fn}: iters must be an integer in [0, {_lib.TSDF_DIFFUSE_MAX_ITERS}], got {iters!r}")
    if int(state.max()) > 2:
        raise ValueError(f"{fn}: state holds {int(state.max())}; 0 UNKNOWN, 1 FIXED and 2 FREE are the states")
    val, state = val.contiguous().clone(), state.contiguous().clone()
    if int(iters) > 0:
        val_tmp, state_tmp = torch.empty_like(val), torch.empty_like(state)
        call("fp_tsdf_diffuse", ptr(val), ptr(state), ptr(val_tmp), ptr(state_tmp), c, nx, ny, nz, int(iters), stream())
    return val, state


def _mesh_grid(fn: str, origin, cell_mm, dims):
    """The checks the two mesh wrappers share -> (grid fp64 [4] on the host, (nx, ny, nz))."""
    import numpy as np
    try:
        grid = np.ascontiguousarray(np.concatenate([np.asarray(origin, np.float64).reshape(3), [float(cell_mm)]]))
        nx, ny, nz = (int(d) for d in dims)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{fn}: origin is three numbers, cell_mm one, dims three integers ({e})")
    if not np.all(np.isfinite(grid)) or not grid[3] > 0:
        raise ValueError(f"{fn}: the origin must be finite and the cell size finite and > 0")
    if min(nx, ny, nz) < 1 or max(nx, ny, nz) > _lib.MESH_MAX_DIM:
        raise ValueError(f"{fn}: dimensions {nx} x {ny} x {nz} outside [1, {_lib.MESH_MAX_DIM}]")
    return grid, (nx, ny, nz)


def _mesh_vertices(fn: str, vertices: torch.Tensor) -> torch.Tensor:
    require_cuda(vertices)
    if vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.shape[0] > _lib.MESH_MAX_ROWS:
        raise ValueError(f"{fn}: vertices must be float32 [V, 3] with V <= {_lib.MESH_MAX_ROWS}, got {vertices.dtype} {tuple(vertices.shape)}")
    return vertices.contiguous()


def mesh_cell_keys(vertices: torch.Tensor, origin, cell_mm: float, dims) -> torch.Tensor:
    """fp_mesh_cell_keys: vertices fp32 [V, 3] -> int64 [V], the cell (k ny + j) nx + i of the grid of `dims` = (nx, ny, nz) cells of
    cell_mm from `origin` each vertex falls into, clamped to the grid.  Checked here, before any launch: ValueError."""
    fn = "mesh_cell_keys"
    vertices = _mesh_vertices(fn, vertices)
    grid, (nx, ny, nz) = _mesh_grid(fn, origin, cell_mm, dims)
    keys = torch.empty(vertices.shape[0], dtype=torch.int64, device=vertices.device)
    call("fp_mesh_cell_keys", ptr(vertices), vertices.shape[0], grid.ctypes.data_as(_lib.vp), nx, ny, nz, ptr(keys), stream())
    return keys


def mesh_cluster_tables(keys: torch.Tensor, faces: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The plumbing between the two mesh kernels, all torch: keys int64 [V] (mesh_cell_keys), faces int32 [F, 3] with every index in
    [0, V) (the caller checks that) -> cells int64 [C] (the occupied cells, ascending: the output vertex order), rank int64 [V] (each
    vertex's cell), vert_order [V] (vertex ids by (rank, id)) with vert_begin [C + 1], corner_order [3 F] (corner ids 3 f + k by
    (rank of the corner's vertex, corner id)) with corner_begin [C + 1]."""
    require_cuda(keys, faces)
    cells, rank = torch.unique(keys, sorted=True, return_inverse=True)
    num_cells = cells.shape[0]

    def grouped(r):
        order = torch.sort(r, stable=True)[1]
        begin = torch.zeros(num_cells + 1, dtype=torch.int64, device=keys.device)
        begin[1:] = torch.cumsum(torch.bincount(r, minlength=num_cells), 0)
        return order.contiguous(), begin
    vert_order, vert_begin = grouped(rank)
    corner_order, corner_begin = grouped(rank[faces.reshape(-1).long()])
    return {"cells": cells.contiguous(), "rank": rank, "vert_order": vert_order, "vert_begin": vert_begin, "corner_order": corner_order,
            "corner_begin": corner_begin}


def mesh_cluster(vertices: torch.Tensor, colors: torch.Tensor, faces: torch.Tensor, tables: Dict[str, torch.Tensor], origin, cell_mm: float,
                 dims, eig_eps: float = 1e-3) -> Dict[str, torch.Tensor]:
    """fp_mesh_cluster: one vertex per occupied cell of `tables` (mesh_cluster_tables), placed where the summed plane quadrics of the
    faces touching the cell are smallest.  vertices, colors fp32 [V, 3], faces int32 [F, 3] (F may be 0) ->
    dict(positions fp32 [C, 3], colors fp32 [C, 3], quadrics fp64 [C, 10], means fp64 [C, 3], err fp64 [C], status int32 [C]: the
    number of kept eigenvalues, or -1 where the solve left the cell's neighbourhood and the mean was taken).  Checked here, before any
    launch: ValueError."""
    import math
    fn = "mesh_cluster"
    vertices = _mesh_vertices(fn, vertices)
    require_cuda(colors, faces, *tables.values())
    num_v = vertices.shape[0]
    if colors.dtype != torch.float32 or tuple(colors.shape) != (num_v, 3):
        raise ValueError(f"{fn}: colors must be float32 [{num_v}, 3], got {colors.dtype} {tuple(colors.shape)}")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3 or 3 * faces.shape[0] > _lib.MESH_MAX_ROWS:
        raise ValueError(f"{fn}: faces must be int32 [F, 3] with 3 F <= {_lib.MESH_MAX_ROWS}, got {faces.dtype} {tuple(faces.shape)}")
    num_f = faces.shape[0]
    grid, (nx, ny, nz) = _mesh_grid(fn, origin, cell_mm, dims)
    if isinstance(eig_eps, bool) or not isinstance(eig_eps, (int, float)) or not math.isfinite(eig_eps) or not 0 <= eig_eps < 1:
        raise ValueError(f"{fn}: eig_eps must be a number in [0, 1), got {eig_eps!r}")
    num_c = tables["cells"].shape[0]
    want = {"cells": num_c, "vert_order": num_v, "vert_begin": num_c + 1, "corner_order": 3 * num_f, "corner_begin": num_c + 1}
    for name, n in want.items():
        t = tables[name]
        if t.dtype != torch.int64 or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError(f"{fn}: tables[{name!r}] must be contiguous int64 [{n}], got {t.dtype} {tuple(t.shape)}")
    if num_v < 1 or not 1 <= num_c <= num_v:
        raise ValueError(f"{fn}: {num_v} vertices in {num_c} cells")
    colors, faces = colors.contiguous(), faces.contiguous()
    dev = vertices.device
    out = {"positions": torch.empty(num_c, 3, dtype=torch.float32, device=dev), "colors": torch.empty(num_c, 3, dtype=torch.float32, device=dev),
           "quadrics": torch.empty(num_c, 10, dtype=torch.float64, device=dev), "means": torch.empty(num_c, 3, dtype=torch.float64, device=dev),
           "err": torch.empty(num_c, dtype=torch.float64, device=dev), "status": torch.empty(num_c, dtype=torch.int32, device=dev)}
    call("fp_mesh_cluster", ptr(vertices), ptr(colors), num_v, ptr(faces) if num_f else None, num_f, ptr(tables["cells"]), num_c,
         ptr(tables["vert_order"]), ptr(tables["vert_begin"]), ptr(tables["corner_order"]) if num_f else None, ptr(tables["corner_begin"]),
         grid.ctypes.data_as(_lib.vp), nx, ny, nz, float(eig_eps), *(ptr(t) for t in out.values()), stream())
    return out


def _lm_inputs(B: int, R, t, row_begin, row_end, has_pose, feats, vertices, max_points: Optional[int]):
    """The conversions every Levenberg-Marquardt solver (refine_util's three refiners, tsdf_track) makes, in the order they are enqueued, and
    the max_points rule: None is read back from the device.
    -> (R [B, 9] f64, t [B, 3] f64, row_begin, row_end, has_pose i32, feats f32 or None, vertices f32, max_points >= 1)."""
    Rin = R.to(torch.float64).reshape(B, 9).contiguous()
    tin = t.to(torch.float64).reshape(B, 3).contiguous()
    rb = row_begin.to(torch.int32).contiguous()
    re = row_end.to(torch.int32).contiguous()
    hp = has_pose.to(torch.int32).contiguous()
    f32 = None if feats is None else feats.float().contiguous()
    v32 = vertices.float().contiguous()
    if max_points is None:
        max_points = int(torch.where(hp != 0, re - rb, torch.zeros_like(re)).max().item()) if B else 0
    return Rin, tin, rb, re, hp, f32, v32, max(1, int(max_points))


def _lm_outputs(B: int, dev, normal_eq_width: int, depth_inliers: bool = False) -> Tuple[Dict[str, torch.Tensor], list]:
    """Allocates such a solver's outputs.  -> (the result dict, the output pointers in the order of the C ABI -- the dict's own, then normal_eq);
    normal_eq_width 0: no normal equations."""
    f64, i32, empty = torch.float64, torch.int32, torch.empty
    out = {"R": empty(B, 9, dtype=f64, device=dev), "t": empty(B, 3, dtype=f64, device=dev), "cost_in": empty(B, dtype=f64, device=dev),
           "cost_out": empty(B, dtype=f64, device=dev), "num_points": empty(B, dtype=i32, device=dev)}
    if depth_inliers:
        out["num_depth_inliers"] = empty(B, dtype=i32, device=dev)
    out["iters_used"], out["status"] = empty(B, dtype=i32, device=dev), empty(B, dtype=i32, device=dev)
    neq = empty(B, normal_eq_width, dtype=f64, device=dev) if normal_eq_width else None
    ptrs = [ptr(v) for v in out.values()]
    ptrs.append(ptr(neq))
    out["R"] = out["R"].reshape(B, 3, 3)
    if neq is not None:
        out["normal_eq"] = neq
    return out, ptrs


def tsdf_track(volume: dict, points: torch.Tensor, row_begin: torch.Tensor, row_end: torch.Tensor, R: torch.Tensor, t: torch.Tensor, max_dist,
               min_count: int, trunc_mm: float, iters: int, has_pose: Optional[torch.Tensor] = None, want_normal_eq: bool = False,
               colors: Optional[torch.Tensor] = None, color_weight: float = 0.0, color_max: float = 0.25) -> dict:
    """Tracks B independent problems against `volume` (fp_tsdf_track): points fp32 [N, 3], camera-frame mm;
    row_begin / row_end int [B]: a problem's rows of points; R [B, 3, 3] / t [B, 3] the start poses, model -> camera; max_dist: the
    inlier distance in mm, a number or one per problem (not validated: a NaN or a value <= 0 skips the problem); trunc_mm: the tau the
    volume was built with; has_pose [B] bool (None: all).  Everything else is checked here, before any launch: ValueError.
    -> dict of device tensors: R [B, 3, 3] f64, t [B, 3] f64, cost_in, cost_out [B] f64, num_points (inliers at the start pose),
    iters_used, status [B] i32 (0 refined, 1 no step accepted, 2 skipped), + normal_eq [B, 28] f64 with want_normal_eq.
    colors fp32 [N, 3] on the points' device, in [0, 1], row-aligned with points: the colour term of DESIGN.md section 31 joins the
    objective (fp_tsdf_track_rgb) with color_weight (mm per unit of colour) and color_max (the channel inlier bound), both finite and
    > 0; the costs and normal_eq are then the joint system's, num_points stays the geometric inlier count.  None: the call above."""
    import numpy as np
    fn = "tsdf_track"
    box, dims = _tsdf_box(fn, volume.get("origin") if isinstance(volume, dict) else None, volume.get("voxel_mm") if isinstance(volume, dict) else None,
                          volume.get("dims", ()) if isinstance(volume, dict) else ())
    _tsdf_state(fn, volume, dims)
    if min(dims) < 2:
        raise ValueError(f"{fn}: dimensions {dims} leave no cell between voxel centres")
    if isinstance(min_count, bool) or not hasattr(min_count, "__index__") or int(min_count) < 1 or int(min_count) > 2**31 - 1:
        raise ValueError(f"{fn}: min_count must be an integer >= 1, got {min_count!r}")
    tau = float(trunc_mm)
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError(f"{fn}: trunc_mm must be finite and > 0, got {trunc_mm!r}")
    if isinstance(iters, bool) or not hasattr(iters, "__index__") or not 0 <= int(iters) <= 1000:
        raise ValueError(f"{fn}: iters must be an integer in [0, 1000], got {iters!r}")
    for name, x in (("points", points), ("row_begin", row_begin), ("row_end", row_end), ("R", R), ("t", t)) + ((("has_pose", has_pose),) if has_pose is not None else ()):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError(f"{fn}: {name} must be a tensor on the device (there is no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{fn}: points {tuple(points.shape)} are not [N, 3]")
    B = int(row_begin.numel())
    if B < 1 or B > 65535 or row_begin.dim() != 1 or tuple(row_end.shape) != (B,) or R.numel() != 9 * B or t.numel() != 3 * B:
        raise ValueError(f"{fn}: row_begin {tuple(row_begin.shape)}, row_end {tuple(row_end.shape)}, R {tuple(R.shape)} and t {tuple(t.shape)} are not "
                         "one batch of 1 .. 65535 problems")
    if has_pose is not None and tuple(has_pose.shape) != (B,):
        raise ValueError(f"{fn}: has_pose {tuple(has_pose.shape)} is not [{B}]")
    md = np.asarray(max_dist.detach().cpu().numpy() if isinstance(max_dist, torch.Tensor) else max_dist, np.float64)
    if md.ndim == 0:
        md = np.full(B, float(md))
    if md.shape != (B,):
        raise ValueError(f"{fn}: max_dist is one number or one per problem, got {md.shape}")
    if colors is not None:
        if not isinstance(colors, torch.Tensor) or not colors.is_cuda or colors.device != points.device:
            raise ValueError(f"{fn}: colors must be a tensor on the device of points (there is no CPU path)")
        if colors.dtype != torch.float32 or tuple(colors.shape) != tuple(points.shape):
            raise ValueError(f"{fn}: colors must be float32 {tuple(points.shape)}, one row per row of points, got {colors.dtype} {tuple(colors.shape)}")
        for name, v in (("color_weight", color_weight), ("color_max", color_max)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not (np.isfinite(v) and v > 0):
                raise ValueError(f"{fn}: {name} must be finite and > 0 with colors, got {v!r}")
    dev = points.device
    hp = torch.ones(B, dtype=torch.int32, device=dev) if has_pose is None else has_pose
    Rin, tin, rb, re, hp, _, p32, max_points = _lm_inputs(B, R, t, row_begin, row_end, hp, None, points, None)
    md_d = _lib.upload_async(torch.from_numpy(np.ascontiguousarray(md)), dev)
    out, outs = _lm_outputs(B, dev, 28 if want_normal_eq else 0)
    nbytes = _lib.tsdf_track_scratch_bytes(B, max_points)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if colors is not None:
        call("fp_tsdf_track_rgb", ptr(volume["sdf_sum"]), ptr(volume["sdf_cnt"]), ptr(volume["rgb_sum"]), ptr(volume["rgb_cnt"]),
             box.ctypes.data_as(_lib.vp), *dims, int(min_count), tau, ptr(p32), ptr(colors.contiguous()), int(p32.shape[0]), ptr(rb), ptr(re), ptr(Rin),
             ptr(tin), ptr(hp), ptr(md_d), float(color_weight), float(color_max), B, max_points, int(iters), ptr(scratch), nbytes, *outs, stream())
        return out
    call("fp_tsdf_track", ptr(volume["sdf_sum"]), ptr(volume["sdf_cnt"]), box.ctypes.data_as(_lib.vp), *dims, int(min_count), tau, ptr(p32),
         int(p32.shape[0]), ptr(rb), ptr(re), ptr(Rin), ptr(tin), ptr(hp), ptr(md_d), B, max_points, int(iters), ptr(scratch), nbytes,
         *outs, stream())
    return out


def mask_distance(masks: torch.Tensor) -> torch.Tensor:
    """The exact squared distance field of binary masks (fp_mask_distance): masks uint8 [B, H, W] on the device,
    non-zero = set, 1 <= H, W <= 16384 -> int32 [B, H, W], the squared distance in pixels from each pixel to the nearest set pixel of
    its mask (0 on a set pixel), 2^30 everywhere in a mask without a set pixel.  B = 0 returns without a launch."""
    if not isinstance(masks, torch.Tensor) or not masks.is_cuda:
        raise ValueError("mask_distance: masks must be a tensor on the device (there is no CPU path)")
    if masks.dtype != torch.uint8 or masks.dim() != 3:
        raise ValueError(f"mask_distance: masks must be uint8 [B, H, W], got {masks.dtype} {tuple(masks.shape)}")
    B, H, W = (int(n) for n in masks.shape)
    if not (1 <= H <= 16384 and 1 <= W <= 16384) or B > 65535:
        raise ValueError(f"mask_distance: {B} masks of {W} x {H}: at most 65535 masks with sides in [1, 16384]")
    d2 = torch.empty((B, H, W), dtype=torch.int32, device=masks.device)
    if B:
        m = masks.contiguous()
        call("fp_mask_distance", ptr(m), B, H, W, ptr(d2), stream())
    return d2


def multiview_refine(points: torch.Tensor, targets: torch.Tensor, view_index: torch.Tensor, view_cam: torch.Tensor, view_T: torch.Tensor,
                     row_begin: torch.Tensor, row_end: torch.Tensor, R: torch.Tensor, t: torch.Tensor, huber_px: float = 10.0, iters: int = 20,
                     has_pose: Optional[torch.Tensor] = None, max_points: Optional[int] = None, want_normal_eq: bool = False) -> dict:
    """Multi-view pose consensus of B independent problems (fp_multiview_refine).  A problem's pose is model -> WORLD;
    its rows [row_begin, row_end) are (view, model point) pairs: points fp32 [N, 3] the model point, targets fp64 [N, 2] the pixel it
    should project to, view_index int32 [N] its row of view_cam fp64 [V, 4] (fx, fy, cx, cy) and view_T fp64 [V, 12] (R_v row-major | t_v,
    world -> camera).  row_begin / row_end int32 [B]; R fp64 [B, 3, 3] / t fp64 [B, 3] the start poses; has_pose [B] bool or int32 (None:
    all); huber_px the Huber delta in pixels; max_points the row cap of a problem the scratch is sized for (None: the longest range).
    Everything is checked here, before any launch, with one read-back for the row ranges and the view indices: ValueError.
    -> dict of device tensors: R [B, 3, 3] f64, t [B, 3] f64, cost_in, cost_out [B] f64, num_points (inliers at the start pose),
    iters_used, status [B] i32 (0 refined, 1 no step accepted, 2 skipped), + normal_eq [B, 28] f64 with want_normal_eq."""
    import math
    fn = "multiview_refine"
    spec = (("points", points, (torch.float32,), 2, 3), ("targets", targets, (torch.float64,), 2, 2), ("view_index", view_index, (torch.int32,), 1, None),
            ("view_cam", view_cam, (torch.float64,), 2, 4), ("view_T", view_T, (torch.float64,), 2, 12), ("row_begin", row_begin, (torch.int32,), 1, None),
            ("row_end", row_end, (torch.int32,), 1, None), ("R", R, (torch.float64,), 3, 3), ("t", t, (torch.float64,), 2, 3))
    if has_pose is not None:
        spec += (("has_pose", has_pose, (torch.int32, torch.bool), 1, None),)
    dev = points.device if isinstance(points, torch.Tensor) else None
    for name, x, dts, nd, last in spec:
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device != dev:
            raise ValueError(f"{fn}: {name} must be a tensor on the device of points (there is no CPU path)")
        if x.dtype not in dts or x.dim() != nd or (last is not None and x.shape[-1] != last):
            raise ValueError(f"{fn}: {name} must be {' or '.join(str(d) for d in dts)} with {nd} dimensions{'' if last is None else f', the last of {last}'}, "
                             f"got {x.dtype} {tuple(x.shape)}")
    N, V, B = int(points.shape[0]), int(view_cam.shape[0]), int(row_begin.shape[0])
    if N < 1 or tuple(targets.shape) != (N, 2) or tuple(view_index.shape) != (N,):
        raise ValueError(f"{fn}: targets {tuple(targets.shape)} and view_index {tuple(view_index.shape)} are not one row per row of points [{N}, 3]")
    if V < 1 or tuple(view_T.shape) != (V, 12):
        raise ValueError(f"{fn}: view_cam {tuple(view_cam.shape)} and view_T {tuple(view_T.shape)} are not [V, 4] and [V, 12] of the same V >= 1 views")
    if B < 1 or B > 65535 or tuple(row_end.shape) != (B,) or tuple(R.shape) != (B, 3, 3) or tuple(t.shape) != (B, 3):
        raise ValueError(f"{fn}: row_begin {tuple(row_begin.shape)}, row_end {tuple(row_end.shape)}, R {tuple(R.shape)} and t {tuple(t.shape)} are not "
                         "one batch of 1 .. 65535 problems")
    if has_pose is not None and tuple(has_pose.shape) != (B,):
        raise ValueError(f"{fn}: has_pose {tuple(has_pose.shape)} is not [{B}]")
    if isinstance(huber_px, bool) or not isinstance(huber_px, (int, float)) or not (math.isfinite(huber_px) and huber_px > 0):
        raise ValueError(f"{fn}: huber_px must be finite and > 0, got {huber_px!r}")
    if isinstance(iters, bool) or not hasattr(iters, "__index__") or not 0 <= int(iters) <= 1000:
        raise ValueError(f"{fn}: iters must be an integer in [0, 1000], got {iters!r}")
    if max_points is not None and (isinstance(max_points, bool) or not hasattr(max_points, "__index__") or int(max_points) < 1):
        raise ValueError(f"{fn}: max_points must be an integer >= 1 or None, got {max_points!r}")
    hp = torch.ones(B, dtype=torch.int32, device=dev) if has_pose is None else has_pose.to(torch.int32)
    # the one read-back: the claimed ranges, then the view indices of the claimed rows
    rb, re, live = row_begin.cpu().numpy().astype("int64"), row_end.cpu().numpy().astype("int64"), hp.cpu().numpy() != 0
    for b in range(B):
        if live[b] and not 0 <= rb[b] <= re[b] <= N:
            raise ValueError(f"{fn}: problem {b}: rows [{rb[b]}, {re[b]}) outside [0, {N}]")
    longest = int((re - rb)[live].max()) if live.any() else 0
    if max_points is not None and longest > int(max_points):
        raise ValueError(f"{fn}: problem {int(((re - rb) * live).argmax())} has {longest} rows, more than max_points {int(max_points)}")
    cap = max(1, longest if max_points is None else int(max_points))
    if N:
        claimed = torch.zeros(N + 1, dtype=torch.int32, device=dev)
        ones = (hp != 0).to(torch.int32)   # (a problem without a pose claims nothing, and its range is not looked at)
        claimed.index_add_(0, torch.where(hp != 0, row_begin, 0).long(), ones)
        claimed.index_add_(0, torch.where(hp != 0, row_end, 0).long(), -ones)
        used = torch.cumsum(claimed[:N], 0) > 0
        bad = used & ((view_index < 0) | (view_index >= V))
        if bool(bad.any()):
            row = int(torch.nonzero(bad)[0])
            raise ValueError(f"{fn}: row {row}: view index {int(view_index[row])} outside [0, {V})")
    out, outs = _lm_outputs(B, dev, 28 if want_normal_eq else 0)
    nbytes = _lib.multiview_scratch_bytes(B, cap)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    points, targets, view_index, view_cam, view_T, row_begin, row_end, Rin, tin, hp = (
        x.contiguous() for x in (points, targets, view_index, view_cam, view_T, row_begin, row_end, R.reshape(B, 9), t, hp))
    call("fp_multiview_refine", ptr(points), ptr(targets), ptr(view_index), N, ptr(view_cam), ptr(view_T), V, ptr(row_begin), ptr(row_end), ptr(Rin),
         ptr(tin), ptr(hp), float(huber_px), B, cap, int(iters), ptr(scratch), nbytes, *outs, stream())
    return out


def _depth_stack(name: str, t: torch.Tensor, dtype) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a tensor on the device (there is no CPU path)")
    if t.dim() != 3 or t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype} [N, H, W]")
    return t.contiguous()


def _depth_planes(planes: torch.Tensor, count: torch.Tensor, n: int):
    if not (isinstance(planes, torch.Tensor) and planes.is_cuda and planes.dtype == torch.float64 and tuple(planes.shape) == (n, _lib.DEPTH_MAX_PLANES, 4)):
        raise ValueError(f"planes must be float64 [{n}, {_lib.DEPTH_MAX_PLANES}, 4] on the device")
    if not (isinstance(count, torch.Tensor) and count.is_cuda and count.dtype == torch.int32 and tuple(count.shape) == (n,)):
        raise ValueError(f"the plane counts must be int32 [{n}] on the device")
    return planes.contiguous(), count.contiguous()


def depth_plane_fit(depth: torch.Tensor, cameras, frame_keys, prior_planes: torch.Tensor, num_prior: torch.Tensor, hypotheses: int = 256,
                    stride: int = 4, plane_thresh_mm: float = 10.0, max_depth_mm: float = 0.0, min_plane_share: float = 0.05, seed: int = 0,
                    want_counts: bool = False):
    """One more supporting plane per frame (fp_depth_plane_fit): depth [N, H, W] fp32 mm on the device, cameras
    [N, 4] and frame_keys [N] on the host, the frames' earlier planes [N, 4, 4] fp64 and their number int32 [N] on the device.
    -> (plane fp64 [N, 4], info int32 [N, 8], the counts of all hypotheses int32 [N, hypotheses] or None).  A refused call raises
    ValueError and writes nothing."""
    import numpy as np
    d = _depth_stack("depth_plane_fit: depth", depth, torch.float32)
    n, h, w = d.shape
    cam = np.ascontiguousarray(np.asarray(cameras, dtype=np.float64).reshape(-1, 4))
    keys = np.ascontiguousarray(np.asarray(frame_keys, dtype=np.uint64).reshape(-1))
    if cam.shape[0] != n or keys.shape[0] != n:
        raise ValueError(f"depth_plane_fit: {n} frames, {cam.shape[0]} cameras, {keys.shape[0]} keys")
    pp, npr = _depth_planes(prior_planes, num_prior, n)
    plane = torch.empty(max(n, 1), 4, dtype=torch.float64, device=d.device)[:n]
    info = torch.empty(max(n, 1), 8, dtype=torch.int32, device=d.device)[:n]
    counts = torch.empty(max(n, 1), max(int(hypotheses), 1), dtype=torch.int32, device=d.device)[:n] if want_counts else None
    nbytes = _lib.depth_plane_scratch_bytes(n, h * w, max(int(hypotheses), 0))
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=d.device)
    call("fp_depth_plane_fit", ptr(d), n, h, w, cam.ctypes.data_as(_lib.vp), keys.ctypes.data_as(_lib.vp), ptr(pp), ptr(npr), int(hypotheses),
         int(stride), float(plane_thresh_mm), float(max_depth_mm), float(min_plane_share), int(seed) & (2**64 - 1),
         ptr(scratch), nbytes, ptr(plane), ptr(info), ptr(counts), stream(), invalid=ValueError)
    return plane, info, counts


def depth_components(depth: torch.Tensor, cameras, slope_fx, planes: torch.Tensor, num_planes: torch.Tensor, max_depth_mm: float = 0.0,
                     object_margin_mm: float = 15.0, connect_mm: float = 5.0) -> torch.Tensor:
    """Foreground and connected components of one level (fp_depth_components): slope_fx [N] fp32 on the host = connect_slope / fx.
    -> labels int32 [N, H, W], the smallest linear index of the pixel's component, -1 for background."""
    import numpy as np
    d = _depth_stack("depth_components: depth", depth, torch.float32)
    n, h, w = d.shape
    cam = np.ascontiguousarray(np.asarray(cameras, dtype=np.float64).reshape(-1, 4))
    sl = np.ascontiguousarray(np.asarray(slope_fx, dtype=np.float32).reshape(-1))
    if cam.shape[0] != n or sl.shape[0] != n:
        raise ValueError(f"depth_components: {n} frames, {cam.shape[0]} cameras, {sl.shape[0]} slopes")
    pl, npl = _depth_planes(planes, num_planes, n)
    labels = torch.empty(max(n, 1), h, w, dtype=torch.int32, device=d.device)[:n]
    nbytes = _lib.depth_components_scratch_bytes(n, h * w)
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=d.device)
    call("fp_depth_components", ptr(d), n, h, w, cam.ctypes.data_as(_lib.vp), sl.ctypes.data_as(_lib.vp), ptr(pl), ptr(npl),
         float(max_depth_mm), float(object_margin_mm), float(np.float32(connect_mm)), ptr(scratch), nbytes,
         ptr(labels), stream(), invalid=ValueError)
    return labels


def component_table(labels: torch.Tensor, min_pixels: int, max_area: int, max_proposals: int, level: int = 0,
                    finer: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The kept components of a label map (fp_component_table): -> (table int32 [N, max_proposals, 7] = (label, area, x0, y0, x1, y1,
    level) by rank, counts int32 [N, 4] = (components, within the area limits, kept, dropped as a finer level's), rank_map int32
    [N, H, W]).  finer: int32 [F, N, max_proposals, 7], the tables of finer levels."""
    lab = _depth_stack("component_table: labels", labels, torch.int32)
    n, h, w = lab.shape
    nf = 0
    if finer is not None:
        if not (finer.is_cuda and finer.dtype == torch.int32 and finer.dim() == 4 and tuple(finer.shape[1:]) == (n, int(max_proposals), 7)):
            raise ValueError(f"component_table: finer must be int32 [F, {n}, {max_proposals}, 7] on the device")
        finer, nf = finer.contiguous(), finer.shape[0]
    p = max(int(max_proposals), 1)
    table = torch.empty(max(n, 1), p, 7, dtype=torch.int32, device=lab.device)[:n]
    counts = torch.empty(max(n, 1), 4, dtype=torch.int32, device=lab.device)[:n]
    rank_map = torch.empty(max(n, 1), h, w, dtype=torch.int32, device=lab.device)[:n]
    nbytes = _lib.component_table_scratch_bytes(n, h * w)
    scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=lab.device)
    call("fp_component_table", ptr(lab), n, h, w, int(min_pixels), int(max_area), int(max_proposals), int(level), ptr(finer), nf,
         ptr(scratch), nbytes, ptr(table), ptr(counts), ptr(rank_map), stream(), invalid=ValueError)
    return table, counts, rank_map


def component_runs(rank_maps: torch.Tensor, num_kept: torch.Tensor, max_proposals: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """COCO's uncompressed run lengths of every kept component of a stack of rank maps (fp_component_runs marks the run boundaries;
    sorting them and taking differences is plumbing): rank_maps int32 [M, H, W], num_kept int32 [M] on the device -> (runs int32
    [total], run_off int32 [M * max_proposals + 1]): the list of rank r of map m is runs[run_off[g] : run_off[g + 1]], g = m *
    max_proposals + r (empty beyond num_kept[m]).  Reads the event count back (one synchronisation)."""
    maps = _depth_stack("component_runs: rank_maps", rank_maps, torch.int32)
    m, h, w = maps.shape
    if not (isinstance(num_kept, torch.Tensor) and num_kept.is_cuda and num_kept.dtype == torch.int32 and tuple(num_kept.shape) == (m,)):
        raise ValueError(f"component_runs: num_kept must be int32 [{m}] on the device")
    kept = num_kept.contiguous()
    count = torch.empty(1, dtype=torch.int32, device=maps.device)
    call("fp_component_runs", ptr(maps), m, h, w, ptr(kept), int(max_proposals), 0, None, ptr(count), stream(), invalid=ValueError)
    total = int(count.item())
    groups = m * int(max_proposals)
    if total == 0:
        return torch.zeros(0, dtype=torch.int32, device=maps.device), torch.zeros(groups + 1, dtype=torch.int32, device=maps.device)
    events = torch.empty(total, dtype=torch.int64, device=maps.device)
    call("fp_component_runs", ptr(maps), m, h, w, ptr(kept), int(max_proposals), total, ptr(events), ptr(count), stream(), invalid=ValueError)
    events = torch.sort(events).values
    group, pos = events >> 32, events & 0xffffffff
    prev = torch.zeros_like(pos)
    prev[1:] = torch.where(group[1:] == group[:-1], pos[:-1], torch.zeros_like(pos[:-1]))
    run_off = torch.zeros(groups + 1, dtype=torch.int64, device=maps.device)
    run_off[1:] = torch.cumsum(torch.bincount(group, minlength=groups), 0)
    return (pos - prev).to(torch.int32), run_off.to(torch.int32)


def texture_mips(rgb: torch.Tensor) -> torch.Tensor:
    """The mip pyramid of a texture (fp_texture_mips): rgb uint8 [H, W, 3] on the device -> int32 [total] holding packed RGBA8
    texels (view as uint32), the levels back to back in the layout of _lib.texture_levels(W, H)."""
    require_cuda(rgb)
    if rgb.dim() != 3 or rgb.shape[2] != 3 or rgb.dtype != torch.uint8:
        raise ValueError("texture_mips: rgb must be uint8 [H, W, 3]")
    h, w = int(rgb.shape[0]), int(rgb.shape[1])
    if not (1 <= h <= _lib.TEXTURE_MAX_SIDE and 1 <= w <= _lib.TEXTURE_MAX_SIDE):
        raise ValueError(f"texture_mips: texture {w} x {h} outside [1, {_lib.TEXTURE_MAX_SIDE}]")
    rgb = rgb.contiguous()
    out = torch.empty(_lib.texture_levels(w, h)[1], dtype=torch.int32, device=rgb.device)
    call("fp_texture_mips", ptr(rgb), w, h, ptr(out), stream())
    return out


def detection_masks(counts: torch.Tensor, run_off: torch.Tensor, canvas_hw: Tuple[int, int], image_hw: Tuple[int, int],
                    open3x3: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Detection masks from their COCO run lengths (fp_detection_masks).  counts int32 [R_total]: the runs of N
    detections, concatenated; run_off int32 [N + 1]: where each detection's runs start (infer_pose_util.pack_rle builds and validates both;
    the kernels clamp the offsets to the array, so a wrong table gives a wrong mask and never a wild read); canvas_hw = (hc, wc) of the
    detector, image_hw = (H, W) of the image centre-cropped out of it.  -> (masks uint8 [N, H, W] of 0 / 1, area int32 [N]), the bits of
    rle_to_binary_mask, open_mask_3x3 (when open3x3) and the [dy : hc - dy, dx : wc - dx] slice."""
    require_cuda(counts, run_off)
    if counts.dtype != torch.int32 or run_off.dtype != torch.int32 or counts.dim() != 1 or run_off.dim() != 1 or run_off.shape[0] < 1:
        raise ValueError("detection_masks: counts must be int32 [R_total] and run_off int32 [N + 1]")
    (hc, wc), (h, w) = (int(v) for v in canvas_hw), (int(v) for v in image_hw)
    if not (1 <= h <= hc and 1 <= w <= wc and hc * wc <= 1 << 30):
        raise ValueError(f"detection_masks: an image of {w} x {h} out of a canvas of {wc} x {hc} (1 <= W <= wc, 1 <= H <= hc, hc wc <= 2^30)")
    counts, run_off = counts.contiguous(), run_off.contiguous()
    n = int(run_off.shape[0]) - 1
    masks = torch.empty(n, h, w, dtype=torch.uint8, device=counts.device)
    area = torch.empty(n, dtype=torch.int32, device=counts.device)
    prefix = torch.empty(max(int(counts.shape[0]), 1), dtype=torch.int32, device=counts.device)
    call("fp_detection_masks", ptr(counts), ptr(run_off), int(counts.shape[0]), n, hc, wc, h, w, int(bool(open3x3)), ptr(prefix), ptr(masks), ptr(area),
         stream())
    return masks, area


def pose_overlap(points: torch.Tensor, ranges: torch.Tensor, centers: torch.Tensor, radii: torch.Tensor, pose_obj: torch.Tensor,
                 valid: torch.Tensor, R: torch.Tensor, t: torch.Tensor, pairs: torch.Tensor, grid: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp_pose_overlap on device tables that have been validated already (pose_nms.pose_overlaps checks them on the
    host before it uploads them): points f32 [M, 3], ranges int32 [O, 2], centers f64 [O, 3], radii f64 [O], pose_obj / valid int32 [N],
    R f64 [N, 9] or [N, 3, 3], t f64 [N, 3], pairs int32 [P, 2].  -> (counts int32 [P, 2], overlap f64 [P], status int32 [P])."""
    require_cuda(points, ranges, centers, radii, pose_obj, valid, R, t, pairs)
    for x, dt in ((points, torch.float32), (ranges, torch.int32), (centers, torch.float64), (radii, torch.float64), (pose_obj, torch.int32),
                  (valid, torch.int32), (R, torch.float64), (t, torch.float64), (pairs, torch.int32)):
        if x.dtype != dt or not x.is_contiguous():
            raise ValueError(f"pose_overlap: a contiguous {dt} table is needed, got {x.dtype}{'' if x.is_contiguous() else ' (strided)'}")
    O, N, P = int(ranges.shape[0]), int(pose_obj.shape[0]), int(pairs.shape[0])
    if centers.numel() != 3 * O or radii.numel() != O or valid.numel() != N or R.numel() != 9 * N or t.numel() != 3 * N or pairs.numel() != 2 * P:
        raise ValueError("pose_overlap: table sizes do not match")
    dev = points.device
    counts = torch.empty(P, 2, dtype=torch.int32, device=dev)
    overlap = torch.empty(P, dtype=torch.float64, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    call("fp_pose_overlap", ptr(points), int(points.shape[0]), ptr(ranges), ptr(centers), ptr(radii), O, ptr(pose_obj), ptr(valid), ptr(R), ptr(t), N,
         ptr(pairs), P, int(grid), ptr(counts), ptr(overlap), ptr(status), stream())
    return counts, overlap, status


def pose_nms_greedy(group_off: torch.Tensor, pair_off: torch.Tensor, pairs: torch.Tensor, overlap: torch.Tensor, status: torch.Tensor,
                    num_poses: int, thresh: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp_pose_nms_greedy on device tables validated already (pose_nms.nms_greedy): group_off / pair_off int32
    [F + 1], pairs int32 [P, 2], overlap f64 [P], status int32 [P].  -> (keep int32 [num_poses], suppressed_by int32 [num_poses]); a pose
    of no frame is kept."""
    require_cuda(group_off, pair_off, pairs, overlap, status)
    for x, dt in ((group_off, torch.int32), (pair_off, torch.int32), (pairs, torch.int32), (overlap, torch.float64), (status, torch.int32)):
        if x.dtype != dt or not x.is_contiguous():
            raise ValueError(f"pose_nms_greedy: a contiguous {dt} table is needed, got {x.dtype}{'' if x.is_contiguous() else ' (strided)'}")
    F, P = int(group_off.shape[0]) - 1, int(overlap.shape[0])
    if F < 0 or int(pair_off.shape[0]) != F + 1 or pairs.numel() != 2 * P or status.numel() != P:
        raise ValueError("pose_nms_greedy: table sizes do not match")
    keep = torch.ones(num_poses, dtype=torch.int32, device=overlap.device)
    by = torch.full((num_poses,), -1, dtype=torch.int32, device=overlap.device)
    call("fp_pose_nms_greedy", ptr(group_off), ptr(pair_off), F, ptr(pairs), ptr(overlap), ptr(status), int(num_poses), P, float(thresh), ptr(keep), ptr(by),
         stream())
    return keep, by


def _detection_tables(name: str, tables) -> None:
    for x, dt in tables:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError(f"{name}: every table is a device tensor (got {'a CPU tensor' if isinstance(x, torch.Tensor) else type(x).__name__}); there is no CPU path")
        if x.dtype != dt or not x.is_contiguous():
            raise ValueError(f"{name}: a contiguous {dt} table is needed, got {x.dtype}{'' if x.is_contiguous() else ' (strided)'}")


def detection_match(est_off: torch.Tensor, gt_off: torch.Tensor, pair_off: torch.Tensor, err: torch.Tensor, gt_valid: torch.Tensor,
                    group_tab: torch.Tensor, ths: torch.Tensor, num_est: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp_detection_match on device tables whose CONTENTS have been validated already (eval_bop24.match_groups checks
    the offsets on the host before it uploads them): est_off / gt_off / pair_off int32 [NG + 1], err f64 [P, 2] (ops.pose_errors' first
    output, not read back), gt_valid int32 [G], group_tab int32 [NG], ths f64 [NTAB, 2, T].  -> (flag int8 [num_est, 2 T], matched_gt int32
    [num_est, 2 T]); an estimate of no group keeps flag 0 and matched_gt -1."""
    _detection_tables("detection_match", ((est_off, torch.int32), (gt_off, torch.int32), (pair_off, torch.int32), (err, torch.float64),
                                          (gt_valid, torch.int32), (group_tab, torch.int32), (ths, torch.float64)))
    NG = int(est_off.shape[0]) - 1
    if ths.dim() != 3 or ths.shape[1] != 2 or not 1 <= int(ths.shape[2]) <= MAX_THS or (NG > 0 and ths.shape[0] < 1):
        raise ValueError(f"detection_match: ths must be [NTAB >= 1, 2, T] with 1 <= T <= {MAX_THS}, got {tuple(ths.shape)}")
    if NG < 0 or int(gt_off.shape[0]) != NG + 1 or int(pair_off.shape[0]) != NG + 1 or group_tab.numel() != NG or err.dim() != 2 or err.shape[1] != 2 \
            or num_est < 0:
        raise ValueError("detection_match: table sizes do not match")
    T = int(ths.shape[2])
    flag = torch.zeros(num_est, 2 * T, dtype=torch.int8, device=err.device)
    matched = torch.full((num_est, 2 * T), -1, dtype=torch.int32, device=err.device)
    call("fp_detection_match", ptr(est_off), ptr(gt_off), ptr(pair_off), NG, ptr(err), int(err.shape[0]), ptr(gt_valid), int(gt_valid.shape[0]),
         ptr(group_tab), ptr(ths), int(ths.shape[0]), T, int(num_est), ptr(flag), ptr(matched), stream())
    return flag, matched


def detection_ap(obj_off: torch.Tensor, order: torch.Tensor, flag: torch.Tensor, n_valid: torch.Tensor,
                 rec_thr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp_detection_ap on device tables validated already (eval_bop24.ap_objects): obj_off int32 [O + 1], order int32
    [N], flag int8 [N_est, C] as detection_match wrote it, n_valid int32 [O], rec_thr f64 [R].  -> (ap f64 [O, C], q f64 [O, C, R], totals
    int32 [O, C, 3])."""
    _detection_tables("detection_ap", ((obj_off, torch.int32), (order, torch.int32), (flag, torch.int8), (n_valid, torch.int32), (rec_thr, torch.float64)))
    O, R = int(obj_off.shape[0]) - 1, int(rec_thr.numel())
    if flag.dim() != 2 or flag.shape[1] % 2 or not 1 <= int(flag.shape[1]) // 2 <= MAX_THS:
        raise ValueError(f"detection_ap: flag must be [N_est, 2 T] with 1 <= T <= {MAX_THS}, got {tuple(flag.shape)}")
    if not 1 <= R <= MAX_REC:
        raise ValueError(f"detection_ap: 1 <= R <= {MAX_REC} recall thresholds are needed, got {R}")
    if O < 0 or n_valid.numel() != O or order.dim() != 1:
        raise ValueError("detection_ap: table sizes do not match")
    C = int(flag.shape[1])
    ap = torch.empty(O, C, dtype=torch.float64, device=flag.device)
    q = torch.empty(O, C, R, dtype=torch.float64, device=flag.device)
    totals = torch.empty(O, C, 3, dtype=torch.int32, device=flag.device)
    call("fp_detection_ap", ptr(obj_off), O, ptr(order), int(order.shape[0]), ptr(flag), int(flag.shape[0]), C // 2, ptr(n_valid), ptr(rec_thr), R,
         ptr(ap), ptr(q), ptr(totals), stream())
    return ap, q, totals


# ---------------------------------------------------------------- proposal labelling
def mask_boxes(masks: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp_mask_boxes: masks uint8 [P, H, W] (0 / non-zero) -> (boxes int32 [P, 4] = (x1, y1, x2, y2), x2 / y2 exclusive; area int32 [P]); an
    empty mask gives (0, 0, 0, 0) and 0."""
    _detection_tables("mask_boxes", ((masks, torch.uint8),))
    if masks.dim() != 3 or masks.shape[1] < 1 or masks.shape[2] < 1:
        raise ValueError(f"mask_boxes: masks must be uint8 [P, H, W] with H, W >= 1, got {tuple(masks.shape)}")
    P, H, W = (int(v) for v in masks.shape)
    boxes = torch.empty(P, 4, dtype=torch.int32, device=masks.device)
    area = torch.empty(P, dtype=torch.int32, device=masks.device)
    call("fp_mask_boxes", ptr(masks), P, H, W, ptr(boxes), ptr(area), stream())
    return boxes, area


def proposal_crops(images: torch.Tensor, masks: torch.Tensor, boxes: torch.Tensor, size: int,
                   image_index: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp_proposal_crops: images f32 [n_img, H, W, 3] in [0, 1], masks uint8 [P, H, W], boxes int32 [P, 4] as mask_boxes writes them,
    image_index int32 [P] or None (proposal p reads image p).  -> (crops f32 [P, 3, size, size], status int32 [P]: 0 cropped, 2 all zero)."""
    tables = [(images, torch.float32), (masks, torch.uint8), (boxes, torch.int32)] + ([(image_index, torch.int32)] if image_index is not None else [])
    _detection_tables("proposal_crops", tables)
    if images.dim() != 4 or images.shape[3] != 3 or masks.dim() != 3 or tuple(masks.shape[1:]) != tuple(images.shape[1:3]):
        raise ValueError(f"proposal_crops: images [n_img, H, W, 3] and masks [P, H, W] of one H x W are needed, got {tuple(images.shape)} and {tuple(masks.shape)}")
    P = int(masks.shape[0])
    if tuple(boxes.shape) != (P, 4) or (image_index is not None and tuple(image_index.shape) != (P,)):
        raise ValueError(f"proposal_crops: boxes must be [{P}, 4] and image_index [{P}]")
    if image_index is None and int(images.shape[0]) < P:
        raise ValueError(f"proposal_crops: {P} proposals but {int(images.shape[0])} images and no image_index")
    if not 1 <= int(size) <= _lib.PROPOSAL_MAX_SIZE:
        raise ValueError(f"proposal_crops: crop size {size} outside [1, {_lib.PROPOSAL_MAX_SIZE}]")
    out = torch.empty(P, 3, int(size), int(size), dtype=torch.float32, device=masks.device)
    status = torch.empty(P, dtype=torch.int32, device=masks.device)
    call("fp_proposal_crops", ptr(images), int(images.shape[0]), int(images.shape[1]), int(images.shape[2]), ptr(masks), ptr(image_index), ptr(boxes),
         P, int(size), ptr(out), ptr(status), stream())
    return out, status


def proposal_scores(desc_n: torch.Tensor, bank_n: torch.Tensor, obj_off: torch.Tensor, max_templates: int, k: int, return_sims: bool = False):
    """fp_proposal_scores: desc_n f32 [P, D], bank_n f32 [N, D] (rows from normalize_rows), obj_off int32 [O + 1] over bank rows (device),
    max_templates: the largest template count of an object (host).  -> (scores f32 [P, O], best_obj int32 [P], best_score f32 [P],
    best_template int32 [P]); with return_sims also the similarities the retrieval left in scratch, f32 [O, P, max_templates] (columns past
    an object's template count are not written)."""
    _detection_tables("proposal_scores", ((desc_n, torch.float32), (bank_n, torch.float32), (obj_off, torch.int32)))
    if desc_n.dim() != 2 or bank_n.dim() != 2 or desc_n.shape[1] != bank_n.shape[1] or obj_off.dim() != 1 or obj_off.shape[0] < 2:
        raise ValueError(f"proposal_scores: desc_n [P, D], bank_n [N, D] and obj_off [O + 1] are needed, got {tuple(desc_n.shape)}, {tuple(bank_n.shape)}, {tuple(obj_off.shape)}")
    P, D, N, O = int(desc_n.shape[0]), int(desc_n.shape[1]), int(bank_n.shape[0]), int(obj_off.shape[0]) - 1
    if not 1 <= int(k) <= _lib.PROPOSAL_MAX_K or int(max_templates) < 1:
        raise ValueError(f"proposal_scores: k = {k} outside [1, {_lib.PROPOSAL_MAX_K}] or max_templates = {max_templates} < 1")
    dev = desc_n.device
    scores = torch.empty(P, O, dtype=torch.float32, device=dev)
    best_obj = torch.empty(P, dtype=torch.int32, device=dev)
    best_score = torch.empty(P, dtype=torch.float32, device=dev)
    best_tpl = torch.empty(P, dtype=torch.int32, device=dev)
    nbytes = _lib.proposal_score_scratch_bytes(P, O, D, int(max_templates), int(k))
    scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    call("fp_proposal_scores", ptr(desc_n), P, D, ptr(bank_n) if N else None, N, ptr(obj_off), O, int(max_templates), int(k), ptr(scratch), nbytes,
         ptr(scores), ptr(best_obj), ptr(best_score), ptr(best_tpl), stream())
    if not return_sims:
        return scores, best_obj, best_score, best_tpl
    sims = scratch[:4 * O * P * int(max_templates)].view(torch.float32).view(O, P, int(max_templates))
    return scores, best_obj, best_score, best_tpl, sims


def proposal_rank(best_obj: torch.Tensor, best_score: torch.Tensor, area: torch.Tensor, crop_status: torch.Tensor, boxes: torch.Tensor,
                  num_obj: int, min_area: int, min_score: float, max_group: int = 256):
    """fp_proposal_rank for the proposals of ONE image.  -> (decision int32 [P] (an index into _lib.PROPOSAL_DECISIONS), order int32 [P],
    group_off int32 [O + 1], pair_off int32 [O + 1], pairs int32 [max_pairs, 2], boxes_ranked int32 [P, 4]), all on the device."""
    _detection_tables("proposal_rank", ((best_obj, torch.int32), (best_score, torch.float32), (area, torch.int32), (crop_status, torch.int32),
                                        (boxes, torch.int32)))
    P = int(best_obj.shape[0])
    if not (best_score.shape == area.shape == crop_status.shape == best_obj.shape) or best_obj.dim() != 1 or tuple(boxes.shape) != (P, 4):
        raise ValueError("proposal_rank: best_obj, best_score, area and crop_status are [P], boxes [P, 4]")
    if P > _lib.PROPOSAL_MAX_RANKED or not 1 <= int(num_obj) <= _lib.PROPOSAL_MAX_RANKED:
        raise ValueError(f"proposal_rank: {P} proposals of {num_obj} objects (at most {_lib.PROPOSAL_MAX_RANKED} each, one object at least)")
    if not 1 <= int(max_group) <= 256 or min_score != min_score:
        raise ValueError(f"proposal_rank: max_group = {max_group} outside [1, 256] or min_score is NaN")
    dev = best_obj.device
    max_pairs = P * (int(max_group) - 1) // 2
    decision = torch.empty(P, dtype=torch.int32, device=dev)
    order = torch.empty(P, dtype=torch.int32, device=dev)
    group_off = torch.empty(int(num_obj) + 1, dtype=torch.int32, device=dev)
    pair_off = torch.empty(int(num_obj) + 1, dtype=torch.int32, device=dev)
    pairs = torch.empty(max_pairs, 2, dtype=torch.int32, device=dev)
    ranked = torch.empty(P, 4, dtype=torch.int32, device=dev)
    call("fp_proposal_rank", ptr(best_obj), ptr(best_score), ptr(area), ptr(crop_status), ptr(boxes), P, int(num_obj), int(min_area), float(min_score),
         int(max_group), max_pairs, ptr(decision), ptr(order), ptr(group_off), ptr(pair_off), ptr(pairs), ptr(ranked), stream())
    return decision, order, group_off, pair_off, pairs, ranked


def box_iou(boxes: torch.Tensor, pairs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp_box_iou: boxes int32 [N, 4] = (x1, y1, x2, y2), x2 / y2 exclusive; pairs int32 [M, 2].  -> (overlap f64 [M], status int32 [M]: 0
    scored, 2 union 0 or an index outside the table), the form pose_nms_greedy takes."""
    _detection_tables("box_iou", ((boxes, torch.int32), (pairs, torch.int32)))
    if boxes.dim() != 2 or boxes.shape[1] != 4 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError(f"box_iou: boxes [N, 4] and pairs [M, 2] are needed, got {tuple(boxes.shape)} and {tuple(pairs.shape)}")
    M = int(pairs.shape[0])
    overlap = torch.empty(M, dtype=torch.float64, device=boxes.device)
    status = torch.empty(M, dtype=torch.int32, device=boxes.device)
    call("fp_box_iou", ptr(boxes), int(boxes.shape[0]), ptr(pairs), M, ptr(overlap), ptr(status), stream())
    return overlap, status


# ---------------------------------------------------------------- the appearance score of a proposal
def proposal_patch_cover(masks: torch.Tensor, boxes: torch.Tensor, size: int, patch_size: int, image_index: Optional[torch.Tensor] = None,
                         n_img: Optional[int] = None) -> torch.Tensor:
    """fp_proposal_patch_cover: masks uint8 [P, H, W], boxes int32 [P, 4] as mask_boxes writes them, the crop size and the ViT's patch size
    (which divides it), image_index int32 [P] over n_img images or None (proposal p reads image p of P).  -> cover int32 [P, (size /
    patch_size)^2]: the pixels of every patch cell of proposal_crops' cut-out that the mask covers, cells in token order."""
    tables = [(masks, torch.uint8), (boxes, torch.int32)] + ([(image_index, torch.int32)] if image_index is not None else [])
    _detection_tables("proposal_patch_cover", tables)
    if masks.dim() != 3 or masks.shape[1] < 1 or masks.shape[2] < 1:
        raise ValueError(f"proposal_patch_cover: masks must be uint8 [P, H, W] with H, W >= 1, got {tuple(masks.shape)}")
    P = int(masks.shape[0])
    if tuple(boxes.shape) != (P, 4) or (image_index is not None and tuple(image_index.shape) != (P,)):
        raise ValueError(f"proposal_patch_cover: boxes must be [{P}, 4] and image_index [{P}]")
    if not 1 <= int(size) <= _lib.PROPOSAL_MAX_SIZE or int(patch_size) < 1 or int(size) % int(patch_size):
        raise ValueError(f"proposal_patch_cover: crop size {size} outside [1, {_lib.PROPOSAL_MAX_SIZE}] or no multiple of the patch size {patch_size}")
    n_img = int(n_img) if n_img is not None else (1 if image_index is not None else max(P, 1))
    g = int(size) // int(patch_size)
    cover = torch.empty(P, g * g, dtype=torch.int32, device=masks.device)
    call("fp_proposal_patch_cover", ptr(masks), n_img, int(masks.shape[1]), int(masks.shape[2]), ptr(image_index), ptr(boxes), P, int(size),
         int(patch_size), ptr(cover), stream())
    return cover


def proposal_appearance(q_n: torch.Tensor, q_cover: torch.Tensor, bank_patch_n: torch.Tensor, bank_cover: torch.Tensor, obj_off: torch.Tensor,
                        best_obj: torch.Tensor, best_template: torch.Tensor, best_score: torch.Tensor, min_cover: int):
    """fp_proposal_appearance: q_n f32 [P, Np, D] and bank_patch_n f32 [N, Np, D] (rows from normalize_rows), q_cover int32 [P, Np] and
    bank_cover int32 [N, Np] (proposal_patch_cover), obj_off int32 [O + 1], best_obj / best_template int32 [P] and best_score f32 [P] as
    proposal_scores takes and writes them.  -> (score f32 [P] = (best_score + appearance) / 2, appearance f32 [P], n_valid int32 [P],
    status int32 [P] (0 scored, 1 no valid query patch, 2 no template row, 3 no valid template patch), best_sim f32 [P, Np],
    best_patch int32 [P, Np]), all on the device."""
    _detection_tables("proposal_appearance", ((q_n, torch.float32), (q_cover, torch.int32), (bank_patch_n, torch.float32), (bank_cover, torch.int32),
                                              (obj_off, torch.int32), (best_obj, torch.int32), (best_template, torch.int32),
                                              (best_score, torch.float32)))
    if q_n.dim() != 3 or bank_patch_n.dim() != 3 or tuple(q_n.shape[1:]) != tuple(bank_patch_n.shape[1:]) or obj_off.dim() != 1 or obj_off.shape[0] < 2:
        raise ValueError(f"proposal_appearance: q_n [P, Np, D], bank_patch_n [N, Np, D] and obj_off [O + 1] are needed, got {tuple(q_n.shape)}, "
                         f"{tuple(bank_patch_n.shape)}, {tuple(obj_off.shape)}")
    P, Np, D = (int(v) for v in q_n.shape)
    N, O = int(bank_patch_n.shape[0]), int(obj_off.shape[0]) - 1
    if tuple(q_cover.shape) != (P, Np) or tuple(bank_cover.shape) != (N, Np) or not (tuple(best_obj.shape) == tuple(best_template.shape)
                                                                                     == tuple(best_score.shape) == (P,)):
        raise ValueError(f"proposal_appearance: q_cover [{P}, {Np}], bank_cover [{N}, {Np}] and best_obj / best_template / best_score [{P}] are needed")
    if D % 4 or D > _lib.APPEARANCE_MAX_DIM or not 1 <= Np <= _lib.APPEARANCE_MAX_PATCHES or P > _lib.APPEARANCE_MAX_PROPOSALS:
        raise ValueError(f"proposal_appearance: D = {D} (a multiple of 4, at most {_lib.APPEARANCE_MAX_DIM}), Np = {Np} (1 .. "
                         f"{_lib.APPEARANCE_MAX_PATCHES}), P = {P} (at most {_lib.APPEARANCE_MAX_PROPOSALS})")
    if isinstance(min_cover, bool) or not isinstance(min_cover, int) or min_cover < 1:
        raise ValueError(f"proposal_appearance: min_cover must be an integer >= 1, got {min_cover!r}")
    dev = q_n.device
    best_sim = torch.empty(P, Np, dtype=torch.float32, device=dev)
    best_patch = torch.empty(P, Np, dtype=torch.int32, device=dev)
    appearance = torch.empty(P, dtype=torch.float32, device=dev)
    n_valid = torch.empty(P, dtype=torch.int32, device=dev)
    status = torch.empty(P, dtype=torch.int32, device=dev)
    score = torch.empty(P, dtype=torch.float32, device=dev)
    call("fp_proposal_appearance", ptr(q_n), ptr(q_cover), P, Np, D, ptr(bank_patch_n) if N else None, ptr(bank_cover) if N else None, N, ptr(obj_off), O,
         ptr(best_obj), ptr(best_template), ptr(best_score), int(min_cover), ptr(best_sim), ptr(best_patch), ptr(appearance), ptr(n_valid),
         ptr(status), ptr(score), stream())
    return score, appearance, n_valid, status, best_sim, best_patch


# ---------------------------------------------------------------- COCO average precision of detections
def mask_pack(masks: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp_mask_pack: masks uint8 [N, H, W] (0 / non-zero) -> (words [N, H, Wq] with Wq = ceil(W / 64), the uint64 words as torch.int64: bit
    x % 64 of word (y, x / 64) is pixel (x, y), the bits beyond W are 0; area int32 [N])."""
    _detection_tables("mask_pack", ((masks, torch.uint8),))
    if masks.dim() != 3 or masks.shape[1] < 1 or masks.shape[2] < 1 or int(masks.shape[1]) * int(masks.shape[2]) > 1 << 30:
        raise ValueError(f"mask_pack: masks must be uint8 [N, H, W] with H, W >= 1 and H W <= 2^30, got {tuple(masks.shape)}")
    N, H, W = (int(v) for v in masks.shape)
    words = torch.empty(N, H, (W + 63) // 64, dtype=torch.int64, device=masks.device)
    area = torch.empty(N, dtype=torch.int32, device=masks.device)
    call("fp_mask_pack", ptr(masks), N, H, W, ptr(words), ptr(area), stream())
    return words, area


def _group_tables(name: str, est_off: torch.Tensor, gt_off: torch.Tensor, pair_off: torch.Tensor) -> int:
    _detection_tables(name, ((est_off, torch.int32), (gt_off, torch.int32), (pair_off, torch.int32)))
    NG = int(est_off.shape[0]) - 1
    if est_off.dim() != 1 or NG < 0 or tuple(gt_off.shape) != (NG + 1,) or tuple(pair_off.shape) != (NG + 1,):
        raise ValueError(f"{name}: est_off, gt_off and pair_off must be int32 [NG + 1]")
    return NG


def group_mask_iou(words_a: torch.Tensor, words_b: torch.Tensor, est_off: torch.Tensor, gt_off: torch.Tensor, pair_off: torch.Tensor,
                   num_pairs: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp_group_mask_iou on device tables whose CONTENTS have been validated already (eval_coco.match_groups' callers build them): words_a
    [Na, ...] and words_b [Nb, ...] as mask_pack wrote them (one row length L), est_off / gt_off / pair_off int32 [NG + 1].  -> (counts int32
    [num_pairs, 2] = (intersection, union), overlap f64 [num_pairs], status int32 [num_pairs]: 0 scored, 2 union 0); a row of no group keeps
    (0, 0), 0 and 2."""
    NG = _group_tables("group_mask_iou", est_off, gt_off, pair_off)
    _detection_tables("group_mask_iou", ((words_a, torch.int64), (words_b, torch.int64)))
    if words_a.dim() < 2 or words_b.dim() < 2 or tuple(words_a.shape[1:]) != tuple(words_b.shape[1:]) or num_pairs < 0:
        raise ValueError(f"group_mask_iou: words_a [Na, ...] and words_b [Nb, ...] of one row shape are needed, got {tuple(words_a.shape)} and {tuple(words_b.shape)}")
    L = 1
    for v in words_a.shape[1:]:
        L *= int(v)
    if not 1 <= L <= 1 << 24:
        raise ValueError(f"group_mask_iou: rows of {L} words (1 .. 2^24)")
    dev = words_a.device
    counts = torch.zeros(num_pairs, 2, dtype=torch.int32, device=dev)
    overlap = torch.zeros(num_pairs, dtype=torch.float64, device=dev)
    status = torch.full((num_pairs,), 2, dtype=torch.int32, device=dev)
    tiles = torch.empty(NG + 1, dtype=torch.int32, device=dev)
    call("fp_group_mask_iou", ptr(words_a), int(words_a.shape[0]), ptr(words_b), int(words_b.shape[0]), L, ptr(est_off), ptr(gt_off), ptr(pair_off), NG,
         int(num_pairs), ptr(tiles), ptr(counts), ptr(overlap), ptr(status), stream())
    return counts, overlap, status


def group_box_iou(boxes_a: torch.Tensor, boxes_b: torch.Tensor, est_off: torch.Tensor, gt_off: torch.Tensor, pair_off: torch.Tensor,
                  num_pairs: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp_group_box_iou: boxes_a f64 [Na, 4] and boxes_b f64 [Nb, 4] as COCO's (x, y, w, h), the group tables as above.  -> (overlap f64
    [num_pairs], status int32 [num_pairs]: 0 scored, 2 when the union is not > 0 or no group owns the row)."""
    NG = _group_tables("group_box_iou", est_off, gt_off, pair_off)
    _detection_tables("group_box_iou", ((boxes_a, torch.float64), (boxes_b, torch.float64)))
    if boxes_a.dim() != 2 or boxes_a.shape[1] != 4 or boxes_b.dim() != 2 or boxes_b.shape[1] != 4 or num_pairs < 0:
        raise ValueError(f"group_box_iou: boxes_a [Na, 4] and boxes_b [Nb, 4] are needed, got {tuple(boxes_a.shape)} and {tuple(boxes_b.shape)}")
    overlap = torch.zeros(num_pairs, dtype=torch.float64, device=boxes_a.device)
    status = torch.full((num_pairs,), 2, dtype=torch.int32, device=boxes_a.device)
    call("fp_group_box_iou", ptr(boxes_a), int(boxes_a.shape[0]), ptr(boxes_b), int(boxes_b.shape[0]), ptr(est_off), ptr(gt_off), ptr(pair_off), NG,
         int(num_pairs), ptr(overlap), ptr(status), stream())
    return overlap, status


def coco_match(est_off: torch.Tensor, gt_off: torch.Tensor, pair_off: torch.Tensor, overlap: torch.Tensor, gt_ignore: torch.Tensor,
               ths: torch.Tensor, num_est: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp_coco_match on device tables whose CONTENTS have been validated already (eval_coco.match_groups checks them on the host before it
    uploads them): the group tables, overlap f64 [P] (not read back), gt_ignore int32 [G], ths f64 [T].  -> (flag int8 [num_est, T],
    matched_gt int32 [num_est, T]); an estimate of no group keeps flag 0 and matched_gt -1."""
    NG = _group_tables("coco_match", est_off, gt_off, pair_off)
    _detection_tables("coco_match", ((overlap, torch.float64), (gt_ignore, torch.int32), (ths, torch.float64)))
    if ths.dim() != 1 or not 1 <= int(ths.shape[0]) <= MAX_THS:
        raise ValueError(f"coco_match: ths must be [T] with 1 <= T <= {MAX_THS}, got {tuple(ths.shape)}")
    if overlap.dim() != 1 or gt_ignore.dim() != 1 or num_est < 0:
        raise ValueError("coco_match: table sizes do not match")
    T = int(ths.shape[0])
    flag = torch.zeros(num_est, T, dtype=torch.int8, device=overlap.device)
    matched = torch.full((num_est, T), -1, dtype=torch.int32, device=overlap.device)
    call("fp_coco_match", ptr(est_off), ptr(gt_off), ptr(pair_off), NG, ptr(overlap), int(overlap.shape[0]), ptr(gt_ignore), int(gt_ignore.shape[0]),
         ptr(ths), T, int(num_est), ptr(flag), ptr(matched), stream())
    return flag, matched
