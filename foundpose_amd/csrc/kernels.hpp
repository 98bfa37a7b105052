// Internal launch interfaces between the C ABI (api.cpp) and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/foundpose_amd.h"

// ---------------------------------------------------------------- f32_tile.hip
enum : int {
  F32_EPI_STORE = 0,        // out = acc
  F32_EPI_DIST_STORE = 1,   // out = max(0, fma(-2, acc, |a|^2 + |b|^2))
  F32_EPI_DIST_ARGMIN = 2,  // atomicMin of (d2,idx) keys per row and per column
  F32_EPI_SUB_VEC = 3,      // out = acc - vec[j]          (PCA: X C^T - mu C^T)
  F32_EPI_BIAS = 4,         // out = acc + bias[j]
  F32_EPI_BIAS_GELU = 5,    // out = gelu_erf(acc + bias[j])
  F32_EPI_LS_RESID = 6,     // out += gamma[j] * (acc + bias[j])
  F32_EPI_TOKENS = 7,       // patch-embed scatter into the token sequence (+ pos-embed)
  F32_EPI_SWIGLU = 8,       // columns interleaved (x1_j, x2_j): out[:, j] = silu(acc_2j + b_2j) * (acc_2j+1 + b_2j+1)
  F32_EPI_DIST_TOPK = 9,    // per row the k smallest (d2, column) keys of this tile -> row_best[row, n_tile, k] (k = row_stride <= 8)
};

struct F32TileArgs {
  const float* A; int lda;
  const float* B; int ldb;
  int K, M, N;
  // ragged grouping (device tables, may be null): pair -> segment of A rows / B rows
  const int* a_seg_off; const int* pair_a_seg; int pair_a_div;  // pair_a_div > 0: segment = pair / pair_a_div
  const int* b_seg_off; const int* pair_b_seg;
  const int* pair_b_base;  // may be null; else pair_b_seg values are relative: + pair_b_base[pair / pair_a_div]
  // epilogue operands
  float* out; int ldo; long long out_pair_stride; int out_row_global;  // out_row_global: row index = a_off + i
  const float* a_sqnorm; const float* b_sqnorm;
  unsigned long long* row_best; int row_stride;
  unsigned long long* col_best; int col_stride;
  // DIST_ARGMIN: 0 = atomicMin into row_best[pair * row_stride + row] / col_best[pair * col_stride + col] (tables preset to ~0);
  // 1 = every tile stores its own slice, no atomics, no preset: row_best[(pair * grid.x + tile_n) * row_stride + row] and
  // col_best[(pair * grid.y + tile_m) * col_stride + col]; the reader takes the min over the live tiles
  int best_parts;
  const float* bias; const float* gamma;
  const float* pos; int tok_np, tok_n, tok_skip;
};

int f32_tile_launch(int epi, const F32TileArgs& a, int max_m, int max_n, int pairs, hipStream_t st);

// ---------------------------------------------------------------- match.hip, retrieve.hip
struct CyclicArgs {
  const int* q_off;        // [B+1] query-point segment per detection
  const int* tpl_ids;      // [B*n_slots] template id per (detection, slot); <0 = empty slot; global, or object-local with tpl_base
  const int* tpl_base;     // [B] first template of the detection's object (null: tpl_ids are global)
  const int* tpl_off;      // [T_total+1] feature segment per template
  const int* feat_base;    // [B] first feature row of the detection's object (ids are reported object-local)
  const float* points;     // [sumQ, 2]
  const float* vertices;   // [N_f, 3]
  const unsigned long long* row_best; int row_stride;  // [pairs, row_parts, row_stride] (d2, template patch): per column tile of the template
  const unsigned long long* col_best; int col_stride;  // [pairs, col_parts, col_stride] (d2, query patch): per row tile of the queries
  int row_parts, col_parts;
  int n_slots, top_k, k_max, q_max;
  int tie_mode;            // 0 canonical (value, index); 1 torch.topk's CPU tie order (stl_order.hpp)
  int* out_count;          // [pairs]
  int* out_q_ids;          // [pairs, k_max]
  int* out_feat_ids;       // [pairs, k_max]
  float* out_dists;        // [pairs, k_max]
  float* out_conf;         // [pairs, k_max]
  float* out_coord_2d;     // [pairs, k_max, 2]
  float* out_coord_3d;     // [pairs, k_max, 3]
};

struct SampleArgs {
  const float* fmap; long long stride_img, stride_c, stride_h, stride_w;
  int C, H, W, img_w, img_h;
  const float* points; const int* point_img; int num_points;
  float* out;  // [num_points, C]
};

struct WarpArgs {
  const void* src; int n_src, src_h, src_w, channels, mode;
  const int* src_index; const double* params; int batch, out_h, out_w, depth_check;
  void* out; float* map_out;
};
int launch_warp_crops(const WarpArgs& a, hipStream_t st);

struct WarpDepthArgs {
  const float* src; int src_h, src_w;
  const double* params; const int* recompute; int batch, out_h, out_w, depth_check;
  float* out;
};
int launch_warp_depth(const WarpDepthArgs& a, hipStream_t st);

// ---------------------------------------------------------------- render.hip
struct RenderArgs {
  const float* verts; const float* normals; const float* colors; int num_verts;
  const int* faces; int num_faces;
  const double* cams; int batch, width, height;
  void* vert_ws; void* tri_ws; int* tile_counts; long long* tile_offsets; int* lists; long long* status;
  float* color; float* depth; unsigned char* mask; int* tri_id; int* boxes;
};
struct TexArgs {                  // a textured model (fp_render_raster_textured); zero for the vertex-coloured raster
  const float* uv;                 // [num_verts, 2]
  const unsigned* texels;          // packed RGBA8 pyramid (fp_texture_mips)
  int levels;                      // level l: texels [off[l], off[l] + w[l] h[l])
  int off[FP_TEXTURE_MAX_LEVELS], w[FP_TEXTURE_MAX_LEVELS], h[FP_TEXTURE_MAX_LEVELS];
  float metallic, roughness, factor[3];
  int srgb;
};
int launch_render_setup(const RenderArgs& a, hipStream_t st);
int launch_render_raster(const RenderArgs& a, hipStream_t st);
int launch_render_raster_textured(const RenderArgs& a, const TexArgs& t, hipStream_t st);
int launch_texture_mips(const unsigned char* rgb, const TexArgs& t, unsigned* pyramid, hipStream_t st);

struct DownsampleArgs {
  const float* color; const float* depth; const unsigned char* mask; int batch, out_h, out_w, factor;
  unsigned char* rgb; unsigned short* depth_u16; unsigned char* mask_out; int* boxes;
};
int launch_template_downsample(const DownsampleArgs& a, hipStream_t st);

int launch_sqnorm_rows(const float* x, long long n, int d, int ld, float* out, hipStream_t st);
int launch_normalize_rows(const float* x, long long n, int d, float eps, float* out, hipStream_t st);
int launch_topk_rows(const float* vals, int rows, int n, int ld, const int* row_len, int k, int largest,
                     float* out_val, int* out_idx, hipStream_t st);
int launch_tfidf_build(const int* word_ids, const float* word_d2, int knn_k, const int* seg_off, int num_segs,
                       const float* idf, int num_words, int soft, float sigma_sq, int sqrt_dists,
                       float* desc, float* desc_n, float eps, hipStream_t st);
int launch_cyclic_select(const CyclicArgs& a, int num_pairs, hipStream_t st);
int launch_sample_bilinear(const SampleArgs& a, hipStream_t st);
int launch_sqrt_inplace(float* x, long long n, hipStream_t st);

// ---------------------------------------------------------------- gemm_kernel.hpp (one gemm_*.hip per operand format)
enum : int {
  GEMM_EPI_BIAS_BF16 = 0,     // out(bf16) = acc + bias
  GEMM_EPI_GELU_BF16 = 1,     // out(bf16) = gelu_erf(acc + bias)
  GEMM_EPI_LS_RESID_F32 = 3,  // out(f32) += gamma * (acc + bias)      (LayerScale + residual)
  GEMM_EPI_TOKENS_F32 = 4,    // patch-embed rows scattered into the token sequence (+ bias + pos-embed)
  GEMM_EPI_BIAS_F32 = 5,      // out(f32) = acc + bias
  GEMM_EPI_RESID_F32 = 7,     // out(f32) += acc + bias (LayerScale already folded into W and bias) + the LayerNorm-fold outputs (xb, stats)
  GEMM_EPI_SWIGLU_BF16 = 6,   // SwiGLU FFN: columns interleaved (x1_j, x2_j) -> out(bf16)[:, j] = silu(x1_j) * x2_j, [M, N/2]
  GEMM_EPI_RESID_HILO = 8,    // as RESID_F32 with the residual stream held as TWO bf16 arrays: x = xb (hi) + xl (lo); reads both, adds acc + bias,
                              // writes hi' = bf16(x'), lo' = bf16(x' - hi') and the LayerNorm row sums -- no fp32 stream, no separate bf16 copy
};

struct GemmBf16Args {
  const __bf16* A; int lda;   // [M, K] activations (M padded to 128)
  const __bf16* W; int ldw;   // [N, K] weights (torch Linear layout)
  int M, N, K, M_valid;
  const float* bias;          // [N] or null
  const float* gamma;         // [N] LayerScale
  void* out; int ldo;
  const float* pos;           // [Np, ldo] fp32 pos-embed rows of the patch tokens
  int tok_np, tok_n, tok_skip;  // patches / tokens per image, first patch token index (1 + registers)
  int tile_override;          // 0 = auto, 64 (x 128) / 128 / 256 / 320 / 352 (BIAS, GELU, RESID_HILO) = force that block tile (benchmarks, tests)
  int m_tiles;                // set by the launcher: row tiles that hold live rows (tiles of padding rows only are not launched)
  unsigned rast_r, rast_gn;
  float out_scale;            // fp8 kernels: > 0 -> the GELU / SwiGLU result leaves as e4m3(value * out_scale) bytes; f16x3: scale of a split-fp16 output
  float acc_scale;            // f16x3 kernels: out = epi(acc * acc_scale + bias), acc_scale = 1 / (scale of A x scale of W)
  unsigned long long* dbg;    // optional [grid, 4] shader-clock stamps: start, prologue done, main loop done, epilogue drained
  // ---- LayerNorm folded into the GEMMs around it (bf16 ViT blocks, vit forward only):
  // producer (LS_RESID): besides the fp32 residual stream it writes xb = bf16(x) -- the next GEMM's A operand -- and per
  // row the partial sums (sum x, sum x^2) of every 128-column group into stats[(column / 128) * M + row]
  __bf16* xb; int ld_xb;
  __bf16* xl;                 // RESID_HILO: the low halves of the stream (row stride ld_xb), read and written next to xb
  float2* stats_out;
  // consumer (BIAS / GELU / SwiGLU epilogues; W carries the LayerNorm gain, bias the LayerNorm shift):
  //   out = epi(rstd_r * (acc - mean_r * colsum_n) + bias_n);  ln_stats [M] = (rstd_r, mean_r * rstd_r) from ln_finalize_launch
  const float2* ln_stats; int ln_parts; float ln_eps;
  const float* colsum;        // [N] fp32 sums of the rows of W
  int* sat;                   // may be null; else [2] sticky saturation counters (common.hpp report_saturation): the split-fp16 / e4m3 epilogues report clamped outputs
};

// The operand format of a GEMM; A and W (and the 16-bit outputs) sit behind the __bf16 pointers whatever it is.
enum class GemmFmt {
  BF16,
  // IEEE fp16 operands and fp16 outputs (out of the 16-bit epilogues, xb / xl of the residual epilogues): the "f16" mode; v_mfma_f32_32x32x16_f16, the
  // nine-coefficient GELU polynomial; an fp16 output beyond +-65504 becomes inf (no report here: see common.hpp)
  F16,
  FP8,  // OCP fp8 e4m3 bytes
  // A [M, 2K] and W [N, 2K] split-fp16 rows (common.hpp), a.K = the logical K (multiple of 32), lda / ldw in halves: the f16x3 mode;
  // out = epi(acc * a.acc_scale + bias); the BIAS / GELU (exact erf) / SwiGLU epilogues write split-fp16 rows again ([M, 2N] halves, values
  // scaled by a.out_scale), LS_RESID / TOKENS / BIAS_F32 write fp32
  F16X3,
  // the same with A and W as f16f8 rows (common.hpp; K a multiple of 64): hi*hi on the fp16 MFMA, the two cross terms on the fp8 MFMA; the
  // GELU / SwiGLU outputs are f16f8 rows, the BIAS output (q | k | v) stays a split-fp16 row for the attention kernel
  F16F8,
};
template <GemmFmt FMT> int gemm_launch_fmt(int epi, const GemmBf16Args& a, hipStream_t st);   // instantiated by the format's gemm_*.hip
int gemm_resid_tile_rows(int m_valid, int n, int cus);   // (gemm_bf16.hip) block-tile height the launcher picks for a RESID_HILO launch that fills the chip: 256 or 352
int gemm_wide_tile_rows(int m, int m_valid, int n, int cus);   // (gemm_bf16.hip) ... and for a BIAS / GELU launch (qkv, fc1) of m padded rows: 256, 320 or 352
int gemm_launch(GemmFmt fmt, int epi, const GemmBf16Args& a, hipStream_t st);   // (api.cpp) the one entry point: gemm_launch_fmt<fmt>

// ---------------------------------------------------------------- dtypes of the C ABI
enum : int { FP_DTYPE_F32 = 0, FP_DTYPE_BF16 = 1, FP_DTYPE_FP8 = 2, FP_DTYPE_F16X3 = 3, FP_DTYPE_F16F8 = 4,   // F16F8: common.hpp "f16f8 rows"
             FP_DTYPE_F16 = 5 };   // plain IEEE fp16 rows: the "f16" mode = the bf16 pipeline (same kernels, same bytes) on fp16 operands

// ---------------------------------------------------------------- attn.hip
struct AttnArgs {
  const void* qkv; int ld_qkv;   // [B*N, 3D] (bf16 or f32): q | k | v column blocks, head-major inside
  void* out; int ld_out;         // [B*N, D]
  int batch, n_tok, dim, heads;
  float out_fp8_scale;           // bf16 kernel: > 0 -> the output leaves as e4m3(o * scale) bytes (ld_out in bytes)
  // query selection (bf16, 64-queries-per-wave kernel; null = every token is a query): image b attends with the tokens
  // sel_rows[sel_off[b] .. sel_off[b+1]) (global rows b * n_tok + token, ascending) over ALL its keys, and output row r of
  // the compact [num_sel, D] result belongs to sel_rows[r]
  const int* sel_rows; const int* sel_off; int max_sel;  // max_sel >= the largest per-image count (sizes the grid)
  // bf16 work split (bit-identical outputs): 0 = 64 queries per wave, K/V by LDS-DMA (default); 1 = 32 queries per wave, register
  // staging (the cross-check)
  int variant;
  int tail_last;                 // set by the launcher (bf16 w64 kernel): the last (short) query tile of every (image, head) pair goes to the END of its XCD's block sequence
  float in_scale, out_scale;     // f16x3 kernel: power-of-two scale the split-fp16 q / k / v rows carry, and the one the output row gets
  int out_fmt;                   // f16x3 kernel: 0 = the output is a split-fp16 row, 1 = an f16f8 row (common.hpp; the f16f8 mode's proj operand)
  int* sat;                      // may be null; else [2] sticky saturation counters: the e4m3 output of the bf16 kernel reports clamps; the split-fp16
                                 // output (a convex combination of v rows that already fit their scale) cannot clamp and reports non-finite values only
};
int attn_launch(const AttnArgs& a, int dtype, hipStream_t st);

// ---------------------------------------------------------------- vit.hip
struct LayerNormArgs {
  const float* x; int ld_x;      // fp32 residual stream
  const float* weight; const float* bias; float eps;
  void* out; int ld_out; int out_dtype;   // FP_DTYPE_FP8: e4m3(y * out_scale) bytes, ld_out in bytes (dim % 256 == 0)
  float out_scale;
  int dim;
  int out_rows;                  // rows to produce
  int out_rows_per_img, in_rows_per_img, in_skip;  // out row r -> in row (r / orpi) * irpi + in_skip + r % orpi
  int* sat;                      // may be null; else [2] sticky saturation counters: split-fp16 / e4m3 outputs report clamps, an fp32 output reports
                                 // non-finite values (the final norm of the "f16" mode)
};
int layernorm_launch(const LayerNormArgs& a, hipStream_t st);
int ln_sample_launch(const float* x, int ld_x, const float* weight, const float* bias, float eps, int apply_norm, int dim, int ntok, int skip,
                     int gh, int gw, int img_w, int img_h, const float* points, const int* point_img, int num_points, float* out, hipStream_t st,
                     const int* row_map = nullptr, int* sat = nullptr);   // sat: non-finite features are counted into sat[0] (the "f16" mode's overflow report)
int gather_rows_launch(const float* x, const int* rows, int n, int dim, float* out, hipStream_t st);
int query_select_launch(const unsigned char* masks, int B, int H, int W, const int* pix_x, const int* pix_y, const float* grid_pts, int G,
                        const long long* cells9, int C, int n_tok, int* scratch, int* counts, float* out_pts, int* out_img, int* q_off, int* sel_rows,
                        int* sel_off, int* row_map, hipStream_t st);
// x [rows, dim] fp32 -> xb = bf16(x) [rows, ld_xb] and stats[0 * stats_stride + row] = (sum x, sum x^2), slots 1..parts-1 zero
// partial sums [parts][rows] (sum x, sum x^2) over `dim` columns -> out[row] = (rstd, mean * rstd)
int ln_finalize_launch(const float2* partial, int parts, int stride, int rows, int dim, float eps, float2* out, hipStream_t st);
int rowstats_cast_launch(const float* x, int rows, int dim, void* xb, int ld_xb, float2* stats, int stats_stride, int parts, hipStream_t st,
                         void* xl = nullptr, bool h16 = false);   // xl: also write lo = bf16(x - bf16(x)) (row stride ld_xb); h16: fp16 instead of bf16
// out[r] = float(xb[row]) + float(xl[row]) (fp32 [n, dim]); row = rows[r], or r when rows is null: the (hi, lo) stream back as fp32
int hilo_rows_launch(const void* xb, const void* xl, int ld, const int* rows, int n, int dim, float* out, hipStream_t st, bool h16 = false);

int patchify_launch(const float* images, int batch, int height, int width, int patch, void* out, int ld_out,
                    int out_dtype, hipStream_t st, float out_scale = 1.f);  // out_scale: FP_DTYPE_F16X3 rows only
int patchify_strided_launch(const float* images, int batch, int height, int width, int patch, int stride, void* out, int ld_out, int out_dtype,
                            hipStream_t st, float out_scale = 1.f);
int prefix_tokens_launch(const float* prefix, int n_prefix, int dim, float* tokens, int batch, int n_tok, hipStream_t st);
int convert_f32_to_bf16_launch(const float* in, void* out, long long n, hipStream_t st);
int quantize_fp8_launch(const void* in, int in_dtype, long long n, float scale, void* out, hipStream_t st);
int launch_knn_merge(const unsigned long long* cand, int rows, int ncand, int k, float* out_d2, int* out_idx, hipStream_t st);
int launch_pack_records(const int* tpl_ids, const float* scores, const int* counts, const int* q_ids, const int* feat_ids, const float* dists, const float* conf,
                        const float* c2d, const float* c3d, int num_det, int n, int K, float* out, hipStream_t st);
int launch_unpack_best(const unsigned long long* best, long long n, float* d2, int* idx, hipStream_t st);

struct CosineArgs {
  const float* desc_n;  // [num_det, W] normalised query descriptors, grouped by object
  const float* bank_n;  // [T_total, W] normalised template descriptors
  const int* det_seg_off;  // [num_obj + 1]
  const int* obj_tpl_off;  // [num_obj + 1]
  int W;
  float* sims; int ld_sims;  // [num_det, ld_sims] finished scores
  int k_slices;              // set by the launcher: 8 when W % 128 == 0, else 1 (canonical chain split)
  unsigned long long* cand;  // [num_det, grid.x, n_top] candidate keys of the fused kernel (null: not wanted)
  int n_top;                 // candidates per (workgroup, detection): the caller's n_top, + 1 in the torch tie order
  int* need_replay;          // [num_det] torch tie order: 1 = the row has a tie among its best n_top + 1 scores
  const void* bank_bf16;     // [T_total, W] bf16 copy of bank_n (prefiltered retrieval only)
  int force_prefilter;       // prefiltered retrieval: take the two-stage form whatever the size (tests, measurements)
  const int* run_flag;       // may be null; else the kernel runs only if *run_flag != 0 (exact fallback of the prefiltered retrieval)
};
int launch_cosine_topk(const CosineArgs& a, int num_det, int num_obj, int max_det_per_obj, int max_templates, int n_top,
                       const int* det_num_templates, float* out_scores, int* out_ids, int tie_mode, hipStream_t st);
int launch_cosine_topk_prefiltered(const CosineArgs& a, int num_det, int num_obj, int max_det_per_obj, int max_templates, int n_top,
                                   const int* det_num_templates, float* out_scores, int* out_ids, int tie_mode, float* extra_scratch, hipStream_t st);
int launch_topn_rows(const float* sims, int ld, int rows, int max_len, const int* row_len, int n_top, float* out_scores,
                     int* out_ids, int tie_mode, hipStream_t st, const int* need_replay = nullptr);

// ---------------------------------------------------------------- pose_eval.hip
struct PoseErrHyp {        // one hypothesis, built on the host by fp_pose_errors
  int pt_off, pt_cnt;      // vertex range in pts
  int sym_off, sym_cnt;    // symmetry range in gt_sym / p_gt
  int tiles, pad;          // ceil(pt_cnt / FP_POSE_ERR_TILE)
  long long part_base;     // first partial of the hypothesis: partials [tiles, sym_cnt]
};
struct PoseErrPart { double sd, pd; int vsd, vpd; };  // per (hypothesis, tile, symmetry): max squared distances + first argmax
struct PoseErrArgs {
  const double* pts; const double* est; const double* p_est; const double* gt_sym; const double* p_gt;
  const PoseErrHyp* hyps;  // [num_hyp] device copy
  PoseErrPart* parts;
  double* err; int* idx;
};
int launch_pose_errors(const PoseErrArgs& a, int num_hyp, int max_tiles, int max_syms, hipStream_t st);

// ---------------------------------------------------------------- pose_add.hip
struct PoseAddPair {       // one (estimate, GT) pair, built on the host by fp_pose_add_errors
  int pt_off, pt_cnt;      // point range in pts
  int tiles, pad;          // ceil(pt_cnt / FP_POSE_ADD_TILE)
  long long part_base;     // first tile partial of the pair: partials [tiles] of (sum_a, sum_n)
  long long pad2;
};
struct PoseAddArgs {
  const double* pts; const double* est; const double* gt;
  const PoseAddPair* pairs;  // [num_pairs] device copy
  double* parts;             // [total tiles, 2]
  double* err;               // [num_pairs, 2] (add, adi)
  int total_pts;
};
int launch_pose_add_errors(const PoseAddArgs& a, int num_pairs, int max_blocks, hipStream_t st);

// ---------------------------------------------------------------- point_extremes.hip
struct PtsPart { double v; int a, b; };  // a workgroup's maximum (a squared distance) and the index / index pair it came from
struct PtsDiameterArgs {
  const double* pts; int V;
  int tiles;               // ceil(V / FP_PTS_TILE); tile pairs a <= b: tiles (tiles + 1) / 2 workgroups and partials
  PtsPart* parts;
  double* out_d; int* out_pair;
};
struct PtsHausdorffArgs {
  const double* pts; int V;
  int stride, nq;          // queries v = 0, stride, ...: nq = ceil(V / stride) of them
  const double* tf;        // [K, 12]
  PtsPart* parts;          // [K, ceil(nq / FP_PTS_TILE)]
  double* out_h; int* out_arg;
};
int launch_pts_diameter(const PtsDiameterArgs& a, hipStream_t st);
int launch_pts_hausdorff(const PtsHausdorffArgs& a, int K, hipStream_t st);

// ---------------------------------------------------------------- refine.hip, depth_refine.hip, rgbd_refine.hip (shared parts: refine_terms.hpp)
struct RefineState {       // Levenberg-Marquardt state of one detection (scratch, FP_REFINE_STATE_BYTES)
  double R[9], t[3];       // current pose
  double Rt[9], tt[3];     // trial pose (the next pass evaluates it)
  double H[21], g[6];      // system at the current pose
  double E, E_in, lam, sigma2;
  int p0, np;              // bank rows [p0, p0 + np)
  int it, active, pending, accepted, skipped, nvalid;
};
struct RgbdState {         // scratch, FP_REFINE_STATE_BYTES: the shared LM state (H, g, E are those of the mixed objective) and the depth decision
  RefineState s;
  int ninl, use_depth;     // depth inliers at the input pose; whether the depth term takes part (depth_weight > 0 and ninl >= 6)
};
struct RefineLmArgs {      // what every refiner has: the camera the pose lives in, the input poses, the bank rows, the outputs, the scratch
  const double* cam; const double* R_in; const double* t_in;
  const int32_t* row_begin; const int32_t* row_end; const float* verts; long long num_rows;
  const int32_t* has_pose; int num_det, max_points, iters, chunks;
  double* R_out; double* t_out; double* cost_in; double* cost_out; int32_t* num_points; int32_t* iters_used; int32_t* status;
  double* normal_eq;       // [num_det, 28] (rgbd: 57) or null
  double* part; int32_t* err;
};
struct RefineMapArgs {     // the feature term: the map, its camera's image size, the points' features, the points valid for the term
  const float* map; long long sb, sy, sx, sc; int gh, gw, C, pad0; double W, H;
  const float* feats; uint8_t* valid;
};
struct RefineDepthArgs {   // the depth term
  const float* depth; int num_images, H, W, pad0; const int32_t* image_index;   // [num_images, H, W] mm, 0 = no measurement
  const double* tau;
};
struct RefineArgs { RefineLmArgs lm; RefineMapArgs f; RefineState* state; };
int launch_featuremetric_refine(const RefineArgs& a, hipStream_t st);
struct DepthRefineArgs { RefineLmArgs lm; RefineDepthArgs d; RefineState* state; };
int launch_depth_refine(const DepthRefineArgs& a, hipStream_t st);
struct RgbdRefineArgs {    // features and depth in one objective; lm.cam is the frame camera
  RefineLmArgs lm; RefineMapArgs f; RefineDepthArgs d;
  const double* fcam;      // [num_det, 4] the feature camera
  const double* A; const double* a;    // [num_det, 9], [num_det, 3]: X_f = A X_c + a, frame camera -> feature camera
  double wd; int32_t* num_depth_inliers;
  RgbdState* state;
};
int launch_rgbd_refine(const RgbdRefineArgs& a, hipStream_t st);

// ---------------------------------------------------------------- vsd.hip
struct VsdPair {                         // one (estimate, GT) pair, built on the host by fp_vsd_counts
  long long test_off, est_off, gt_off;   // element offsets of the three depth images (index * height * width)
  int x0, y0, bw, bh;                    // the box scanned: bw x bh pixels from (x0, y0); 0 x 0 when empty
  long long blk0;                        // first workgroup of the pair: ceil(bw * bh / FP_VSD_BLOCK_PIXELS) of them
  double fx, fy, cx, cy, diameter;
  float delta;                           // (float)delta: numpy compares the fp32 difference in fp32
  int pad;
};
struct VsdArgs {
  const float* depth_test; const float* depth_est; const float* depth_gt;
  const VsdPair* pairs;                  // [num_pairs] device copy
  int num_pairs, width, num_taus, pad;
  double taus[FP_VSD_MAX_TAUS];
  long long* counts;                     // [num_pairs, 2 + num_taus], zeroed by the host on the stream
};
int launch_vsd_counts(const VsdArgs& a, long long num_blocks, hipStream_t st);

// ---------------------------------------------------------------- gt_info.hip
struct GtVisInst {                       // one GT instance, built on the host by fp_gt_visibility
  long long test_off;                    // element offset of the frame's depth image (index * height * width)
  long long blk0;                        // first workgroup of the instance: ceil(bw * bh / FP_GT_VIS_BLOCK_PIXELS) of them
  int x0, y0, bw, bh;                    // the box scanned, in render coordinates: bw x bh pixels from (x0, y0); 0 x 0 when empty
  int ox, oy;                            // where the image starts inside the render
  double fx, fy, cx, cy;                 // of the image
  float delta;                           // (float)delta: numpy compares the fp32 difference in fp32
  int pad;
};
struct GtVisArgs {
  const float* depth_test;               // [num_test, height, width]
  const float* depth_obj;                // [num_inst, render_h, render_w]
  const GtVisInst* inst;                 // [num_inst] device copy
  int num_inst, height, width, render_h, render_w, pad;
  int* out;                              // [num_inst, 11], initialised by gt_vis_init_kernel
  uint8_t* mask; uint8_t* mask_visib;    // [num_inst, height, width], zeroed by the host on the stream
};
int launch_gt_visibility(const GtVisArgs& a, long long num_blocks, hipStream_t st);

// ---------------------------------------------------------------- tsdf.hip
struct TsdfVolume { double ox, oy, oz, h; int nx, ny, nz, pad; };   // voxel (i, j, k) is centred at origin + ((i, j, k) + 0.5) h; x fastest
struct TsdfFrame { double fx, fy, cx, cy, R[9], t[3]; };            // one frame's camera and model -> camera pose (FP_TSDF_FRAME_DOUBLES doubles)
struct TsdfIntegrateArgs {
  TsdfVolume vol;
  const float* depth; const uint8_t* mask; const uint8_t* rgb;      // [num_frames, height, width (, 3)]
  const TsdfFrame* frames;                                          // [num_frames] device copy
  int num_frames, height, width, pad;
  double tau;
  float* sdf_sum; int* sdf_cnt; float* rgb_sum; int* rgb_cnt;       // rgb_sum: 3 planes
};
struct TsdfExtractArgs {
  TsdfVolume vol;
  const float* sdf_sum; const int* sdf_cnt; const float* rgb_sum; const int* rgb_cnt;
  int min_count, pad;
  int* counts;                                                      // count: [cells]
  const long long* offsets; long long num_triangles;                // emit: [cells], and the length of the outputs
  long long* keys; float* pos; float* col;                          // emit: [3 T], [3 T, 3], [3 T, 3]
};
int launch_tsdf_integrate(const TsdfIntegrateArgs& a, hipStream_t st);
int launch_tsdf_extract(const TsdfExtractArgs& a, bool emit, hipStream_t st);

// ---------------------------------------------------------------- tsdf_fill.hip
struct TsdfDiffuseArgs {                                            // one Jacobi iteration: (val, state) -> (val_out, state_out)
  const float* val; const uint8_t* state;                           // [channels, nz, ny, nx], [nz, ny, nx]: 0 UNKNOWN, 1 FIXED, 2 FREE
  float* val_out; uint8_t* state_out;
  int channels, nx, ny, nz;
};
int launch_tsdf_diffuse(const TsdfDiffuseArgs& a, hipStream_t st);

// ---------------------------------------------------------------- simplify.hip
struct MeshGrid { double ox, oy, oz, c; int nx, ny, nz, pad; };     // cell (i, j, k) spans origin + (i, j, k) c .. + c; x fastest
struct MeshKeysArgs {
  MeshGrid grid;
  const float* verts; long long num_vertices;                       // [V, 3]
  long long* keys;                                                  // [V]
};
struct MeshClusterArgs {
  MeshGrid grid;
  const float* verts; const float* colors; long long num_vertices;  // [V, 3] each
  const int* faces; long long num_faces;                            // [F, 3]
  const long long* cell_keys; long long num_cells;                  // [C]
  const long long* vert_order; const long long* vert_begin;         // [V], [C + 1]
  const long long* corner_order; const long long* corner_begin;     // [3 F], [C + 1]
  double eig_eps;
  float* pos; float* col; double* quadrics; double* means; double* err; int* status;   // [C, 3], [C, 3], [C, 10], [C, 3], [C], [C]
};
int launch_mesh_cell_keys(const MeshKeysArgs& a, hipStream_t st);
int launch_mesh_cluster(const MeshClusterArgs& a, hipStream_t st);

// ---------------------------------------------------------------- tsdf_track.hip (the LM parts: refine_terms.hpp)
struct TsdfTrackArgs {     // lm.verts are the camera-frame points, lm.cam is not used
  RefineLmArgs lm;
  TsdfVolume vol;
  const float* sdf_sum; const int* sdf_cnt;
  int min_count, pad;
  double tau;              // trunc_mm: r = tau phi
  const double* max_dist;  // [num_det] the inlier distance (mm)
  RefineState* state;
};
struct TsdfTrackRgbArgs {  // fp_tsdf_track_rgb: the geometric arguments as they stand, and what the colour term reads (section 31)
  TsdfTrackArgs g;
  const float* rgb_sum; const int* rgb_cnt;   // rgb_sum: 3 planes
  const float* colors;     // [num_rows, 3], row-aligned with lm.verts
  double color_weight;     // lambda: mm per unit of colour
  double color_max;        // the channel inlier bound
};
int launch_tsdf_track(const TsdfTrackArgs& a, hipStream_t st);
int launch_tsdf_track_rgb(const TsdfTrackRgbArgs& a, hipStream_t st);

// ---------------------------------------------------------------- multiview.hip (the LM parts: refine_terms.hpp)
struct MultiviewArgs {     // fp_multiview_refine (section 37): lm.verts are the rows' model points, lm.cam is not used; the pose is model -> world
  RefineLmArgs lm;
  const double* target;    // [num_rows, 2] the pixel (u*, v*) a row's point should project to in its view
  const int32_t* view;     // [num_rows] the row's view: an index into the two tables below
  const double* view_cam;  // [num_views, 4] fx, fy, cx, cy
  const double* view_T;    // [num_views, 12] R_v row-major | t_v, world -> camera
  int num_views, pad;
  double delta;            // huber_px
  RefineState* state;
};
int launch_multiview_refine(const MultiviewArgs& a, hipStream_t st);

// ---------------------------------------------------------------- mask_refine.hip (the LM parts: refine_terms.hpp)
struct MaskDistanceArgs { const uint8_t* masks; int32_t* d2; int B, H, W; };   // fp_mask_distance (section 38)
int launch_mask_distance(const MaskDistanceArgs& a, hipStream_t st);
struct MaskRefineState {   // scratch, FP_REFINE_STATE_BYTES: the shared LM state and the detection's contour rows [k0, k0 + nk)
  RefineState s;
  int k0, nk;
};
struct MaskRefineArgs {    // fp_mask_refine (section 38): lm.cam is the frame camera, lm.part / lm.chunks the forward records
  RefineLmArgs lm;
  const int32_t* d2; int H, W;          // [num_det, H, W] squared distances to the detection's mask
  const int32_t* contour;               // [num_contour, 2] (x, y)
  const int32_t* cbegin; const int32_t* cend; long long num_contour;
  int max_contour, bchunks;             // the cap of a detection's contour rows; ceil(max_contour / FP_REFINE_CHUNK)
  double delta;                         // huber_px
  double* bpart;                        // [num_det, bchunks, FP_REFINE_RECORD] the backward records
  double* pu; double* pv; int32_t* pf;  // [num_det, max_points] a point's projection and whether it is in front, at the trial pose
  MaskRefineState* state;
};
int launch_mask_refine(const MaskRefineArgs& a, hipStream_t st);

// ---------------------------------------------------------------- depth_proposals.hip
struct DpFrame {                        // one frame, built on the host by fp_depth_plane_fit / fp_depth_components
  double fx, fy, cx, cy;
  unsigned long long key;                // the sampler's frame key (plane fit only)
  float slope_fx;                        // connect_slope / fx (components only)
  int pad;
};
struct DpPlaneArgs {
  const float* depth;                    // [n, h, w]
  const DpFrame* frames;                 // [n] device copy
  const double* prior;                   // [n, FP_DEPTH_MAX_PLANES, 4]
  const int* num_prior;                  // [n]
  int n, h, w, hyp, stride, chunks;
  double thresh, max_depth, min_share;
  unsigned long long seed;
  unsigned char* elig;                   // [n, h w]
  int* cnt2;                             // [n, 2] valid, eligible; zeroed by the host on the stream
  int* hyp_cnt;                          // [n, hyp]
  double* state;                         // [n, 16]
  double* part;                          // [n, chunks, 8]
  double* plane_out;                     // [n, 4]
  int* info;                             // [n, 8]
};
int launch_depth_plane_fit(const DpPlaneArgs& a, hipStream_t st);
struct DpCompArgs {
  const float* depth;                    // [n, h, w]
  const DpFrame* frames;                 // [n] device copy
  const double* planes;                  // [n, FP_DEPTH_MAX_PLANES, 4]
  const int* num_planes;                 // [n]
  int n, h, w;
  float connect_mm;
  double max_depth, margin;
  int* parent;                           // [n, h w] scratch
  int* labels;                           // [n, h, w]
};
int launch_depth_components(const DpCompArgs& a, hipStream_t st);
struct DpTableArgs {
  const int* labels;                     // [n, h, w]
  const int* finer;                      // [num_finer, n, max_prop, 7] tables of finer levels, or NULL
  int n, h, w, min_pixels, max_area, max_prop, level, num_finer;
  int* slots;                            // [n, h w, 6] scratch
  int* cand;                             // [n, h w] scratch
  int* ncand;                            // [n] scratch
  int* table;                            // [n, max_prop, 7]
  int* counts;                           // [n, 4]
  int* rank_map;                         // [n, h, w]
};
int launch_component_table(const DpTableArgs& a, hipStream_t st);
struct DpRunsArgs {
  const int* rank_map;                   // [m, h, w]
  const int* num_kept;                   // [m]
  int m, h, w, max_prop;
  long long capacity;
  long long* events;                     // [capacity]
  int* count;                            // [1], zeroed by the host on the stream
};
int launch_component_runs(const DpRunsArgs& a, hipStream_t st);

// ---------------------------------------------------------------- vis.hip
int launch_vis_mask_tint(const uint8_t* img, const uint8_t* mask, long long pixels, uint8_t* out, hipStream_t st);
int launch_vis_contour(const uint8_t* mask, int batch, int h, int w, int dil, int r, int g, int b, uint8_t* img, hipStream_t st);
int launch_vis_scene_composite(const float* depth, const uint8_t* colours, int layers, int h, int w, const uint8_t* img, uint8_t* out,
                               int* ids, hipStream_t st);
int launch_vis_resize_area(const uint8_t* src, int batch, int h, int w, int oh, int ow, uint8_t* out, hipStream_t st);
int launch_vis_pca_colorize(const float* map, int batch, int gh, int gw, int C, int h, int w, int num, int den, float* range, uint8_t* out,
                            hipStream_t st);
int launch_vis_draw_matches(const float* segs, const int* counts, int batch, int max_matches, int h, int w, const float* colour, float alpha,
                            float lw, float radius, uint8_t* tile, hipStream_t st);

// ---------------------------------------------------------------- pnp.hip
struct PnpArgs {
  const float* coord_2d;   // [pairs, k_max, 2] pixels
  const float* coord_3d;   // [pairs, k_max, 3] model space
  const int* counts;       // [pairs] valid correspondences per pair
  const double* cam;       // [pairs / n_slots, 4] fx, fy, cx, cy of each detection's (crop) camera
  int n_slots, k_max, iters, lm_iters, min_corresp;
  double thresh, conf;
  unsigned long long seed;
  const unsigned long long* pair_keys;  // [pairs] sampler key of each pair, or null: the pair's index in the launch
  int* success;            // [pairs]
  double* R;               // [pairs, 9] row-major model -> camera
  double* t;               // [pairs, 3]
  int* n_inliers;          // [pairs] RANSAC inliers of the winning model (= the reference's `quality`)
  unsigned char* inlier_mask;  // [pairs, k_max]
  double* ransac_pose;     // [pairs, 12] the winning model before refinement (R | t), may be null
};
int launch_pnp_ransac(const PnpArgs& a, int num_pairs, hipStream_t st);

// ---------------------------------------------------------------- kabsch.hip
struct KabschArgs {
  const float* coord_2d;   // [pairs, k_max, 2] pixels in the solve camera
  const float* coord_3d;   // [pairs, k_max, 3] model space (mm)
  const int* counts;       // [pairs] correspondences per pair (clamped to [0, k_max])
  const double* cam;       // [dets, 4] fx, fy, cx, cy of each detection's solve camera (dets = pairs / n_slots)
  const double* frame_cam; // [dets, 4] ... of its frame's camera
  const double* A;         // [dets, 9] row-major rotation solve camera -> frame camera
  const int* image_index;  // [dets] the detection's image in `depth`
  const double* tau;       // [dets] inlier threshold (mm)
  const float* depth;      // [num_images, H, W] mm, 0 = no measurement
  int num_images, H, W;
  int n_slots, k_max, iters, refit, min_corresp;
  double conf;
  unsigned long long seed;
  const unsigned long long* pair_keys;  // [pairs] sampler key of each pair, or null: the pair's index in the launch
  int* success;            // [pairs] 1, 0 (no pose), -1 (image index outside the stack / threshold not positive: nothing read)
  double* R;               // [pairs, 9] row-major model -> solve camera
  double* t;               // [pairs, 3]
  int* n_inliers;          // [pairs] inliers of the winning hypothesis
  int* num_valid;          // [pairs] correspondences with a depth measurement
  unsigned char* inlier_mask;  // [pairs, k_max]
  double* ransac_pose;     // [pairs, 12] the winning hypothesis before the refit (R | t), may be null
};
int launch_kabsch_ransac(const KabschArgs& a, int num_pairs, hipStream_t st);

// ---------------------------------------------------------------- verify.hip
struct VerifyArgs {
  const int* success;      // [pairs] > 0: the pair has a pose
  const double* R;         // [pairs, 9] row-major model -> solve camera
  const double* t;         // [pairs, 3]
  const double* cam;       // [dets, 4] fx, fy, cx, cy of each detection's frame camera (dets = pairs / n_slots)
  const double* A;         // [dets, 9] row-major rotation solve camera -> frame camera
  const int* image_index;  // [dets] the detection's image in `depth`
  const double* tau;       // [dets] tolerance (mm)
  const int* ranges;       // [dets, 2] the detection's object in `points`: [begin, end), clamped to [0, m_total]
  const double* center;    // [dets, 3] centre of the object's sample
  const double* radius;    // [dets] its radius about that centre
  const float* points;     // [m_total, 3] the compact samples of all objects
  int m_total;
  const float* depth;      // [num_images, H, W] mm, 0 = no measurement
  int num_images, H, W;
  int n_slots, grid, min_visible;
  int* counts;             // [pairs, 6] n_vis, n_in, n_occ, n_free, n_hole, n_out
  double* score;           // [pairs] n_in / n_vis, 0 below min_visible
  int* status;             // [pairs] 0 scored, 1 too few visible points, 2 skipped, -1 bad image index / tolerance (nothing read)
};
int launch_pose_verify_depth(const VerifyArgs& a, int num_pairs, hipStream_t st);

// ---------------------------------------------------------------- mask_verify.hip
struct MaskVerifyArgs {
  const int* success;      // [pairs] > 0: the pair has a pose
  const double* R;         // [pairs, 9] row-major model -> solve camera
  const double* t;         // [pairs, 3]
  const double* cam;       // [dets, 4] fx, fy, cx, cy of each detection's frame camera (dets = pairs / n_slots)
  const double* A;         // [dets, 9] row-major rotation solve camera -> frame camera
  const int* ranges;       // [dets, 2] the detection's object in `points`: [begin, end), clamped to [0, m_total]
  const double* center;    // [dets, 3] centre of the object's sample
  const double* radius;    // [dets] its radius about that centre
  const float* points;     // [m_total, 3] the compact samples of all objects
  int m_total;
  const unsigned char* masks;  // [dets, H, W] each detection's mask in the frame camera's image, non-zero = set
  const int* area;         // [dets] the number of set pixels of the detection's mask
  int H, W;
  int n_slots, grid, min_pixels;
  int* counts;             // [pairs, 4] n_both, n_model_only, n_mask_only, n_cells
  double* score;           // [pairs] n_both / (n_both + n_model_only + n_mask_only), 0 below min_pixels model pixels
  int* status;             // [pairs] 0 scored, 1 too few model pixels, 2 skipped
};
int launch_pose_verify_mask(const MaskVerifyArgs& a, int num_pairs, hipStream_t st);

// ---------------------------------------------------------------- det_masks.hip
constexpr int DM_TILE_W = 64, DM_TILE_H = 16;  // one workgroup per tile of the output image
struct DetMaskArgs {
  const int* counts;       // [num_runs] the concatenated run lengths of the detections
  const int* run_off;      // [num_det + 1] where each detection's runs start (clamped to [0, num_runs] by the kernels)
  int num_runs;
  int hc, wc;              // the detector's canvas
  int H, W;                // the image, centre-cropped out of the canvas
  int* prefix;             // [num_runs] scratch: the inclusive prefix sums of each detection's runs
  unsigned char* masks;    // [num_det, H, W] 0 / 1
  int* area;               // [num_det] set pixels of each mask
  int tiles_x, tiles_y;    // filled in by the launcher
};
int launch_detection_masks(DetMaskArgs a, int num_det, int open3x3, hipStream_t st);

// ---------------------------------------------------------------- pose_nms.hip
constexpr int PN_MIN_GRID = 8, PN_MAX_GRID = 32;  // the side of the occupancy grid: at most 32^3 bits = 4 KB of LDS
constexpr int PN_MAX_GROUP = 256;                 // poses of one frame: one thread each
struct PoseOverlapArgs {
  const float* points;     // [m_total, 3] the compact samples of all objects
  int m_total;
  const int* ranges;       // [objects, 2] each object in `points`: [begin, end), clamped to [0, m_total]
  const double* center;    // [objects, 3] centre of the object's sample
  const double* radius;    // [objects] its radius about that centre
  int n_objects;
  const int* pose_obj;     // [poses] the pose's object
  const int* valid;        // [poses] > 0: the pose takes part
  const double* R;         // [poses, 9] row-major model -> the frame's common coordinates
  const double* t;         // [poses, 3]
  int n_poses;
  const int* pairs;        // [pairs, 2] (i, j): how much of i's sample lies in j's occupied cells
  int grid;
  int* counts;             // [pairs, 2] n_in, n_cells
  double* overlap;         // [pairs] n_in / n_i
  int* status;             // [pairs] 0 scored, 1 disjoint spheres, 2 skipped
};
int launch_pose_overlap(const PoseOverlapArgs& a, int num_pairs, hipStream_t st);

struct PoseNmsArgs {
  const int* group_off;    // [groups + 1] the poses of each frame, in rank order
  const int* pair_off;     // [groups + 1] the pairs of each frame
  const int* pairs;        // [n_pairs, 2] pose indices
  const double* overlap;   // [n_pairs]
  const int* status;       // [n_pairs] 0: the overlap counts
  double thresh;
  int n_poses, n_pairs;
  int* keep;               // [n_poses] 1 kept, 0 suppressed
  int* suppressed_by;      // [n_poses] the pose that suppressed it, or -1
};
int launch_pose_nms_greedy(const PoseNmsArgs& a, int num_groups, hipStream_t st);

// ---------------------------------------------------------------- detection_ap.hip
constexpr int DA_THREADS = 256;        // a workgroup of the AP kernel: one (object, column)
constexpr int DA_MAX_GROUP_GT = 256;   // GT instances of one (image, object): 4 per lane
constexpr int DA_MAX_THS = 16;         // thresholds per error type
constexpr int DA_MAX_REC = 128;        // recall thresholds: one thread each
struct GroupTables {       // groups of rows of a (estimates, in rank order) and of b (GT instances): csrc/group_parts.hpp reads them
  const int* est_off;      // [groups + 1] each group's rows of a
  const int* gt_off;       // [groups + 1] its rows of b
  const int* pair_off;     // [groups + 1] its rows of the pair tables: E_g x G_g, row-major
  int n_groups, n_a, n_b, n_pairs;
};
struct DetMatchArgs {
  GroupTables t;           // n_a = estimates, n_b = GT instances
  const double* err;       // [n_pairs, 2] (mssd, mspd), what fp_pose_errors wrote
  const int* gt_valid;     // [n_b] > 0: a valid GT
  const int* group_tab;    // [groups] the group's row of ths
  const double* ths;       // [n_tab, 2, T]
  int n_tab, T;
  signed char* flag;       // [n_a, 2 T] 1 true positive, 0 false positive, 2 ignored
  int* matched_gt;         // [n_a, 2 T] the group-local GT index or -1
};
int launch_detection_match(const DetMatchArgs& a, hipStream_t st);

struct DetApArgs {
  const int* obj_off;      // [objects + 1] each object's stretch of order
  const int* order;        // [n_order] rows of flag, per object in global rank order
  const signed char* flag; // [n_est, 2 T]
  const int* n_valid;      // [objects] valid GT instances over all target images
  const double* rec_thr;   // [R]
  int n_order, n_est, T, R;
  double* ap;              // [objects, 2 T]
  double* q;               // [objects, 2 T, R] the interpolated precision at each recall threshold
  int* totals;             // [objects, 2 T, 3] tp, fp, ignored
};
int launch_detection_ap(const DetApArgs& a, int num_objects, hipStream_t st);

// ---------------------------------------------------------------- coco_eval.hip
constexpr int CE_THREADS = 256;                 // a workgroup of the packing and of the overlap kernels
#ifndef FP_COCO_TILE_A                          // (tools/bench_coco.py times a 1 x 1 build beside this one: tools/build_variant.sh ... -DFP_COCO_TILE_A=1 -DFP_COCO_TILE_B=1)
#define FP_COCO_TILE_A 4
#endif
#ifndef FP_COCO_TILE_B
#define FP_COCO_TILE_B 4
#endif
constexpr int CE_TILE_A = FP_COCO_TILE_A, CE_TILE_B = FP_COCO_TILE_B;  // rows of a x rows of b whose words one workgroup holds in registers
struct MaskPackArgs {
  const unsigned char* masks;  // [N, H, W] 0 / non-zero
  int H, W, Wq;                // Wq = ceil(W / 64), filled in by the entry point
  unsigned long long* words;   // [N, H, Wq] bit x % 64 of word (y, x / 64) = pixel (x, y)
  int* area;                   // [N] set pixels
};
int launch_mask_pack(const MaskPackArgs& a, int num_masks, hipStream_t st);

struct GroupMaskIouArgs {
  GroupTables t;
  const unsigned long long* words_a;  // [n_a, L]
  const unsigned long long* words_b;  // [n_b, L]
  int L;
  int* tile_off;               // [groups + 1] scratch: where each group's tiles start
  int* counts;                 // [n_pairs, 2] intersection, union
  double* overlap;             // [n_pairs]
  int* status;                 // [n_pairs] 0 scored, 2 union 0
};
int launch_group_mask_iou(const GroupMaskIouArgs& a, hipStream_t st);

struct GroupBoxIouArgs {
  GroupTables t;
  const double* boxes_a;       // [n_a, 4] x, y, w, h
  const double* boxes_b;       // [n_b, 4]
  double* overlap;             // [n_pairs]
  int* status;                 // [n_pairs] 0 scored, 2 union not > 0 or a row of no group
};
int launch_group_box_iou(const GroupBoxIouArgs& a, hipStream_t st);

struct CocoMatchArgs {
  GroupTables t;               // n_a = estimates, n_b = GT instances
  const double* overlap;       // [n_pairs] as either overlap kernel wrote it
  const int* gt_ignore;        // [n_b] != 0: an ignored instance
  const double* ths;           // [T]
  int T;
  signed char* flag;           // [n_a, T] 1 matched non-ignored, 2 matched ignored, 0 unmatched
  int* matched_gt;             // [n_a, T] the group-local GT index or -1
};
int launch_coco_match(const CocoMatchArgs& a, hipStream_t st);

// ---------------------------------------------------------------- proposals.hip
constexpr int PC_MAX_SIZE = 1024;      // the crop's side: the axis tables and three rows of it fit the 64 KiB of a workgroup's LDS
constexpr int PS_MAX_K = 16;           // similarities averaged per (proposal, object)
struct MaskBoxArgs {
  const unsigned char* masks;  // [P, H, W] 0 / non-zero
  int H, W;
  int* box;                // [P, 4] x1, y1, x2, y2 (x2, y2 exclusive); all 0 for an empty mask
  int* area;               // [P] set pixels
};
int launch_mask_boxes(const MaskBoxArgs& a, int num_prop, hipStream_t st);

struct ProposalCropArgs {
  const float* images;     // [n_img, H, W, 3] HWC
  const unsigned char* masks;  // [P, H, W]
  const int* image_index;  // [P] or null: proposal p reads image p
  const int* boxes;        // [P, 4] as mask_boxes writes them
  int n_img, H, W, S;
  float* out;              // [P, 3, S, S] CHW, every element written
  int* status;             // [P] 0 cropped, 2 empty box / box outside the image / image_index outside its table (all-zero crop)
  int band_rows, chunk_rows;  // filled in by the launcher: output rows per workgroup, source rows per pass through LDS
};
int launch_proposal_crops(ProposalCropArgs a, int num_prop, hipStream_t st);

struct ProposalScoreArgs {
  const float* desc_n;     // [P, D]
  const int* obj_off;      // [O + 1] over the N bank rows, as the caller gave it
  int P, D, N, O, k, max_templates;
  float* rep;              // [O, P, D] scratch: the descriptors, once per object
  int* seg_off;            // [O + 1] scratch: o P
  int* tpl_off;            // [O + 1] scratch: obj_off clamped into the bank and to max_templates rows per object
  int* det_nt;             // [O P] scratch: the template count of each listed row's object
  const float* top_val;    // [O P, k] what the retrieval wrote: the best k similarities, best first, ties to the lower template
  const int* top_idx;      // [O P, k] their object-local template ids
  float* scores;           // [P, O]
  int* best_obj;           // [P]
  float* best_score;       // [P]
  int* best_template;      // [P]
};
int launch_proposal_prep(const ProposalScoreArgs& a, hipStream_t st);
int launch_proposal_aggregate(const ProposalScoreArgs& a, hipStream_t st);

constexpr int PR_MAX_PROPOSALS = 4096, PR_MAX_OBJECTS = 4096;  // of one image: one workgroup ranks them
enum { PR_CANDIDATE = 0, PR_SMALL = 1, PR_EMPTY = 2, PR_NO_OBJECT = 3, PR_LOW_SCORE = 4, PR_GROUP_LIMIT = 5 };  // FP_PROPOSAL_* of the header
struct ProposalRankArgs {
  const int* best_obj;     // [P] as proposal_scores wrote it
  const float* best_score; // [P]
  const int* area;         // [P] as mask_boxes wrote it
  const int* crop_status;  // [P] as proposal_crops wrote it
  const int* boxes;        // [P, 4]
  int P, O, min_area, max_group, max_pairs;
  float min_score;
  int* decision;           // [P] PR_*
  int* order;              // [P] the proposal at each place of the layout, -1 behind the last candidate
  int* group_off;          // [O + 1] the places of each object's candidates, in rank order
  int* pair_off;           // [O + 1] the pairs of each object
  int* pairs;              // [max_pairs, 2] places (a, b), a < b; (-1, -1) behind the last pair
  int* boxes_ranked;       // [P, 4] the boxes in layout order, zeros behind the last candidate
};
int launch_proposal_rank(const ProposalRankArgs& a, hipStream_t st);

struct BoxIouArgs {
  const int* boxes;        // [n_boxes, 4] x1, y1, x2, y2 (x2, y2 exclusive)
  const int* pairs;        // [n_pairs, 2] box indices
  int n_boxes, n_pairs;
  double* overlap;         // [n_pairs] intersection / union
  int* status;             // [n_pairs] 0 scored, 2 union 0 or an index outside the table
};
int launch_box_iou(const BoxIouArgs& a, hipStream_t st);

// the appearance score of a proposal
struct PatchCoverArgs {
  const unsigned char* masks;  // [P, H, W]
  const int* image_index;  // [P] or null: only its range is checked, as proposal_crops checks it
  const int* boxes;        // [P, 4] as mask_boxes writes them
  int n_img, H, W, S, ps;
  int* cover;              // [P, (S / ps)^2] covered pixels of every patch cell, row-major; every element written
};
int launch_proposal_patch_cover(const PatchCoverArgs& a, int num_prop, hipStream_t st);

constexpr int PA_MAX_DIM = 4096, PA_MAX_PATCHES = 8192;
struct ProposalAppearanceArgs {
  const float* q;          // [P, Np, D] rows from normalize_rows
  const int* q_cover;      // [P, Np]
  const float* bank;       // [N, Np, D]
  const int* bank_cover;   // [N, Np]
  const int* obj_off;      // [O + 1] over the N bank rows, as the caller gave it
  const int* best_obj;     // [P] as proposal_scores wrote them
  const int* best_template;
  const float* best_score;
  int P, Np, D, N, O, min_cover;
  float* best_sim;         // [P, Np] (0, -1) for an invalid query patch and for every patch of a row whose status is not 0
  int* best_patch;         // [P, Np]
  float* appearance;       // [P]
  int* n_valid;            // [P]
  int* status;             // [P] 0 scored, 1 no valid query patch, 2 no template row, 3 no valid template patch
  float* score;            // [P] (best_score + appearance) * 0.5f
};
int launch_proposal_appearance(const ProposalAppearanceArgs& a, hipStream_t st);
