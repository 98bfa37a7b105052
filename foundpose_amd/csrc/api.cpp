// C ABI of libfoundpose_amd.so (declared in include/foundpose_amd.h): argument checking, scratch carving
// and kernel sequencing.  No device allocation, no global mutable state, no synchronisation except the table uploads of
// fp_pose_errors, fp_vsd_counts, fp_gt_visibility, fp_depth_plane_fit, fp_depth_components and fp_tsdf_integrate (each waits for its own copy) and the range check read back by the five Levenberg-Marquardt solvers (fp_featuremetric_refine, fp_depth_refine, fp_rgbd_refine, fp_tsdf_track and its colour sibling fp_tsdf_track_rgb, fp_multiview_refine).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

#include "../../include/foundpose_amd.h"
#include "../../include/foundpose_amd_multiview.h"
#include "../../include/foundpose_amd_mask_refine.h"
#include "common.hpp"
#include "kernels.hpp"

static thread_local char g_err[512] = "";

void fp_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

#define ST(s) reinterpret_cast<hipStream_t>(s)
#define TRY(expr)              \
  do {                         \
    int rc__ = (expr);         \
    if (rc__ != FP_OK) return rc__; \
  } while (0)
#define HIP_TRY(expr, what)                                             \
  do {                                                                  \
    hipError_t e__ = (expr);                                            \
    if (e__ != hipSuccess) {                                            \
      fp_set_error("%s: %s", what, hipGetErrorString(e__));             \
      return FP_ERR_HIP;                                                \
    }                                                                   \
  } while (0)

static F32TileArgs zero_tile_args() {
  F32TileArgs a;
  memset(&a, 0, sizeof(a));
  return a;
}

int gemm_launch(GemmFmt fmt, int epi, const GemmBf16Args& a, hipStream_t st) {
  switch (fmt) {
    case GemmFmt::BF16: return gemm_launch_fmt<GemmFmt::BF16>(epi, a, st);
    case GemmFmt::F16: return gemm_launch_fmt<GemmFmt::F16>(epi, a, st);
    case GemmFmt::FP8: return gemm_launch_fmt<GemmFmt::FP8>(epi, a, st);
    case GemmFmt::F16X3: return gemm_launch_fmt<GemmFmt::F16X3>(epi, a, st);
    case GemmFmt::F16F8: return gemm_launch_fmt<GemmFmt::F16F8>(epi, a, st);
  }
  fp_set_error("gemm: unknown operand format %d", (int)fmt);
  return FP_ERR_INVALID;
}

extern "C" {

int fp_abi_version(void) { return FP_ABI_VERSION; }
const char* fp_last_error(void) { return g_err; }

// ------------------------------------------------------------------ matching half
int fp_sqnorm_rows(const float* x, int64_t n, int d, float* out, fp_stream_t stream) {
  FP_REQUIRE(n == 0 || (x && out), "fp_sqnorm_rows: null pointer");   // (an empty tensor has no storage: null is what it hands over)
  return launch_sqnorm_rows(x, n, d, d, out, ST(stream));
}

int fp_normalize_rows(const float* x, int64_t n, int d, float eps, float* out, fp_stream_t stream) {
  FP_REQUIRE(n == 0 || (x && out), "fp_normalize_rows: null pointer");
  return launch_normalize_rows(x, n, d, eps, out, ST(stream));
}

int fp_knn_l2(const float* q, const float* q_sqnorm, int m, const float* db, const float* db_sqnorm, int n, int d,
              int k, void* scratch, float* out_d2, int32_t* out_idx, fp_stream_t stream) {
  FP_REQUIRE(q && q_sqnorm && db && db_sqnorm && scratch && out_idx, "fp_knn_l2: null pointer");
  FP_REQUIRE(k >= 1 && n >= 1 && d >= 4, "fp_knn_l2: bad sizes (n=%d d=%d k=%d)", n, d, k);
  if (m == 0) return FP_OK;
  F32TileArgs a = zero_tile_args();
  a.A = q; a.lda = d; a.B = db; a.ldb = d; a.K = d; a.M = m; a.N = n;
  a.a_sqnorm = q_sqnorm; a.b_sqnorm = db_sqnorm;
  if (k == 1) {
    unsigned long long* best = reinterpret_cast<unsigned long long*>(scratch);
    HIP_TRY(hipMemsetAsync(best, 0xFF, (size_t)m * 8, ST(stream)), "fp_knn_l2: memset");
    a.row_best = best; a.row_stride = 0; a.col_best = nullptr;
    TRY(f32_tile_launch(F32_EPI_DIST_ARGMIN, a, m, n, 1, ST(stream)));
    return launch_unpack_best(best, m, out_d2, out_idx, ST(stream));
  }
  FP_REQUIRE(out_d2, "fp_knn_l2: out_d2 is required for k > 1");
  if (k <= 8) {  // fused: every distance tile emits its k best per row, a merge over the n-tiles finishes the row
    const int nt = (n + 127) / 128;
    a.row_best = reinterpret_cast<unsigned long long*>(scratch); a.row_stride = k;
    TRY(f32_tile_launch(F32_EPI_DIST_TOPK, a, m, n, 1, ST(stream)));
    return launch_knn_merge(a.row_best, m, nt * k, k, out_d2, out_idx, ST(stream));
  }
  float* dist = reinterpret_cast<float*>(scratch);
  a.out = dist; a.ldo = n;
  TRY(f32_tile_launch(F32_EPI_DIST_STORE, a, m, n, 1, ST(stream)));
  return launch_topk_rows(dist, m, n, n, nullptr, k, 0, out_d2, out_idx, ST(stream));
}

int fp_tfidf_build(const int32_t* word_ids, const float* word_d2, int knn_k, const int32_t* seg_off, int num_segs,
                   const float* idf, int num_words, int soft_assign, float soft_sigma_squared, int sqrt_dists,
                   float* desc, float* desc_n, float eps, fp_stream_t stream) {
  FP_REQUIRE(word_ids && word_d2 && seg_off && idf && desc, "fp_tfidf_build: null pointer");
  return launch_tfidf_build(word_ids, word_d2, knn_k, seg_off, num_segs, idf, num_words, soft_assign,
                            soft_sigma_squared, sqrt_dists, desc, desc_n, eps, ST(stream));
}

// What both cosine entries pass to the kernels, and the one place that carves FP_COSINE_SCRATCH_FLOATS(num_det, max_templates) floats: the scores
// [num_det, max_templates], the candidate keys (8 bytes each, hence the pad to an even float offset), and in the macro's last num_det floats one
// replay flag per detection.
static CosineArgs cosine_args(const float* desc_n, const int32_t* det_seg_off, const float* bank_n, const int32_t* obj_tpl_off, int num_det,
                              int max_templates, int num_words, float* scratch) {
  CosineArgs c;
  memset(&c, 0, sizeof(c));
  c.desc_n = desc_n; c.bank_n = bank_n; c.det_seg_off = det_seg_off; c.obj_tpl_off = obj_tpl_off; c.W = num_words;
  c.sims = scratch; c.ld_sims = max_templates;
  const size_t scores = (size_t)num_det * max_templates;
  c.cand = reinterpret_cast<unsigned long long*>(scratch + scores + (scores & 1));
  c.need_replay = reinterpret_cast<int*>(scratch + FP_COSINE_SCRATCH_FLOATS(num_det, max_templates) - (size_t)num_det);
  return c;
}
static_assert(FP_COSINE_SCRATCH_FLOATS(3, 5) - 3 == 2 * 3 * 5 + 16 * 3 + 2, "the replay flags start 2 * scores + 16 * num_det + 2 floats into the cosine scratch");

int fp_cosine_topk(const float* desc_n, const int32_t* det_seg_off, const int32_t* det_num_templates, int num_det,
                   int max_det_per_obj, const float* bank_n, const int32_t* obj_tpl_off, int num_obj,
                   int max_templates, int num_words, int n_top, float* scratch_sims, float* out_scores,
                   int32_t* out_ids, int tie_mode, fp_stream_t stream) {
  FP_REQUIRE(desc_n && det_seg_off && det_num_templates && bank_n && obj_tpl_off && scratch_sims && out_scores && out_ids,
             "fp_cosine_topk: null pointer");
  FP_REQUIRE(num_obj >= 1 && max_templates >= 1 && n_top >= 1, "fp_cosine_topk: bad sizes");
  if (num_det == 0) return FP_OK;
  FP_REQUIRE(tie_mode == 0 || tie_mode == 1, "fp_cosine_topk: tie_mode must be 0 (canonical) or 1 (torch)");
  if (num_words % 16 == 0) {
    // one arithmetic (8 k-slice chains when num_words % 128 == 0) whatever the batch: a score never depends on how many
    // detections share the launch; > 32 detections of an object are served in 32-detection chunks by the same kernel
    const CosineArgs c = cosine_args(desc_n, det_seg_off, bank_n, obj_tpl_off, num_det, max_templates, num_words, scratch_sims);
    return launch_cosine_topk(c, num_det, num_obj, max_det_per_obj, max_templates, n_top, det_num_templates, out_scores,
                              out_ids, tie_mode, ST(stream));
  }
  // descriptor sizes that are not a multiple of 16 words: generic fp32 tile, k-ascending chains
  F32TileArgs a = zero_tile_args();
  a.A = desc_n; a.lda = num_words; a.B = bank_n; a.ldb = num_words; a.K = num_words;
  a.a_seg_off = det_seg_off; a.b_seg_off = obj_tpl_off;
  a.out = scratch_sims; a.ldo = max_templates; a.out_row_global = 1;
  TRY(f32_tile_launch(F32_EPI_STORE, a, max_det_per_obj, max_templates, num_obj, ST(stream)));
  return launch_topn_rows(scratch_sims, max_templates, num_det, max_templates, det_num_templates, n_top, out_scores, out_ids, tie_mode, ST(stream));
}

int fp_cosine_topk_prefiltered(const float* desc_n, const int32_t* det_seg_off, const int32_t* det_num_templates, int num_det, int max_det_per_obj,
                               const float* bank_n, const void* bank_n_bf16, const int32_t* obj_tpl_off, int num_obj, int max_templates, int num_words,
                               int n_top, float* scratch, float* out_scores, int32_t* out_ids, int tie_mode, fp_stream_t stream) {
  FP_REQUIRE(desc_n && det_seg_off && det_num_templates && bank_n && bank_n_bf16 && obj_tpl_off && scratch && out_scores && out_ids,
             "fp_cosine_topk_prefiltered: null pointer");
  FP_REQUIRE(num_obj >= 1 && max_templates >= 1 && n_top >= 1, "fp_cosine_topk_prefiltered: bad sizes");
  if (num_det == 0) return FP_OK;
  const int force = (tie_mode >> 8) & 1;  // FP_COSINE_FORCE_PREFILTER: the two-stage form whatever the size (tests, measurements)
  tie_mode &= 0xff;
  FP_REQUIRE(tie_mode == 0 || tie_mode == 1, "fp_cosine_topk_prefiltered: tie_mode must be 0 (canonical) or 1 (torch)");
  if (num_words % 16 != 0)  // the generic exact path
    return fp_cosine_topk(desc_n, det_seg_off, det_num_templates, num_det, max_det_per_obj, bank_n, obj_tpl_off, num_obj, max_templates, num_words, n_top,
                          scratch, out_scores, out_ids, tie_mode, stream);
  CosineArgs c = cosine_args(desc_n, det_seg_off, bank_n, obj_tpl_off, num_det, max_templates, num_words, scratch);
  c.force_prefilter = force;
  c.bank_bf16 = bank_n_bf16;
  float* extra = scratch + FP_COSINE_SCRATCH_FLOATS(num_det, max_templates) + (FP_COSINE_SCRATCH_FLOATS(num_det, max_templates) & 1);
  return launch_cosine_topk_prefiltered(c, num_det, num_obj, max_det_per_obj, max_templates, n_top, det_num_templates, out_scores, out_ids, tie_mode, extra,
                                        ST(stream));
}

int fp_cyclic_buddies(const float* query_feats, const float* query_sqnorm, const float* query_points,
                      const int32_t* q_off, int num_det, int q_max, const float* bank_feats,
                      const float* bank_sqnorm, const int32_t* tpl_off, int p_max, const float* vertices,
                      const int32_t* tpl_ids, const int32_t* tpl_base, const int32_t* feat_base, int n_slots, int d, int top_k, int k_max,
                      void* scratch, int32_t* out_count, int32_t* out_q_ids, int32_t* out_feat_ids,
                      float* out_dists, float* out_conf, float* out_coord_2d, float* out_coord_3d, int tie_mode,
                      fp_stream_t stream) {
  FP_REQUIRE(query_feats && query_sqnorm && query_points && q_off && bank_feats && bank_sqnorm && tpl_off && vertices &&
                 tpl_ids && feat_base && scratch && out_count && out_q_ids && out_feat_ids && out_dists && out_conf &&
                 out_coord_2d && out_coord_3d,
             "fp_cyclic_buddies: null pointer");
  FP_REQUIRE(q_max >= 1 && p_max >= 1 && n_slots >= 1, "fp_cyclic_buddies: bad sizes");
  const int pairs = num_det * n_slots;
  if (pairs == 0) return FP_OK;
  CyclicArgs c;
  memset(&c, 0, sizeof(c));
  // partial nearest-neighbour tables, one slice per distance tile (no atomics, no preset): [pairs, col tiles, q_max] + [pairs, row tiles, p_max]
  const int row_parts = (p_max + 127) / 128, col_parts = (q_max + 127) / 128;
  unsigned long long* row_best = reinterpret_cast<unsigned long long*>(scratch);
  unsigned long long* col_best = row_best + (size_t)pairs * row_parts * q_max;
  F32TileArgs a = zero_tile_args();
  a.A = query_feats; a.lda = d; a.B = bank_feats; a.ldb = d; a.K = d;
  a.a_seg_off = q_off; a.pair_a_div = n_slots;
  a.b_seg_off = tpl_off; a.pair_b_seg = tpl_ids; a.pair_b_base = tpl_base;
  a.a_sqnorm = query_sqnorm; a.b_sqnorm = bank_sqnorm;
  a.row_best = row_best; a.row_stride = q_max; a.col_best = col_best; a.col_stride = p_max; a.best_parts = 1;
  TRY(f32_tile_launch(F32_EPI_DIST_ARGMIN, a, q_max, p_max, pairs, ST(stream)));
  c.row_best = row_best; c.row_stride = q_max; c.col_best = col_best; c.col_stride = p_max;
  c.row_parts = row_parts; c.col_parts = col_parts;
  c.q_off = q_off; c.tpl_ids = tpl_ids; c.tpl_base = tpl_base; c.tpl_off = tpl_off; c.feat_base = feat_base;
  c.points = query_points; c.vertices = vertices;
  c.n_slots = n_slots; c.top_k = top_k; c.k_max = k_max; c.q_max = q_max; c.tie_mode = tie_mode;
  c.out_count = out_count; c.out_q_ids = out_q_ids; c.out_feat_ids = out_feat_ids; c.out_dists = out_dists;
  c.out_conf = out_conf; c.out_coord_2d = out_coord_2d; c.out_coord_3d = out_coord_3d;
  return launch_cyclic_select(c, pairs, ST(stream));
}

int fp_pack_records(const int32_t* template_ids, const float* template_scores, const int32_t* counts, const int32_t* q_ids, const int32_t* feat_ids,
                    const float* dists, const float* conf, const float* coord_2d, const float* coord_3d, int num_det, int n_slots, int k_max, float* out,
                    fp_stream_t stream) {
  FP_REQUIRE(template_ids && template_scores && counts && q_ids && feat_ids && dists && conf && coord_2d && coord_3d && out, "fp_pack_records: null pointer");
  FP_REQUIRE(num_det >= 0 && n_slots >= 1 && k_max >= 1, "fp_pack_records: bad sizes");
  return launch_pack_records(template_ids, template_scores, counts, q_ids, feat_ids, dists, conf, coord_2d, coord_3d, num_det, n_slots, k_max, out, ST(stream));
}

int fp_sample_bilinear(const float* fmap, int64_t stride_img, int64_t stride_c, int64_t stride_h, int64_t stride_w,
                       int C, int H, int W, int img_w, int img_h, const float* points, const int32_t* point_img,
                       int num_points, float* out, fp_stream_t stream) {
  FP_REQUIRE(num_points == 0 || (fmap && points && out), "fp_sample_bilinear: null pointer");
  SampleArgs a;
  a.fmap = fmap; a.stride_img = stride_img; a.stride_c = stride_c; a.stride_h = stride_h; a.stride_w = stride_w;
  a.C = C; a.H = H; a.W = W; a.img_w = img_w; a.img_h = img_h;
  a.points = points; a.point_img = point_img; a.num_points = num_points; a.out = out;
  return launch_sample_bilinear(a, ST(stream));
}

int fp_pca_project(const float* x, int n, int D, const float* components, int d, const float* mean_proj, float* out,
                   fp_stream_t stream) {
  FP_REQUIRE(n == 0 || (x && components && out), "fp_pca_project: null pointer");
  if (n == 0) return FP_OK;
  F32TileArgs a = zero_tile_args();
  a.A = x; a.lda = D; a.B = components; a.ldb = D; a.K = D; a.M = n; a.N = d;
  a.out = out; a.ldo = d; a.bias = mean_proj;
  return f32_tile_launch(mean_proj ? F32_EPI_SUB_VEC : F32_EPI_STORE, a, n, d, 1, ST(stream));
}

static int pnp_ransac_entry(const char* who, const float* coord_2d, const float* coord_3d, const int32_t* counts, const double* cameras,
                            const uint64_t* pair_keys, int num_pairs, int n_slots, int k_max, int ransac_iters, double inlier_thresh, double confidence,
                            int lm_iters, int min_corresp, uint64_t seed, int32_t* out_success, double* out_R, double* out_t, int32_t* out_num_inliers,
                            uint8_t* out_inlier_mask, double* out_ransac_pose, fp_stream_t stream) {
  FP_REQUIRE(coord_2d && coord_3d && counts && cameras && out_success && out_R && out_t && out_num_inliers && out_inlier_mask,
             "%s: null pointer", who);
  FP_REQUIRE(num_pairs >= 0 && n_slots >= 1 && num_pairs % n_slots == 0, "%s: num_pairs must be a multiple of n_slots", who);
  PnpArgs a;
  memset(&a, 0, sizeof(a));
  a.coord_2d = coord_2d; a.coord_3d = coord_3d; a.counts = counts; a.cam = cameras;
  a.n_slots = n_slots; a.k_max = k_max; a.iters = ransac_iters; a.lm_iters = lm_iters; a.min_corresp = min_corresp;
  a.thresh = inlier_thresh; a.conf = confidence; a.seed = seed;
  a.pair_keys = reinterpret_cast<const unsigned long long*>(pair_keys);
  a.success = out_success; a.R = out_R; a.t = out_t; a.n_inliers = out_num_inliers; a.inlier_mask = out_inlier_mask;
  a.ransac_pose = out_ransac_pose;
  return launch_pnp_ransac(a, num_pairs, ST(stream));
}

int fp_pnp_ransac(const float* coord_2d, const float* coord_3d, const int32_t* counts, const double* cameras, int num_pairs, int n_slots,
                  int k_max, int ransac_iters, double inlier_thresh, double confidence, int lm_iters, int min_corresp, uint64_t seed,
                  int32_t* out_success, double* out_R, double* out_t, int32_t* out_num_inliers, uint8_t* out_inlier_mask,
                  double* out_ransac_pose, fp_stream_t stream) {
  return pnp_ransac_entry("fp_pnp_ransac", coord_2d, coord_3d, counts, cameras, nullptr, num_pairs, n_slots, k_max, ransac_iters, inlier_thresh,
                          confidence, lm_iters, min_corresp, seed, out_success, out_R, out_t, out_num_inliers, out_inlier_mask, out_ransac_pose, stream);
}

int fp_pnp_ransac_keyed(const float* coord_2d, const float* coord_3d, const int32_t* counts, const double* cameras, const uint64_t* pair_keys,
                        int num_pairs, int n_slots, int k_max, int ransac_iters, double inlier_thresh, double confidence, int lm_iters,
                        int min_corresp, uint64_t seed, int32_t* out_success, double* out_R, double* out_t, int32_t* out_num_inliers,
                        uint8_t* out_inlier_mask, double* out_ransac_pose, fp_stream_t stream) {
  FP_REQUIRE(pair_keys, "fp_pnp_ransac_keyed: null pair_keys");
  return pnp_ransac_entry("fp_pnp_ransac_keyed", coord_2d, coord_3d, counts, cameras, pair_keys, num_pairs, n_slots, k_max, ransac_iters, inlier_thresh,
                          confidence, lm_iters, min_corresp, seed, out_success, out_R, out_t, out_num_inliers, out_inlier_mask, out_ransac_pose, stream);
}

int fp_kabsch_ransac(const float* coord_2d, const float* coord_3d, const int32_t* counts, const double* solve_cameras, const double* frame_cameras,
                     const double* A, const int32_t* image_index, const double* inlier_thresh_mm, const float* depth, int num_images, int H, int W,
                     const uint64_t* pair_keys, int num_pairs, int n_slots, int k_max, int ransac_iters, double confidence, int refit,
                     int min_corresp, uint64_t seed, int32_t* out_success, double* out_R, double* out_t, int32_t* out_num_inliers,
                     int32_t* out_num_valid, uint8_t* out_inlier_mask, double* out_ransac_pose, fp_stream_t stream) {
  FP_REQUIRE(coord_2d && coord_3d && counts && solve_cameras && frame_cameras && A && image_index && inlier_thresh_mm && depth && out_success &&
             out_R && out_t && out_num_inliers && out_num_valid && out_inlier_mask, "fp_kabsch_ransac: null pointer");
  FP_REQUIRE(num_pairs >= 0 && n_slots >= 1 && num_pairs % n_slots == 0, "fp_kabsch_ransac: num_pairs must be a multiple of n_slots");
  KabschArgs a;
  memset(&a, 0, sizeof(a));
  a.coord_2d = coord_2d; a.coord_3d = coord_3d; a.counts = counts; a.cam = solve_cameras; a.frame_cam = frame_cameras; a.A = A;
  a.image_index = image_index; a.tau = inlier_thresh_mm; a.depth = depth; a.num_images = num_images; a.H = H; a.W = W;
  a.n_slots = n_slots; a.k_max = k_max; a.iters = ransac_iters; a.refit = refit ? 1 : 0; a.min_corresp = min_corresp;
  a.conf = confidence; a.seed = seed;
  a.pair_keys = reinterpret_cast<const unsigned long long*>(pair_keys);
  a.success = out_success; a.R = out_R; a.t = out_t; a.n_inliers = out_num_inliers; a.num_valid = out_num_valid;
  a.inlier_mask = out_inlier_mask; a.ransac_pose = out_ransac_pose;
  return launch_kabsch_ransac(a, num_pairs, ST(stream));
}

int fp_pose_verify_depth(const int32_t* success, const double* R, const double* t, const double* frame_cameras, const double* A,
                         const int32_t* image_index, const double* thresh_mm, const int32_t* point_ranges, const double* centers, const double* radii,
                         const float* points, int num_points, const float* depth, int num_images, int H, int W, int num_pairs, int n_slots, int grid,
                         int min_visible, int32_t* out_counts, double* out_score, int32_t* out_status, fp_stream_t stream) {
  FP_REQUIRE(success && R && t && frame_cameras && A && image_index && thresh_mm && point_ranges && centers && radii && depth && out_counts &&
             out_score && out_status, "fp_pose_verify_depth: null pointer");
  FP_REQUIRE(points || num_points == 0, "fp_pose_verify_depth: null points");
  FP_REQUIRE(num_pairs >= 0 && n_slots >= 1 && num_pairs % n_slots == 0, "fp_pose_verify_depth: num_pairs must be a multiple of n_slots");
  VerifyArgs a;
  memset(&a, 0, sizeof(a));
  a.success = success; a.R = R; a.t = t; a.cam = frame_cameras; a.A = A; a.image_index = image_index; a.tau = thresh_mm;
  a.ranges = point_ranges; a.center = centers; a.radius = radii; a.points = points; a.m_total = num_points;
  a.depth = depth; a.num_images = num_images; a.H = H; a.W = W; a.n_slots = n_slots; a.grid = grid; a.min_visible = min_visible;
  a.counts = out_counts; a.score = out_score; a.status = out_status;
  return launch_pose_verify_depth(a, num_pairs, ST(stream));
}

int fp_pose_verify_mask(const int32_t* success, const double* R, const double* t, const double* frame_cameras, const double* A,
                        const int32_t* point_ranges, const double* centers, const double* radii, const float* points, int num_points,
                        const uint8_t* masks, const int32_t* mask_areas, int H, int W, int num_pairs, int n_slots, int grid, int min_pixels,
                        int32_t* out_counts, double* out_score, int32_t* out_status, fp_stream_t stream) {
  FP_REQUIRE(success && R && t && frame_cameras && A && point_ranges && centers && radii && masks && mask_areas && out_counts && out_score &&
             out_status, "fp_pose_verify_mask: null pointer");
  FP_REQUIRE(points || num_points == 0, "fp_pose_verify_mask: null points");
  FP_REQUIRE(num_pairs >= 0 && n_slots >= 1 && num_pairs % n_slots == 0, "fp_pose_verify_mask: num_pairs must be a multiple of n_slots");
  MaskVerifyArgs a;
  memset(&a, 0, sizeof(a));
  a.success = success; a.R = R; a.t = t; a.cam = frame_cameras; a.A = A;
  a.ranges = point_ranges; a.center = centers; a.radius = radii; a.points = points; a.m_total = num_points;
  a.masks = masks; a.area = mask_areas; a.H = H; a.W = W; a.n_slots = n_slots; a.grid = grid; a.min_pixels = min_pixels;
  a.counts = out_counts; a.score = out_score; a.status = out_status;
  return launch_pose_verify_mask(a, num_pairs, ST(stream));
}

int fp_detection_masks(const int32_t* counts, const int32_t* run_off, int num_runs, int num_det, int hc, int wc, int H, int W, int open3x3,
                       int32_t* scratch_prefix, uint8_t* out_masks, int32_t* out_area, fp_stream_t stream) {
  FP_REQUIRE(num_det >= 0 && num_runs >= 0, "fp_detection_masks: %d detections with %d runs", num_det, num_runs);
  FP_REQUIRE(H >= 1 && W >= 1 && H <= hc && W <= wc, "fp_detection_masks: an image of %d x %d out of a canvas of %d x %d (1 <= W <= wc, 1 <= H <= hc)", W, H, wc, hc);
  FP_REQUIRE((long long)hc * wc <= (1ll << 30), "fp_detection_masks: a canvas of %d x %d (at most 2^30 pixels: the pixel index is an int)", wc, hc);
  if (num_det == 0) return FP_OK;
  FP_REQUIRE(run_off && out_masks && out_area, "fp_detection_masks: null pointer");
  FP_REQUIRE((counts && scratch_prefix) || num_runs == 0, "fp_detection_masks: null counts / scratch_prefix");
  DetMaskArgs a;
  memset(&a, 0, sizeof(a));
  a.counts = counts; a.run_off = run_off; a.num_runs = num_runs; a.hc = hc; a.wc = wc; a.H = H; a.W = W;
  a.prefix = scratch_prefix; a.masks = out_masks; a.area = out_area;
  return launch_detection_masks(a, num_det, open3x3, ST(stream));
}

int fp_pose_overlap(const float* points, int num_points, const int32_t* point_ranges, const double* centers, const double* radii,
                    int num_objects, const int32_t* pose_obj, const int32_t* valid, const double* R, const double* t, int num_poses,
                    const int32_t* pairs, int num_pairs, int grid, int32_t* out_counts, double* out_overlap, int32_t* out_status,
                    fp_stream_t stream) {
  FP_REQUIRE(num_pairs >= 0 && num_poses >= 0 && num_objects >= 0, "fp_pose_overlap: negative count");
  if (num_pairs == 0) return FP_OK;
  FP_REQUIRE(point_ranges && centers && radii && pose_obj && valid && R && t && pairs && out_counts && out_overlap && out_status,
             "fp_pose_overlap: null pointer");
  FP_REQUIRE(points || num_points == 0, "fp_pose_overlap: null points");
  PoseOverlapArgs a;
  memset(&a, 0, sizeof(a));
  a.points = points; a.m_total = num_points; a.ranges = point_ranges; a.center = centers; a.radius = radii; a.n_objects = num_objects;
  a.pose_obj = pose_obj; a.valid = valid; a.R = R; a.t = t; a.n_poses = num_poses; a.pairs = pairs; a.grid = grid;
  a.counts = out_counts; a.overlap = out_overlap; a.status = out_status;
  return launch_pose_overlap(a, num_pairs, ST(stream));
}

int fp_pose_nms_greedy(const int32_t* group_off, const int32_t* pair_off, int num_groups, const int32_t* pairs, const double* overlap,
                       const int32_t* status, int num_poses, int num_pairs, double thresh, int32_t* out_keep, int32_t* out_suppressed_by,
                       fp_stream_t stream) {
  FP_REQUIRE(num_groups >= 0 && num_poses >= 0 && num_pairs >= 0, "fp_pose_nms_greedy: negative count");
  if (num_groups == 0) return FP_OK;
  FP_REQUIRE(group_off && pair_off && out_keep && out_suppressed_by, "fp_pose_nms_greedy: null pointer");
  FP_REQUIRE((pairs && overlap && status) || num_pairs == 0, "fp_pose_nms_greedy: null pairs / overlap / status");
  PoseNmsArgs a;
  memset(&a, 0, sizeof(a));
  a.group_off = group_off; a.pair_off = pair_off; a.pairs = pairs; a.overlap = overlap; a.status = status; a.thresh = thresh;
  a.n_poses = num_poses; a.n_pairs = num_pairs; a.keep = out_keep; a.suppressed_by = out_suppressed_by;
  return launch_pose_nms_greedy(a, num_groups, ST(stream));
}

static GroupTables group_tables(const int32_t* est_off, const int32_t* gt_off, const int32_t* pair_off, int num_groups, int num_a, int num_b,
                                int num_pairs) {
  GroupTables t;
  t.est_off = est_off; t.gt_off = gt_off; t.pair_off = pair_off; t.n_groups = num_groups; t.n_a = num_a; t.n_b = num_b; t.n_pairs = num_pairs;
  return t;
}

int fp_detection_match(const int32_t* est_off, const int32_t* gt_off, const int32_t* pair_off, int num_groups, const double* err,
                       int num_pairs, const int32_t* gt_valid, int num_gt, const int32_t* group_tab, const double* ths, int num_tabs,
                       int num_ths, int num_est, int8_t* out_flag, int32_t* out_matched_gt, fp_stream_t stream) {
  FP_REQUIRE(num_groups >= 0 && num_pairs >= 0 && num_gt >= 0 && num_est >= 0 && num_tabs >= 0, "fp_detection_match: negative count");
  if (num_groups == 0) return FP_OK;
  FP_REQUIRE(est_off && gt_off && pair_off && group_tab && ths, "fp_detection_match: null pointer");
  FP_REQUIRE((out_flag && out_matched_gt) || num_est == 0, "fp_detection_match: null output");
  FP_REQUIRE(err || num_pairs == 0, "fp_detection_match: null err");
  FP_REQUIRE(gt_valid || num_gt == 0, "fp_detection_match: null gt_valid");
  DetMatchArgs a;
  memset(&a, 0, sizeof(a));
  a.t = group_tables(est_off, gt_off, pair_off, num_groups, num_est, num_gt, num_pairs);
  a.err = err; a.gt_valid = gt_valid; a.group_tab = group_tab; a.ths = ths; a.n_tab = num_tabs; a.T = num_ths;
  a.flag = (signed char*)out_flag; a.matched_gt = out_matched_gt;
  return launch_detection_match(a, ST(stream));
}

int fp_detection_ap(const int32_t* obj_off, int num_objects, const int32_t* order, int num_order, const int8_t* flag, int num_est,
                    int num_ths, const int32_t* n_valid, const double* rec_thr, int num_rec, double* out_ap, double* out_q,
                    int32_t* out_totals, fp_stream_t stream) {
  FP_REQUIRE(num_objects >= 0 && num_order >= 0 && num_est >= 0, "fp_detection_ap: negative count");
  if (num_objects == 0) return FP_OK;
  FP_REQUIRE(obj_off && n_valid && rec_thr && out_ap && out_q && out_totals, "fp_detection_ap: null pointer");
  FP_REQUIRE((order && flag) || num_order == 0, "fp_detection_ap: null order / flag");
  DetApArgs a;
  memset(&a, 0, sizeof(a));
  a.obj_off = obj_off; a.order = order; a.flag = (const signed char*)flag; a.n_valid = n_valid; a.rec_thr = rec_thr;
  a.n_order = num_order; a.n_est = num_est; a.T = num_ths; a.R = num_rec; a.ap = out_ap; a.q = out_q; a.totals = out_totals;
  return launch_detection_ap(a, num_objects, ST(stream));
}

// ------------------------------------------------------------------ proposal labelling
int fp_mask_boxes(const uint8_t* masks, int num_prop, int H, int W, int32_t* out_box, int32_t* out_area, fp_stream_t stream) {
  FP_REQUIRE(num_prop >= 0, "fp_mask_boxes: %d proposals", num_prop);
  if (num_prop == 0) return FP_OK;
  FP_REQUIRE(masks && out_box && out_area, "fp_mask_boxes: null pointer");
  MaskBoxArgs a;
  memset(&a, 0, sizeof(a));
  a.masks = masks; a.H = H; a.W = W; a.box = out_box; a.area = out_area;
  return launch_mask_boxes(a, num_prop, ST(stream));
}

int fp_proposal_crops(const float* images, int n_img, int H, int W, const uint8_t* masks, const int32_t* image_index, const int32_t* boxes,
                      int num_prop, int S, float* out, int32_t* out_status, fp_stream_t stream) {
  FP_REQUIRE(num_prop >= 0, "fp_proposal_crops: %d proposals", num_prop);
  if (num_prop == 0) return FP_OK;
  FP_REQUIRE(images && masks && boxes && out && out_status, "fp_proposal_crops: null pointer");
  ProposalCropArgs a;
  memset(&a, 0, sizeof(a));
  a.images = images; a.masks = masks; a.image_index = image_index; a.boxes = boxes; a.n_img = n_img; a.H = H; a.W = W; a.S = S;
  a.out = out; a.status = out_status;
  return launch_proposal_crops(a, num_prop, ST(stream));
}

int fp_proposal_scores(const float* desc_n, int num_prop, int dim, const float* bank_n, int num_bank, const int32_t* obj_off, int num_obj,
                       int max_templates, int k, void* scratch, size_t scratch_bytes, float* out_scores, int32_t* out_best_obj,
                       float* out_best_score, int32_t* out_best_template, fp_stream_t stream) {
  FP_REQUIRE(num_prop >= 0 && num_bank >= 0, "fp_proposal_scores: negative count");
  FP_REQUIRE(num_obj >= 1 && dim >= 1 && max_templates >= 1, "fp_proposal_scores: %d objects of at most %d templates, %d words", num_obj, max_templates, dim);
  FP_REQUIRE(k >= 1 && k <= FP_PROPOSAL_MAX_K, "fp_proposal_scores: k = %d outside [1, %d]", k, FP_PROPOSAL_MAX_K);
  FP_REQUIRE((long long)num_obj * num_prop <= (1ll << 20), "fp_proposal_scores: %d proposals x %d objects (at most 2^20 rows in one call)", num_prop, num_obj);
  if (num_prop == 0) return FP_OK;
  FP_REQUIRE(desc_n && obj_off && scratch && out_scores && out_best_obj && out_best_score && out_best_template, "fp_proposal_scores: null pointer");
  FP_REQUIRE(bank_n || num_bank == 0, "fp_proposal_scores: null bank");
  FP_REQUIRE((reinterpret_cast<size_t>(scratch) & 15) == 0, "fp_proposal_scores: scratch must be 16-byte aligned");
  FP_REQUIRE(scratch_bytes >= FP_PROPOSAL_SCORE_SCRATCH_BYTES(num_prop, num_obj, dim, max_templates, k),
             "fp_proposal_scores: scratch of %zu bytes, %zu needed", scratch_bytes,
             (size_t)FP_PROPOSAL_SCORE_SCRATCH_BYTES(num_prop, num_obj, dim, max_templates, k));
  const size_t rows = (size_t)num_obj * num_prop;
  auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
  char* s = static_cast<char*>(scratch);
  float* cos_scratch = reinterpret_cast<float*>(s);  s += up16(4 * FP_COSINE_SCRATCH_FLOATS(rows, max_templates));
  ProposalScoreArgs a;
  memset(&a, 0, sizeof(a));
  a.desc_n = desc_n; a.obj_off = obj_off; a.P = num_prop; a.D = dim; a.N = num_bank; a.O = num_obj; a.k = k; a.max_templates = max_templates;
  a.rep = reinterpret_cast<float*>(s);      s += up16(4 * rows * dim);
  a.seg_off = reinterpret_cast<int*>(s);    s += up16(4 * ((size_t)num_obj + 1));
  a.tpl_off = reinterpret_cast<int*>(s);    s += up16(4 * ((size_t)num_obj + 1));
  a.det_nt = reinterpret_cast<int*>(s);     s += up16(4 * rows);
  float* top_val = reinterpret_cast<float*>(s);  s += up16(4 * rows * k);
  int* top_idx = reinterpret_cast<int*>(s);
  a.top_val = top_val; a.top_idx = top_idx;
  a.scores = out_scores; a.best_obj = out_best_obj; a.best_score = out_best_score; a.best_template = out_best_template;
  TRY(launch_proposal_prep(a, ST(stream)));
  // the library's own retrieval, canonical tie order: its kernels, its summation order, its bits (a bank of no rows is never read: every
  // object then has no template)
  TRY(fp_cosine_topk(a.rep, a.seg_off, a.det_nt, (int)rows, num_prop, bank_n ? bank_n : desc_n, a.tpl_off, num_obj, max_templates, dim, k, cos_scratch,
                     top_val, top_idx, 0, stream));
  return launch_proposal_aggregate(a, ST(stream));
}

int fp_proposal_rank(const int32_t* best_obj, const float* best_score, const int32_t* area, const int32_t* crop_status, const int32_t* boxes,
                     int num_prop, int num_obj, int min_area, float min_score, int max_group, int max_pairs, int32_t* out_decision,
                     int32_t* out_order, int32_t* out_group_off, int32_t* out_pair_off, int32_t* out_pairs, int32_t* out_boxes_ranked,
                     fp_stream_t stream) {
  FP_REQUIRE(num_prop >= 0 && max_pairs >= 0, "fp_proposal_rank: negative count");
  FP_REQUIRE(out_group_off && out_pair_off, "fp_proposal_rank: null pointer");
  FP_REQUIRE((best_obj && best_score && area && crop_status && boxes && out_decision && out_order && out_boxes_ranked) || num_prop == 0,
             "fp_proposal_rank: null pointer");
  FP_REQUIRE(out_pairs || max_pairs == 0, "fp_proposal_rank: null pairs");
  ProposalRankArgs a;
  memset(&a, 0, sizeof(a));
  a.best_obj = best_obj; a.best_score = best_score; a.area = area; a.crop_status = crop_status; a.boxes = boxes;
  a.P = num_prop; a.O = num_obj; a.min_area = min_area; a.max_group = max_group; a.max_pairs = max_pairs; a.min_score = min_score;
  a.decision = out_decision; a.order = out_order; a.group_off = out_group_off; a.pair_off = out_pair_off; a.pairs = out_pairs;
  a.boxes_ranked = out_boxes_ranked;
  return launch_proposal_rank(a, ST(stream));
}

int fp_box_iou(const int32_t* boxes, int num_boxes, const int32_t* pairs, int num_pairs, double* out_overlap, int32_t* out_status,
               fp_stream_t stream) {
  FP_REQUIRE(num_boxes >= 0 && num_pairs >= 0, "fp_box_iou: negative count");
  if (num_pairs == 0) return FP_OK;
  FP_REQUIRE(pairs && out_overlap && out_status, "fp_box_iou: null pointer");
  FP_REQUIRE(boxes || num_boxes == 0, "fp_box_iou: null boxes");
  BoxIouArgs a;
  memset(&a, 0, sizeof(a));
  a.boxes = boxes; a.pairs = pairs; a.n_boxes = num_boxes; a.n_pairs = num_pairs; a.overlap = out_overlap; a.status = out_status;
  return launch_box_iou(a, ST(stream));
}

// ------------------------------------------------------------------ the appearance score of a proposal
int fp_proposal_patch_cover(const uint8_t* masks, int n_img, int H, int W, const int32_t* image_index, const int32_t* boxes, int num_prop, int S,
                            int patch_size, int32_t* out_cover, fp_stream_t stream) {
  FP_REQUIRE(num_prop >= 0, "fp_proposal_patch_cover: %d proposals", num_prop);
  FP_REQUIRE((masks && boxes && out_cover) || num_prop == 0, "fp_proposal_patch_cover: null pointer");
  PatchCoverArgs a;
  memset(&a, 0, sizeof(a));
  a.masks = masks; a.image_index = image_index; a.boxes = boxes; a.n_img = n_img; a.H = H; a.W = W; a.S = S; a.ps = patch_size;
  a.cover = out_cover;
  return launch_proposal_patch_cover(a, num_prop, ST(stream));
}

int fp_proposal_appearance(const float* q_n, const int32_t* q_cover, int num_prop, int num_patches, int dim, const float* bank_patch_n,
                           const int32_t* bank_cover, int num_bank, const int32_t* obj_off, int num_obj, const int32_t* best_obj,
                           const int32_t* best_template, const float* best_score, int min_cover, float* out_best_sim, int32_t* out_best_patch,
                           float* out_appearance, int32_t* out_n_valid, int32_t* out_status, float* out_score, fp_stream_t stream) {
  FP_REQUIRE(num_prop >= 0 && num_bank >= 0, "fp_proposal_appearance: negative count");
  FP_REQUIRE(obj_off, "fp_proposal_appearance: null obj_off");
  FP_REQUIRE((q_n && q_cover && best_obj && best_template && best_score && out_best_sim && out_best_patch && out_appearance && out_n_valid &&
              out_status && out_score) || num_prop == 0, "fp_proposal_appearance: null pointer");
  FP_REQUIRE((bank_patch_n && bank_cover) || num_bank == 0, "fp_proposal_appearance: null bank");
  ProposalAppearanceArgs a;
  memset(&a, 0, sizeof(a));
  a.q = q_n; a.q_cover = q_cover; a.bank = bank_patch_n; a.bank_cover = bank_cover; a.obj_off = obj_off; a.best_obj = best_obj;
  a.best_template = best_template; a.best_score = best_score; a.P = num_prop; a.Np = num_patches; a.D = dim; a.N = num_bank; a.O = num_obj;
  a.min_cover = min_cover; a.best_sim = out_best_sim; a.best_patch = out_best_patch; a.appearance = out_appearance; a.n_valid = out_n_valid;
  a.status = out_status; a.score = out_score;
  return launch_proposal_appearance(a, ST(stream));
}

// ------------------------------------------------------------------ COCO average precision of detections
int fp_mask_pack(const uint8_t* masks, int num_masks, int H, int W, uint64_t* out_words, int32_t* out_area, fp_stream_t stream) {
  FP_REQUIRE(num_masks >= 0, "fp_mask_pack: %d masks", num_masks);
  if (num_masks == 0) return FP_OK;
  FP_REQUIRE(masks && out_words && out_area, "fp_mask_pack: null pointer");
  MaskPackArgs a;
  memset(&a, 0, sizeof(a));
  a.masks = masks; a.H = H; a.W = W; a.Wq = W >= 1 ? (W - 1) / 64 + 1 : 0; a.words = reinterpret_cast<unsigned long long*>(out_words); a.area = out_area;
  return launch_mask_pack(a, num_masks, ST(stream));
}

int fp_group_mask_iou(const uint64_t* words_a, int num_a, const uint64_t* words_b, int num_b, int L, const int32_t* est_off,
                      const int32_t* gt_off, const int32_t* pair_off, int num_groups, int num_pairs, int32_t* scratch_tiles,
                      int32_t* out_counts, double* out_overlap, int32_t* out_status, fp_stream_t stream) {
  FP_REQUIRE(num_groups >= 0 && num_a >= 0 && num_b >= 0 && num_pairs >= 0, "fp_group_mask_iou: negative count");
  if (num_groups == 0 || num_pairs == 0) return FP_OK;
  FP_REQUIRE(est_off && gt_off && pair_off && scratch_tiles && out_counts && out_overlap && out_status, "fp_group_mask_iou: null pointer");
  FP_REQUIRE((words_a || num_a == 0) && (words_b || num_b == 0), "fp_group_mask_iou: null words");
  GroupMaskIouArgs a;
  memset(&a, 0, sizeof(a));
  a.t = group_tables(est_off, gt_off, pair_off, num_groups, num_a, num_b, num_pairs);
  a.words_a = reinterpret_cast<const unsigned long long*>(words_a); a.words_b = reinterpret_cast<const unsigned long long*>(words_b); a.L = L;
  a.tile_off = scratch_tiles; a.counts = out_counts; a.overlap = out_overlap; a.status = out_status;
  return launch_group_mask_iou(a, ST(stream));
}

int fp_group_box_iou(const double* boxes_a, int num_a, const double* boxes_b, int num_b, const int32_t* est_off, const int32_t* gt_off,
                     const int32_t* pair_off, int num_groups, int num_pairs, double* out_overlap, int32_t* out_status, fp_stream_t stream) {
  FP_REQUIRE(num_groups >= 0 && num_a >= 0 && num_b >= 0 && num_pairs >= 0, "fp_group_box_iou: negative count");
  if (num_groups == 0 || num_pairs == 0) return FP_OK;
  FP_REQUIRE(est_off && gt_off && pair_off && out_overlap && out_status, "fp_group_box_iou: null pointer");
  FP_REQUIRE((boxes_a || num_a == 0) && (boxes_b || num_b == 0), "fp_group_box_iou: null boxes");
  GroupBoxIouArgs a;
  memset(&a, 0, sizeof(a));
  a.t = group_tables(est_off, gt_off, pair_off, num_groups, num_a, num_b, num_pairs);
  a.boxes_a = boxes_a; a.boxes_b = boxes_b; a.overlap = out_overlap; a.status = out_status;
  return launch_group_box_iou(a, ST(stream));
}

int fp_coco_match(const int32_t* est_off, const int32_t* gt_off, const int32_t* pair_off, int num_groups, const double* overlap,
                  int num_pairs, const int32_t* gt_ignore, int num_gt, const double* ths, int num_ths, int num_est, int8_t* out_flag,
                  int32_t* out_matched_gt, fp_stream_t stream) {
  FP_REQUIRE(num_groups >= 0 && num_pairs >= 0 && num_gt >= 0 && num_est >= 0, "fp_coco_match: negative count");
  FP_REQUIRE(num_ths >= 1 && num_ths <= FP_DETECTION_MAX_THS, "fp_coco_match: num_ths must be in [1, %d] (got %d)", FP_DETECTION_MAX_THS, num_ths);
  if (num_groups == 0) return FP_OK;
  FP_REQUIRE(est_off && gt_off && pair_off && ths, "fp_coco_match: null pointer");
  FP_REQUIRE((out_flag && out_matched_gt) || num_est == 0, "fp_coco_match: null output");
  FP_REQUIRE(overlap || num_pairs == 0, "fp_coco_match: null overlap");
  FP_REQUIRE(gt_ignore || num_gt == 0, "fp_coco_match: null gt_ignore");
  CocoMatchArgs a;
  memset(&a, 0, sizeof(a));
  a.t = group_tables(est_off, gt_off, pair_off, num_groups, num_est, num_gt, num_pairs);
  a.overlap = overlap; a.gt_ignore = gt_ignore; a.ths = ths; a.T = num_ths; a.flag = (signed char*)out_flag; a.matched_gt = out_matched_gt;
  return launch_coco_match(a, ST(stream));
}

// ------------------------------------------------------------------ ViT building blocks
int fp_patchify(const float* images, int B, int H, int W, int patch, void* out, int ld_out, int out_dtype,
                fp_stream_t stream) {
  FP_REQUIRE(images && out, "fp_patchify: null pointer");
  return patchify_launch(images, B, H, W, patch, out, ld_out, out_dtype, ST(stream), (out_dtype == FP_DTYPE_F16X3 || out_dtype == FP_DTYPE_F16F8) ? FP_SPLIT_SCALE_ACT : 1.f);
}

int fp_layernorm(const float* x, int ld_x, const float* weight, const float* bias, float eps, void* out, int ld_out,
                 int out_dtype, int dim, int out_rows, int out_rows_per_img, int in_rows_per_img, int in_skip,
                 fp_stream_t stream) {
  FP_REQUIRE(x && weight && bias && out, "fp_layernorm: null pointer");
  LayerNormArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.ld_x = ld_x; a.weight = weight; a.bias = bias; a.eps = eps; a.out = out; a.ld_out = ld_out;
  a.out_dtype = out_dtype; a.out_scale = 0.f; a.dim = dim; a.out_rows = out_rows;
  a.out_rows_per_img = out_rows_per_img > 0 ? out_rows_per_img : (out_rows > 0 ? out_rows : 1);
  a.in_rows_per_img = in_rows_per_img > 0 ? in_rows_per_img : a.out_rows_per_img;
  a.in_skip = in_skip;
  return layernorm_launch(a, ST(stream));
}

int fp_gemm_bf16(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int M_valid, const float* bias,
                 const float* gamma, void* out, int ldo, int epilogue, fp_stream_t stream) {
  FP_REQUIRE(A && W && out, "fp_gemm_bf16: null pointer");
  const int tile = (epilogue >> 8) & 0xfff;  // tuning bits: force the 128 or 256 block tile
  const bool f16 = (epilogue >> 21) & 1;     // FP_GEMM_F16: IEEE fp16 operands and 16-bit outputs
  epilogue &= 0xff;
  FP_REQUIRE(tile == 0 || tile == 64 || tile == 128 || tile == 256 || tile == 320 || (tile == 352 && (epilogue == GEMM_EPI_BIAS_BF16 || epilogue == GEMM_EPI_GELU_BF16)),
             "fp_gemm_bf16: bad tile override %d", tile);

  FP_REQUIRE(epilogue == GEMM_EPI_BIAS_BF16 || epilogue == GEMM_EPI_GELU_BF16 || epilogue == GEMM_EPI_LS_RESID_F32 ||
                 epilogue == GEMM_EPI_BIAS_F32 || epilogue == GEMM_EPI_SWIGLU_BF16,
             "fp_gemm_bf16: epilogue %d is not available through this entry point", epilogue);
  FP_REQUIRE(epilogue != GEMM_EPI_LS_RESID_F32 || gamma, "fp_gemm_bf16: gamma required");
  GemmBf16Args a;
  memset(&a, 0, sizeof(a));
  a.A = reinterpret_cast<const __bf16*>(A); a.lda = lda; a.W = reinterpret_cast<const __bf16*>(W); a.ldw = ldw;
  a.M = M; a.N = N; a.K = K; a.M_valid = M_valid; a.bias = bias; a.gamma = gamma; a.out = out; a.ldo = ldo;
  a.tile_override = tile;
  return gemm_launch(f16 ? GemmFmt::F16 : GemmFmt::BF16, epilogue, a, ST(stream));
}

int fp_gemm_bf16_ln(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int M_valid, const float* bias, void* out, int ldo,
                    int epilogue, const float* colsum, const float* ln_row, void* xb, int ld_xb, float* stats, fp_stream_t stream) {
  FP_REQUIRE(A && W && out && bias, "fp_gemm_bf16_ln: null pointer");
  const int tile = (epilogue >> 8) & 0xfff;
  const bool f16 = (epilogue >> 21) & 1;     // FP_GEMM_F16: IEEE fp16 operands, 16-bit outputs and (hi, lo) stream
  epilogue &= 0xff;
  FP_REQUIRE(tile == 0 || tile == 64 || tile == 128 || tile == 256 || tile == 320 ||
                 (tile == 352 && (epilogue == GEMM_EPI_RESID_HILO || epilogue == GEMM_EPI_BIAS_BF16 || epilogue == GEMM_EPI_GELU_BF16)),
             "fp_gemm_bf16_ln: bad tile override %d", tile);
  GemmBf16Args a;
  memset(&a, 0, sizeof(a));
  a.A = reinterpret_cast<const __bf16*>(A); a.lda = lda; a.W = reinterpret_cast<const __bf16*>(W); a.ldw = ldw;
  a.M = M; a.N = N; a.K = K; a.M_valid = M_valid; a.bias = bias; a.out = out; a.ldo = ldo; a.tile_override = tile;
  if (epilogue == GEMM_EPI_RESID_HILO) {  // producer on the (hi, lo) stream: `out` is the LOW-half array (bf16, row stride ld_xb), xb the high halves
    FP_REQUIRE(xb && stats, "fp_gemm_bf16_ln: epilogue 8 needs xb, out (= the low halves) and stats");
    a.xb = reinterpret_cast<__bf16*>(xb); a.ld_xb = ld_xb; a.xl = reinterpret_cast<__bf16*>(out); a.stats_out = reinterpret_cast<float2*>(stats);
    a.out = nullptr;
  } else if (epilogue == GEMM_EPI_RESID_F32) {  // producer: x += acc + bias, plus bf16(x) and the partial row sums
    FP_REQUIRE((xb == nullptr) == (stats == nullptr), "fp_gemm_bf16_ln: xb and stats go together");
    FP_REQUIRE(!xb || (N % 128 == 0 && ld_xb >= N && ld_xb % 4 == 0), "fp_gemm_bf16_ln: N must be a multiple of 128 and ld_xb cover the row");
    a.xb = reinterpret_cast<__bf16*>(xb); a.ld_xb = ld_xb; a.stats_out = reinterpret_cast<float2*>(stats);
  } else {                               // consumer: epi(rstd * (acc - mean * colsum) + bias)
    FP_REQUIRE(epilogue == GEMM_EPI_BIAS_BF16 || epilogue == GEMM_EPI_GELU_BF16 || epilogue == GEMM_EPI_SWIGLU_BF16,
               "fp_gemm_bf16_ln: epilogue %d has no folded-LayerNorm form", epilogue);
    FP_REQUIRE(colsum && ln_row, "fp_gemm_bf16_ln: colsum and ln_row are required");
    a.colsum = colsum; a.ln_stats = reinterpret_cast<const float2*>(ln_row); a.ln_eps = 1e-6f;
  }
  return gemm_launch(f16 ? GemmFmt::F16 : GemmFmt::BF16, epilogue, a, ST(stream));
}

int fp_gemm_resid_tile_rows(int M_valid, int N, int num_cus) { return gemm_resid_tile_rows(M_valid, N, num_cus); }
int fp_gemm_wide_tile_rows(int M, int M_valid, int N, int num_cus) { return gemm_wide_tile_rows(M, M_valid, N, num_cus); }

int fp_ln_finalize(const float* stats, int parts, int stats_stride, int rows, int dim, float eps, float* ln_row, fp_stream_t stream) {
  FP_REQUIRE(stats && ln_row && parts >= 1 && dim >= 1, "fp_ln_finalize: bad arguments");
  return ln_finalize_launch(reinterpret_cast<const float2*>(stats), parts, stats_stride, rows, dim, eps, reinterpret_cast<float2*>(ln_row), ST(stream));
}

#ifdef FP_GEMM_TIMELINE
// Measurement build only (tools/build_variant.sh -DFP_GEMM_TIMELINE, tools/gemm_timeline.py): the same GEMM writing four
// shader-clock stamps per workgroup into a caller-owned buffer of dbg_len >= 4 * grid u64 slots.
int fp_gemm_bf16_timeline(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int M_valid, const float* bias,
                          const float* gamma, void* out, int ldo, int epilogue, unsigned long long* dbg, int64_t dbg_len,
                          fp_stream_t stream) {
  FP_REQUIRE(A && W && out && dbg, "fp_gemm_bf16_timeline: null pointer");
  FP_REQUIRE(dbg_len >= 4ll * ((M + 127) / 128) * ((N + 127) / 128) * 2, "fp_gemm_bf16_timeline: stamp buffer too small");
  GemmBf16Args a;
  memset(&a, 0, sizeof(a));
  a.A = reinterpret_cast<const __bf16*>(A); a.lda = lda; a.W = reinterpret_cast<const __bf16*>(W); a.ldw = ldw;
  a.M = M; a.N = N; a.K = K; a.M_valid = M_valid; a.bias = bias; a.gamma = gamma; a.out = out; a.ldo = ldo;
  a.tile_override = (epilogue >> 8) & 0xfff;
  a.dbg = dbg;
  return gemm_launch(GemmFmt::BF16, epilogue & 0xff, a, ST(stream));
}
#endif

int fp_gemm_fp8(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int M_valid, const float* bias,
                const float* col_scale, void* out, int ldo, int epilogue, float out_scale, fp_stream_t stream) {
  FP_REQUIRE(A && W && out, "fp_gemm_fp8: null pointer");
  FP_REQUIRE(out_scale >= 0.f, "fp_gemm_fp8: out_scale must be >= 0");
  GemmBf16Args a;
  memset(&a, 0, sizeof(a));
  a.A = reinterpret_cast<const __bf16*>(A); a.lda = lda; a.W = reinterpret_cast<const __bf16*>(W); a.ldw = ldw;
  a.M = M; a.N = N; a.K = K; a.M_valid = M_valid; a.bias = bias; a.gamma = col_scale; a.out = out; a.ldo = ldo;
  a.out_scale = out_scale;
  a.tile_override = (epilogue >> 8) & 0xfff;  // tuning bits: 256 / 320 force that block tile (benchmarks, tests)
  FP_REQUIRE(a.tile_override == 0 || a.tile_override == 256 || a.tile_override == 320, "fp_gemm_fp8: bad tile override %d", a.tile_override);
  return gemm_launch(GemmFmt::FP8, epilogue & 0xff, a, ST(stream));
}

int fp_gemm_split(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int M_valid, const float* bias, const float* gamma,
                  void* out, int ldo, int epilogue, float acc_scale, float out_scale, fp_stream_t stream) {
  FP_REQUIRE(A && W && out, "fp_gemm_split: null pointer");
  const int tile = (epilogue >> 8) & 0xfff;
  const bool f16f8 = (epilogue >> 20) & 1;   // FP_GEMM_SPLIT_F16F8: the operands (and a GELU / SwiGLU output) are f16f8 rows
  epilogue &= 0xff;
  FP_REQUIRE(tile == 0 || tile == 128 || tile == 256, "fp_gemm_split: bad tile override %d", tile);
  FP_REQUIRE(epilogue == GEMM_EPI_BIAS_BF16 || epilogue == GEMM_EPI_GELU_BF16 || epilogue == GEMM_EPI_LS_RESID_F32 ||
                 epilogue == GEMM_EPI_BIAS_F32 || epilogue == GEMM_EPI_SWIGLU_BF16,
             "fp_gemm_split: epilogue %d is not available through this entry point", epilogue);
  GemmBf16Args a;
  memset(&a, 0, sizeof(a));
  a.A = reinterpret_cast<const __bf16*>(A); a.lda = lda; a.W = reinterpret_cast<const __bf16*>(W); a.ldw = ldw;
  a.M = M; a.N = N; a.K = K; a.M_valid = M_valid; a.bias = bias; a.gamma = gamma; a.out = out; a.ldo = ldo;
  a.tile_override = tile; a.acc_scale = acc_scale; a.out_scale = out_scale;
  return gemm_launch(f16f8 ? GemmFmt::F16F8 : GemmFmt::F16X3, epilogue, a, ST(stream));
}

int fp_attention_split(const void* qkv, int ld_qkv, void* out, int ld_out, int B, int n_tok, int dim, int heads, float in_scale, float out_scale,
                       int out_dtype, fp_stream_t stream) {
  FP_REQUIRE(qkv && out, "fp_attention_split: null pointer");
  const int variant = (out_dtype >> 8) & 0xff;  // test bits, as in fp_attention: 0 and 1 run the lock-step kernel; 2 (the role-split kernel, removed) is unsupported
  out_dtype &= 0xff;
  FP_REQUIRE(out_dtype == FP_DTYPE_F16X3 || out_dtype == FP_DTYPE_F16F8, "fp_attention_split: the output is a split-fp16 row (FP_F16X3) or an f16f8 row (FP_F16F8)");
  FP_REQUIRE(variant <= 2, "fp_attention_split: unknown kernel variant %d", variant);
  // in_scale >= 1: the kernel's lazy-rescale threshold is a constant in raw score units (1 / (0.125 log2 e), attn.hip SPLIT_LAZY_TH) and the scores carry
  // in_scale^2 -- in exponent units the reference trails the maximum by at most 1 / in_scale^2, so p' = 2^14 p <= 2^15 fits fp16 for in_scale >= 1 only
  FP_REQUIRE(in_scale >= 1.f && out_scale > 0.f, "fp_attention_split: in_scale must be >= 1 (the split P is packed unclamped: p' <= 2^15 needs it) and out_scale positive");
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.variant = variant;
  a.qkv = qkv; a.ld_qkv = ld_qkv; a.out = out; a.ld_out = ld_out;
  a.batch = B; a.n_tok = n_tok; a.dim = dim; a.heads = heads; a.in_scale = in_scale; a.out_scale = out_scale;
  a.out_fmt = out_dtype == FP_DTYPE_F16F8 ? 1 : 0;
  return attn_launch(a, FP_DTYPE_F16X3, ST(stream));
}

int fp_layernorm_scaled(const float* x, int ld_x, const float* weight, const float* bias, float eps, void* out, int ld_out, int out_dtype, float out_scale,
                        int dim, int out_rows, fp_stream_t stream) {
  FP_REQUIRE(x && weight && bias && out, "fp_layernorm_scaled: null pointer");
  FP_REQUIRE(out_dtype == FP_DTYPE_FP8 || out_dtype == FP_DTYPE_F16X3 || out_dtype == FP_DTYPE_F16F8, "fp_layernorm_scaled: the scaled outputs are fp8 bytes, split-fp16 rows and f16f8 rows");
  LayerNormArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.ld_x = ld_x; a.weight = weight; a.bias = bias; a.eps = eps; a.out = out; a.ld_out = ld_out;
  a.out_dtype = out_dtype; a.out_scale = out_scale; a.dim = dim; a.out_rows = out_rows;
  a.out_rows_per_img = out_rows > 0 ? out_rows : 1; a.in_rows_per_img = a.out_rows_per_img; a.in_skip = 0;
  return layernorm_launch(a, ST(stream));
}

int fp_quantize_fp8(const void* in, int in_dtype, int64_t n, float scale, void* out, fp_stream_t stream) {
  FP_REQUIRE(in && out, "fp_quantize_fp8: null pointer");
  FP_REQUIRE(in_dtype == FP_F32 || in_dtype == FP_BF16, "fp_quantize_fp8: input must be fp32 or bf16");
  FP_REQUIRE(scale > 0.f, "fp_quantize_fp8: scale must be positive");
  return quantize_fp8_launch(in, in_dtype, n, scale, out, ST(stream));
}

int fp_gemm_f32(const float* A, int lda, const float* W, int ldw, int M, int N, int K, const float* bias,
                const float* gamma, float* out, int ldo, int epilogue, fp_stream_t stream) {
  FP_REQUIRE(A && W && out, "fp_gemm_f32: null pointer");
  FP_REQUIRE(epilogue == F32_EPI_STORE || epilogue == F32_EPI_BIAS || epilogue == F32_EPI_BIAS_GELU ||
                 epilogue == F32_EPI_LS_RESID || epilogue == F32_EPI_SUB_VEC || epilogue == F32_EPI_SWIGLU,
             "fp_gemm_f32: epilogue %d is not available through this entry point", epilogue);
  FP_REQUIRE(epilogue != F32_EPI_LS_RESID || gamma, "fp_gemm_f32: gamma required");
  if (M == 0) return FP_OK;
  F32TileArgs a = zero_tile_args();
  a.A = A; a.lda = lda; a.B = W; a.ldb = ldw; a.K = K; a.M = M; a.N = N;
  a.out = out; a.ldo = ldo; a.bias = bias; a.gamma = gamma;
  return f32_tile_launch(epilogue, a, M, N, 1, ST(stream));
}

int fp_attention(const void* qkv, int ld_qkv, void* out, int ld_out, int B, int n_tok,
                 int dim, int heads, int dtype, fp_stream_t stream) {
  FP_REQUIRE(qkv && out, "fp_attention: null pointer");
  AttnArgs a;
  memset(&a, 0, sizeof(a));
  a.qkv = qkv; a.ld_qkv = ld_qkv; a.out = out; a.ld_out = ld_out;
  a.batch = B; a.n_tok = n_tok; a.dim = dim; a.heads = heads;
  a.variant = (dtype >> 8) & 0xff;  // tuning / test bits: which bf16 work split runs (FP_ATTN_VARIANT_*)
  return attn_launch(a, dtype & 0xff, ST(stream));
}

int fp_convert_f32_to_bf16(const float* in, void* out, int64_t n, fp_stream_t stream) {
  FP_REQUIRE(in && out, "fp_convert_f32_to_bf16: null pointer");
  return convert_f32_to_bf16_launch(in, out, n, ST(stream));
}

int fp_warp_crops(const void* src, int n_src, int src_h, int src_w, int channels, int mode, const int32_t* src_index,
                  const double* params, int batch, int out_h, int out_w, int depth_check, void* out, float* map_out,
                  fp_stream_t stream) {
  FP_REQUIRE(src && params && out, "fp_warp_crops: null pointer");
  FP_REQUIRE(mode == FP_WARP_LINEAR || mode == FP_WARP_NEAREST, "fp_warp_crops: unknown mode %d", mode);
  FP_REQUIRE(n_src >= 1 && src_h >= 1 && src_w >= 1 && batch >= 1 && out_h >= 1 && out_w >= 1, "fp_warp_crops: empty problem");
  FP_REQUIRE(mode == FP_WARP_LINEAR ? channels >= 1 : channels == 1, "fp_warp_crops: a nearest-mode source is a single-channel u8 mask");
  FP_REQUIRE(src_index || batch <= n_src, "fp_warp_crops: %d crops but %d source images and no src_index", batch, n_src);
  WarpArgs a{src, n_src, src_h, src_w, channels, mode, src_index, params, batch, out_h, out_w, depth_check, out, map_out};
  return launch_warp_crops(a, ST(stream));
}

int fp_warp_depth(const float* src, int src_h, int src_w, const double* params, const int32_t* recompute, int batch,
                  int out_h, int out_w, int depth_check, float* out, fp_stream_t stream) {
  FP_REQUIRE(src && params && out, "fp_warp_depth: null pointer");
  FP_REQUIRE(src_h >= 1 && src_w >= 1 && batch >= 1 && out_h >= 1 && out_w >= 1, "fp_warp_depth: empty problem");
  WarpDepthArgs a{src, src_h, src_w, params, recompute, batch, out_h, out_w, depth_check, out};
  return launch_warp_depth(a, ST(stream));
}

static int render_args(const float* verts, const float* normals, const float* colors, int num_verts, const int32_t* faces,
                       int num_faces, const double* cams, int batch, int width, int height, void* vert_ws, void* tri_ws,
                       int32_t* tile_counts, int64_t* tile_offsets, int32_t* lists, int64_t* status, float* color,
                       float* depth, uint8_t* mask, int32_t* tri_id, int32_t* boxes, RenderArgs* a) {
  FP_REQUIRE(verts && normals && colors && faces && cams && vert_ws && tri_ws && tile_counts && tile_offsets && status,
             "fp_render: null pointer");
  FP_REQUIRE(num_verts >= 1 && num_faces >= 1 && batch >= 1, "fp_render: empty problem");
  FP_REQUIRE(width >= 1 && height >= 1 && width <= FP_RENDER_MAX_SIDE && height <= FP_RENDER_MAX_SIDE,
             "fp_render: viewport %d x %d outside [1, %d]", width, height, FP_RENDER_MAX_SIDE);
  FP_REQUIRE((long long)batch * num_faces < (1ll << 40) && (long long)batch * num_verts < (1ll << 40), "fp_render: batch too large");
  *a = RenderArgs{verts, normals, colors, num_verts, faces, num_faces, cams, batch, width, height, vert_ws, tri_ws,
                  tile_counts, reinterpret_cast<long long*>(tile_offsets), lists, reinterpret_cast<long long*>(status),
                  color, depth, mask, tri_id, boxes};
  return FP_OK;
}

int fp_render_setup(const float* verts, const float* normals, const float* colors, int num_verts, const int32_t* faces,
                    int num_faces, const double* cams, int batch, int width, int height, void* vert_ws, void* tri_ws,
                    int32_t* tile_counts, int64_t* tile_offsets, int32_t* lists, int64_t* status, float* color,
                    float* depth, uint8_t* mask, int32_t* tri_id, int32_t* boxes, fp_stream_t stream) {
  RenderArgs a;
  TRY(render_args(verts, normals, colors, num_verts, faces, num_faces, cams, batch, width, height, vert_ws, tri_ws,
                  tile_counts, tile_offsets, lists, status, color, depth, mask, tri_id, boxes, &a));
  return launch_render_setup(a, ST(stream));
}

int fp_render_raster(const float* verts, const float* normals, const float* colors, int num_verts, const int32_t* faces,
                     int num_faces, const double* cams, int batch, int width, int height, void* vert_ws, void* tri_ws,
                     int32_t* tile_counts, int64_t* tile_offsets, int32_t* lists, int64_t* status, float* color,
                     float* depth, uint8_t* mask, int32_t* tri_id, int32_t* boxes, fp_stream_t stream) {
  RenderArgs a;
  TRY(render_args(verts, normals, colors, num_verts, faces, num_faces, cams, batch, width, height, vert_ws, tri_ws,
                  tile_counts, tile_offsets, lists, status, color, depth, mask, tri_id, boxes, &a));
  FP_REQUIRE(lists && depth && mask, "fp_render_raster: null pointer");
  return launch_render_raster(a, ST(stream));
}

// the level table of a pyramid (layout of include/foundpose_amd.h); sides already validated
static void texture_levels(int width, int height, TexArgs* t) {
  int w = width, h = height, off = 0, l = 0;
  for (;; ++l) {
    t->off[l] = off, t->w[l] = w, t->h[l] = h;
    off += w * h;
    if (w == 1 && h == 1) break;
    w = w > 1 ? w >> 1 : 1, h = h > 1 ? h >> 1 : 1;
  }
  t->levels = l + 1;
}

int fp_texture_mips(const uint8_t* rgb, int width, int height, uint32_t* pyramid, fp_stream_t stream) {
  FP_REQUIRE(rgb && pyramid, "fp_texture_mips: null pointer");
  FP_REQUIRE(width >= 1 && height >= 1 && width <= FP_TEXTURE_MAX_SIDE && height <= FP_TEXTURE_MAX_SIDE,
             "fp_texture_mips: texture %d x %d outside [1, %d]", width, height, FP_TEXTURE_MAX_SIDE);
  TexArgs t;
  memset(&t, 0, sizeof(t));
  texture_levels(width, height, &t);
  return launch_texture_mips(rgb, t, pyramid, ST(stream));
}

int fp_render_raster_textured(const float* verts, const float* normals, const float* colors, int num_verts, const int32_t* faces,
                              int num_faces, const double* cams, int batch, int width, int height, void* vert_ws, void* tri_ws,
                              int32_t* tile_counts, int64_t* tile_offsets, int32_t* lists, int64_t* status, float* color,
                              float* depth, uint8_t* mask, int32_t* tri_id, int32_t* boxes, const float* uv,
                              const uint32_t* pyramid, int tex_width, int tex_height, const float* material, fp_stream_t stream) {
  RenderArgs a;
  TRY(render_args(verts, normals, colors, num_verts, faces, num_faces, cams, batch, width, height, vert_ws, tri_ws,
                  tile_counts, tile_offsets, lists, status, color, depth, mask, tri_id, boxes, &a));
  FP_REQUIRE(lists && depth && mask && uv && pyramid && material, "fp_render_raster_textured: null pointer");
  FP_REQUIRE(tex_width >= 1 && tex_height >= 1 && tex_width <= FP_TEXTURE_MAX_SIDE && tex_height <= FP_TEXTURE_MAX_SIDE,
             "fp_render_raster_textured: texture %d x %d outside [1, %d]", tex_width, tex_height, FP_TEXTURE_MAX_SIDE);
  for (int k = 0; k < 6; ++k)
    FP_REQUIRE(material[k] >= 0.f && material[k] <= 1.f, "fp_render_raster_textured: material[%d] = %g is NaN or outside [0, 1]", k,
               (double)material[k]);
  TexArgs t;
  memset(&t, 0, sizeof(t));
  texture_levels(tex_width, tex_height, &t);
  t.uv = uv, t.texels = pyramid;
  t.metallic = material[0], t.roughness = material[1];
  t.factor[0] = material[2], t.factor[1] = material[3], t.factor[2] = material[4];
  t.srgb = material[5] != 0.f;
  return launch_render_raster_textured(a, t, ST(stream));
}

int fp_template_downsample(const float* color, const float* depth, const uint8_t* mask, int batch, int out_h, int out_w,
                           int factor, uint8_t* rgb, uint16_t* depth_u16, uint8_t* mask_out, int32_t* boxes,
                           fp_stream_t stream) {
  FP_REQUIRE(color && depth && mask && rgb && depth_u16 && mask_out, "fp_template_downsample: null pointer");
  FP_REQUIRE(batch >= 1 && out_h >= 1 && out_w >= 1 && factor >= 1 && factor <= 16, "fp_template_downsample: bad shape");
  DownsampleArgs a{color, depth, mask, batch, out_h, out_w, factor, rgb, depth_u16, mask_out, boxes};
  return launch_template_downsample(a, ST(stream));
}

// ------------------------------------------------------------------ pose evaluation
int fp_pose_errors(const double* pts, int total_pts, const double* est, const double* p_est, const double* gt_sym, const double* p_gt,
                   int total_syms, const int32_t* ranges, int num_hyp, void* scratch, size_t scratch_bytes, double* err, int32_t* idx,
                   fp_stream_t stream) {
  FP_REQUIRE(pts && est && p_est && gt_sym && p_gt && ranges && scratch && err && idx, "fp_pose_errors: null pointer");
  FP_REQUIRE(num_hyp >= 1 && num_hyp <= 65535, "fp_pose_errors: num_hyp %d outside [1, 65535]", num_hyp);
  FP_REQUIRE(total_pts >= 1 && total_syms >= 1, "fp_pose_errors: empty vertex or symmetry array");
  std::vector<PoseErrHyp> hyps(num_hyp);
  long long parts = 0;
  int max_tiles = 0, max_syms = 0;
  for (int h = 0; h < num_hyp; ++h) {
    const int32_t* r = ranges + 4 * (size_t)h;
    FP_REQUIRE(r[1] >= 1 && r[3] >= 1, "fp_pose_errors: hypothesis %d has an empty vertex or symmetry range", h);
    FP_REQUIRE(r[0] >= 0 && (long long)r[0] + r[1] <= total_pts, "fp_pose_errors: hypothesis %d: vertices [%d, +%d) outside [0, %d)", h, r[0], r[1], total_pts);
    FP_REQUIRE(r[2] >= 0 && (long long)r[2] + r[3] <= total_syms, "fp_pose_errors: hypothesis %d: symmetries [%d, +%d) outside [0, %d)", h, r[2], r[3], total_syms);
    const int tiles = (int)(((long long)r[1] + FP_POSE_ERR_TILE - 1) / FP_POSE_ERR_TILE);
    hyps[h] = PoseErrHyp{r[0], r[1], r[2], r[3], tiles, 0, parts};
    parts += (long long)tiles * r[3];
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
    max_syms = r[3] > max_syms ? r[3] : max_syms;
  }
  const size_t table = 32 * (((size_t)num_hyp + 7) / 8) * 8;
  FP_REQUIRE(scratch_bytes >= table + sizeof(PoseErrPart) * (size_t)parts, "fp_pose_errors: scratch holds %zu bytes, %zu needed", scratch_bytes,
             table + sizeof(PoseErrPart) * (size_t)parts);
  static_assert(sizeof(PoseErrHyp) == 32 && sizeof(PoseErrPart) == 24, "layout of FP_POSE_ERR_SCRATCH_BYTES");
  // the one synchronous step of the library: the table lives in this frame, so the copy completes before it goes out of scope
  HIP_TRY(hipMemcpyWithStream(scratch, hyps.data(), sizeof(PoseErrHyp) * (size_t)num_hyp, hipMemcpyHostToDevice, ST(stream)), "fp_pose_errors: table upload");
  PoseErrArgs a{pts, est, p_est, gt_sym, p_gt, reinterpret_cast<const PoseErrHyp*>(scratch),
                reinterpret_cast<PoseErrPart*>(static_cast<char*>(scratch) + table), err, idx};
  return launch_pose_errors(a, num_hyp, max_tiles, max_syms, ST(stream));
}

int fp_pose_add_errors(const double* pts, int total_pts, const double* est, const double* gt, const int32_t* ranges, int num_pairs,
                       void* scratch, size_t scratch_bytes, double* err, fp_stream_t stream) {
  FP_REQUIRE(pts && est && gt && ranges && scratch && err, "fp_pose_add_errors: null pointer");
  FP_REQUIRE(num_pairs >= 1 && num_pairs <= 65535, "fp_pose_add_errors: num_pairs %d outside [1, 65535]", num_pairs);
  FP_REQUIRE(total_pts >= 1, "fp_pose_add_errors: empty point array");
  std::vector<PoseAddPair> pairs(num_pairs);
  long long parts = 0;
  int max_tiles = 0;
  for (int h = 0; h < num_pairs; ++h) {
    const int32_t* r = ranges + 2 * (size_t)h;
    FP_REQUIRE(r[1] >= 1, "fp_pose_add_errors: pair %d has an empty point range", h);
    FP_REQUIRE(r[0] >= 0 && (long long)r[0] + r[1] <= total_pts, "fp_pose_add_errors: pair %d: points [%d, +%d) outside [0, %d)", h, r[0], r[1], total_pts);
    const int tiles = (int)(((long long)r[1] + FP_POSE_ADD_TILE - 1) / FP_POSE_ADD_TILE);
    pairs[h] = PoseAddPair{r[0], r[1], tiles, 0, parts, 0};
    parts += tiles;
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
  }
  const size_t table = 32 * (((size_t)num_pairs + 7) / 8) * 8;
  FP_REQUIRE(scratch_bytes >= table + 16 * (size_t)parts, "fp_pose_add_errors: scratch holds %zu bytes, %zu needed", scratch_bytes, table + 16 * (size_t)parts);
  static_assert(sizeof(PoseAddPair) == 32, "layout of FP_POSE_ADD_SCRATCH_BYTES");
  // synchronous as in fp_pose_errors: the table lives in this frame
  HIP_TRY(hipMemcpyWithStream(scratch, pairs.data(), sizeof(PoseAddPair) * (size_t)num_pairs, hipMemcpyHostToDevice, ST(stream)), "fp_pose_add_errors: table upload");
  PoseAddArgs a{pts, est, gt, reinterpret_cast<const PoseAddPair*>(scratch), reinterpret_cast<double*>(static_cast<char*>(scratch) + table), err, total_pts};
  const int tiles_per_block = FP_POSE_ADD_BLOCK / FP_POSE_ADD_TILE;
  return launch_pose_add_errors(a, num_pairs, (max_tiles + tiles_per_block - 1) / tiles_per_block, ST(stream));
}

int fp_pts_diameter(const double* pts, int V, void* scratch, size_t scratch_bytes, double* out_d, int32_t* out_pair, fp_stream_t stream) {
  FP_REQUIRE(pts && scratch && out_d && out_pair, "fp_pts_diameter: null pointer");
  FP_REQUIRE(V >= 1 && V <= FP_PTS_DIAMETER_MAX_V, "fp_pts_diameter: V %d outside [1, %d]", V, FP_PTS_DIAMETER_MAX_V);
  FP_REQUIRE(scratch_bytes >= FP_PTS_DIAMETER_SCRATCH_BYTES(V), "fp_pts_diameter: scratch holds %zu bytes, %zu needed", scratch_bytes,
             (size_t)FP_PTS_DIAMETER_SCRATCH_BYTES(V));
  static_assert(sizeof(PtsPart) == 16, "layout of FP_PTS_*_SCRATCH_BYTES");
  PtsDiameterArgs a{pts, V, (int)FP_PTS_TILES(V), static_cast<PtsPart*>(scratch), out_d, out_pair};
  return launch_pts_diameter(a, ST(stream));
}

int fp_directed_hausdorff(const double* pts, int V, int query_stride, const double* transforms, int K, void* scratch,
                          size_t scratch_bytes, double* out_h, int32_t* out_arg, fp_stream_t stream) {
  FP_REQUIRE(pts && transforms && scratch && out_h && out_arg, "fp_directed_hausdorff: null pointer");
  FP_REQUIRE(K >= 1 && K <= 65535, "fp_directed_hausdorff: K %d outside [1, 65535]", K);
  FP_REQUIRE(V >= 1, "fp_directed_hausdorff: empty point array");
  FP_REQUIRE(query_stride >= 1, "fp_directed_hausdorff: query_stride %d < 1", query_stride);
  const size_t need = FP_PTS_HAUSDORFF_SCRATCH_BYTES(V, query_stride, K);
  FP_REQUIRE(scratch_bytes >= need, "fp_directed_hausdorff: scratch holds %zu bytes, %zu needed", scratch_bytes, need);
  const int nq = (int)(((long long)V + query_stride - 1) / query_stride);
  PtsHausdorffArgs a{pts, V, query_stride, nq, transforms, static_cast<PtsPart*>(scratch), out_h, out_arg};
  return launch_pts_hausdorff(a, K, ST(stream));
}

// ------------------------------------------------------------------ the five Levenberg-Marquardt solvers: the three pose refinements; fp_tsdf_track and fp_multiview_refine further down
// the argument checks the solvers share; `f` / `d` / `depth_weight`: the feature map, the depth stack and the weight of the entries that have one
static int refine_check(const char* fn, const RefineLmArgs& lm, const RefineMapArgs* f, const RefineDepthArgs* d, const double* depth_weight) {
  if (f) {
    FP_REQUIRE(f->gh >= 2 && f->gw >= 2, "%s: the feature map is %d x %d, at least 2 x 2 needed", fn, f->gh, f->gw);
    FP_REQUIRE(f->C >= 1 && f->W >= 1 && f->H >= 1, "%s: C %d, image %d x %d", fn, f->C, (int)f->W, (int)f->H);
    FP_REQUIRE(f->sb >= 0 && f->sy >= 0 && f->sx >= 0 && f->sc >= 0, "%s: negative map stride", fn);
  }
  if (d) FP_REQUIRE(d->num_images >= 1 && d->H >= 2 && d->W >= 2, "%s: %d depth images of %d x %d, at least one of 2 x 2 needed", fn, d->num_images, d->W, d->H);
  if (depth_weight) FP_REQUIRE(*depth_weight >= 0.0 && *depth_weight < INFINITY, "%s: depth_weight %g is not a finite number >= 0", fn, *depth_weight);
  FP_REQUIRE(lm.num_det >= 1 && lm.num_det <= 65535, "%s: num_det %d outside [1, 65535]", fn, lm.num_det);
  FP_REQUIRE(lm.max_points >= 1 && lm.num_rows >= 0, "%s: max_points %d, num_rows %lld", fn, lm.max_points, lm.num_rows);
  FP_REQUIRE(lm.iters >= 0 && lm.iters <= 1000, "%s: iters %d outside [0, 1000]", fn, lm.iters);
  return FP_OK;
}

// carves the scratch: states (at its start: the caller's) | partial records of `record` doubles per (detection, chunk) | valid flags (where
// `valid` is given) | err, and clears err
static int refine_carve(const char* fn, RefineLmArgs& lm, void* scratch, size_t scratch_bytes, size_t need, int record, uint8_t** valid, hipStream_t st) {
  FP_REQUIRE(scratch_bytes >= need, "%s: scratch holds %zu bytes, %zu needed", fn, scratch_bytes, need);
  lm.chunks = (lm.max_points + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK;
  char* sp = static_cast<char*>(scratch) + (size_t)FP_REFINE_STATE_BYTES * lm.num_det;
  lm.part = reinterpret_cast<double*>(sp);
  sp += 8 * (size_t)record * lm.num_det * lm.chunks;
  if (valid) {
    *valid = reinterpret_cast<uint8_t*>(sp);
    sp += (((size_t)lm.num_det * lm.max_points + 7) / 8) * 8;
  }
  lm.err = reinterpret_cast<int32_t*>(sp);
  if (hipError_t e = hipMemsetAsync(lm.err, 0, sizeof(int32_t), st); e != hipSuccess) {
    fp_set_error("%s: clear: %s", fn, hipGetErrorString(e));
    return FP_ERR_HIP;
  }
  return FP_OK;
}

// the one wait of a solver's call, after every iteration is enqueued: a bad row range or image index is reported here, never read.
// `rows_fmt`: the caller's words for a bad row range
static int refine_report(const char* fn, const RefineLmArgs& lm, int num_images, hipStream_t st,
                         const char* rows_fmt = "%s: detection %d: bank rows outside [0, %lld) or more than max_points %d",
                         const char* index_fmt = "%s: detection %d: image index outside [0, %d)") {
  int32_t bad = 0;
  if (hipError_t e = hipMemcpyWithStream(&bad, lm.err, sizeof(int32_t), hipMemcpyDeviceToHost, st); e != hipSuccess) {
    fp_set_error("%s: status read: %s", fn, hipGetErrorString(e));
    return FP_ERR_HIP;
  }
  FP_REQUIRE(bad <= 0, rows_fmt, fn, bad - 1, lm.num_rows, lm.max_points);
  FP_REQUIRE(bad == 0, index_fmt, fn, -bad - 1, num_images);
  return FP_OK;
}

static RefineLmArgs refine_lm_args(const double* cameras, const double* R_in, const double* t_in, const int32_t* row_begin, const int32_t* row_end,
                                   const float* vertices, int64_t num_rows, const int32_t* has_pose, int num_det, int max_points, int iters,
                                   double* R_out, double* t_out, double* cost_in, double* cost_out, int32_t* num_points, int32_t* iters_used,
                                   int32_t* status, double* normal_eq) {
  return RefineLmArgs{cameras, R_in, t_in, row_begin, row_end, vertices, (long long)num_rows, has_pose, num_det, max_points, iters, 0,
                      R_out, t_out, cost_in, cost_out, num_points, iters_used, status, normal_eq, nullptr, nullptr};
}

int fp_featuremetric_refine(const float* map, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int gh, int gw, int C, int W, int H,
                            const double* cameras, const double* R_in, const double* t_in, const int32_t* row_begin,
                            const int32_t* row_end, const float* feats, const float* vertices, int64_t num_rows,
                            const int32_t* has_pose, int num_det, int max_points, int iters, void* scratch, size_t scratch_bytes,
                            double* R_out, double* t_out, double* cost_in, double* cost_out, int32_t* num_points,
                            int32_t* iters_used, int32_t* status, double* normal_eq, fp_stream_t stream) {
  const char* fn = "fp_featuremetric_refine";
  FP_REQUIRE(map && cameras && R_in && t_in && row_begin && row_end && feats && vertices && has_pose && scratch && R_out && t_out &&
             cost_in && cost_out && num_points && iters_used && status, "fp_featuremetric_refine: null pointer");
  static_assert(sizeof(RefineState) <= FP_REFINE_STATE_BYTES, "FP_REFINE_STATE_BYTES");
  RefineArgs a;
  memset(&a, 0, sizeof(a));
  a.lm = refine_lm_args(cameras, R_in, t_in, row_begin, row_end, vertices, num_rows, has_pose, num_det, max_points, iters, R_out, t_out, cost_in,
                        cost_out, num_points, iters_used, status, normal_eq);
  a.f = RefineMapArgs{map, sb, sy, sx, sc, gh, gw, C, 0, (double)W, (double)H, feats, nullptr};
  TRY(refine_check(fn, a.lm, &a.f, nullptr, nullptr));
  a.state = static_cast<RefineState*>(scratch);
  TRY(refine_carve(fn, a.lm, scratch, scratch_bytes, FP_REFINE_SCRATCH_BYTES(num_det, max_points), FP_REFINE_RECORD, &a.f.valid, ST(stream)));
  TRY(launch_featuremetric_refine(a, ST(stream)));
  return refine_report(fn, a.lm, 0, ST(stream));   // no image index: err is never negative here
}

int fp_depth_refine(const float* depth, int num_images, int H, int W, const int32_t* image_index, const double* cameras,
                    const double* R_in, const double* t_in, const int32_t* row_begin, const int32_t* row_end, const float* vertices,
                    int64_t num_rows, const int32_t* has_pose, const double* tau, int num_det, int max_points, int iters,
                    void* scratch, size_t scratch_bytes, double* R_out, double* t_out, double* cost_in, double* cost_out,
                    int32_t* num_points, int32_t* iters_used, int32_t* status, double* normal_eq, fp_stream_t stream) {
  const char* fn = "fp_depth_refine";
  FP_REQUIRE(depth && image_index && cameras && R_in && t_in && row_begin && row_end && vertices && has_pose && tau && scratch && R_out &&
             t_out && cost_in && cost_out && num_points && iters_used && status, "fp_depth_refine: null pointer");
  DepthRefineArgs a;
  memset(&a, 0, sizeof(a));
  a.lm = refine_lm_args(cameras, R_in, t_in, row_begin, row_end, vertices, num_rows, has_pose, num_det, max_points, iters, R_out, t_out, cost_in,
                        cost_out, num_points, iters_used, status, normal_eq);
  a.d = RefineDepthArgs{depth, num_images, H, W, 0, image_index, tau};
  TRY(refine_check(fn, a.lm, nullptr, &a.d, nullptr));
  a.state = static_cast<RefineState*>(scratch);
  TRY(refine_carve(fn, a.lm, scratch, scratch_bytes, FP_DEPTH_REFINE_SCRATCH_BYTES(num_det, max_points), FP_REFINE_RECORD, nullptr, ST(stream)));
  TRY(launch_depth_refine(a, ST(stream)));
  return refine_report(fn, a.lm, num_images, ST(stream));
}

int fp_rgbd_refine(const float* map, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int gh, int gw, int C, int W, int H,
                   const double* feature_cameras, const double* A, const double* a_vec, const float* depth, int num_images, int Hd, int Wd,
                   const int32_t* image_index, const double* frame_cameras, const double* R_in, const double* t_in,
                   const int32_t* row_begin, const int32_t* row_end, const float* feats, const float* vertices, int64_t num_rows,
                   const int32_t* has_pose, const double* tau, double depth_weight, int num_det, int max_points, int iters,
                   void* scratch, size_t scratch_bytes, double* R_out, double* t_out, double* cost_in, double* cost_out,
                   int32_t* num_points, int32_t* num_depth_inliers, int32_t* iters_used, int32_t* status, double* normal_eq,
                   fp_stream_t stream) {
  const char* fn = "fp_rgbd_refine";
  FP_REQUIRE(map && feature_cameras && A && a_vec && depth && image_index && frame_cameras && R_in && t_in && row_begin && row_end && feats &&
             vertices && has_pose && tau && scratch && R_out && t_out && cost_in && cost_out && num_points && num_depth_inliers && iters_used &&
             status, "fp_rgbd_refine: null pointer");
  static_assert(sizeof(RgbdState) <= FP_REFINE_STATE_BYTES, "FP_REFINE_STATE_BYTES");
  RgbdRefineArgs a;
  memset(&a, 0, sizeof(a));
  a.lm = refine_lm_args(frame_cameras, R_in, t_in, row_begin, row_end, vertices, num_rows, has_pose, num_det, max_points, iters, R_out, t_out,
                        cost_in, cost_out, num_points, iters_used, status, normal_eq);
  a.f = RefineMapArgs{map, sb, sy, sx, sc, gh, gw, C, 0, (double)W, (double)H, feats, nullptr};
  a.d = RefineDepthArgs{depth, num_images, Hd, Wd, 0, image_index, tau};
  a.fcam = feature_cameras; a.A = A; a.a = a_vec; a.wd = depth_weight; a.num_depth_inliers = num_depth_inliers;
  TRY(refine_check(fn, a.lm, &a.f, &a.d, &depth_weight));
  a.state = static_cast<RgbdState*>(scratch);
  TRY(refine_carve(fn, a.lm, scratch, scratch_bytes, FP_RGBD_REFINE_SCRATCH_BYTES(num_det, max_points), 2 * FP_REFINE_RECORD, &a.f.valid, ST(stream)));
  TRY(launch_rgbd_refine(a, ST(stream)));
  return refine_report(fn, a.lm, num_images, ST(stream));
}

// ------------------------------------------------------------------ VSD
int fp_vsd_counts(const float* depth_test, int num_test, const float* depth_est, int num_est, const float* depth_gt, int num_gt,
                  int height, int width, const int32_t* pairs, const double* params, int num_pairs, const double* taus,
                  int num_taus, void* scratch, size_t scratch_bytes, int64_t* counts, fp_stream_t stream) {
  FP_REQUIRE(depth_test && depth_est && depth_gt && pairs && params && taus && scratch && counts, "fp_vsd_counts: null pointer");
  FP_REQUIRE(num_pairs >= 1, "fp_vsd_counts: num_pairs %d < 1", num_pairs);
  FP_REQUIRE(num_taus >= 1 && num_taus <= FP_VSD_MAX_TAUS, "fp_vsd_counts: num_taus %d outside [1, %d]", num_taus, FP_VSD_MAX_TAUS);
  FP_REQUIRE(height >= 1 && width >= 1 && num_test >= 1 && num_est >= 1 && num_gt >= 1,
             "fp_vsd_counts: empty image size or stack (%d x %d; %d, %d, %d images)", height, width, num_test, num_est, num_gt);
  FP_REQUIRE(scratch_bytes >= FP_VSD_SCRATCH_BYTES(num_pairs), "fp_vsd_counts: scratch holds %zu bytes, %zu needed", scratch_bytes,
             FP_VSD_SCRATCH_BYTES(num_pairs));
  VsdArgs a;
  memset(&a, 0, sizeof(a));
  for (int t = 0; t < num_taus; ++t) {
    FP_REQUIRE(taus[t] == taus[t], "fp_vsd_counts: tau %d is NaN", t);
    a.taus[t] = taus[t];
  }
  static_assert(sizeof(VsdPair) == 96, "layout of FP_VSD_SCRATCH_BYTES");
  std::vector<VsdPair> tab(num_pairs);
  const long long img = (long long)height * width;
  long long blocks = 0;
  for (int p = 0; p < num_pairs; ++p) {
    const int32_t* r = pairs + 7 * (size_t)p;
    const double* q = params + 6 * (size_t)p;
    FP_REQUIRE(r[0] >= 0 && r[0] < num_test && r[1] >= 0 && r[1] < num_est && r[2] >= 0 && r[2] < num_gt,
               "fp_vsd_counts: pair %d: indices (%d, %d, %d) outside (%d, %d, %d)", p, r[0], r[1], r[2], num_test, num_est, num_gt);
    FP_REQUIRE(r[3] >= 0 && r[4] >= 0 && r[3] <= r[5] + 1 && r[4] <= r[6] + 1 && r[5] < width && r[6] < height,
               "fp_vsd_counts: pair %d: box (%d, %d, %d, %d) outside the %d x %d image", p, r[3], r[4], r[5], r[6], width, height);
    FP_REQUIRE(q[0] > 0 && q[1] > 0 && q[5] > 0, "fp_vsd_counts: pair %d: fx, fy and the diameter must be > 0", p);
    FP_REQUIRE(q[4] == q[4], "fp_vsd_counts: pair %d: delta is NaN", p);
    VsdPair& v = tab[p];
    v.test_off = r[0] * img, v.est_off = r[1] * img, v.gt_off = r[2] * img;
    v.x0 = r[3], v.y0 = r[4];
    v.bw = r[5] - r[3] + 1, v.bh = r[6] - r[4] + 1;
    if (v.bw == 0 || v.bh == 0) v.bw = v.bh = 0;
    v.blk0 = blocks;
    v.fx = q[0], v.fy = q[1], v.cx = q[2], v.cy = q[3], v.diameter = q[5];
    v.delta = (float)q[4];
    v.pad = 0;
    blocks += ((long long)v.bw * v.bh + FP_VSD_BLOCK_PIXELS - 1) / FP_VSD_BLOCK_PIXELS;
  }
  FP_REQUIRE(blocks <= 0x7fffffffll, "fp_vsd_counts: %lld workgroups exceed the grid", blocks);
  HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * (size_t)num_pairs * (2 + num_taus), ST(stream)), "fp_vsd_counts: zeroing");
  if (blocks == 0) return FP_OK;
  // the table lives in this frame, so the copy completes before it goes out of scope
  HIP_TRY(hipMemcpyWithStream(scratch, tab.data(), sizeof(VsdPair) * (size_t)num_pairs, hipMemcpyHostToDevice, ST(stream)), "fp_vsd_counts: table upload");
  a.depth_test = depth_test, a.depth_est = depth_est, a.depth_gt = depth_gt;
  a.pairs = reinterpret_cast<const VsdPair*>(scratch);
  a.num_pairs = num_pairs, a.width = width, a.num_taus = num_taus;
  a.counts = reinterpret_cast<long long*>(counts);
  return launch_vsd_counts(a, blocks, ST(stream));
}

// ------------------------------------------------------------------ GT annotations from renders
int fp_gt_visibility(const float* depth_test, int num_test, int height, int width, const float* depth_obj, int render_height,
                     int render_width, const int32_t* inst, const double* params, int num_inst, void* scratch, size_t scratch_bytes,
                     int32_t* out, uint8_t* mask, uint8_t* mask_visib, fp_stream_t stream) {
  FP_REQUIRE(depth_test && depth_obj && inst && params && scratch && out && mask && mask_visib, "fp_gt_visibility: null pointer");
  FP_REQUIRE(num_inst >= 1 && num_inst <= FP_GT_VIS_MAX_INST, "fp_gt_visibility: num_inst %d outside [1, %d]", num_inst, FP_GT_VIS_MAX_INST);
  FP_REQUIRE(height >= 1 && width >= 1 && num_test >= 1 && render_height >= 1 && render_width >= 1,
             "fp_gt_visibility: empty image, render or stack (%d x %d in %d x %d; %d images)", width, height, render_width, render_height, num_test);
  FP_REQUIRE((long long)render_width * render_height <= 0x7fffffffll, "fp_gt_visibility: a render of %d x %d has more than 2^31 - 1 pixels",
             render_width, render_height);
  FP_REQUIRE(scratch_bytes >= FP_GT_VIS_SCRATCH_BYTES(num_inst), "fp_gt_visibility: scratch holds %zu bytes, %zu needed", scratch_bytes,
             FP_GT_VIS_SCRATCH_BYTES(num_inst));
  static_assert(sizeof(GtVisInst) == 80, "layout of FP_GT_VIS_SCRATCH_BYTES");
  std::vector<GtVisInst> tab(num_inst);
  const long long img = (long long)height * width;
  long long blocks = 0;
  for (int p = 0; p < num_inst; ++p) {
    const int32_t* r = inst + 7 * (size_t)p;
    const double* q = params + 5 * (size_t)p;
    FP_REQUIRE(r[0] >= 0 && r[0] < num_test, "fp_gt_visibility: instance %d: test index %d outside [0, %d)", p, r[0], num_test);
    FP_REQUIRE(r[1] >= 0 && r[2] >= 0 && r[1] <= (long long)r[3] + 1 && r[2] <= (long long)r[4] + 1 && r[3] < render_width && r[4] < render_height,
               "fp_gt_visibility: instance %d: box (%d, %d, %d, %d) outside the %d x %d render", p, r[1], r[2], r[3], r[4], render_width, render_height);
    FP_REQUIRE(r[5] >= 0 && r[6] >= 0 && (long long)r[5] + width <= render_width && (long long)r[6] + height <= render_height,
               "fp_gt_visibility: instance %d: the %d x %d image at (%d, %d) leaves the %d x %d render", p, width, height, r[5], r[6],
               render_width, render_height);
    FP_REQUIRE(q[0] > 0 && q[1] > 0, "fp_gt_visibility: instance %d: fx and fy must be > 0", p);
    FP_REQUIRE(q[4] == q[4], "fp_gt_visibility: instance %d: delta is NaN", p);
    GtVisInst& v = tab[p];
    v.test_off = r[0] * img;
    v.x0 = r[1], v.y0 = r[2];
    v.bw = r[3] - r[1] + 1, v.bh = r[4] - r[2] + 1;
    if (v.bw == 0 || v.bh == 0) v.bw = v.bh = 0;
    v.ox = r[5], v.oy = r[6];
    v.blk0 = blocks;
    v.fx = q[0], v.fy = q[1], v.cx = q[2], v.cy = q[3];
    v.delta = (float)q[4];
    v.pad = 0;
    blocks += ((long long)v.bw * v.bh + FP_GT_VIS_BLOCK_PIXELS - 1) / FP_GT_VIS_BLOCK_PIXELS;
  }
  FP_REQUIRE(blocks <= 0x7fffffffll, "fp_gt_visibility: %lld workgroups exceed the grid", blocks);
  const size_t mask_bytes = (size_t)num_inst * (size_t)img;
  HIP_TRY(hipMemsetAsync(mask, 0, mask_bytes, ST(stream)), "fp_gt_visibility: zeroing mask");
  HIP_TRY(hipMemsetAsync(mask_visib, 0, mask_bytes, ST(stream)), "fp_gt_visibility: zeroing mask_visib");
  // the table lives in this frame, so the copy completes before it goes out of scope
  HIP_TRY(hipMemcpyWithStream(scratch, tab.data(), sizeof(GtVisInst) * (size_t)num_inst, hipMemcpyHostToDevice, ST(stream)), "fp_gt_visibility: table upload");
  GtVisArgs a;
  memset(&a, 0, sizeof(a));
  a.depth_test = depth_test, a.depth_obj = depth_obj;
  a.inst = reinterpret_cast<const GtVisInst*>(scratch);
  a.num_inst = num_inst, a.height = height, a.width = width, a.render_h = render_height, a.render_w = render_width;
  a.out = out, a.mask = mask, a.mask_visib = mask_visib;
  return launch_gt_visibility(a, blocks, ST(stream));
}

// ------------------------------------------------------------------ TSDF fusion and surface extraction
}  // extern "C"

// the checks the three TSDF entries share: the box (origin, voxel size) and the dimensions
static int tsdf_volume(const char* who, const double* box, int nx, int ny, int nz, int min_dim, TsdfVolume& vol) {
  FP_REQUIRE(nx >= min_dim && ny >= min_dim && nz >= min_dim && nx <= FP_TSDF_MAX_DIM && ny <= FP_TSDF_MAX_DIM && nz <= FP_TSDF_MAX_DIM,
             "%s: dimensions %d x %d x %d outside [%d, %d]", who, nx, ny, nz, min_dim, FP_TSDF_MAX_DIM);
  FP_REQUIRE((long long)nx * ny * nz <= FP_TSDF_MAX_VOXELS, "%s: %d x %d x %d voxels exceed %lld", who, nx, ny, nz, (long long)FP_TSDF_MAX_VOXELS);
  memset(&vol, 0, sizeof(vol));
  vol.nx = nx, vol.ny = ny, vol.nz = nz;
  if (box != nullptr) {
    FP_REQUIRE(std::isfinite(box[0]) && std::isfinite(box[1]) && std::isfinite(box[2]) && std::isfinite(box[3]) && box[3] > 0,
               "%s: the origin must be finite and the voxel size finite and > 0", who);
    vol.ox = box[0], vol.oy = box[1], vol.oz = box[2], vol.h = box[3];
  }
  return FP_OK;
}

extern "C" {

int fp_tsdf_integrate(const float* depth, const uint8_t* mask, const uint8_t* rgb, int num_frames, int height, int width,
                      const double* frames, const double* box, int nx, int ny, int nz, double trunc_mm, void* scratch,
                      size_t scratch_bytes, float* sdf_sum, int32_t* sdf_cnt, float* rgb_sum, int32_t* rgb_cnt, fp_stream_t stream) {
  FP_REQUIRE(depth && mask && rgb && frames && box && scratch && sdf_sum && sdf_cnt && rgb_sum && rgb_cnt, "fp_tsdf_integrate: null pointer");
  FP_REQUIRE(num_frames >= 1 && num_frames <= FP_TSDF_MAX_FRAMES, "fp_tsdf_integrate: num_frames %d outside [1, %d]", num_frames, FP_TSDF_MAX_FRAMES);
  FP_REQUIRE(height >= 1 && width >= 1 && (long long)height * width <= 0x7fffffffll, "fp_tsdf_integrate: images of %d x %d pixels", width, height);
  FP_REQUIRE(std::isfinite(trunc_mm) && trunc_mm > 0, "fp_tsdf_integrate: the truncation distance must be finite and > 0");
  FP_REQUIRE(scratch_bytes >= FP_TSDF_SCRATCH_BYTES(num_frames), "fp_tsdf_integrate: scratch holds %zu bytes, %zu needed", scratch_bytes,
             FP_TSDF_SCRATCH_BYTES(num_frames));
  static_assert(sizeof(TsdfFrame) == 8 * FP_TSDF_FRAME_DOUBLES, "layout of FP_TSDF_SCRATCH_BYTES: a frame row is the device record");
  TsdfIntegrateArgs a;
  memset(&a, 0, sizeof(a));
  TRY(tsdf_volume("fp_tsdf_integrate", box, nx, ny, nz, 1, a.vol));
  for (int f = 0; f < num_frames; ++f) {
    const double* q = frames + (size_t)FP_TSDF_FRAME_DOUBLES * f;
    for (int c = 0; c < FP_TSDF_FRAME_DOUBLES; ++c)
      FP_REQUIRE(std::isfinite(q[c]), "fp_tsdf_integrate: frame %d: entry %d of its camera and pose is not finite", f, c);
    FP_REQUIRE(q[0] > 0 && q[1] > 0, "fp_tsdf_integrate: frame %d: fx and fy must be > 0", f);
  }
  // the caller's table is the device record as it stands; the call waits for the copy, so the caller may free it on return
  HIP_TRY(hipMemcpyWithStream(scratch, frames, sizeof(TsdfFrame) * (size_t)num_frames, hipMemcpyHostToDevice, ST(stream)), "fp_tsdf_integrate: table upload");
  a.depth = depth, a.mask = mask, a.rgb = rgb;
  a.frames = reinterpret_cast<const TsdfFrame*>(scratch);
  a.num_frames = num_frames, a.height = height, a.width = width;
  a.tau = trunc_mm;
  a.sdf_sum = sdf_sum, a.sdf_cnt = sdf_cnt, a.rgb_sum = rgb_sum, a.rgb_cnt = rgb_cnt;
  return launch_tsdf_integrate(a, ST(stream));
}

int fp_tsdf_count_triangles(const float* sdf_sum, const int32_t* sdf_cnt, int nx, int ny, int nz, int min_count, int32_t* counts,
                            fp_stream_t stream) {
  FP_REQUIRE(sdf_sum && sdf_cnt && counts, "fp_tsdf_count_triangles: null pointer");
  FP_REQUIRE(min_count >= 1, "fp_tsdf_count_triangles: min_count %d must be >= 1", min_count);
  TsdfExtractArgs a;
  memset(&a, 0, sizeof(a));
  TRY(tsdf_volume("fp_tsdf_count_triangles", nullptr, nx, ny, nz, 2, a.vol));
  a.sdf_sum = sdf_sum, a.sdf_cnt = sdf_cnt, a.min_count = min_count, a.counts = counts;
  return launch_tsdf_extract(a, false, ST(stream));
}

int fp_tsdf_emit_triangles(const float* sdf_sum, const int32_t* sdf_cnt, const float* rgb_sum, const int32_t* rgb_cnt, const double* box,
                           int nx, int ny, int nz, int min_count, const int64_t* offsets, int64_t num_triangles, int64_t* keys,
                           float* positions, float* colors, fp_stream_t stream) {
  FP_REQUIRE(sdf_sum && sdf_cnt && rgb_sum && rgb_cnt && box && offsets, "fp_tsdf_emit_triangles: null pointer");
  FP_REQUIRE(min_count >= 1, "fp_tsdf_emit_triangles: min_count %d must be >= 1", min_count);
  FP_REQUIRE(num_triangles >= 0 && num_triangles <= FP_TSDF_MAX_TRIANGLES, "fp_tsdf_emit_triangles: %lld triangles outside [0, %lld]",
             (long long)num_triangles, (long long)FP_TSDF_MAX_TRIANGLES);
  FP_REQUIRE(num_triangles == 0 || (keys && positions && colors), "fp_tsdf_emit_triangles: null output");
  TsdfExtractArgs a;
  memset(&a, 0, sizeof(a));
  TRY(tsdf_volume("fp_tsdf_emit_triangles", box, nx, ny, nz, 2, a.vol));
  if (num_triangles == 0) return FP_OK;
  a.sdf_sum = sdf_sum, a.sdf_cnt = sdf_cnt, a.rgb_sum = rgb_sum, a.rgb_cnt = rgb_cnt, a.min_count = min_count;
  a.offsets = reinterpret_cast<const long long*>(offsets), a.num_triangles = num_triangles;
  a.keys = reinterpret_cast<long long*>(keys), a.pos = positions, a.col = colors;
  return launch_tsdf_extract(a, true, ST(stream));
}

int fp_tsdf_diffuse(float* val, uint8_t* state, float* val_tmp, uint8_t* state_tmp, int channels, int nx, int ny, int nz, int iters,
                    fp_stream_t stream) {
  FP_REQUIRE(val && state && val_tmp && state_tmp, "fp_tsdf_diffuse: null pointer");
  FP_REQUIRE(val != val_tmp && state != state_tmp, "fp_tsdf_diffuse: the scratch buffers must not be the buffers themselves");
  FP_REQUIRE(channels == 1 || channels == 3, "fp_tsdf_diffuse: channels %d must be 1 or 3", channels);
  FP_REQUIRE(iters >= 0 && iters <= FP_TSDF_DIFFUSE_MAX_ITERS, "fp_tsdf_diffuse: iters %d outside [0, %d]", iters, FP_TSDF_DIFFUSE_MAX_ITERS);
  TsdfVolume vol;
  TRY(tsdf_volume("fp_tsdf_diffuse", nullptr, nx, ny, nz, 1, vol));
  TsdfDiffuseArgs a;
  memset(&a, 0, sizeof(a));
  a.channels = channels, a.nx = nx, a.ny = ny, a.nz = nz;
  for (int t = 0; t < iters; ++t) {                                 // even iterations read the buffers, odd ones the scratch
    const bool fwd = t % 2 == 0;
    a.val = fwd ? val : val_tmp, a.state = fwd ? state : state_tmp;
    a.val_out = fwd ? val_tmp : val, a.state_out = fwd ? state_tmp : state;
    TRY(launch_tsdf_diffuse(a, ST(stream)));
  }
  if (iters % 2 == 1) {                                             // the result lands in val / state
    const size_t n = (size_t)nx * ny * nz;
    HIP_TRY(hipMemcpyAsync(val, val_tmp, sizeof(float) * n * channels, hipMemcpyDeviceToDevice, ST(stream)), "fp_tsdf_diffuse: copy back");
    HIP_TRY(hipMemcpyAsync(state, state_tmp, n, hipMemcpyDeviceToDevice, ST(stream)), "fp_tsdf_diffuse: copy back");
  }
  return FP_OK;
}

// ------------------------------------------------------------------ mesh simplification (simplify.hip)
}  // extern "C"

// the checks the two mesh entries share: the grid (origin, cell size) and its dimensions
static int mesh_grid(const char* who, const double* grid, int nx, int ny, int nz, MeshGrid& g) {
  FP_REQUIRE(grid != nullptr, "%s: null pointer", who);
  FP_REQUIRE(nx >= 1 && ny >= 1 && nz >= 1 && nx <= FP_MESH_MAX_DIM && ny <= FP_MESH_MAX_DIM && nz <= FP_MESH_MAX_DIM,
             "%s: dimensions %d x %d x %d outside [1, %d]", who, nx, ny, nz, FP_MESH_MAX_DIM);
  FP_REQUIRE(std::isfinite(grid[0]) && std::isfinite(grid[1]) && std::isfinite(grid[2]) && std::isfinite(grid[3]) && grid[3] > 0,
             "%s: the origin must be finite and the cell size finite and > 0", who);
  memset(&g, 0, sizeof(g));
  g.ox = grid[0], g.oy = grid[1], g.oz = grid[2], g.c = grid[3];
  g.nx = nx, g.ny = ny, g.nz = nz;
  return FP_OK;
}

extern "C" {

int fp_mesh_cell_keys(const float* vertices, int64_t num_vertices, const double* grid, int nx, int ny, int nz, int64_t* keys,
                      fp_stream_t stream) {
  FP_REQUIRE(num_vertices >= 0 && num_vertices <= FP_MESH_MAX_ROWS, "fp_mesh_cell_keys: %lld vertices outside [0, %lld]",
             (long long)num_vertices, (long long)FP_MESH_MAX_ROWS);
  FP_REQUIRE(num_vertices == 0 || (vertices && keys), "fp_mesh_cell_keys: null pointer");
  MeshKeysArgs a;
  memset(&a, 0, sizeof(a));
  TRY(mesh_grid("fp_mesh_cell_keys", grid, nx, ny, nz, a.grid));
  a.verts = vertices, a.num_vertices = num_vertices, a.keys = reinterpret_cast<long long*>(keys);
  return launch_mesh_cell_keys(a, ST(stream));
}

int fp_mesh_cluster(const float* vertices, const float* colors, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                    const int64_t* cell_keys, int64_t num_cells, const int64_t* vert_order, const int64_t* vert_begin,
                    const int64_t* corner_order, const int64_t* corner_begin, const double* grid, int nx, int ny, int nz, double eig_eps,
                    float* positions, float* out_colors, double* quadrics, double* means, double* err, int32_t* status,
                    fp_stream_t stream) {
  const char* fn = "fp_mesh_cluster";
  FP_REQUIRE(num_vertices >= 1 && num_vertices <= FP_MESH_MAX_ROWS, "%s: %lld vertices outside [1, %lld]", fn, (long long)num_vertices,
             (long long)FP_MESH_MAX_ROWS);
  FP_REQUIRE(num_faces >= 0 && 3 * num_faces <= FP_MESH_MAX_ROWS, "%s: %lld faces: 3 F outside [0, %lld]", fn, (long long)num_faces,
             (long long)FP_MESH_MAX_ROWS);
  FP_REQUIRE(num_cells >= 1 && num_cells <= num_vertices, "%s: %lld cells outside [1, %lld vertices]", fn, (long long)num_cells,
             (long long)num_vertices);
  FP_REQUIRE(vertices && colors && cell_keys && vert_order && vert_begin && corner_begin && positions && out_colors && quadrics && means &&
             err && status, "%s: null pointer", fn);
  FP_REQUIRE(num_faces == 0 || (faces && corner_order), "%s: null faces or corner_order with %lld faces", fn, (long long)num_faces);
  FP_REQUIRE(std::isfinite(eig_eps) && eig_eps >= 0 && eig_eps < 1, "%s: eig_eps must lie in [0, 1)", fn);
  MeshClusterArgs a;
  memset(&a, 0, sizeof(a));
  TRY(mesh_grid(fn, grid, nx, ny, nz, a.grid));
  a.verts = vertices, a.colors = colors, a.num_vertices = num_vertices;
  a.faces = faces, a.num_faces = num_faces;
  a.cell_keys = reinterpret_cast<const long long*>(cell_keys), a.num_cells = num_cells;
  a.vert_order = reinterpret_cast<const long long*>(vert_order), a.vert_begin = reinterpret_cast<const long long*>(vert_begin);
  a.corner_order = reinterpret_cast<const long long*>(corner_order), a.corner_begin = reinterpret_cast<const long long*>(corner_begin);
  a.eig_eps = eig_eps;
  a.pos = positions, a.col = out_colors, a.quadrics = quadrics, a.means = means, a.err = err, a.status = status;
  return launch_mesh_cluster(a, ST(stream));
}

int fp_tsdf_track(const float* sdf_sum, const int32_t* sdf_cnt, const double* box, int nx, int ny, int nz, int min_count, double trunc_mm,
                  const float* points, int64_t num_rows, const int32_t* row_begin, const int32_t* row_end, const double* R_in,
                  const double* t_in, const int32_t* has_pose, const double* max_dist, int num_det, int max_points, int iters,
                  void* scratch, size_t scratch_bytes, double* R_out, double* t_out, double* cost_in, double* cost_out,
                  int32_t* num_points, int32_t* iters_used, int32_t* status, double* normal_eq, fp_stream_t stream) {
  const char* fn = "fp_tsdf_track";
  FP_REQUIRE(sdf_sum && sdf_cnt && box && points && row_begin && row_end && R_in && t_in && has_pose && max_dist && scratch && R_out && t_out &&
             cost_in && cost_out && num_points && iters_used && status, "fp_tsdf_track: null pointer");
  FP_REQUIRE(min_count >= 1, "fp_tsdf_track: min_count %d must be >= 1", min_count);
  FP_REQUIRE(std::isfinite(trunc_mm) && trunc_mm > 0, "fp_tsdf_track: the truncation distance must be finite and > 0");
  TsdfTrackArgs a;
  memset(&a, 0, sizeof(a));
  TRY(tsdf_volume(fn, box, nx, ny, nz, 2, a.vol));
  a.lm = refine_lm_args(nullptr, R_in, t_in, row_begin, row_end, points, num_rows, has_pose, num_det, max_points, iters, R_out, t_out, cost_in,
                        cost_out, num_points, iters_used, status, normal_eq);
  TRY(refine_check(fn, a.lm, nullptr, nullptr, nullptr));
  a.sdf_sum = sdf_sum, a.sdf_cnt = sdf_cnt, a.min_count = min_count, a.tau = trunc_mm, a.max_dist = max_dist;
  a.state = static_cast<RefineState*>(scratch);
  TRY(refine_carve(fn, a.lm, scratch, scratch_bytes, FP_TSDF_TRACK_SCRATCH_BYTES(num_det, max_points), FP_REFINE_RECORD, nullptr, ST(stream)));
  TRY(launch_tsdf_track(a, ST(stream)));
  // no image index: err is never negative here
  return refine_report(fn, a.lm, 0, ST(stream), "%s: problem %d: rows outside [0, %lld) or more than max_points %d");
}

int fp_tsdf_track_rgb(const float* sdf_sum, const int32_t* sdf_cnt, const float* rgb_sum, const int32_t* rgb_cnt, const double* box, int nx,
                      int ny, int nz, int min_count, double trunc_mm, const float* points, const float* colors, int64_t num_rows,
                      const int32_t* row_begin, const int32_t* row_end, const double* R_in, const double* t_in, const int32_t* has_pose,
                      const double* max_dist, double color_weight, double color_max, int num_det, int max_points, int iters, void* scratch,
                      size_t scratch_bytes, double* R_out, double* t_out, double* cost_in, double* cost_out, int32_t* num_points,
                      int32_t* iters_used, int32_t* status, double* normal_eq, fp_stream_t stream) {
  const char* fn = "fp_tsdf_track_rgb";
  FP_REQUIRE(sdf_sum && sdf_cnt && rgb_sum && rgb_cnt && box && points && colors && row_begin && row_end && R_in && t_in && has_pose && max_dist &&
             scratch && R_out && t_out && cost_in && cost_out && num_points && iters_used && status, "fp_tsdf_track_rgb: null pointer");
  FP_REQUIRE(min_count >= 1, "fp_tsdf_track_rgb: min_count %d must be >= 1", min_count);
  FP_REQUIRE(std::isfinite(trunc_mm) && trunc_mm > 0, "fp_tsdf_track_rgb: the truncation distance must be finite and > 0");
  FP_REQUIRE(std::isfinite(color_weight) && color_weight > 0, "fp_tsdf_track_rgb: color_weight must be finite and > 0");
  FP_REQUIRE(std::isfinite(color_max) && color_max > 0, "fp_tsdf_track_rgb: color_max must be finite and > 0");
  TsdfTrackRgbArgs a;
  memset(&a, 0, sizeof(a));
  TRY(tsdf_volume(fn, box, nx, ny, nz, 2, a.g.vol));
  a.g.lm = refine_lm_args(nullptr, R_in, t_in, row_begin, row_end, points, num_rows, has_pose, num_det, max_points, iters, R_out, t_out, cost_in,
                          cost_out, num_points, iters_used, status, normal_eq);
  TRY(refine_check(fn, a.g.lm, nullptr, nullptr, nullptr));
  a.g.sdf_sum = sdf_sum, a.g.sdf_cnt = sdf_cnt, a.g.min_count = min_count, a.g.tau = trunc_mm, a.g.max_dist = max_dist;
  a.rgb_sum = rgb_sum, a.rgb_cnt = rgb_cnt, a.colors = colors, a.color_weight = color_weight, a.color_max = color_max;
  a.g.state = static_cast<RefineState*>(scratch);
  TRY(refine_carve(fn, a.g.lm, scratch, scratch_bytes, FP_TSDF_TRACK_SCRATCH_BYTES(num_det, max_points), FP_REFINE_RECORD, nullptr, ST(stream)));
  TRY(launch_tsdf_track_rgb(a, ST(stream)));
  return refine_report(fn, a.g.lm, 0, ST(stream), "%s: problem %d: rows outside [0, %lld) or more than max_points %d");
}

int fp_multiview_refine(const float* points, const double* targets, const int32_t* view_index, int64_t num_rows, const double* view_cam,
                        const double* view_T, int num_views, const int32_t* row_begin, const int32_t* row_end, const double* R_in,
                        const double* t_in, const int32_t* has_pose, double huber_px, int num_det, int max_points, int iters, void* scratch,
                        size_t scratch_bytes, double* R_out, double* t_out, double* cost_in, double* cost_out, int32_t* num_points,
                        int32_t* iters_used, int32_t* status, double* normal_eq, fp_stream_t stream) {
  const char* fn = "fp_multiview_refine";
  FP_REQUIRE(points && targets && view_index && view_cam && view_T && row_begin && row_end && R_in && t_in && has_pose && scratch && R_out &&
             t_out && cost_in && cost_out && num_points && iters_used && status, "fp_multiview_refine: null pointer");
  FP_REQUIRE(num_views >= 1, "fp_multiview_refine: num_views %d must be >= 1", num_views);
  FP_REQUIRE(std::isfinite(huber_px) && huber_px > 0, "fp_multiview_refine: huber_px must be finite and > 0");
  MultiviewArgs a;
  memset(&a, 0, sizeof(a));
  a.lm = refine_lm_args(nullptr, R_in, t_in, row_begin, row_end, points, num_rows, has_pose, num_det, max_points, iters, R_out, t_out, cost_in,
                        cost_out, num_points, iters_used, status, normal_eq);
  TRY(refine_check(fn, a.lm, nullptr, nullptr, nullptr));
  a.target = targets, a.view = view_index, a.view_cam = view_cam, a.view_T = view_T, a.num_views = num_views, a.delta = huber_px;
  a.state = static_cast<RefineState*>(scratch);
  TRY(refine_carve(fn, a.lm, scratch, scratch_bytes, FP_DEPTH_REFINE_SCRATCH_BYTES(num_det, max_points), FP_REFINE_RECORD, nullptr, ST(stream)));
  TRY(launch_multiview_refine(a, ST(stream)));
  return refine_report(fn, a.lm, num_views, ST(stream), "%s: problem %d: rows outside [0, %lld) or more than max_points %d",
                       "%s: problem %d: a row's view index outside [0, %d)");
}

// ------------------------------------------------------------------ silhouette refinement (include/foundpose_amd_mask_refine.h)
int fp_mask_distance(const uint8_t* masks, int num_masks, int H, int W, int32_t* d2, fp_stream_t stream) {
  FP_REQUIRE(masks && d2, "fp_mask_distance: null pointer");
  FP_REQUIRE(num_masks >= 1 && num_masks <= 65535, "fp_mask_distance: num_masks %d outside [1, 65535]", num_masks);
  FP_REQUIRE(H >= 1 && H <= FP_MASK_MAX_SIDE && W >= 1 && W <= FP_MASK_MAX_SIDE, "fp_mask_distance: masks of %d x %d, sides in [1, %d] needed", W, H,
             FP_MASK_MAX_SIDE);
  return launch_mask_distance(MaskDistanceArgs{masks, d2, num_masks, H, W}, ST(stream));
}

int fp_mask_refine(const int32_t* d2, int H, int W, const int32_t* contour, int64_t num_contour, const int32_t* contour_begin,
                   const int32_t* contour_end, const double* cameras, const double* R_in, const double* t_in, const int32_t* row_begin,
                   const int32_t* row_end, const float* vertices, int64_t num_rows, const int32_t* has_pose, double huber_px, int num_det,
                   int max_points, int max_contour, int iters, void* scratch, size_t scratch_bytes, double* R_out, double* t_out,
                   double* cost_in, double* cost_out, int32_t* num_points, int32_t* iters_used, int32_t* status, double* normal_eq,
                   fp_stream_t stream) {
  const char* fn = "fp_mask_refine";
  FP_REQUIRE(d2 && contour && contour_begin && contour_end && cameras && R_in && t_in && row_begin && row_end && vertices && has_pose && scratch &&
             R_out && t_out && cost_in && cost_out && num_points && iters_used && status, "fp_mask_refine: null pointer");
  FP_REQUIRE(H >= 1 && H <= FP_MASK_MAX_SIDE && W >= 1 && W <= FP_MASK_MAX_SIDE, "fp_mask_refine: masks of %d x %d, sides in [1, %d] needed", W, H,
             FP_MASK_MAX_SIDE);
  FP_REQUIRE(num_contour >= 0 && num_contour <= 0x7fffffffll && max_contour >= 1, "fp_mask_refine: num_contour %lld, max_contour %d",
             (long long)num_contour, max_contour);
  FP_REQUIRE(std::isfinite(huber_px) && huber_px > 0, "fp_mask_refine: huber_px must be finite and > 0");
  static_assert(sizeof(MaskRefineState) <= FP_REFINE_STATE_BYTES, "FP_REFINE_STATE_BYTES");
  MaskRefineArgs a;
  memset(&a, 0, sizeof(a));
  a.lm = refine_lm_args(cameras, R_in, t_in, row_begin, row_end, vertices, num_rows, has_pose, num_det, max_points, iters, R_out, t_out, cost_in,
                        cost_out, num_points, iters_used, status, normal_eq);
  TRY(refine_check(fn, a.lm, nullptr, nullptr, nullptr));
  a.d2 = d2, a.H = H, a.W = W, a.contour = contour, a.cbegin = contour_begin, a.cend = contour_end, a.num_contour = num_contour;
  a.max_contour = max_contour, a.bchunks = (max_contour + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK, a.delta = huber_px;
  a.state = static_cast<MaskRefineState*>(scratch);
  // states | forward records | err (refine_carve), then what this solver adds: backward records | u | v | in-front flags
  TRY(refine_carve(fn, a.lm, scratch, scratch_bytes, FP_MASK_REFINE_SCRATCH_BYTES(num_det, max_points, max_contour), FP_REFINE_RECORD, nullptr, ST(stream)));
  char* sp = reinterpret_cast<char*>(a.lm.err) + 8;
  a.bpart = reinterpret_cast<double*>(sp);
  sp += 8 * (size_t)FP_REFINE_RECORD * num_det * a.bchunks;
  a.pu = reinterpret_cast<double*>(sp);
  sp += 8 * (size_t)num_det * max_points;
  a.pv = reinterpret_cast<double*>(sp);
  sp += 8 * (size_t)num_det * max_points;
  a.pf = reinterpret_cast<int32_t*>(sp);
  TRY(launch_mask_refine(a, ST(stream)));
  return refine_report(fn, a.lm, (int)num_contour, ST(stream), "%s: detection %d: bank rows outside [0, %lld) or more than max_points %d",
                       "%s: detection %d: contour rows outside [0, %d] or more than max_contour");
}

// ------------------------------------------------------------------ mask proposals from depth
}  // extern "C"

// the checks the two depth entries share; the frame table goes into `tab`
static int depth_frames(const char* who, const void* depth, int num_frames, int height, int width, const double* cameras, double max_depth_mm,
                        std::vector<DpFrame>& tab) {
  FP_REQUIRE(depth && cameras, "%s: null pointer", who);
  FP_REQUIRE(num_frames >= 1 && num_frames <= FP_DEPTH_MAX_FRAMES, "%s: num_frames %d outside [1, %d]", who, num_frames, FP_DEPTH_MAX_FRAMES);
  FP_REQUIRE(height >= 1 && width >= 1 && (long long)height * width <= 0x7fffffffll, "%s: an image of %d x %d (1 .. 2^31 - 1 pixels)", who, width, height);
  FP_REQUIRE(max_depth_mm >= 0.0 && std::isfinite(max_depth_mm), "%s: max_depth_mm must be finite and >= 0", who);
  tab.resize(num_frames);
  for (int f = 0; f < num_frames; ++f) {
    const double* c = cameras + 4 * (size_t)f;
    FP_REQUIRE(std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]) && std::isfinite(c[3]) && c[0] > 0 && c[1] > 0,
               "%s: frame %d: the camera must be finite with fx, fy > 0", who, f);
    memset(&tab[f], 0, sizeof(DpFrame));
    tab[f].fx = c[0], tab[f].fy = c[1], tab[f].cx = c[2], tab[f].cy = c[3];
  }
  return FP_OK;
}

extern "C" {

int fp_depth_plane_fit(const float* depth, int num_frames, int height, int width, const double* cameras, const uint64_t* frame_keys,
                       const double* prior_planes, const int32_t* num_prior, int hypotheses, int stride, double plane_thresh_mm,
                       double max_depth_mm, double min_plane_share, uint64_t seed, void* scratch, size_t scratch_bytes,
                       double* plane_out, int32_t* info, int32_t* hyp_counts, fp_stream_t stream) {
  FP_REQUIRE(frame_keys && prior_planes && num_prior && scratch && plane_out && info, "fp_depth_plane_fit: null pointer");
  std::vector<DpFrame> tab;
  TRY(depth_frames("fp_depth_plane_fit", depth, num_frames, height, width, cameras, max_depth_mm, tab));
  FP_REQUIRE(hypotheses >= 1 && hypotheses <= FP_DEPTH_MAX_HYPOTHESES, "fp_depth_plane_fit: hypotheses %d outside [1, %d]", hypotheses, FP_DEPTH_MAX_HYPOTHESES);
  FP_REQUIRE(stride >= 1 && stride <= 64, "fp_depth_plane_fit: stride %d outside [1, 64]", stride);
  FP_REQUIRE(plane_thresh_mm > 0.0 && std::isfinite(plane_thresh_mm), "fp_depth_plane_fit: plane_thresh_mm must be finite and > 0");
  FP_REQUIRE(min_plane_share >= 0.0 && min_plane_share <= 1.0, "fp_depth_plane_fit: min_plane_share outside [0, 1]");
  const size_t hw = (size_t)height * width, n = (size_t)num_frames;
  FP_REQUIRE(scratch_bytes >= FP_DEPTH_PLANE_SCRATCH_BYTES(n, hw, hypotheses), "fp_depth_plane_fit: scratch holds %zu bytes, %zu needed",
             scratch_bytes, FP_DEPTH_PLANE_SCRATCH_BYTES(n, hw, hypotheses));
  static_assert(sizeof(DpFrame) == 48, "layout of the frame table");
  for (int f = 0; f < num_frames; ++f) tab[f].key = frame_keys[f];
  char* s = reinterpret_cast<char*>(scratch);
  DpPlaneArgs a;
  memset(&a, 0, sizeof(a));
  a.depth = depth, a.prior = prior_planes, a.num_prior = num_prior;
  a.n = num_frames, a.h = height, a.w = width, a.hyp = hypotheses, a.stride = stride;
  a.chunks = (int)((hw + FP_DEPTH_PLANE_CHUNK - 1) / FP_DEPTH_PLANE_CHUNK);
  a.thresh = plane_thresh_mm, a.max_depth = max_depth_mm, a.min_share = min_plane_share, a.seed = seed;
  a.frames = reinterpret_cast<const DpFrame*>(s);
  a.cnt2 = reinterpret_cast<int*>(s + 64 * n);
  a.state = reinterpret_cast<double*>(s + 128 * n);
  a.elig = reinterpret_cast<unsigned char*>(s + 256 * n);
  int* hyp_scratch = reinterpret_cast<int*>(s + 256 * n + 16 * ((n * hw + 15) / 16));
  a.hyp_cnt = hyp_counts ? hyp_counts : hyp_scratch;
  a.part = reinterpret_cast<double*>(reinterpret_cast<char*>(hyp_scratch) + 8 * ((n * (size_t)hypotheses + 1) / 2));
  a.plane_out = plane_out, a.info = info;
  // the table lives in this frame, so the copy completes before it goes out of scope
  HIP_TRY(hipMemcpyWithStream(s, tab.data(), sizeof(DpFrame) * n, hipMemcpyHostToDevice, ST(stream)), "fp_depth_plane_fit: table upload");
  HIP_TRY(hipMemsetAsync(a.cnt2, 0, 8 * n, ST(stream)), "fp_depth_plane_fit: zeroing the counters");
  return launch_depth_plane_fit(a, ST(stream));
}

int fp_depth_components(const float* depth, int num_frames, int height, int width, const double* cameras, const float* slope_fx,
                        const double* planes, const int32_t* num_planes, double max_depth_mm, double object_margin_mm, float connect_mm,
                        void* scratch, size_t scratch_bytes, int32_t* labels, fp_stream_t stream) {
  FP_REQUIRE(slope_fx && planes && num_planes && scratch && labels, "fp_depth_components: null pointer");
  std::vector<DpFrame> tab;
  TRY(depth_frames("fp_depth_components", depth, num_frames, height, width, cameras, max_depth_mm, tab));
  FP_REQUIRE(std::isfinite(object_margin_mm), "fp_depth_components: object_margin_mm must be finite");
  FP_REQUIRE(connect_mm >= 0.f && std::isfinite(connect_mm), "fp_depth_components: connect_mm must be finite and >= 0");
  const size_t hw = (size_t)height * width, n = (size_t)num_frames;
  for (int f = 0; f < num_frames; ++f) {
    FP_REQUIRE(slope_fx[f] >= 0.f && std::isfinite(slope_fx[f]), "fp_depth_components: frame %d: slope_fx must be finite and >= 0", f);
    tab[f].slope_fx = slope_fx[f];
  }
  FP_REQUIRE(scratch_bytes >= FP_DEPTH_COMPONENTS_SCRATCH_BYTES(n, hw), "fp_depth_components: scratch holds %zu bytes, %zu needed", scratch_bytes,
             FP_DEPTH_COMPONENTS_SCRATCH_BYTES(n, hw));
  char* s = reinterpret_cast<char*>(scratch);
  DpCompArgs a;
  memset(&a, 0, sizeof(a));
  a.depth = depth, a.planes = planes, a.num_planes = num_planes;
  a.n = num_frames, a.h = height, a.w = width, a.connect_mm = connect_mm, a.max_depth = max_depth_mm, a.margin = object_margin_mm;
  a.frames = reinterpret_cast<const DpFrame*>(s);
  a.parent = reinterpret_cast<int*>(s + 64 * n);
  a.labels = labels;
  HIP_TRY(hipMemcpyWithStream(s, tab.data(), sizeof(DpFrame) * n, hipMemcpyHostToDevice, ST(stream)), "fp_depth_components: table upload");
  return launch_depth_components(a, ST(stream));
}

int fp_component_table(const int32_t* labels, int num_frames, int height, int width, int min_pixels, int max_area, int max_proposals,
                       int level, const int32_t* finer, int num_finer, void* scratch, size_t scratch_bytes, int32_t* table,
                       int32_t* counts, int32_t* rank_map, fp_stream_t stream) {
  FP_REQUIRE(labels && scratch && table && counts && rank_map, "fp_component_table: null pointer");
  FP_REQUIRE(num_frames >= 1 && num_frames <= FP_DEPTH_MAX_FRAMES, "fp_component_table: num_frames %d outside [1, %d]", num_frames, FP_DEPTH_MAX_FRAMES);
  FP_REQUIRE(height >= 1 && width >= 1 && (long long)height * width <= 0x7fffffffll, "fp_component_table: an image of %d x %d (1 .. 2^31 - 1 pixels)",
             width, height);
  FP_REQUIRE(min_pixels >= 1 && max_area >= min_pixels, "fp_component_table: min_pixels %d, max_area %d (1 <= min_pixels <= max_area)", min_pixels, max_area);
  FP_REQUIRE(max_proposals >= 1 && max_proposals <= FP_DEPTH_MAX_PROPOSALS, "fp_component_table: max_proposals %d outside [1, %d]", max_proposals,
             FP_DEPTH_MAX_PROPOSALS);
  FP_REQUIRE(level >= 0 && level <= 2 && num_finer >= 0 && num_finer <= 2, "fp_component_table: level %d, num_finer %d (both in [0, 2])", level, num_finer);
  FP_REQUIRE((num_finer == 0) == (finer == nullptr), "fp_component_table: finer and num_finer disagree");
  const size_t hw = (size_t)height * width, n = (size_t)num_frames;
  FP_REQUIRE(scratch_bytes >= FP_COMPONENT_TABLE_SCRATCH_BYTES(n, hw), "fp_component_table: scratch holds %zu bytes, %zu needed", scratch_bytes,
             FP_COMPONENT_TABLE_SCRATCH_BYTES(n, hw));
  char* s = reinterpret_cast<char*>(scratch);
  DpTableArgs a;
  memset(&a, 0, sizeof(a));
  a.labels = labels, a.finer = finer;
  a.n = num_frames, a.h = height, a.w = width, a.min_pixels = min_pixels, a.max_area = max_area, a.max_prop = max_proposals, a.level = level;
  a.num_finer = num_finer;
  a.ncand = reinterpret_cast<int*>(s);
  a.cand = reinterpret_cast<int*>(s + 16 * n);
  a.slots = reinterpret_cast<int*>(s + 16 * n + 4 * n * hw);
  a.table = table, a.counts = counts, a.rank_map = rank_map;
  return launch_component_table(a, ST(stream));
}

int fp_component_runs(const int32_t* rank_map, int num_maps, int height, int width, const int32_t* num_kept, int max_proposals,
                      int64_t capacity, int64_t* events, int32_t* num_events, fp_stream_t stream) {
  FP_REQUIRE(rank_map && num_kept && num_events, "fp_component_runs: null pointer");
  FP_REQUIRE(num_maps >= 1 && height >= 1 && width >= 1 && (long long)height * width <= 0x7fffffffll, "fp_component_runs: %d maps of %d x %d", num_maps,
             width, height);
  FP_REQUIRE(max_proposals >= 1 && max_proposals <= FP_DEPTH_MAX_PROPOSALS, "fp_component_runs: max_proposals %d outside [1, %d]", max_proposals,
             FP_DEPTH_MAX_PROPOSALS);
  FP_REQUIRE(num_maps <= 65535 && (long long)num_maps * ((long long)height * width + 1 + max_proposals) <= (1ll << 30),
             "fp_component_runs: %d maps of %d x %d exceed 2^30 positions (or 65535 maps)", num_maps, width, height);
  FP_REQUIRE(capacity >= 0 && (capacity == 0 || events), "fp_component_runs: capacity %lld without an events array", (long long)capacity);
  DpRunsArgs a;
  memset(&a, 0, sizeof(a));
  a.rank_map = rank_map, a.num_kept = num_kept;
  a.m = num_maps, a.h = height, a.w = width, a.max_prop = max_proposals, a.capacity = capacity;
  a.events = reinterpret_cast<long long*>(events), a.count = num_events;
  HIP_TRY(hipMemsetAsync(num_events, 0, 4, ST(stream)), "fp_component_runs: zeroing the counter");
  if (capacity > 0) HIP_TRY(hipMemsetAsync(events, 0x7f, 8 * (size_t)capacity, ST(stream)), "fp_component_runs: filling events");
  return launch_component_runs(a, ST(stream));
}

// ------------------------------------------------------------------ ViT forward (launch sequence in C++)
}  // extern "C"

namespace {
enum { VIT_FULL = 0, VIT_PREFIX = 1, VIT_LAST_SELECTED = 2 };
struct VitSelection { const int32_t* rows; const int32_t* off; int num, max_per_img; };
enum { QKV = 0, PROJ = 1, FC1 = 2, FC2 = 3 };   // the GEMMs of a block, in order; also the index of fp_vit_block.act_scale
struct VitEpilogues { int tokens, bias, gelu, swiglu, resid; };
constexpr VitEpilogues kF32Epi{F32_EPI_TOKENS, F32_EPI_BIAS, F32_EPI_BIAS_GELU, F32_EPI_SWIGLU, F32_EPI_LS_RESID};
constexpr VitEpilogues kGemmEpi{GEMM_EPI_TOKENS_F32, GEMM_EPI_BIAS_BF16, GEMM_EPI_GELU_BF16, GEMM_EPI_SWIGLU_BF16, GEMM_EPI_LS_RESID_F32};
// folded LayerNorms: LayerScale is in the matrices; the residual GEMMs also emit the next GEMM's 16-bit operand and row sums (RESID_HILO in front
// of the hooked block)
constexpr VitEpilogues kFoldEpi{GEMM_EPI_TOKENS_F32, GEMM_EPI_BIAS_BF16, GEMM_EPI_GELU_BF16, GEMM_EPI_SWIGLU_BF16, GEMM_EPI_RESID_F32};

GemmBf16Args zero_gemm_args() {
  GemmBf16Args g;
  memset(&g, 0, sizeof(g));
  return g;
}

// VIT_FULL: embedding + blocks 0..layer.  VIT_PREFIX: embedding + blocks 0..layer-1, leaving what block `layer` starts from: the fp32
// stream ws->x -- or, for a folded-LayerNorm model with layer > 0, the (xb, xl) pair and the LayerNorm row sums ONLY: ws->x is then stale (it
// holds the token embedding) and must not be read by a caller.  VIT_LAST_SELECTED: block `layer` alone, computed for the selected tokens only
// (queries of the attention, rows of proj / fc1 / fc2) on top of a VIT_PREFIX run -- keys and values are all tokens.
//
// Every block runs the same steps: norm 1 -> qkv -> attention -> (the selected rows) -> proj -> norm 2 -> fc1 -> fc2.  The model's family decides
// how a step normalises, which GEMM launcher runs and what the epilogues take:
//   fp32, bf16  LayerNorm kernel, LayerScale in the residual epilogue;
//   folded      (bf16 / f16 with ln_fold) the LayerNorms folded into the GEMMs around them: qkv / fc1 read the 16-bit copy of the stream and
//               normalise in their epilogue from the row sums the residual GEMMs emit (ln_finalize turns them into per-row constants);
//   split       (f16x3 / f16f8) every GEMM / attention operand is a split-fp16 (or f16f8) row written by the kernel in front of it with a fixed
//               power-of-two scale; b.act_scale[j] = 1 / (scale of the input x scale of the matrix) undoes both in the epilogue of GEMM j;
//   fp8         every GEMM input is produced as e4m3 bytes (ws->a8; the hidden activations reuse ws->h) by the kernel in front of it with the
//               block's static scales; the matrices carry a per-column dequantisation scale (gamma).
// Residual stream, LayerNorm and softmax are fp32 in every family.
int vit_forward_impl(const fp_vit_model* m, const fp_vit_workspace* ws, const float* images, int B, int H, int W, int layer, int mode,
                     const VitSelection* sel, fp_stream_t stream) {
  FP_REQUIRE(m && ws && (images || mode == VIT_LAST_SELECTED) && m->blocks, "fp_vit_forward: null pointer");
  FP_REQUIRE(layer >= -1 && layer < m->depth, "fp_vit_forward: layer %d out of range (depth %d)", layer, m->depth);  // -1: token embedding only
  const int pstride = m->patch_stride > 0 ? m->patch_stride : m->patch;  // the conv stride of the patch embedding (dinov2_utils.py:364-389)
  FP_REQUIRE(pstride != m->patch || (H % m->patch == 0 && W % m->patch == 0), "fp_vit_forward: image size must be a multiple of the patch size");
  FP_REQUIRE(H >= m->patch && W >= m->patch && (pstride == m->patch || mode == VIT_FULL), "fp_vit_forward: image smaller than a patch, or token selection with stride != patch size");
  const int D = m->dim, hid = m->hidden, np = (1 + (H - m->patch) / pstride) * (1 + (W - m->patch) / pstride), ntok = 1 + m->registers + np;
  const int Mtok = B * ntok, Mp = B * np;
  FP_REQUIRE(ws->m_pad >= Mtok && ws->m_pad % 128 == 0, "fp_vit_forward: workspace m_pad (%d) too small for %d tokens or not a multiple of 128", ws->m_pad, Mtok);
  FP_REQUIRE(ws->m_patch_pad >= Mp && ws->m_patch_pad % 128 == 0, "fp_vit_forward: workspace m_patch_pad too small");
  FP_REQUIRE(ws->patches && ws->x && ws->y && ws->qkv && ws->h, "fp_vit_forward: workspace buffer missing");
  hipStream_t st = ST(stream);

  // ---- the plan of this call: family, operand type, row strides, launchers
  const int wdt = m->weight_dtype;
  const bool f8 = wdt == FP_DTYPE_FP8;      // e4m3 block matrices; activations and patch embed stay bf16
  const bool sx = wdt == FP_DTYPE_F16F8;    // f16f8 rows (common.hpp): the split mode with the cross terms on the fp8 pipe
  const bool sp = wdt == FP_DTYPE_F16X3 || sx;
  const bool h16 = wdt == FP_DTYPE_F16;     // the "f16" mode: the folded bf16 pipeline (folded LayerNorms, (hi, lo) stream) on IEEE fp16 operands
  const bool bf = wdt == FP_DTYPE_BF16 || f8 || h16;
  const bool fold = m->ln_fold && bf && !f8;
  const int adt = sx ? FP_DTYPE_F16F8 : (sp ? FP_DTYPE_F16X3 : (h16 ? FP_DTYPE_F16 : (bf ? FP_DTYPE_BF16 : FP_DTYPE_F32)));
  const int em = sp ? 2 : 1;                // stored elements per logical element of an operand row
  // row strides of the operands and matrices, 0 = dense: elements (split rows: halves); the fp8 family's e4m3 operands and matrices: bytes
  const int ldy = ws->ld_y ? ws->ld_y : em * D, ldh = ws->ld_h ? ws->ld_h : em * hid, ldq = ws->ld_qkv ? ws->ld_qkv : em * 3 * D;
  const int ldwd = m->ld_w_dim ? m->ld_w_dim : em * D, ldwh = m->ld_w_hidden ? m->ld_w_hidden : em * hid;
  FP_REQUIRE(!h16 || m->ln_fold, "fp_vit_forward: weight_dtype FP_F16 runs the folded-LayerNorm pipeline only (ln_fold = 1, dim %% 128 == 0)");
  FP_REQUIRE(!sx || (D % 64 == 0 && hid % 64 == 0 && m->patch_k_pad % 64 == 0), "fp_vit_forward: the f16f8 mode needs dim, hidden and patch_k_pad to be multiples of 64");
  FP_REQUIRE(!sp || m->patch_acc_scale > 0.f, "fp_vit_forward: the f16x3 mode needs patch_acc_scale");
  FP_REQUIRE(!f8 || (ws->a8 && ws->m_pad % 256 == 0 && D % 128 == 0 && hid % 128 == 0), "fp_vit_forward: the fp8 mode needs workspace a8, m_pad %% 256 == 0 and dim, hidden multiples of 128");
  FP_REQUIRE(!f8 || (ldy % 16 == 0 && ldh % 16 == 0 && ldwd % 16 == 0 && ldwh % 16 == 0), "fp_vit_forward: fp8 row strides (bytes) must keep 16-byte alignment");
  FP_REQUIRE(ldy >= em * D && ldh >= em * hid && ldq >= em * 3 * D && ldwd >= em * D && ldwh >= em * hid &&
                 ldy % 8 == 0 && ldh % 8 == 0 && ldq % 8 == 0 && ldwd % 8 == 0 && ldwh % 8 == 0,
             "fp_vit_forward: operand row strides must cover the row and keep 16-byte alignment");
  FP_REQUIRE(!fold || (ws->xb && ws->xl && ws->stats), "fp_vit_forward: ln_fold needs workspace xb, xl and stats");
  FP_REQUIRE(!fold || D % 128 == 0, "fp_vit_forward: ln_fold needs dim %% 128 == 0");
  FP_REQUIRE(mode == VIT_FULL || fold || sp || f8, "fp_vit_forward_prefix / fp_vit_block_selected: bf16 model with ln_fold, an fp8 or an f16x3 model");
  const bool f32 = !bf && !sp;             // the fp32 family: its GEMMs run on the fp32 tile (fmt unused)
  const GemmFmt fmt = sx ? GemmFmt::F16F8 : sp ? GemmFmt::F16X3 : f8 ? GemmFmt::FP8 : h16 ? GemmFmt::F16 : GemmFmt::BF16;
  const VitEpilogues& epi = f32 ? kF32Epi : fold ? kFoldEpi : kGemmEpi;
  const int role_epi[4] = {epi.bias, epi.resid, m->ffn_swiglu ? epi.swiglu : epi.gelu, epi.resid};  // fc1 with SwiGLU: fc1_w rows interleaved (x1_j, x2_j)
  void* const norm_out = fold ? ws->xb : f8 ? ws->a8 : ws->y;   // the A operand of qkv and fc1
  void* const attn_out = f8 ? ws->a8 : ws->y;                    // the A operand of proj
  const int attn_dt = f32 ? FP_DTYPE_F32 : sp ? FP_DTYPE_F16X3 : h16 ? FP_DTYPE_F16 : FP_DTYPE_BF16;
  // folded LayerNorms: one partial sum per 128-column group of the residual GEMMs, whatever tile they run with; then (rstd, mean * rstd) per row
  const int ln_parts = D / 128;
  float2* stats = reinterpret_cast<float2*>(ws->stats);
  float2* ln_row = fold ? stats + (size_t)ln_parts * ws->m_pad : nullptr;

  // the rows every GEMM and norm runs on: the patch rows of the embedding, then all tokens, then (VIT_LAST_SELECTED) the selected ones
  int rows_valid = Mp, rows_pad = ws->m_patch_pad;
  auto gemm = [&](GemmFmt k, int e, GemmBf16Args g) -> int {
    g.M = rows_pad; g.M_valid = rows_valid;
    if (!f32) return gemm_launch(k, e, g, st);
    F32TileArgs a = zero_tile_args();   // the fp32 tile takes the valid rows only
    a.A = reinterpret_cast<const float*>(g.A); a.lda = g.lda; a.B = reinterpret_cast<const float*>(g.W); a.ldb = g.ldw;
    a.K = g.K; a.M = rows_valid; a.N = g.N; a.out = static_cast<float*>(g.out); a.ldo = g.ldo; a.bias = g.bias; a.gamma = g.gamma;
    a.pos = g.pos; a.tok_np = g.tok_np; a.tok_n = g.tok_n; a.tok_skip = g.tok_skip;
    return f32_tile_launch(e, a, rows_valid, g.N, 1, st);
  };

  // tokens: [cls + pos0 | registers | patch_embed(x) + pos]
  if (mode != VIT_LAST_SELECTED) {
    if (pstride == m->patch) TRY(patchify_launch(images, B, H, W, m->patch, ws->patches, em * m->patch_k_pad, adt, st, FP_SPLIT_SCALE_ACT));
    else TRY(patchify_strided_launch(images, B, H, W, m->patch, pstride, ws->patches, em * m->patch_k_pad, adt, st, FP_SPLIT_SCALE_ACT));
    TRY(prefix_tokens_launch(m->prefix, 1 + m->registers, D, ws->x, B, ntok, st));
    GemmBf16Args g = zero_gemm_args();
    g.A = reinterpret_cast<const __bf16*>(ws->patches); g.lda = em * m->patch_k_pad;
    g.W = reinterpret_cast<const __bf16*>(m->patch_w); g.ldw = em * m->patch_k_pad;
    g.N = D; g.K = m->patch_k_pad; g.bias = m->patch_b; g.out = ws->x; g.ldo = D;
    g.pos = m->pos_patch; g.tok_np = np; g.tok_n = ntok; g.tok_skip = 1 + m->registers;
    g.acc_scale = sp ? m->patch_acc_scale : 0.f;
    TRY(gemm(f8 ? GemmFmt::BF16 : fmt, epi.tokens, g));   // (the fp8 family embeds in bf16)
    // the folded chain starts from the token embedding: its 16-bit copy (hi, lo) and row sums
    if (fold && layer >= 0) TRY(rowstats_cast_launch(ws->x, Mtok, D, ws->xb, ldy, stats, ws->m_pad, ln_parts, st, ws->xl, h16));
  }
  rows_valid = Mtok, rows_pad = ws->m_pad;

  // x (rows xr) -> the A operand of qkv (j = QKV) or fc1 (j = FC1).  Folded: the row constants of the GEMM's normalising epilogue (the residual
  // GEMM filed its partial sums with a stride of ITS row count: rows_pad).
  auto norm = [&](const fp_vit_block& b, int j, const float* xr) -> int {
    if (fold) return ln_finalize_launch(stats, ln_parts, rows_pad, rows_valid, D, 1e-6f, ln_row, st);
    LayerNormArgs ln;
    memset(&ln, 0, sizeof(ln));
    ln.x = xr; ln.ld_x = D; ln.weight = j == QKV ? b.ln1_w : b.ln2_w; ln.bias = j == QKV ? b.ln1_b : b.ln2_b; ln.eps = 1e-6f;
    ln.out = norm_out; ln.ld_out = ldy; ln.out_dtype = f8 ? FP_DTYPE_FP8 : adt;
    ln.out_scale = sp ? FP_SPLIT_SCALE_ACT : f8 ? b.act_scale[j] : 0.f;
    ln.dim = D; ln.out_rows = ln.out_rows_per_img = ln.in_rows_per_img = rows_valid;
    ln.sat = ws->sat;
    return layernorm_launch(ln, st);
  };
  auto attention = [&](const fp_vit_block& b) -> int {
    AttnArgs at;
    memset(&at, 0, sizeof(at));
    at.qkv = ws->qkv; at.ld_qkv = ldq; at.out = attn_out; at.ld_out = ldy;
    at.batch = B; at.n_tok = ntok; at.dim = D; at.heads = m->heads;
    at.sat = ws->sat;
    // f16f8: q | k | v stay split-fp16 rows (the attention's own three-MFMA products), its output is proj's f16f8 operand
    if (sp) at.in_scale = FP_SPLIT_SCALE_QKV, at.out_scale = FP_SPLIT_SCALE_ACT, at.out_fmt = sx ? 1 : 0;
    if (f8) at.out_fp8_scale = b.act_scale[PROJ];
    if (sel) at.sel_rows = sel->rows, at.sel_off = sel->off, at.max_sel = sel->max_per_img;
    return attn_launch(at, attn_dt, st);
  };
  // The hooked block for the selected tokens only.  K and V need every token: norm 1 and the qkv GEMM run on all rows (its Q columns of
  // unselected rows are the only wasted work); attention takes its queries through the index list and writes compact rows; from there on every
  // operand has num_sel rows, and row r of every compact buffer is token sel->rows[r].  The per-row arithmetic (GEMM chains, 128-column stat
  // groups, static scales) does not depend on where a row sits, so the selected rows carry the bits the full block would have given them.
  auto select_rows = [&](float*& xr) -> int {
    xr = reinterpret_cast<float*>(ws->qkv);   // qkv is dead after the attention: [num_sel, D] fp32 rows of the stream
    if (fold && layer > 0) TRY(hilo_rows_launch(ws->xb, ws->xl, ldy, sel->rows, sel->num, D, xr, st, h16));   // the blocks in front left (hi, lo) pairs
    else TRY(gather_rows_launch(ws->x, sel->rows, sel->num, D, xr, st));
    const int pad = (sel->num + 255) / 256 * 256;
    rows_valid = sel->num, rows_pad = pad < ws->m_pad ? pad : ws->m_pad;
    return FP_OK;
  };
  // GEMM j of block b; xr: the residual rows; pair: a folded block in front of the hooked one (the stream is the (hi, lo) pair)
  auto block_gemm = [&](const fp_vit_block& b, int j, float* xr, bool pair) -> int {
    const void* const Wt[4] = {b.qkv_w, b.proj_w, b.fc1_w, b.fc2_w};
    const float* const bias[4] = {b.qkv_b, b.proj_b, b.fc1_b, b.fc2_b};
    const float* const col_scale[4] = {b.qkv_s, b.proj_s, b.fc1_s, b.fc2_s};
    const bool resid = j == PROJ || j == FC2;
    GemmBf16Args g = zero_gemm_args();
    g.A = reinterpret_cast<const __bf16*>(j == FC2 ? ws->h : j == PROJ ? attn_out : norm_out); g.lda = j == FC2 ? ldh : ldy;
    g.W = reinterpret_cast<const __bf16*>(Wt[j]); g.ldw = j == FC2 ? ldwh : ldwd;
    g.N = j == QKV ? 3 * D : j == FC1 ? (m->ffn_swiglu ? 2 : 1) * hid : D; g.K = j == FC2 ? hid : D;
    g.bias = bias[j];
    g.out = j == QKV ? ws->qkv : j == FC1 ? ws->h : xr; g.ldo = j == QKV ? ldq : j == FC1 ? ldh : D;
    if (f8) g.gamma = col_scale[j];
    else if (!fold && resid) g.gamma = j == PROJ ? b.ls1 : b.ls2;
    if (sp || h16) g.acc_scale = b.act_scale[j];   // f16: 1 / (power-of-two scale of the matrix)
    if (sp) g.out_scale = j == QKV ? FP_SPLIT_SCALE_QKV : j == FC1 ? FP_SPLIT_SCALE_HID : 0.f;
    if (f8 && j == FC1) g.out_scale = b.act_scale[FC2];   // the hidden activations leave as fc2's e4m3 input
    if (sp || f8) g.sat = ws->sat;
    if (fold && !resid) {
      g.ln_stats = ln_row; g.ln_parts = ln_parts; g.ln_eps = 1e-6f; g.colsum = j == QKV ? b.qkv_colsum : b.fc1_colsum;
    }
    if (fold && resid && (j == PROJ || pair)) {   // the next norm's row sums and 16-bit operand (fc2 of the hooked block feeds no norm)
      g.xb = reinterpret_cast<__bf16*>(ws->xb); g.ld_xb = ldy; g.stats_out = stats; g.xl = reinterpret_cast<__bf16*>(ws->xl);
    }
    FP_REQUIRE(g.W && (g.gamma || fold || !resid) && g.out_scale >= 0.f, "fp_vit_forward: GEMM %d: matrix or LayerScale missing, or a negative output scale", j);
    return gemm(fmt, resid && pair ? GEMM_EPI_RESID_HILO : role_epi[j], g);
  };

  const int i_first = mode == VIT_LAST_SELECTED ? layer : 0, i_last = mode == VIT_PREFIX ? layer - 1 : layer;
  for (int i = i_first; i <= i_last; ++i) {
    const fp_vit_block& b = m->blocks[i];
    FP_REQUIRE(!fold || (b.qkv_colsum && b.fc1_colsum), "fp_vit_forward: ln_fold needs the column sums of qkv_w / fc1_w");
    // Folded blocks in FRONT of the hooked one keep the residual stream as (hi, lo) 16-bit arrays (ws->xb, ws->xl) instead of fp32 + a 16-bit
    // copy: the residual GEMMs then read 4 and write 4 bytes per element instead of 4 + 6 (hi IS the next GEMM's A operand), 16 mantissa bits
    // per update.  The hooked block itself runs on an fp32 stream rebuilt from the pair (all rows, or the selected rows only), so the engine's
    // token-selected form and the full form stay bit-identical.
    const bool pair = fold && i < layer;
    float* xr = ws->x;   // the residual rows the block updates
    if (fold && mode == VIT_FULL && i == layer && i > 0) TRY(hilo_rows_launch(ws->xb, ws->xl, ldy, nullptr, Mtok, D, ws->x, st, h16));
    // x += ls1 * proj(attn(ln1(x)))
    TRY(norm(b, QKV, xr));
    TRY(block_gemm(b, QKV, xr, pair));
    TRY(attention(b));
    if (sel) TRY(select_rows(xr));
    TRY(block_gemm(b, PROJ, xr, pair));
    // x += ls2 * fc2(act(fc1(ln2(x))))
    TRY(norm(b, FC1, xr));
    TRY(block_gemm(b, FC1, xr, pair));
    TRY(block_gemm(b, FC2, xr, pair));
  }
  return FP_OK;
}
}  // namespace

extern "C" {

int fp_vit_forward(const fp_vit_model* m, const fp_vit_workspace* ws, const float* images, int B, int H, int W,
                   int layer, fp_stream_t stream) {
  return vit_forward_impl(m, ws, images, B, H, W, layer, VIT_FULL, nullptr, stream);
}

int fp_vit_forward_prefix(const fp_vit_model* m, const fp_vit_workspace* ws, const float* images, int B, int H, int W,
                          int layer, fp_stream_t stream) {
  FP_REQUIRE(layer >= 0, "fp_vit_forward_prefix: layer must be >= 0");
  return vit_forward_impl(m, ws, images, B, H, W, layer, VIT_PREFIX, nullptr, stream);
}

int fp_vit_block_selected(const fp_vit_model* m, const fp_vit_workspace* ws, int B, int H, int W, int layer,
                          const int32_t* sel_rows, const int32_t* sel_off, int num_sel, int max_sel_per_img, fp_stream_t stream) {
  FP_REQUIRE(sel_rows && sel_off, "fp_vit_block_selected: null pointer");
  FP_REQUIRE(layer >= 0 && num_sel >= 1 && max_sel_per_img >= 1 && max_sel_per_img <= num_sel, "fp_vit_block_selected: bad sizes (layer %d, %d selected, at most %d per image)",
             layer, num_sel, max_sel_per_img);
  FP_REQUIRE(m && ws && num_sel <= ws->m_pad, "fp_vit_block_selected: more selected tokens than workspace rows");
  const VitSelection sel{sel_rows, sel_off, num_sel, max_sel_per_img};
  return vit_forward_impl(m, ws, nullptr, B, H, W, layer, VIT_LAST_SELECTED, &sel, stream);
}

int fp_vit_features(const fp_vit_model* m, const fp_vit_workspace* ws, int B, int n_patches, int apply_norm,
                    float* fmap, float* cls, fp_stream_t stream) {
  FP_REQUIRE(m && ws && fmap, "fp_vit_features: null pointer");
  const int D = m->dim, ntok = 1 + m->registers + n_patches;
  hipStream_t st = ST(stream);
  if (apply_norm) {
    LayerNormArgs ln;
    memset(&ln, 0, sizeof(ln));
    ln.x = ws->x; ln.ld_x = D; ln.weight = m->norm_w; ln.bias = m->norm_b; ln.eps = 1e-6f;
    ln.out_dtype = FP_DTYPE_F32; ln.dim = D; ln.in_rows_per_img = ntok; ln.ld_out = D;
    ln.sat = m->weight_dtype == FP_DTYPE_F16 ? ws->sat : nullptr;   // the "f16" mode's overflow report: non-finite features (common.hpp)
    ln.out = fmap; ln.out_rows = B * n_patches; ln.out_rows_per_img = n_patches; ln.in_skip = 1 + m->registers;
    TRY(layernorm_launch(ln, st));
    if (cls) {
      ln.out = cls; ln.out_rows = B; ln.out_rows_per_img = 1; ln.in_skip = 0;
      TRY(layernorm_launch(ln, st));
    }
  } else {
    HIP_TRY(hipMemcpy2DAsync(fmap, (size_t)n_patches * D * 4, ws->x + (size_t)(1 + m->registers) * D, (size_t)ntok * D * 4,
                             (size_t)n_patches * D * 4, B, hipMemcpyDeviceToDevice, st), "fp_vit_features: copy");
    if (cls)
      HIP_TRY(hipMemcpy2DAsync(cls, (size_t)D * 4, ws->x, (size_t)ntok * D * 4, (size_t)D * 4, B, hipMemcpyDeviceToDevice, st),
              "fp_vit_features: copy cls");
  }
  return FP_OK;
}

int fp_vit_sample_features(const fp_vit_model* m, const fp_vit_workspace* ws, int B, int grid_h, int grid_w, int apply_norm, int img_w, int img_h,
                           const float* points, const int32_t* point_img, int num_points, float* out, fp_stream_t stream) {
  FP_REQUIRE(m && ws && ws->x && points && out, "fp_vit_sample_features: null pointer");
  FP_REQUIRE(B >= 1 && grid_h >= 1 && grid_w >= 1 && img_w >= 1 && img_h >= 1, "fp_vit_sample_features: bad sizes");
  const int ntok = 1 + m->registers + grid_h * grid_w;
  return ln_sample_launch(ws->x, m->dim, m->norm_w, m->norm_b, 1e-6f, apply_norm, m->dim, ntok, 1 + m->registers, grid_h, grid_w, img_w, img_h,
                          points, point_img, num_points, out, ST(stream), nullptr, m->weight_dtype == FP_DTYPE_F16 ? ws->sat : nullptr);
}

int fp_query_select(const uint8_t* masks, int B, int H, int W, const int32_t* pix_x, const int32_t* pix_y, const float* grid_points, int num_points,
                    const int64_t* point_cells, int num_cells, int n_tok, int32_t* scratch, int32_t* counts, float* out_points, int32_t* out_point_img,
                    int32_t* out_q_off, int32_t* sel_rows, int32_t* sel_off, int32_t* row_map, fp_stream_t stream) {
  FP_REQUIRE(masks && pix_x && pix_y && grid_points && scratch && counts && out_points && out_point_img, "fp_query_select: null pointer");
  FP_REQUIRE(!point_cells || (sel_rows && sel_off && row_map), "fp_query_select: the token selection needs sel_rows, sel_off and row_map");
  return query_select_launch(masks, B, H, W, pix_x, pix_y, grid_points, num_points, reinterpret_cast<const long long*>(point_cells), num_cells, n_tok,
                             scratch, counts, out_points, out_point_img, out_q_off, sel_rows, sel_off, row_map, ST(stream));
}

int fp_vit_sample_features_selected(const fp_vit_model* m, const fp_vit_workspace* ws, int B, int grid_h, int grid_w, int apply_norm, int img_w,
                                    int img_h, const float* points, const int32_t* point_img, int num_points, const int32_t* row_map, float* out,
                                    fp_stream_t stream) {
  FP_REQUIRE(m && ws && ws->qkv && points && out && row_map, "fp_vit_sample_features_selected: null pointer");
  FP_REQUIRE(B >= 1 && grid_h >= 1 && grid_w >= 1 && img_w >= 1 && img_h >= 1, "fp_vit_sample_features_selected: bad sizes");
  const int ntok = 1 + m->registers + grid_h * grid_w;
  // fp_vit_block_selected left the selected tokens' rows of the residual stream, compact, where the qkv projections were
  return ln_sample_launch(reinterpret_cast<const float*>(ws->qkv), m->dim, m->norm_w, m->norm_b, 1e-6f, apply_norm, m->dim, ntok, 1 + m->registers,
                          grid_h, grid_w, img_w, img_h, points, point_img, num_points, out, ST(stream), row_map, m->weight_dtype == FP_DTYPE_F16 ? ws->sat : nullptr);
}

// ------------------------------------------------------------------ result pictures (vis.hip)
static bool vis_side(int v) { return v >= 1 && v <= FP_VIS_MAX_SIDE; }

int fp_vis_pca_colorize(const float* map, int batch, int gh, int gw, int C, int out_h, int out_w, int dim_num, int dim_den, float* range,
                        uint8_t* out, fp_stream_t stream) {
  FP_REQUIRE(map && range && out, "fp_vis_pca_colorize: null pointer");
  FP_REQUIRE(batch >= 1 && batch <= 65535 && vis_side(gh) && vis_side(gw) && vis_side(out_h) && vis_side(out_w),
             "fp_vis_pca_colorize: bad sizes (batch %d, map %d x %d, picture %d x %d)", batch, gh, gw, out_h, out_w);
  FP_REQUIRE(C >= 3, "fp_vis_pca_colorize: the map needs at least 3 channels, got %d", C);
  FP_REQUIRE(dim_num >= 0 && dim_num <= dim_den && dim_den >= 1 && dim_den <= 255, "fp_vis_pca_colorize: dimming %d / %d outside 0 <= num <= den <= 255",
             dim_num, dim_den);
  return launch_vis_pca_colorize(map, batch, gh, gw, C, out_h, out_w, dim_num, dim_den, range, out, ST(stream));
}

int fp_vis_mask_tint(const uint8_t* img, const uint8_t* mask, int batch, int h, int w, uint8_t* out, fp_stream_t stream) {
  FP_REQUIRE(img && mask && out, "fp_vis_mask_tint: null pointer");
  FP_REQUIRE(batch >= 1 && batch <= 65535 && vis_side(h) && vis_side(w), "fp_vis_mask_tint: bad sizes (batch %d, %d x %d)", batch, h, w);
  return launch_vis_mask_tint(img, mask, (long long)batch * h * w, out, ST(stream));
}

int fp_vis_contour(const uint8_t* mask, int batch, int h, int w, int dilate_iterations, int r, int g, int b, uint8_t* img,
                   fp_stream_t stream) {
  FP_REQUIRE(mask && img, "fp_vis_contour: null pointer");
  FP_REQUIRE(batch >= 1 && batch <= 65535 && vis_side(h) && vis_side(w), "fp_vis_contour: bad sizes (batch %d, %d x %d)", batch, h, w);
  FP_REQUIRE(dilate_iterations >= 0 && dilate_iterations <= FP_VIS_MAX_DILATE, "fp_vis_contour: dilate_iterations %d outside [0, %d]",
             dilate_iterations, FP_VIS_MAX_DILATE);
  FP_REQUIRE(r >= 0 && r <= 255 && g >= 0 && g <= 255 && b >= 0 && b <= 255, "fp_vis_contour: colour (%d, %d, %d) outside [0, 255]", r, g, b);
  return launch_vis_contour(mask, batch, h, w, dilate_iterations, r, g, b, img, ST(stream));
}

int fp_vis_resize_area(const uint8_t* src, int batch, int h, int w, int out_h, int out_w, uint8_t* out, fp_stream_t stream) {
  FP_REQUIRE(src && out, "fp_vis_resize_area: null pointer");
  FP_REQUIRE(batch >= 1 && batch <= 65535 && vis_side(h) && vis_side(w) && out_h >= 1 && out_w >= 1, "fp_vis_resize_area: bad sizes");
  FP_REQUIRE(out_h <= h && out_w <= w, "fp_vis_resize_area: %d x %d -> %d x %d is not a downscaling", w, h, out_w, out_h);
  return launch_vis_resize_area(src, batch, h, w, out_h, out_w, out, ST(stream));
}

int fp_vis_draw_matches(const float* segments, const int32_t* counts, int batch, int max_matches, int h, int w, const float* colour,
                        float alpha, float lw, float radius, uint8_t* tile, fp_stream_t stream) {
  FP_REQUIRE(segments && counts && colour && tile, "fp_vis_draw_matches: null pointer");
  FP_REQUIRE(batch >= 1 && batch <= 65535 && vis_side(h) && vis_side(w), "fp_vis_draw_matches: bad sizes (batch %d, %d x %d)", batch, h, w);
  FP_REQUIRE(max_matches >= 1 && max_matches <= FP_VIS_MAX_MATCHES, "fp_vis_draw_matches: max_matches %d outside [1, %d]", max_matches,
             FP_VIS_MAX_MATCHES);
  FP_REQUIRE((reinterpret_cast<uintptr_t>(segments) & 15) == 0, "fp_vis_draw_matches: segments must be 16-byte aligned");
  FP_REQUIRE(alpha >= 0.f && alpha <= 1.f && lw >= 0.f && lw <= 64.f && radius >= 0.f && radius <= 64.f,
             "fp_vis_draw_matches: alpha in [0, 1], lw and radius in [0, 64]");
  for (int c = 0; c < 3; ++c) FP_REQUIRE(colour[c] >= 0.f && colour[c] <= 255.f, "fp_vis_draw_matches: colour outside [0, 255]");
  return launch_vis_draw_matches(segments, counts, batch, max_matches, h, w, colour, alpha, lw, radius, tile, ST(stream));
}

int fp_vis_scene_composite(const float* depth, const uint8_t* colours, int layers, int h, int w, const uint8_t* img, uint8_t* out,
                           int32_t* ids, fp_stream_t stream) {
  FP_REQUIRE(depth && colours && img && out && ids, "fp_vis_scene_composite: null pointer");
  FP_REQUIRE(layers >= 1 && layers <= FP_VIS_MAX_LAYERS && vis_side(h) && vis_side(w), "fp_vis_scene_composite: bad sizes (%d layers, %d x %d)",
             layers, h, w);
  return launch_vis_scene_composite(depth, colours, layers, h, w, img, out, ids, ST(stream));
}

}  // extern "C"
