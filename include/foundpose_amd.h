/* foundpose_amd -- C ABI of the MI355X (gfx950) FoundPose hot path.
 *
 * The reference (facebookresearch/foundpose) has NO native/FFI layer: its boundary for this path is the
 * Python call surface used by scripts/infer.py:468-542.  This header is the new native boundary that the
 * drop-in Python modules in foundpose_amd/ (same names and signatures as the reference's utils modules) bind with
 * ctypes.  Each entry point cites the reference computation it replaces (paths relative to the reference
 * root).  Conventions:
 *   - every pointer is a DEVICE pointer unless it says "host"; the caller owns all memory (no allocation
 *     inside the library), including scratch; all work is enqueued on `stream` (a hipStream_t), nothing
 *     synchronises; the library keeps no mutable global state besides the thread-local error string and idempotent
 *     per-device caches (which kernels already had their dynamic-LDS limit raised on a device, its CU count), and
 *     reads no environment variable
 *   - return value: 0 = ok, 1 = invalid argument, 2 = unsupported, 3 = HIP failure; fp_last_error() gives text
 *   - indices on the device are int32; distances/scores fp32; L2 distances are SQUARED (faiss convention)
 *   - canonical ordering of every top-k: best value first, ties broken by the lowest index
 */
#ifndef FOUNDPOSE_AMD_H
#define FOUNDPOSE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fp_stream_t; /* hipStream_t */

enum { FP_F32 = 0, FP_BF16 = 1, FP_FP8 = 2, FP_F16X3 = 3, FP_F16F8 = 4, FP_F16 = 5 }; /* element types of activation / weight buffers (FP_FP8: OCP e4m3
                                                               weights, fp_vit_model only; FP_F16X3: split-fp16 rows, FP_F16F8: f16f8 rows, see below;
                                                               FP_F16: plain IEEE fp16 -- the "f16" mode, see FP_GEMM_F16) */

/* ---- split-fp16 rows (the "f16x3" near-exact mode) --------------------------------------------------------------------
 * The reference computes the backbone in fp32 (scripts/infer.py:468-473).  The fp32-input MFMA runs at 1/16 of the fp16 /
 * bf16 rate on this part, so the near-exact mode carries every GEMM / attention operand as a PAIR of fp16 numbers and builds
 * each product from three fp16 MFMAs with fp32 accumulation: x ~ (hi + lo) / s, hi = f16(s x), lo = f16(s x - hi) (22 mantissa
 * bits; s a power of two that places typical magnitudes well inside the fp16 normal range, saturation at +-65504), and
 * a b = hi_a hi_b + hi_a lo_b + lo_a hi_b (the dropped lo lo term is <= 2^-22 relative).
 * Storage: a logical row of K values (K % 32 == 0) is 2K halves: group g = k / 32 holds hi(x[32g .. 32g + 31]) in halves
 * [64g, 64g + 32) and lo(...) in [64g + 32, 64g + 64).  Fixed scales of the activation rows inside fp_vit_forward: */
#define FP_SPLIT_SCALE_ACT 16.f /* LayerNorm outputs, attention outputs, normalised pixels of the patch rows: saturation at +-4094 */
#define FP_SPLIT_SCALE_QKV 16.f /* q, k, v rows written by the qkv GEMM: saturation at +-4094 */
#define FP_SPLIT_SCALE_HID 4.f  /* hidden activations written by the GELU / SwiGLU epilogue: saturation at +-16376 */
/* (A pair represents x to within max(2^-22 |x|, 2^-25 / s): the lo half of a small value is an fp16 subnormal, which the MFMA
 *  multiplies like any other number, so a modest scale costs nothing on O(1) activations and leaves three decades of head room for
 *  the outlier channels of real checkpoints.) */

/* ---- f16f8 rows (the "f16f8" mode: the split product with its two cross terms on the fp8 pipe) ---------------------------------
 * a b = hi_a hi_b + (hi_a lo_b + lo_a hi_b): the cross terms are ~2^-11 of the product, so they do not need fp16 operands.  An f16f8
 * row keeps the fp16 high halves and carries e4m3 copies of hi and lo for the cross terms, which run as two 64-wide
 * v_mfma_scale_f32_32x32x64_f8f6f4 (twice the fp16 rate): 8 instead of 12 fp16-MFMA units per 64 k at the same 4 bytes per element.
 * Storage: a logical row of K values (K % 64 == 0) is 4K bytes; group g = k / 64 holds  bytes [256g, 256g + 128): hi = f16(s x) (64 halves);
 * [256g + 128, 256g + 192): e4m3(hi 2^-7); [256g + 192, 256g + 256): e4m3((s x - hi) 2^4).  Same scales s and saturation report as the
 * split-fp16 rows.  A product carries ~14 mantissa bits at the worst (measured on fc2, K = 4096: max error 1.3e-5 of the output scale
 * against 1.9e-6 for f16x3); fp_vit_forward with weight_dtype FP_F16F8 uses these rows for every GEMM operand, while q | k | v and the
 * attention's own products stay split-fp16 (three fp16 MFMAs). */
#define FP_GEMM_SPLIT_F16F8 (1 << 20) /* OR-ed into fp_gemm_split's `epilogue`: A, W (and a GELU / SwiGLU output) are f16f8 rows, K % 64 == 0 */

/* ---- plain fp16 rows (the "f16" mode) ------------------------------------------------------------------------------------------
 * The bf16 pipeline of fp_vit_forward -- folded LayerNorms, (hi, lo) residual stream, the same kernels, tiles and bytes -- on IEEE fp16 operands
 * (v_mfma_f32_32x32x16_f16 runs at the bf16 rate): 11 significant bits per operand instead of 8, and a GELU polynomial good to 3.8e-5 (bf16 epilogue: 4e-4).
 * fp16 has bf16's speed but not its range: a 16-bit output beyond +-65504 becomes inf (nothing is clamped).  An inf poisons its row's residual stream and, through
 * the next attention's keys and values, every token of the image, so the pipeline's last kernel (fp_vit_features / fp_vit_sample_features*) counts non-finite
 * features into fp_vit_workspace.sat[0]; the Python extractor raises FoundPoseSaturationError for such a batch (apply_norm = 0: the caller checks the copy).
 * No operand scales: the residual stream and the activations of DINOv2 checkpoints sit orders of magnitude inside the range, values below 6e-5 keep an
 * absolute error <= 3e-8 (fp16 subnormals, which the MFMA honours). */
#define FP_GEMM_F16 (1 << 21) /* OR-ed into fp_gemm_bf16's / fp_gemm_bf16_ln's `epilogue`: A, W, the 16-bit outputs and the (xb, xl) stream are IEEE fp16 */

#define FP_ABI_VERSION 20
int fp_abi_version(void);
const char* fp_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Descriptor matching half
 * ---------------------------------------------------------------------------------------------- */

/* out[i] = |x_i|^2 as a k-ascending fp32 fma chain.  Part of faiss IndexFlatL2 (utils/knn_util.py:48-50).
 * Here and in fp_normalize_rows, fp_sample_bilinear and fp_pca_project a count of 0 is a no-op, and the pointers may then be null. */
int fp_sqnorm_rows(const float* x, int64_t n, int d, float* out, fp_stream_t stream);

/* out = x / max(|x|, eps) per row: the per-operand normalisation of torch cosine_similarity
 * (utils/template_util.py:167); run once per bank on template_descs. */
int fp_normalize_rows(const float* x, int64_t n, int d, float eps, float* out, fp_stream_t stream);

/* Exact brute-force L2 k-NN: KNN.fit + KNN.search with metric "l2" (utils/knn_util.py:38-106).
 * q [m,d], db [n,d], precomputed squared norms of both.  Scratch: FP_KNN_SCRATCH_BYTES(m, n, k): k == 1: m*8 bytes; 2 <= k <= 8:
 * m * max(ceil(n/128) * k * 8, 704) bytes (candidate keys, no distance matrix); k > 8: m*n*4 bytes.  out_d2 [m,k] (squared),
 * out_idx [m,k] int32, ascending, ties -> lowest index, (inf, -1) past the database size. */
#define FP_KNN_SCRATCH_BYTES(m, n, k) \
  ((k) == 1 ? (size_t)(m) * 8 : ((k) <= 8 ? (size_t)(m) * ((size_t)(((n) + 127) / 128) * (k) * 8 > 704 ? (size_t)(((n) + 127) / 128) * (k) * 8 : 704) : (size_t)(m) * (n) * 4))
int fp_knn_l2(const float* q, const float* q_sqnorm, int m, const float* db, const float* db_sqnorm, int n,
              int d, int k, void* scratch, float* out_d2, int32_t* out_idx, fp_stream_t stream);

/* tf-idf descriptors for `num_segs` point sets (one detection's query patches each):
 * calc_tfidf (utils/template_util.py:31-71) + the query-side normalisation of cosine_similarity.
 * word_ids/word_d2 [sumQ, knn_k] from fp_knn_l2 against the visual words; seg_off [num_segs+1].
 * sqrt_dists=1 applies the sqrt of find_nearest_object_features (template_util.py:26-27) before the
 * soft-assignment weights (the bank side, template_util.py:112-119, passes 0).
 * desc [num_segs, num_words]; desc_n (may be null) = desc / max(|desc|, eps). */
int fp_tfidf_build(const int32_t* word_ids, const float* word_d2, int knn_k, const int32_t* seg_off, int num_segs,
                   const float* idf, int num_words, int soft_assign, float soft_sigma_squared, int sqrt_dists,
                   float* desc, float* desc_n, float eps, fp_stream_t stream);

/* Template retrieval: cosine similarity of each detection's descriptor against the template descriptors of
 * its object + top-n (tfidf_matching, utils/template_util.py:167-174).  Detections are grouped by object:
 * det_seg_off [num_obj+1] over rows of desc_n, obj_tpl_off [num_obj+1] over rows of bank_n (both
 * normalised), det_num_templates [num_det] = template count of each detection's object.  scratch_sims:
 * FP_COSINE_SCRATCH_FLOATS(num_det, max_templates) floats -- the finished scores [num_det, max_templates] (left there
 * for the caller) followed by the candidate keys of the fused top-n and one replay flag per detection.  Canonical fp32 summation order of a score:
 * num_words % 128 == 0: 8 contiguous k-slices, each an fma chain visiting every 16-block of k as
 * [0,4,8,12,1,5,...,15], slice sums added in slice order; num_words % 16 == 0: one such chain; else k ascending.
 * The order depends on num_words only -- never on the batch: more than 32 detections of one object are served in
 * 32-detection chunks by the same kernel.  out_scores/out_ids [num_det, n_top]; ids are object-local template ids,
 * -1 / -inf past the object's template count.  tie_mode: 0 = canonical (score, then lowest id); 1 = the tie order of
 * torch.topk on a CPU tensor (libstdc++ partial_sort / nth_element+sort replayed on the device; rows of any length,
 * n_top <= 32).  With n_top <= 7 the replay runs only for rows whose best n_top + 1 scores contain a tie (equal values,
 * +-0 or NaN): strictly decreasing scores make the top-n list unique, so the canonical list IS torch's. */
#define FP_COSINE_SCRATCH_FLOATS(num_det, max_templates) (2 * (size_t)(num_det) * (size_t)(max_templates) + 17 * (size_t)(num_det) + 2)
int fp_cosine_topk(const float* desc_n, const int32_t* det_seg_off, const int32_t* det_num_templates, int num_det,
                   int max_det_per_obj,
                   const float* bank_n, const int32_t* obj_tpl_off, int num_obj, int max_templates, int num_words,
                   int n_top, float* scratch_sims, float* out_scores, int32_t* out_ids, int tie_mode, fp_stream_t stream);

/* The same retrieval, same outputs bit for bit, in two stages (what match_batch calls): a first pass over an fp16 copy of the bank
 * (bank_n_f16 [T_total, num_words], round to nearest even; half the bytes, 1/16 of the matrix time) leaves approximate scores,
 * provably within eps = 2^-10 x 1.5625 of the exact ones for L2-normalised rows (bound derived in csrc/match.hip); every template within 2 eps of the (n_top + 1)-th best approximate score
 * -- a superset of the exact top n_top + 1, however large -- is then re-scored with the exact fp32 chain of fp_cosine_topk, and the
 * top n_top of those exact scores is the answer.  tie_mode 1: a row whose best n_top + 1 exact scores contain a tie needs its whole
 * row for the replay of torch.topk's order; such rows release fp_cosine_topk's single-pass kernel and the replay behind a device-side
 * flag (both exit at once otherwise).  The three dependent launches cost ~10 us of latency each, so the two-stage form is taken only
 * when the single pass would stream more than ~250 MB (max_templates x ceil(max_det_per_obj / 32) >= 30 000; tie_mode |
 * FP_COSINE_FORCE_PREFILTER forces it); otherwise, and when num_words is not a multiple of 1024 (<= 4096 with tie_mode 0, <= 2048 with
 * tie_mode 1: the strict order's exact fallback is the <= 2048-word single-pass kernel), for more than 65536
 * templates per object or n_top > 7, the call IS fp_cosine_topk.  scratch: FP_COSINE_PREFILTER_SCRATCH_FLOATS(num_det, max_templates) floats.
 * HARD PRECONDITIONS of the candidate bound (not checked; fp_cosine_topk has none of them and stays exact for any input): every row of
 * desc_n and bank_n has L2 norm <= 1 (what fp_normalize_rows writes), and bank_n_f16 is the round-to-nearest-even fp16 image of bank_n
 * element for element.  Unnormalised rows or any other fp16 copy void the superset guarantee -- true top-n templates can then be dropped
 * silently.  The Python side (foundpose_amd/bank.py) builds both from the same tensor. */
#define FP_COSINE_FORCE_PREFILTER 256
#define FP_COSINE_PREFILTER_SCRATCH_FLOATS(num_det, max_templates) (FP_COSINE_SCRATCH_FLOATS(num_det, max_templates) + 3 * (size_t)(num_det) * (size_t)(max_templates) + 32 * (size_t)(num_det) + 16)
int fp_cosine_topk_prefiltered(const float* desc_n, const int32_t* det_seg_off, const int32_t* det_num_templates, int num_det, int max_det_per_obj,
                               const float* bank_n, const void* bank_n_f16, const int32_t* obj_tpl_off, int num_obj, int max_templates, int num_words,
                               int n_top, float* scratch, float* out_scores, int32_t* out_ids, int tie_mode, fp_stream_t stream);

/* Cyclic best-buddy matching of every detection against its n_slots retrieved templates and assembly of the
 * 2D-3D correspondences (cyclic_buddies_matching + the gather in establish_correspondences,
 * utils/corresp_util.py:34-70,107-155).
 *   query_feats [sumQ,d], query_sqnorm [sumQ], query_points [sumQ,2], q_off [B+1]
 *   bank_feats [N_f,d] sorted by template, bank_sqnorm [N_f], tpl_off [T_total+1], vertices [N_f,3]
 *   tpl_ids [B*n_slots] template ids, <0 = empty slot: object-local (as fp_cosine_topk reports them) when tpl_base [B] = first
 *   template of each detection's object is given, GLOBAL ids when tpl_base is NULL
 *   feat_base [B]: first feature row of the detection's object (reported feature ids are object-local)
 *   scratch: FP_CYCLIC_SCRATCH_BYTES(B * n_slots, q_max, p_max) bytes (nearest-neighbour keys of both directions, one slice of keys per
 *   128 x 128 distance tile of the all-pairs exact-fp32 search; nothing has to be preset)
 * outputs, padded to k_max >= top_k per (detection, slot): count, query ids, object feature ids (= the
 * reference's nn_vertex_ids), cycle distances, confidences, coord_2d, coord_3d.  tie_mode as in fp_cosine_topk: 1 makes
 * the order (and the choice among tied distances at the top_k boundary) identical to the reference's
 * torch.topk(-cycle_dists, k). */
#define FP_CYCLIC_SCRATCH_TILES(pairs, q_max, p_max) \
  (8 * (size_t)(pairs) * ((size_t)(((p_max) + 127) / 128) * (size_t)(q_max) + (size_t)(((q_max) + 127) / 128) * (size_t)(p_max)))
#define FP_CYCLIC_SCRATCH_CAND(pairs, q_max, p_max) \
  (8 * (size_t)(pairs) * ((size_t)(q_max) + (size_t)(p_max)) + 448 * (size_t)(pairs) * (size_t)((q_max) > (p_max) ? (q_max) : (p_max)))
#define FP_CYCLIC_SCRATCH_BYTES(pairs, q_max, p_max) \
  (FP_CYCLIC_SCRATCH_TILES(pairs, q_max, p_max) > FP_CYCLIC_SCRATCH_CAND(pairs, q_max, p_max) ? FP_CYCLIC_SCRATCH_TILES(pairs, q_max, p_max) \
                                                                                             : FP_CYCLIC_SCRATCH_CAND(pairs, q_max, p_max))
int fp_cyclic_buddies(const float* query_feats, const float* query_sqnorm, const float* query_points,
                      const int32_t* q_off, int num_det, int q_max, const float* bank_feats,
                      const float* bank_sqnorm, const int32_t* tpl_off, int p_max, const float* vertices,
                      const int32_t* tpl_ids, const int32_t* tpl_base, const int32_t* feat_base, int n_slots, int d, int top_k, int k_max,
                      void* scratch, int32_t* out_count, int32_t* out_q_ids, int32_t* out_feat_ids,
                      float* out_dists, float* out_conf, float* out_coord_2d, float* out_coord_3d, int tie_mode,
                      fp_stream_t stream);

/* The fixed-size record of each detection for the one exchange step of a multi-GPU run (an RCCL all-gather of these rows):
 * out [num_det, n_slots * (3 + 9 * k_max)] 32-bit words typed fp32 -- per slot (template id, score, count), then per correspondence
 * (query id, feature id = nn_vertex_ids, distance, confidence, x, y, X, Y, Z).  Integer fields keep their bit patterns (ids above
 * 2^24 survive). */
int fp_pack_records(const int32_t* template_ids, const float* template_scores, const int32_t* counts, const int32_t* q_ids, const int32_t* feat_ids,
                    const float* dists, const float* conf, const float* coord_2d, const float* coord_3d, int num_det, int n_slots, int k_max, float* out,
                    fp_stream_t stream);

/* Coarse pose of every (detection, template slot) pair from its 2D-3D correspondences: estimate_pose
 * (utils/pnp_util.py:20-84 = cv2.solvePnPRansac(..., SOLVEPNP_ITERATIVE) + cv2.solvePnPRefineLM on the inliers), the call
 * scripts/infer.py:552-580 makes once per retrieved template.  Inputs are fp_cyclic_buddies' padded outputs: coord_2d
 * [num_pairs, k_max, 2], coord_3d [num_pairs, k_max, 3], counts [num_pairs]; cameras [num_pairs / n_slots, 4] f64 =
 * (fx, fy, cx, cy) of each detection's crop camera.  RANSAC over `ransac_iters` P3P hypotheses (3 points + 1 to choose
 * among the solutions), inlier = reprojection error <= inlier_thresh px, the first model with the most inliers inside the
 * adaptively shortened budget (confidence) wins, then <= lm_iters Levenberg-Marquardt iterations on its inliers (20 for
 * the refinement inside solvePnPRansac, +20 with pnp_refine_lm).  Pairs with fewer than min_corresp (6, infer.py:556)
 * correspondences or without a model fail (success 0).  Outputs: success, R [.,9] row-major and t [.,3] (model ->
 * camera, f64), the RANSAC inlier count (the reference's `quality`), the inlier mask [., k_max], and (may be null) the
 * winning model before refinement [., 12].  cv2's own arithmetic and random stream are not reproduced (cv2 is not
 * available to pin them): same scheme, different minimal solver and sampler -- see csrc/pnp.hip. */
int fp_pnp_ransac(const float* coord_2d, const float* coord_3d, const int32_t* counts, const double* cameras, int num_pairs, int n_slots,
                  int k_max, int ransac_iters, double inlier_thresh, double confidence, int lm_iters, int min_corresp, uint64_t seed,
                  int32_t* out_success, double* out_R, double* out_t, int32_t* out_num_inliers, uint8_t* out_inlier_mask,
                  double* out_ransac_pose, fp_stream_t stream);

/* fp_pnp_ransac with the sampler key of every pair given by the caller: pair_keys [num_pairs].  fp_pnp_ransac draws the hypotheses of a
 * pair from (seed, the pair's index in the launch), so a pair's hypotheses change with its neighbours in the batch; here they are drawn
 * from (seed, pair_keys[pair]) and a pair's result is the same in whatever launch and at whatever position it runs.  With
 * pair_keys[i] == i the results are those of fp_pnp_ransac bit for bit (same kernel). */
int fp_pnp_ransac_keyed(const float* coord_2d, const float* coord_3d, const int32_t* counts, const double* cameras, const uint64_t* pair_keys,
                        int num_pairs, int n_slots, int k_max, int ransac_iters, double inlier_thresh, double confidence, int lm_iters,
                        int min_corresp, uint64_t seed, int32_t* out_success, double* out_R, double* out_t, int32_t* out_num_inliers,
                        uint8_t* out_inlier_mask, double* out_ransac_pose, fp_stream_t stream);

/* Coarse pose of every (detection, template slot) pair from its 2D-3D correspondences and the frame's depth image: a rigid 3D-3D RANSAC
 * on depth-lifted correspondences (this project's own stage, the reference has none).  coord_2d / coord_3d / counts
 * as in fp_pnp_ransac (counts clamped to [0, k_max]).  Per detection (num_pairs / n_slots of them): solve_cameras [., 4] f64 = (fx, fy, cx,
 * cy) of the camera the pixels are in, frame_cameras [., 4] of the frame's own camera, A [., 9] f64 the row-major rotation solve camera ->
 * frame camera (the two share their centre), image_index [.] into depth [num_images, H, W] fp32 mm (0 = no measurement), inlier_thresh_mm
 * [.] f64 (> 0).  A pixel (u, v) is lifted in fp64: d = ((u - cx) / fx, (v - cy) / fy, 1), d_f = A d, invalid if d_f.z <= 1e-9; the depth
 * pixel (rint(fx_f d_f.x / d_f.z + cx_f), rint(...)) (half to even), invalid outside the image or where the depth is <= 0 (never read
 * outside); Y = depth / d_f.z * d, stored as fp32, is the measured point in the SOLVE camera.  num_valid counts the valid ones; fewer than
 * min_corresp (>= 3) fail the pair.  Hypothesis h: 3 distinct valid indices from fp_pnp_ransac's sampler (seed, pair_keys[pair] or, with
 * pair_keys null, the pair's index; an invalid or repeated draw is redrawn, at most 64 times per index), rejected unless every edge has
 * | |X_i - X_j| - |Y_i - Y_j| | <= 2 tau, fitted in closed form from the two triangle frames; its score is the number of valid
 * correspondences with |R X + t - Y| <= tau.  The first hypothesis with the most (> 2) inliers inside the adaptively shortened budget
 * (confidence, 3 model points) wins; with refit != 0 the output pose is Horn's closed-form least-squares fit on its inliers, otherwise the
 * hypothesis itself.  Outputs as fp_pnp_ransac's (model -> solve camera) plus out_num_valid [num_pairs]; out_success is 1, 0, or -1 for a
 * detection whose image_index is outside [0, num_images) or whose threshold is not positive (nothing of the stack is read for it).
 * k_max <= 4096, ransac_iters <= 4096.  Every sum has a fixed order: a pair's result depends on (seed, its key, its own data) only. */
int fp_kabsch_ransac(const float* coord_2d, const float* coord_3d, const int32_t* counts, const double* solve_cameras, const double* frame_cameras,
                     const double* A, const int32_t* image_index, const double* inlier_thresh_mm, const float* depth, int num_images, int H, int W,
                     const uint64_t* pair_keys, int num_pairs, int n_slots, int k_max, int ransac_iters, double confidence, int refit,
                     int min_corresp, uint64_t seed, int32_t* out_success, double* out_R, double* out_t, int32_t* out_num_inliers,
                     int32_t* out_num_valid, uint8_t* out_inlier_mask, double* out_ransac_pose, fp_stream_t stream);

/* Hypothesis verification against depth (this project's own stage): the point sample of the whole model placed at
 * the pose of every (detection, template slot) pair, its self-occlusion decided by a G x G z-buffer of the sample, each visible point
 * classified against the frame's depth image.  Per pair: success [num_pairs] (> 0: the pair has a pose), R [., 9] / t [., 3] f64 row-major
 * model -> solve camera (fp_pnp_ransac's / fp_kabsch_ransac's outputs).  Per detection (num_pairs / n_slots of them): frame_cameras [., 4]
 * f64 = (fx, fy, cx, cy), A [., 9] f64 the rotation solve camera -> frame camera, image_index [.] into depth [num_images, H, W] fp32 mm
 * (0 = no measurement), thresh_mm [.] f64 (tau), point_ranges [., 2] = [begin, end) of the detection's object in points [num_points, 3]
 * fp32 (clamped to [0, num_points]), centers [., 3] / radii [.] f64: the sample's centre c and its radius rho about c.  All arithmetic is
 * fp64, every step one rounded operation in this order (no FMA contraction), sums of products with k ascending:
 *   R_f = A R, t_f = A t;  C = R_f c + t_f; status 2 unless C.z > rho + 1;  u_c = fx C.x / C.z + cx, v_c alike;
 *   r_px = max(fx, fy) rho / (C.z - rho), cell side h = 2 r_px / G; a pixel (u, v) lies in cell
 *   (clamp(floor((u - (u_c - r_px)) / h), 0, G - 1), clamp(floor((v - (v_c - r_px)) / h), 0, G - 1)) (the clamp is part of the contract);
 *   pass 1: X_c = R_f X + t_f, ignored when X_c.z <= 1; u = fx x / z + cx, v alike; zbuf[cell] = min(zbuf[cell], (float)z), cells start at +inf;
 *   pass 2: a point with z > 1 is visible iff z <= (double)zbuf[cell] + tau; a visible point adds 1 to n_vis and to exactly one of
 *     n_out (px = rint(u), py = rint(v), half to even, outside [0, W-1] x [0, H-1]: never read), n_hole (D[py, px] <= 0), and with
 *     r = D - z: n_in (|r| <= tau), n_occ (r < -tau), n_free (r > tau).
 * out_counts [num_pairs, 6] = (n_vis, n_in, n_occ, n_free, n_hole, n_out); out_score [num_pairs] f64 = n_in / n_vis when n_vis >=
 * min_visible (>= 1), else 0; out_status [num_pairs]: 0 scored, 1 fewer than min_visible visible points, 2 skipped (success <= 0, an empty
 * point range, or C.z <= rho + 1; counts and score 0), -1 for a detection whose image_index is outside [0, num_images) or whose tau is not
 * positive and finite (nothing of the stack is read for it; counts and score 0).  grid G in [8, 128].  A pair's result depends on its own
 * data only: it is the same bits alone, in any batch and at any position. */
int fp_pose_verify_depth(const int32_t* success, const double* R, const double* t, const double* frame_cameras, const double* A,
                         const int32_t* image_index, const double* thresh_mm, const int32_t* point_ranges, const double* centers, const double* radii,
                         const float* points, int num_points, const float* depth, int num_images, int H, int W, int num_pairs, int n_slots, int grid,
                         int min_visible, int32_t* out_counts, double* out_score, int32_t* out_status, fp_stream_t stream);

/* Hypothesis verification against the detection's mask (this project's own stage): the point sample of the whole
 * model placed at the pose of every (detection, template slot) pair, the cells of a G x G grid its points project into taken as the model's
 * silhouette, and that silhouette compared with the detection's mask.  success, R, t, frame_cameras, A, point_ranges, centers, radii, points
 * and num_points are fp_pose_verify_depth's.  masks [num_pairs / n_slots, H, W] uint8: each detection's own mask in the frame camera's image
 * (non-zero = set); mask_areas [.] int32: the number of set pixels of each.  All arithmetic is fp64, every step one rounded operation in
 * this order (no FMA contraction):
 *   R_f, t_f, C, status 2 unless C.z > rho + 1, u_c, v_c, r_px, u0 = u_c - r_px, v0 = v_c - r_px, h = 2 r_px / G: fp_pose_verify_depth's;
 *   pass 1: every sampled point with X_c.z > 1 sets the bit of its cell (fp_pose_verify_depth's cell, the clamp included) in a bitmap;
 *   pass 2: a pixel (px, py), integers in [0, W-1] x [0, H-1], has ix = floor((px - u0) / h), iy alike (no clamp); it is a model pixel iff
 *     0 <= ix < G, 0 <= iy < G and the bit of cell iy G + ix is set; n_both counts the model pixels whose mask byte is non-zero,
 *     n_model_only the others.  No byte outside the image is read, whatever the pose.
 * out_counts [num_pairs, 4] = (n_both, n_model_only, n_mask_only = area - n_both, n_cells = set bits of the bitmap); out_score [num_pairs]
 * f64 = n_both / (n_both + n_model_only + n_mask_only), one division of two integers converted to double, when n_both + n_model_only >=
 * min_pixels (>= 1), else 0; out_status [num_pairs]: 0 scored, 1 fewer than min_pixels model pixels (counts reported), 2 skipped (success
 * <= 0, an empty point range, or C.z <= rho + 1; counts and score 0).  grid G in [8, 128]; H W at most 2^30.  A pair's result depends on
 * its own data only: it is the same bits alone, in any batch and at any position. */
int fp_pose_verify_mask(const int32_t* success, const double* R, const double* t, const double* frame_cameras, const double* A,
                        const int32_t* point_ranges, const double* centers, const double* radii, const float* points, int num_points,
                        const uint8_t* masks, const int32_t* mask_areas, int H, int W, int num_pairs, int n_slots, int grid, int min_pixels,
                        int32_t* out_counts, double* out_score, int32_t* out_status, fp_stream_t stream);

/* Detection masks from their COCO run lengths (the device_masks path of infer_batched): what
 * infer_pose_util.rle_to_binary_mask, open_mask_3x3 and the centre crop of the host path compute, for num_det detections in one call.
 * counts [num_runs] int32: the run lengths of all detections, concatenated; run_off [num_det + 1] int32: detection n owns the R =
 * run_off[n + 1] - run_off[n] runs from run_off[n] on (offsets are clamped to [0, num_runs], nothing outside counts is read).  hc, wc: the
 * detector's canvas, shared by the call; H <= hc, W <= wc: the image; hc wc at most 2^30.
 *   decode: with s_i the inclusive prefix sums of the detection's runs (a negative count counts as 0, the sums saturate at 2^31 - 1), canvas
 *     pixel (x, y) has the column-major index p = x hc + y and k = the number of s_i <= p; it is set iff k < R and k is odd (runs alternate
 *     0 / 1 starting with 0; a total short of hc wc leaves the rest 0, what lies beyond hc wc is ignored);
 *   opening (open3x3 != 0), on the canvas: an eroded pixel is 1 iff every pixel of its 3 x 3 that lies inside the canvas is 1, a dilated
 *     pixel is 1 iff any pixel of its 3 x 3 of the eroded image that lies inside the canvas is 1;
 *   crop: dx = (wc - W) / 2, dy = (hc - H) / 2 (integer division); out_masks[n, y, x] = canvas pixel (x + dx, y + dy), 0 or 1.
 * out_masks [num_det, H, W] uint8, every byte written; out_area [num_det] int32: the set pixels of each mask.  scratch_prefix: num_runs
 * int32.  num_det = 0 returns without a launch.  A detection's result depends on its own runs only: it is the same bits alone, in any
 * batch and at any position.  (Added without a change of FP_ABI_VERSION: no existing entry point changed.) */
int fp_detection_masks(const int32_t* counts, const int32_t* run_off, int num_runs, int num_det, int hc, int wc, int H, int W, int open3x3,
                       int32_t* scratch_prefix, uint8_t* out_masks, int32_t* out_area, fp_stream_t stream);

/* Duplicate suppression between the poses of one frame (this project's own stage), first half: for every ordered
 * pair (i, j) = pairs[p] of poses given in ONE common coordinate frame, the fraction of i's model sample that lies in space occupied by j's
 * model.  points [num_points, 3] f32, point_ranges [num_objects, 2] ([begin, end), clamped to [0, num_points]), centers [num_objects, 3]
 * and radii [num_objects] f64: the compact samples fp_pose_verify_depth uses, per OBJECT here; pose_obj [num_poses] int32: each pose's
 * object; valid [num_poses] int32 (> 0: the pose takes part); R [num_poses, 9] row-major and t [num_poses, 3] f64; pairs [num_pairs, 2]
 * int32.  All arithmetic is fp64, every step one rounded operation in this order (no FMA contraction), products summed k ascending:
 *   skip: status 2 if either pose is not valid, either point range is empty or !(rho_j > 0);
 *   spheres: C_p = R_p c_p + t_p (fp_pose_verify_depth's order), d2 = ((dx dx + dy dy) + dz dz) of C_i - C_j, s = rho_i + rho_j; status 1
 *     if !(d2 <= s s) (disjoint spheres, or a NaN): no point is read;
 *   grid of j in j's own model frame: x0 = c_j - rho_j per axis, h = 2 rho_j / G;
 *   pass 1: every point x of j's sample sets bit (iz G + iy) G + ix of a bitmap, per axis i = (int) fmin(fmax(floor((x - x0) / h), 0),
 *     G - 1) (fmax / fmin drop a NaN: cell 0);
 *   pass 2: every point x of i's sample: X = R_i x + t_i, d = X - t_j, y_k = (R_j[0,k] d_0 + R_j[1,k] d_1) + R_j[2,k] d_2, q_k =
 *     floor((y_k - x0_k) / h) without a clamp; the point is inside the cube iff 0 <= q_k < G on all three axes, decided in fp64 before
 *     any conversion to an integer; n_in counts the inside points whose cell's bit is set.
 * out_counts [num_pairs, 2] = (n_in, n_cells = set bits of the bitmap); out_overlap [num_pairs] f64 = n_in / n_i, one division of two
 * integers converted to double, n_i the number of points of i's sample; out_status [num_pairs]: 0 scored, 1 disjoint spheres, 2 skipped
 * (counts and overlap 0 for both).  grid G in [8, 32].  The caller validates pose_obj and pairs (device arrays the entry point cannot
 * read); an index outside its table that arrives all the same gives status 2 and nothing is read through it.  A pair's result depends on
 * its own data only: it is the same bits alone, in any batch and at any position.  (Added without a change of FP_ABI_VERSION: no existing
 * entry point changed.) */
int fp_pose_overlap(const float* points, int num_points, const int32_t* point_ranges, const double* centers, const double* radii,
                    int num_objects, const int32_t* pose_obj, const int32_t* valid, const double* R, const double* t, int num_poses,
                    const int32_t* pairs, int num_pairs, int grid, int32_t* out_counts, double* out_overlap, int32_t* out_status,
                    fp_stream_t stream);

/* ... second half: greedy suppression per frame.  group_off [num_groups + 1] int32: frame g owns the poses [group_off[g], group_off[g + 1]),
 * at most 256 of them, laid out IN RANK ORDER (the caller sorts by score descending, equal scores in input order); pair_off
 * [num_groups + 1] int32: frame g owns the pairs [pair_off[g], pair_off[g + 1]) of pairs [num_pairs, 2] (pose indices in that layout),
 * overlap [num_pairs] f64 and status [num_pairs] int32 (the three as the first half takes and writes them).  Poses a and b of a frame
 * conflict iff some pair (a, b) or (b, a) has status 0 and overlap >= thresh.  For r = 0, 1, ...: if the pose of rank r is still alive,
 * every alive pose of a later rank that conflicts with it is suppressed by it.  out_keep [num_poses] int32 (1 kept, 0 suppressed);
 * out_suppressed_by [num_poses] int32: the pose index of the suppressor (the first kept pose in rank order that conflicts), -1 for a kept
 * pose.  An empty frame and a frame of one pose are legal; offsets are clamped to their arrays and a frame to 256 poses (the caller
 * refuses larger ones); a pair that names a pose outside its frame is ignored.  Only poses of some frame are written.  (Added without a
 * change of FP_ABI_VERSION.) */
int fp_pose_nms_greedy(const int32_t* group_off, const int32_t* pair_off, int num_groups, const int32_t* pairs, const double* overlap,
                       const int32_t* status, int num_poses, int num_pairs, double thresh, int32_t* out_keep, int32_t* out_suppressed_by,
                       fp_stream_t stream);

/* The score of the BOP 6D detection task (restates the published behaviour of bop_toolkit's detection scores), first
 * half: greedy matching of every estimate group, once per column.  A group is the estimates of one (image, object); a column is
 * c = type * num_ths + k, type 0 = MSSD, 1 = MSPD, k < num_ths, 1 <= num_ths <= FP_DETECTION_MAX_THS, so there are C = 2 num_ths columns.
 * est_off / gt_off / pair_off [num_groups + 1] int32: group g owns the estimates [est_off[g], est_off[g + 1]) -- E_g of them, laid out IN
 * RANK ORDER (the caller sorts by score descending, equal scores in input order) --, the GT instances [gt_off[g], gt_off[g + 1]) -- G_g
 * <= FP_DETECTION_MAX_GROUP_GT of them, 0 is legal -- and the rows [pair_off[g], pair_off[g] + E_g G_g) of err [num_pairs, 2] f64 =
 * (mssd, mspd), row-major [E_g x G_g]: fp_pose_errors' out_err as it lies on the device.  gt_valid [num_gt] int32 (> 0: valid);
 * group_tab [num_groups] int32: the group's row of ths [num_tabs, 2, num_ths] f64 (the caller multiplies the thresholds out).
 * Rule per (group, column): for e = 0 .. E_g - 1 the estimate takes the not yet matched GT with the lowest error STRICTLY below the
 * threshold, ties to the lower GT index; a NaN error never matches; the matched GT is used up whether valid or not.
 * out_flag [num_est, C] int8: 1 matched to a valid GT (true positive), 2 matched to an invalid GT (ignored), 0 unmatched (false positive);
 * out_matched_gt [num_est, C] int32: the group-local GT index or -1.  Only estimates of some group are written.  Offsets are clamped to
 * their arrays, a group to 256 GT instances (the caller refuses more) and to the rows err has.  A group's result depends on its own data
 * only: the same bytes alone, in any batch and at any position.  (Added without a change of FP_ABI_VERSION: no existing entry point
 * changed.) */
#define FP_DETECTION_MAX_THS 16
#define FP_DETECTION_MAX_GROUP_GT 256
#define FP_DETECTION_MAX_REC 128
int fp_detection_match(const int32_t* est_off, const int32_t* gt_off, const int32_t* pair_off, int num_groups, const double* err,
                       int num_pairs, const int32_t* gt_valid, int num_gt, const int32_t* group_tab, const double* ths, int num_tabs,
                       int num_ths, int num_est, int8_t* out_flag, int32_t* out_matched_gt, fp_stream_t stream);

/* ... second half: the average precision per (object, column).  obj_off [num_objects + 1] int32: object o owns order[obj_off[o],
 * obj_off[o + 1]) of order [num_order] int32, the rows of flag [num_est, C] of its estimates over ALL images in global rank order (score
 * descending, equal scores in input order; sorted by the caller); n_valid [num_objects] int32: its valid GT instances over all target
 * images; rec_thr [num_rec] f64, 1 <= num_rec <= FP_DETECTION_MAX_REC.  Rule per (o, c): the estimates with flag 2 are dropped; over the
 * kept ones tp_k / fp_k are the inclusive running counts of flags 1 / 0, p_k = (double) tp_k / (double) (tp_k + fp_k), r_k = (double) tp_k
 * / (double) n_valid[o], pe_k = max over j >= k of p_j; q_i = pe_k* with k* the first kept k whose r_k >= rec_thr[i], 0 when there is
 * none; ap = (((q_0 + q_1) + q_2) + ...) / (double) num_rec, one rounded add each (no FMA contraction).  n_valid[o] <= 0: ap = -1, q = 0.
 * out_ap [num_objects, C] f64, out_q [num_objects, C, num_rec] f64, out_totals [num_objects, C, 3] int32 = (tp, fp, ignored).  All but
 * the divisions is integer arithmetic and maxima.  Offsets and rows are clamped to their arrays.  (Added without a change of
 * FP_ABI_VERSION.) */
int fp_detection_ap(const int32_t* obj_off, int num_objects, const int32_t* order, int num_order, const int8_t* flag, int num_est,
                    int num_ths, const int32_t* n_valid, const double* rec_thr, int num_rec, double* out_ap, double* out_q,
                    int32_t* out_totals, fp_stream_t stream);

/* Labelling of class-agnostic mask proposals (this project's own restatement of the published behaviour of CNOS's
 * second half), 1 of 4: the tight box and the area of every mask.  masks [num_prop, H, W] uint8, 0 / non-zero; H W at most 2^30.
 * out_box [num_prop, 4] int32 = (x1, y1, x2, y2) of the set pixels, x2 and y2 EXCLUSIVE; out_area [num_prop] int32.  An empty mask gives
 * (0, 0, 0, 0) and area 0.  Integers only (minima, maxima and a count): nothing is clamped; H, W < 1 or H W > 2^30 is refused.  A mask's
 * result depends on its own bytes only: it is the same bits alone, in any batch and at any position.  (Added without a change of
 * FP_ABI_VERSION: no existing entry point changed.) */
int fp_mask_boxes(const uint8_t* masks, int num_prop, int H, int W, int32_t* out_box, int32_t* out_area, fp_stream_t stream);

/* ... 2 of 4: the cut-out.  images [n_img, H, W, 3] fp32 HWC in [0, 1]; masks [num_prop, H, W] uint8; image_index [num_prop] int32 or
 * null (proposal p then reads image p); boxes [num_prop, 4] as fp_mask_boxes writes them; S in [1, FP_PROPOSAL_MAX_SIZE].
 * out [num_prop, 3, S, S] fp32 CHW, EVERY element written; out_status [num_prop] int32.  With w = x2 - x1, h = y2 - y1, L = max(w, h):
 *   w' = max(1, (2 w S + L) / (2 L)) and h' alike in integer arithmetic (w S / L rounded half up; the longer side becomes exactly S);
 *   ox = (S - w') / 2, oy = (S - h') / 2 (integer division): out[p, c, oy + i, ox + x] for i < h', x < w' is the window, all else is 0.
 *   Inside the window the value is the separable antialiased-bilinear resample of image * (mask != 0) restricted to the box -- the
 *   semantics of torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False).  Per axis n_in -> n_out, in fp64:
 *   scale = n_in / n_out, sup = max(scale, 1); output i has centre c = scale (i + 0.5), taps lo = max(0, (int)(c - sup + 0.5)) up to, not
 *   including, hi = min(n_in, (int)(c + sup + 0.5)); raw weight r_j = max(0, 1 - |(j - c + 0.5) / sup|), their sum n added j ascending,
 *   weight w_j = (float)(r_j (1 / n)).  Order, in fp32: horizontally u = fma(w_j, v_j, u) from 0 with j ascending along x for every source
 *   row, then vertically out = fma(w_j, u_j, out) from 0 with j ascending along y.  A masked-out pixel enters as 0 and keeps its weight.
 * Nothing is clamped; nothing outside the box is read.  Status 0: cropped; 2: an empty box (x2 <= x1 or y2 <= y1), a box that leaves the
 * image, or an image_index outside [0, n_img): the crop is all zero and neither the image nor the mask is read.  S outside its range,
 * more than 65535 proposals in one call or H W > 2^30 is refused.  A proposal's crop depends on its own box, mask and image only: it is the
 * same bits alone, in any batch and at any position.  (Added without a change of FP_ABI_VERSION.) */
#define FP_PROPOSAL_MAX_SIZE 1024
int fp_proposal_crops(const float* images, int n_img, int H, int W, const uint8_t* masks, const int32_t* image_index, const int32_t* boxes,
                      int num_prop, int S, float* out, int32_t* out_status, fp_stream_t stream);

/* ... 3 of 4: the score of every (proposal, object) and the label.  desc_n [num_prop, dim] and bank_n [num_bank, dim] fp32, rows
 * L2-normalised by fp_normalize_rows; obj_off [num_obj + 1] int32 over bank rows (device); max_templates: the largest template count of
 * an object (host; a longer object is cut to it); k in [1, FP_PROPOSAL_MAX_K].  A similarity is the dot product in fp_cosine_topk's
 * canonical summation order for num_words = dim: the call lists the proposals once per object in scratch and runs fp_cosine_topk's own
 * kernels on them with tie_mode 0, so the bits are that chain's.  With T_o the object's template count, m = min(k, T_o) and v_1 >= ... >=
 * v_m its m largest similarities (equal values ordered by the lower template id):
 *   score(p, o) = (((v_1 + v_2) + ...) + v_m) / (float)m, fp32, one rounded add each left to right and ONE division; T_o = 0: -inf.
 * out_scores [num_prop, num_obj]; out_best_obj [num_prop] int32: the object of the highest score, ties to the lower object index, a NaN
 * never wins and neither does -inf; out_best_score [num_prop]; out_best_template [num_prop] int32: the object-local id of v_1 of the best
 * object.  A proposal for which no object scores gets (-1, -inf, -1).  obj_off is clamped into [0, num_bank] and made non-decreasing
 * before anything is read through it.  scratch: FP_PROPOSAL_SCORE_SCRATCH_BYTES(num_prop, num_obj, dim, max_templates, k) bytes, 16-byte
 * aligned; the finished similarities stay at its start, [num_obj, num_prop, max_templates] floats (row (o, p), column = template of o), for
 * the caller.  k outside its range, num_obj < 1, dim < 1 or num_obj num_prop > 2^20 is refused; num_prop = 0 returns without a launch.
 * A proposal's results depend on its own descriptor and the bank only: they are the same bits alone, in any batch and at any position.
 * (Added without a change of FP_ABI_VERSION.) */
#define FP_PROPOSAL_MAX_K 16
#define FP_PROPOSAL_SCORE_SCRATCH_BYTES(num_prop, num_obj, dim, max_templates, k)                                                  \
  (16 * ((4 * FP_COSINE_SCRATCH_FLOATS((size_t)(num_obj) * (num_prop), max_templates) + 15) / 16) +                               \
   16 * ((4 * (size_t)(num_obj) * (num_prop) * (dim) + 15) / 16) + 2 * 16 * ((4 * ((size_t)(num_obj) + 1) + 15) / 16) +           \
   16 * ((4 * (size_t)(num_obj) * (num_prop) + 15) / 16) + 2 * 16 * ((4 * (size_t)(num_obj) * (num_prop) * (k) + 15) / 16))
int fp_proposal_scores(const float* desc_n, int num_prop, int dim, const float* bank_n, int num_bank, const int32_t* obj_off, int num_obj,
                       int max_templates, int k, void* scratch, size_t scratch_bytes, float* out_scores, int32_t* out_best_obj,
                       float* out_best_score, int32_t* out_best_template, fp_stream_t stream);

/* ... between 3 and 4: every proposal's decision, and the candidates of ONE image laid out for the suppression, without a read-back.
 * best_obj / best_score [num_prop] as fp_proposal_scores wrote them, area [num_prop] and boxes [num_prop, 4] as fp_mask_boxes did,
 * crop_status [num_prop] as fp_proposal_crops did.  out_decision [num_prop] int32, the first rule that applies:
 *   FP_PROPOSAL_SMALL area < min_area; FP_PROPOSAL_EMPTY crop_status != 0; FP_PROPOSAL_NO_OBJECT best_obj outside [0, num_obj);
 *   FP_PROPOSAL_LOW_SCORE !(best_score >= min_score) (a NaN too); else the proposal is a candidate of the group of its object, ranked
 *   by score descending, equal scores in input order: FP_PROPOSAL_GROUP_LIMIT for rank >= max_group, else FP_PROPOSAL_CANDIDATE.
 * The layout lists the groups in object order, each in rank order: out_group_off [num_obj + 1]; out_order [num_prop]: the proposal at
 * each place (-1 behind the last); out_boxes_ranked [num_prop, 4]: its box (zeros behind the last); out_pair_off [num_obj + 1] and
 * out_pairs [max_pairs, 2]: for a group of n candidates at places g0 .. g0 + n - 1 its n (n - 1) / 2 pairs (g0 + a, g0 + b), a < b, a-major;
 * the unused tail holds (-1, -1), which fp_box_iou answers with status 2 and fp_pose_nms_greedy never reads.  max_pairs >= num_prop
 * (max_group - 1) / 2.  One workgroup: at most FP_PROPOSAL_MAX_RANKED proposals and as many objects, max_group in [1, 256]; more, or a
 * NaN min_score, is refused.  Integer counting and float comparisons only.  (Added without a change of FP_ABI_VERSION.) */
#define FP_PROPOSAL_CANDIDATE 0
#define FP_PROPOSAL_SMALL 1
#define FP_PROPOSAL_EMPTY 2
#define FP_PROPOSAL_NO_OBJECT 3
#define FP_PROPOSAL_LOW_SCORE 4
#define FP_PROPOSAL_GROUP_LIMIT 5
#define FP_PROPOSAL_MAX_RANKED 4096
int fp_proposal_rank(const int32_t* best_obj, const float* best_score, const int32_t* area, const int32_t* crop_status, const int32_t* boxes,
                     int num_prop, int num_obj, int min_area, float min_score, int max_group, int max_pairs, int32_t* out_decision,
                     int32_t* out_order, int32_t* out_group_off, int32_t* out_pair_off, int32_t* out_pairs, int32_t* out_boxes_ranked,
                     fp_stream_t stream);

/* ... 4 of 4: intersection over union of integer boxes, in the form fp_pose_nms_greedy takes.  boxes [num_boxes, 4] int32 = (x1, y1, x2,
 * y2) with x2, y2 exclusive; pairs [num_pairs, 2] int32.  Per pair, in int64: area = max(x2 - x1, 0) max(y2 - y1, 0) of each box,
 * intersection = max(min(x2) - max(x1), 0) max(min(y2) - max(y1), 0) (0 if either area is 0), union = area_i + area_j - intersection;
 * out_overlap [num_pairs] f64 = (double)intersection / (double)union, one division of the two integers converted to double;
 * out_status [num_pairs] int32: 0 scored; 2: union 0, or an index outside [0, num_boxes) -- the overlap is 0 and nothing is read through
 * the index.  A pair's result depends on its two boxes only: it is the same bits alone, in any batch and at any position.  (Added without
 * a change of FP_ABI_VERSION.) */
int fp_box_iou(const int32_t* boxes, int num_boxes, const int32_t* pairs, int num_pairs, double* out_overlap, int32_t* out_status,
               fp_stream_t stream);

/* The appearance score of a proposal (the patch-descriptor score of CNOS's later versions and of SAM-6D's instance
 * segmentation stage, restated), 1 of 2: which ViT patches of a cut-out belong to the object.  masks, image_index, boxes, n_img, H, W and
 * S as fp_proposal_crops takes them; patch_size divides S (else refused); g = S / patch_size.  out_cover [num_prop, g g] int32, cells
 * row-major (the token order of the ViT), EVERY element written.  With w, h, L, w', h', ox, oy as fp_proposal_crops defines them, crop
 * pixel (X, Y) lies in the window iff ox <= X < ox + w' and oy <= Y < oy + h'; it then reads the mask byte at
 *   sx = x1 + ((2 (X - ox) + 1) w) / (2 w'),  sy = y1 + ((2 (Y - oy) + 1) h) / (2 h')   (integer divisions in int64; always inside the box)
 * and is covered iff that byte is non-zero.  cover(cell) = the covered pixels among the cell's patch_size^2.  A proposal whose crop status
 * would be 2 (an empty box, a box that leaves the image, an image_index outside [0, n_img)) gets all zeros and nothing is read.  Integers
 * only; a proposal's row depends on its own box and mask only: the same bits alone, in any batch and at any position.  (Added without a
 * change of FP_ABI_VERSION: no existing entry point changed.) */
int fp_proposal_patch_cover(const uint8_t* masks, int n_img, int H, int W, const int32_t* image_index, const int32_t* boxes, int num_prop, int S,
                            int patch_size, int32_t* out_cover, fp_stream_t stream);

/* ... 2 of 2: the score.  q_n [num_prop, num_patches, dim] fp32: the proposals' patch tokens, rows L2-normalised by fp_normalize_rows;
 * q_cover [num_prop, num_patches] int32; bank_patch_n [num_bank, num_patches, dim] and bank_cover [num_bank, num_patches]: the same of the
 * templates, in the row order of fp_proposal_scores' bank; obj_off [num_obj + 1], best_obj / best_template / best_score [num_prop] as
 * fp_proposal_scores takes and writes them (all on the device); min_cover >= 1.  Per proposal p:
 *   row     obj_off is clamped into [0, num_bank] and made non-decreasing; row = obj_off[best_obj] + best_template.  best_obj outside
 *           [0, num_obj) or best_template outside [0, T_o): status 2, and nothing is read through either index.
 *   valid   query patch j iff q_cover[p, j] >= min_cover; template patch i iff bank_cover[row, i] >= min_cover.
 *   sim     sim(j, i) = the fp32 chain acc = fmaf(q[k], t[k], acc), k = 0 .. dim - 1 ascending from acc = 0, one accumulator per (j, i).
 *   best    for a valid j: out_best_sim[p, j] = the maximum over the valid i from -inf, replaced only on v > best (equal values keep the
 *           lower i, a NaN never wins), out_best_patch[p, j] = that i (-1 if none won); an invalid j gets (0.0f, -1).
 *   score   out_n_valid[p] = the number of valid j; out_appearance[p] = (((s_j1 + s_j2) + ...)) / (float)n_valid in fp32 over the valid j
 *           ascending, one rounded add each and ONE division.
 *   status  0 scored; 1 no valid query patch; 2 no template row (n_valid = 0); 3 the template has no valid patch.  A status other than 0
 *           gives appearance 0, n_valid as counted, and (0.0f, -1) in every element of the row of out_best_sim / out_best_patch.
 *   out_score[p] = (best_score[p] + appearance[p]) * 0.5f; -inf stays -inf.
 * Every element of every output is written.  dim % 4 != 0, dim > 4096, num_patches outside [1, 8192], num_prop > 65535, num_obj < 1 or
 * min_cover < 1 is refused; num_prop = 0 returns without a launch.  A proposal's results depend on its own row and its template's only: the
 * same bits alone, in any batch and at any position.  (Added without a change of FP_ABI_VERSION.) */
int fp_proposal_appearance(const float* q_n, const int32_t* q_cover, int num_prop, int num_patches, int dim, const float* bank_patch_n,
                           const int32_t* bank_cover, int num_bank, const int32_t* obj_off, int num_obj, const int32_t* best_obj,
                           const int32_t* best_template, const float* best_score, int min_cover, float* out_best_sim, int32_t* out_best_patch,
                           float* out_appearance, int32_t* out_n_valid, int32_t* out_status, float* out_score, fp_stream_t stream);

/* COCO average precision of a detections file (foundpose_amd/eval_coco.py): BOP's 2D detection and 2D segmentation
 * scores.  Restates the published behaviour of pycocotools' COCOeval for instances without iscrowd; tests/coco_ref.py restates every entry.
 * 1 of 4: byte masks -> bit masks.  masks [num_masks, H, W] uint8, 0 unset / any non-zero byte set; H W at most 2^30.  out_words
 * [num_masks, H, Wq] uint64 with Wq = ceil(W / 64): bit x % 64 of word (y, x / 64) is pixel (x, y), the bits beyond W in a row's last word
 * are 0, EVERY word is written; out_area [num_masks] int32: the set pixels.  H, W < 1 or H W > 2^30 is refused; num_masks = 0 returns
 * without a launch.  A mask's result depends on its own bytes only: it is the same bits alone, in any batch and at any position.  (Added
 * without a change of FP_ABI_VERSION: no existing entry point changed.) */
int fp_mask_pack(const uint8_t* masks, int num_masks, int H, int W, uint64_t* out_words, int32_t* out_area, fp_stream_t stream);

/* ... 2 of 4: intersection over union of bit masks, group by group.  words_a [num_a, L] and words_b [num_b, L] uint64 as fp_mask_pack
 * wrote them (L = H Wq, 1 <= L <= 2^24); est_off / gt_off / pair_off [num_groups + 1] int32, the three tables fp_detection_match takes:
 * group g owns the rows [est_off[g], est_off[g + 1]) of a (E_g of them), [gt_off[g], gt_off[g + 1]) of b (G_g) and the E_g G_g output
 * rows from pair_off[g], row-major [E_g x G_g].  Per pair, in integers: inter = sum popcount(a & b), union = area_a + (area_b - inter)
 * with the areas the popcounts of the rows themselves; out_counts [num_pairs, 2] int32 = (inter, union); out_overlap [num_pairs] f64 =
 * (double)inter / (double)union, one division of two integers converted to double; out_status [num_pairs] int32: 0 scored, 2 union 0
 * (overlap 0).  Exact, so independent of any summation order.  Only rows of some group are written.  Offsets are clamped to their arrays
 * and a group to the rows the outputs have; nothing is read through an offset as it arrived.  scratch_tiles: num_groups + 1 int32.
 * A group's result depends on its own rows only: the same bytes alone, in any batch and at any position.  (Added without a change of
 * FP_ABI_VERSION.) */
int fp_group_mask_iou(const uint64_t* words_a, int num_a, const uint64_t* words_b, int num_b, int L, const int32_t* est_off,
                      const int32_t* gt_off, const int32_t* pair_off, int num_groups, int num_pairs, int32_t* scratch_tiles,
                      int32_t* out_counts, double* out_overlap, int32_t* out_status, fp_stream_t stream);

/* ... 2 of 4 for boxes: boxes_a [num_a, 4] and boxes_b [num_b, 4] f64 as COCO's (x, y, w, h), the same group tables.  Per pair, in fp64,
 * every step one rounded operation in this order (no FMA contraction):
 *   iw = fmin(xa + wa, xb + wb) - fmax(xa, xb), ih alike in y; inter = (iw > 0 && ih > 0) ? iw ih : 0;
 *   union = (wa ha + wb hb) - inter; overlap = inter / union.
 * out_status: 0 scored; 2 when !(union > 0) -- a NaN too -- or for an output row that no group owns: the overlap is 0.  EVERY row of
 * out_overlap / out_status [num_pairs] is written.  Offsets are clamped as above.  (Added without a change of FP_ABI_VERSION.) */
int fp_group_box_iou(const double* boxes_a, int num_a, const double* boxes_b, int num_b, const int32_t* est_off, const int32_t* gt_off,
                     const int32_t* pair_off, int num_groups, int num_pairs, double* out_overlap, int32_t* out_status, fp_stream_t stream);

/* ... 3 of 4: COCO's matching rule, once per (group, threshold).  The group tables as above with a = the estimates, laid out IN RANK ORDER
 * (the caller sorts by score descending, equal scores in input order, and cuts a group to max_dets), and b = the GT instances, G_g <=
 * FP_DETECTION_MAX_GROUP_GT; overlap [num_pairs] f64 as either call above wrote it; gt_ignore [num_gt] int32 (!= 0: an ignored
 * instance; the caller lays a group's non-ignored instances out first, as pycocotools does); ths [num_ths] f64 ON THE DEVICE, 1 <=
 * num_ths <= FP_DETECTION_MAX_THS, every threshold in (0, 1] (the caller checks the values).  Rule per (group, t), for e = 0 .. E_g - 1:
 * with b = fmin(ths[t], 1 - 1e-10) the candidates are the not yet matched instances with overlap >= b (a NaN never is); the estimate takes
 * the non-ignored candidate of the highest overlap if there is one, otherwise the ignored candidate of the highest overlap; equal
 * overlaps go to the HIGHER GT index; the matched instance is used up whether ignored or not.  This is the loop of evaluateImg in closed
 * form: its `if ious < iou: continue` lets a later equal candidate replace an earlier one.
 * out_flag [num_est, num_ths] int8: 1 matched to a non-ignored instance, 2 matched to an ignored one, 0 unmatched -- fp_detection_match's
 * codes, so fp_detection_ap takes the flags as they are (an even number of columns: the caller repeats the last column of an odd
 * num_ths); out_matched_gt [num_est, num_ths] int32: the group-local GT index or -1.  Only estimates of some group are written.  Offsets
 * are clamped to their arrays, a group to 256 instances (the caller refuses more) and to the rows overlap has.  A group's result depends
 * on its own data only: the same bytes alone, in any batch and at any position.  (Added without a change of FP_ABI_VERSION.) */
int fp_coco_match(const int32_t* est_off, const int32_t* gt_off, const int32_t* pair_off, int num_groups, const double* overlap,
                  int num_pairs, const int32_t* gt_ignore, int num_gt, const double* ths, int num_ths, int num_est, int8_t* out_flag,
                  int32_t* out_matched_gt, fp_stream_t stream);

/* sample_feature_map_at_points (utils/feature_util.py:100-131): bilinear grid_sample, zeros padding,
 * align_corners=False.  fmap addressed by element strides (image, channel, y, x); point_img (may be null)
 * maps each point to its image.  out [num_points, C]. */
int fp_sample_bilinear(const float* fmap, int64_t stride_img, int64_t stride_c, int64_t stride_h, int64_t stride_w,
                       int C, int H, int W, int img_w, int img_h, const float* points, const int32_t* point_img,
                       int num_points, float* out, fp_stream_t stream);

/* PCAProjector.transform (utils/projector_util.py:66-69): out = x @ C^T - mean_proj, mean_proj = mu @ C^T
 * (computed with the same kernel by passing x = mu, n = 1, mean_proj = null). */
int fp_pca_project(const float* x, int n, int D, const float* components, int d, const float* mean_proj,
                   float* out, fp_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Feature extraction half (DINOv2 ViT; the reference reaches it through
 * DinoFeatureExtractor.forward, utils/dinov2_utils.py:115-158)
 * ---------------------------------------------------------------------------------------------- */

typedef struct {
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ls1, *ls2; /* fp32 [D] */
  const void *qkv_w, *proj_w, *fc1_w, *fc2_w;             /* [N,K] row-major (torch Linear), bf16 or f32 */
  const float *qkv_b, *proj_b, *fc1_b, *fc2_b;            /* fp32 */
  /* weight_dtype == FP_FP8 only: the four matrices hold OCP e4m3 bytes quantised per output channel, *_s [N] are the
   * dequantisation scales of the output columns, 1 / (act_scale x weight scale of the channel) -- proj_s and fc2_s
   * already multiplied by ls1 / ls2 --, the four biases are divided by (1 / (act_scale x weight scale)), and
   * act_scale[0..3] quantise the inputs of qkv, proj, fc1, fc2 (static per-tensor scales from a calibration batch) */
  const float *qkv_s, *proj_s, *fc1_s, *fc2_s;
  float act_scale[4];
  /* weight_dtype == FP_F16X3 (FP_F16F8: the same with f16f8 rows): the four matrices are split-fp16 rows ([N, 2K] halves) of s_w W with a power-of-two s_w per
   * matrix, and act_scale[0..3] = 1 / (scale of the GEMM's input rows x s_w) for qkv, proj, fc1, fc2: the epilogue computes
   * acc * act_scale + bias.  ls1 / ls2 are applied as usual. */
  /* weight_dtype == FP_F16: the four (folded) matrices may be stored times a power of two s_w each -- fp16 keeps its 11 bits only down to 6e-5, which a
   * LayerScale-folded matrix of small gammas would undershoot -- with act_scale[0..3] = 1 / s_w for qkv, proj, fc1, fc2 (0 = unscaled); colsum is then the
   * row sum of the STORED matrix. */
  /* fp_vit_model.ln_fold only: fp32 [N] sums of the rows of the (gain-folded, bf16-rounded) qkv_w / fc1_w */
  const float *qkv_colsum, *fc1_colsum;
} fp_vit_block;

typedef struct {
  int dim, depth, heads, hidden, registers, patch;
  int ffn_swiglu;          /* 1 for ViT-g: fc1_w/fc1_b hold mlp.w12 with rows INTERLEAVED (x1_j, x2_j) [2*hidden, D],
                              fc2_w/fc2_b hold mlp.w3 [D, hidden]; h = silu(x1) * x2 is fused into the first GEMM */
  int weight_dtype;        /* FP_BF16 | FP_F32 | FP_F16: dtype of the matrices and of the activation buffers (FP_F16 needs ln_fold = 1); FP_FP8: e4m3 block
                              matrices (see fp_vit_block), bf16 activation buffers and patch-embed weight */
  const void* patch_w;     /* [D, patch_k_pad]: conv weight flattened (c,py,px), zero padded */
  int patch_k_pad;         /* multiple of 64 */
  const float* patch_b;    /* [D] */
  const float* pos_patch;  /* [Np, D] pos-embed rows of the patch tokens for the current grid */
  const float* prefix;     /* [1+registers, D]: cls_token + pos[0], then the register tokens */
  const float *norm_w, *norm_b;
  const fp_vit_block* blocks; /* HOST array of `depth` entries */
  int ld_w_dim, ld_w_hidden;  /* row strides (elements) of the block matrices with K = dim (qkv, proj, fc1) and with
                                 K = hidden (fc2); 0 = dense (dim / hidden).  A stride that is not a multiple of 2 KiB
                                 keeps the 8 rows of a staging instruction off one L2 channel */
  int patch_stride;        /* conv stride of the patch embedding; 0 = patch (the shipped configs).  Smaller strides (the reference's
                              patch_vit_resolution, utils/dinov2_utils.py:364-389) give overlapping patches: 1 + (size - patch) / stride
                              tokens per axis, pos_patch then holds the reference's strided position encoding; full forward only */
  float patch_acc_scale;   /* FP_F16X3 only: 1 / (FP_SPLIT_SCALE_ACT x scale of the split patch_w [D, 2 * patch_k_pad]) */
  int ln_fold;             /* FP_BF16 / FP_F16 only.  1: the two LayerNorms of a block are folded into the GEMMs around them -- no
                              LayerNorm kernel runs inside the blocks.  qkv_w / fc1_w then hold W * diag(ln weight) (bf16),
                              qkv_b / fc1_b hold b + W ln_bias, *_colsum the row sums of those matrices; proj_w / fc2_w hold
                              diag(LayerScale) W and proj_b / fc2_b hold LayerScale * b (ls1 / ls2 are then unused); the
                              residual GEMMs (proj, fc2) also emit bf16(x) and per-row (sum x, sum x^2), and the qkv / fc1
                              epilogues compute rstd * (acc - mean * colsum) + bias.  Needs workspace xb / stats / xl. */
} fp_vit_model;

typedef struct {
  void* patches; /* [m_patch_pad, patch_k_pad] activation dtype */
  float* x;      /* [m_pad, D] fp32 residual stream */
  void* y;       /* [m_pad, D] activation dtype (LN output / attention output) */
  void* qkv;     /* [m_pad, 3D] */
  void* h;       /* [m_pad, hidden] */
  void* a8;      /* FP_FP8 only: [m_pad, max(D, hidden)] bytes, the quantised input of the GEMM about to run; m_pad must
                    then be a multiple of 256 */
  int ld_y, ld_h, ld_qkv; /* row strides (elements) of y, h and qkv; 0 = dense (D / hidden / 3D) */
  int m_pad;     /* rows allocated, multiple of 128, >= B*(1+R+Np); a multiple of 1280 (whole 256- AND 320-row tiles) lets the wide bf16 / fp8
                    GEMMs of a large batch take their taller tile (DinoFeatureExtractor.padded_rows) */
  int m_patch_pad; /* multiple of 128, >= B*Np */
  void* xb;      /* ln_fold only: [m_pad, D] bf16 copy of the residual stream (row stride ld_y), the A operand of qkv / fc1 */
  float* stats;  /* ln_fold only: [D / 128 + 1, m_pad, 2] fp32: partial row sums (sum x, sum x^2) per 128-column group of the
                    producer, then one slot of (rstd, mean * rstd) per row */
  int32_t* sat;  /* may be NULL; else [2] STICKY saturation counters, only ever incremented (the caller zeroes and reads them):
                    [0] FP_F16X3: a producer of split-fp16 rows (LayerNorm, the qkv / GELU / SwiGLU epilogues) clamped |s x| > 65504,
                        i.e. an activation beyond +-4094 (LayerNorm outputs, q, k, v) or +-16376 (hidden) -- the near-exact mode's
                        features are then NOT the fp32 arithmetic's; the Python extractor raises FoundPoseSaturationError on it;
                        FP_F16: the last kernel of the pipeline (final norm / sampling) produced a non-finite feature -- an fp16 activation
                        beyond +-65504 somewhere in the backbone (see "plain fp16 rows");
                    [1] FP_FP8: a quantising producer (LayerNorm, attention output, GELU / SwiGLU epilogue) clamped |s x| > 448
                        (an input beyond its static calibration scale).
                    Counted per reporting thread, not per element: non-zero means "at least one live output row clamped".
                    The attention output and the softmax probabilities of the f16x3 mode cannot clamp (a convex combination of v rows
                    that fit their scale; p <= 2) and do not report; padding rows never report. */
  void* xl;      /* ln_fold only (required): [m_pad, D] bf16 (row stride ld_y), the LOW halves of the residual stream.  The blocks in front of
                    the hooked one keep the stream as the pair (xb, xl) -- x = hi + lo, hi' = bf16(x'), lo' = bf16(x' - hi'): 16 mantissa bits per
                    update -- and their residual GEMMs read 4 + write 4 bytes per element instead of 4 + 6 (no fp32 read-modify-write beside a
                    separate bf16 copy); the hooked block runs on an fp32 stream rebuilt from the pair. */
} fp_vit_workspace;

/* images [B,3,H,W] fp32 in [0,1] -> ws->x holds the output of blocks[layer] for every token
 * (what the reference's forward hook captures, dinov2_utils.py:160-211), blocks after `layer` are not run
 * (layer = -1: the token embedding only -- used by the fp8 calibration pass). */
int fp_vit_forward(const fp_vit_model* model, const fp_vit_workspace* ws, const float* images, int B, int H, int W,
                   int layer, fp_stream_t stream);

/* Final LayerNorm on CLS + patch tokens with the register tokens dropped (dinov2_utils.py:138-142,304):
 * fmap [B, Np, D] fp32 token-major (the reference's [B,D,Hp,Wp] is a permuted view of it), cls [B, D].
 * apply_norm = 0 copies the raw tokens. */
int fp_vit_features(const fp_vit_model* model, const fp_vit_workspace* ws, int B, int n_patches, int apply_norm,
                    float* fmap, float* cls, fp_stream_t stream);

/* Final LayerNorm + sample_feature_map_at_points in one pass (SURVEY 8b `fp_ln_gather_pca`, its LayerNorm + gather half;
 * fp_pca_project finishes): out[p, :] = bilinear sample (feature_util.py:100-131) at points[p] (image coordinates, image
 * img_w x img_h, detection point_img[p]) of LayerNorm(tokens) (dinov2_utils.py:138-142; apply_norm = 0: raw tokens),
 * computed from the residual stream fp_vit_forward left in ws->x -- the [B, Np, D] feature map is never written.
 * Bit-identical to fp_vit_features followed by fp_sample_bilinear.  out [num_points, D] fp32. */
int fp_vit_sample_features(const fp_vit_model* model, const fp_vit_workspace* ws, int B, int grid_h, int grid_w, int apply_norm, int img_w,
                           int img_h, const float* points, const int32_t* point_img, int num_points, float* out, fp_stream_t stream);

/* Query-token selection in the hooked block (bf16 model with ln_fold, fp8 model, or f16x3 model).  The reference runs the backbone on every token and
 * then reads the feature map at the query points only (utils/dinov2_utils.py:257,304 -> utils/feature_util.py:100-131 at the
 * points of scripts/infer.py:452-466): the hooked block's OUTPUT is needed for the patch tokens under the sampling taps and
 * for no other token, while its keys and values still come from all tokens.  Three calls replace fp_vit_forward +
 * fp_vit_sample_features with identical sampled features (bit for bit: a token's row never depends on which rows share its
 * GEMM tile or attention block):
 *   fp_vit_forward_prefix   embedding + blocks 0..layer-1 (what block `layer` starts from stays in the workspace).  The workspace
 *                           state between the calls is PRIVATE to them: for a folded-LayerNorm model (the (hi, lo) residual stream) and layer > 0 the
 *                           stream lives in the (ws->xb, ws->xl) pair only and ws->x is UNDEFINED (it still holds the token
 *                           embedding); do not read ws->x after a prefix run -- fp_vit_block_selected rebuilds the rows it needs;
 *   fp_vit_block_selected   block `layer`: LayerNorm constants and the qkv projection for all tokens, then attention
 *                           queries, proj, fc1 and fc2 for the selected tokens only.  sel_rows [num_sel] = global token
 *                           rows (b * n_tok + token), ascending, grouped by image; sel_off [B + 1] = offsets of the images
 *                           in sel_rows; max_sel_per_img >= the largest per-image count (host value: it sizes the grid).
 *                           The selected rows of the residual stream are left compact ([num_sel, D] fp32) in ws->qkv;
 *   fp_vit_sample_features_selected   as fp_vit_sample_features, reading those rows through row_map [B * grid_h * grid_w]:
 *                           patch cell -> its row in the compact buffer, < 0 if the cell was not selected.  Every tap of
 *                           every point must be selected (a missed tap returns NaN features, never a silently wrong row). */
/* Query points of a batch and, optionally, the token selection above -- on the device, two small launches, no host
 * round trip (generate_grid_points + filter_points_by_mask, utils/feature_util.py:19-41, called per detection at
 * scripts/infer.py:359,478).  masks [B, H, W] u8; grid point g = grid_points[g] (x, y) with pixel (pix_x[g], pix_y[g]) =
 * int(point + 0.5); it is a query point of image b iff the pixel lies strictly inside the canvas and on the mask.
 * -> counts [B] points per image (+ [B, 2B) selected tokens per image when point_cells is given: copy them to the host);
 *    out_points [B * num_points, 2] / out_point_img [B * num_points]: the first sum(counts) rows are the query points,
 *    grouped by image, grid order inside (the order of the reference's boolean indexing); out_q_off [B + 1] (may be null).
 * point_cells (may be null) [num_points, 9] i64 = the patch cells the sampling of grid point g may read (the 3 x 3 cells
 * around the cell its sampling position rounds to; num_cells for "outside the map") -> sel_rows [B * num_cells] (first
 * sum(counts[B:]) entries valid), sel_off [B + 1], row_map [B * num_cells] as fp_vit_block_selected /
 * fp_vit_sample_features_selected take them.  scratch: B * (num_points + num_cells) i32. */
int fp_query_select(const uint8_t* masks, int B, int H, int W, const int32_t* pix_x, const int32_t* pix_y, const float* grid_points, int num_points,
                    const int64_t* point_cells, int num_cells, int n_tok, int32_t* scratch, int32_t* counts, float* out_points, int32_t* out_point_img,
                    int32_t* out_q_off, int32_t* sel_rows, int32_t* sel_off, int32_t* row_map, fp_stream_t stream);
int fp_vit_forward_prefix(const fp_vit_model* model, const fp_vit_workspace* ws, const float* images, int B, int H, int W, int layer,
                          fp_stream_t stream);
int fp_vit_block_selected(const fp_vit_model* model, const fp_vit_workspace* ws, int B, int H, int W, int layer, const int32_t* sel_rows,
                          const int32_t* sel_off, int num_sel, int max_sel_per_img, fp_stream_t stream);
int fp_vit_sample_features_selected(const fp_vit_model* model, const fp_vit_workspace* ws, int B, int grid_h, int grid_w, int apply_norm,
                                    int img_w, int img_h, const float* points, const int32_t* point_img, int num_points,
                                    const int32_t* row_map, float* out, fp_stream_t stream);

/* Building blocks, exported for unit tests and for callers that schedule the layers themselves. */
int fp_patchify(const float* images, int B, int H, int W, int patch, void* out, int ld_out, int out_dtype,
                fp_stream_t stream);
int fp_layernorm(const float* x, int ld_x, const float* weight, const float* bias, float eps, void* out, int ld_out,
                 int out_dtype, int dim, int out_rows, int out_rows_per_img, int in_rows_per_img, int in_skip,
                 fp_stream_t stream);
/* epilogue: 0 bias->bf16, 1 bias+gelu->bf16, 3 LayerScale*(.)+residual (fp32 in place), 5 bias->f32,
 * 6 SwiGLU (interleaved column pairs -> [M, N/2] bf16);
 * tuning bits: epilogue | (128 << 8), | (256 << 8), | (320 << 8) or | (352 << 8) forces that block tile (default: chosen from the shape; 320 = the 320 x 256
 * tile of the bias / GELU epilogues, M a multiple of 320; 352 = their 352 x 256 tile, N a multiple of 256 and 0 < M_valid <= M; every tile gives the same
 * bits).  Row tiles without live rows (>= M_valid) are not launched. */
int fp_gemm_bf16(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int M_valid, const float* bias,
                 const float* gamma, void* out, int ldo, int epilogue, fp_stream_t stream);
/* The GEMMs of a block with the LayerNorm folded in (fp_vit_model.ln_fold), exported for unit tests and benchmarks.
 * epilogue 8 (producer on the (hi, lo) stream, fp_vit_workspace.xl): x = xb + out (both bf16 [M, ld_xb]: high and LOW halves), x' = x + acc + bias,
 *   xb = bf16(x'), out = bf16(x' - xb), stats as for epilogue 7.
 * epilogue 7 (producer, proj / fc2 with LayerScale folded into W and bias): out(f32) += acc + bias; if xb != NULL also
 *   xb[M, ld_xb] = bf16(out) and stats[(col / 128) * M + row] = (sum, sum of squares) of the row over that 128-column
 *   group (float2 per slot, N / 128 slots of M rows).
 * epilogues 0 / 1 / 6 (consumer, qkv / fc1 with the LayerNorm gain folded into W, the shift into bias):
 *   out = epi(ln_row[r].x * acc - ln_row[r].y * colsum[n] + bias[n]), ln_row [M, 2] = (rstd, mean * rstd) per row from
 *   fp_ln_finalize, colsum [N] = row sums of W.  Tuning bits as in fp_gemm_bf16. */
int fp_gemm_bf16_ln(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int M_valid, const float* bias, void* out, int ldo,
                    int epilogue, const float* colsum, const float* ln_row, void* xb, int ld_xb, float* stats, fp_stream_t stream);
/* Block-tile height (256 or 352 rows) the launcher gives an epilogue-8 launch of M_valid live rows x N columns that fills a device of num_cus compute units:
 * 352 where it takes fewer rounds of tiles and fewer tile rows per compute unit.  Pure host arithmetic (no device needed); `352 << 8` in the tuning bits of
 * fp_gemm_bf16_ln forces that tile for epilogue 8 (N a multiple of 256, 0 < M_valid <= M; every tile gives the same bits). */
int fp_gemm_resid_tile_rows(int M_valid, int N, int num_cus);
/* ... and the height (256, 320 or 352 rows) it gives an epilogue-0 or -1 launch (plain or folded form, bf16 or fp16 operands) of M padded rows, M_valid of them
 * live, x N columns: the least of rounds of tiles x tile height x a measured factor per height; 320 only where M is a whole number of 256- and 320-row tiles.
 * Pure host arithmetic; degenerate arguments give 256.  (Added without a change of FP_ABI_VERSION: no existing entry point changed.) */
int fp_gemm_wide_tile_rows(int M, int M_valid, int N, int num_cus);
/* stats [parts, stats_stride, 2] partial row sums over `dim` columns in total -> ln_row [rows, 2] = (rstd, mean * rstd). */
int fp_ln_finalize(const float* stats, int parts, int stats_stride, int rows, int dim, float eps, float* ln_row, fp_stream_t stream);

/* fp8 GEMM (BASELINE config 5, "ViT-g/14 fp8"): A [M, K] and W [N, K] hold OCP e4m3 bytes (fp_quantize_fp8), products
 * and accumulation in fp32 on the block-scaled MFMA with unit scales (v_mfma_scale_f32_32x32x64_f8f6f4, twice the bf16
 * rate).  out = epilogue((acc + bias[n]) * col_scale[n]): col_scale = 1 / (activation scale x weight scale of channel
 * n) (x LayerScale gamma for epilogue 3), bias pre-divided by col_scale.  Epilogues 0, 1, 3, 6 as fp_gemm_bf16;
 * M, N multiples of 256, K a multiple of 128.
 * out_scale > 0 (epilogues 1 and 6 only): the result feeds the next fp8 GEMM and is written as e4m3(value * out_scale)
 * bytes, ldo in bytes; out_scale = 0: bf16 / fp32 output as fp_gemm_bf16. */
int fp_gemm_fp8(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int M_valid, const float* bias,
                const float* col_scale, void* out, int ldo, int epilogue, float out_scale, fp_stream_t stream);
/* out[i] = e4m3(clamp(in[i] * scale, +-448)), round to nearest even; in fp32 or bf16 (in_dtype FP_F32 / FP_BF16) */
/* Split-fp16 GEMM (f16x3): A [M, 2K] and W [N, 2K] halves (split rows, scales s_a and s_w), K the LOGICAL depth (multiple of 32),
 * lda / ldw in halves.  v = acc * acc_scale + bias with acc_scale = 1 / (s_a s_w), then the epilogue numbered as for
 * fp_gemm_bf16: 0 (bias), 1 (GELU, the exact erf form here) and 6 (SwiGLU) write a split row again ([M, 2N] -- SwiGLU: [M, N] --
 * halves, values x out_scale, ldo in halves); 3 (out += gamma v) and 5 (bias) write fp32. */
int fp_gemm_split(const void* A, int lda, const void* W, int ldw, int M, int N, int K, int M_valid, const float* bias, const float* gamma,
                  void* out, int ldo, int epilogue, float acc_scale, float out_scale, fp_stream_t stream);
/* Attention on split rows: qkv [B*N, 6D] halves (q | k | v, each 2D, split-fp16 rows of scale in_scale) -> out [B*N, 2D] halves (scale out_scale);
 * out_dtype FP_F16X3: a split-fp16 row, FP_F16F8: an f16f8 row (the f16f8 mode's proj operand); optionally OR-ed with FP_ATTN_VARIANT(v), test bits as in
 * fp_attention: 0 and 1 both run the lock-step kernel; 2 (the role-split kernel, removed after measuring not faster: profiles/EXPERIMENTS.md section 0b)
 * returns FP_ERR_UNSUPPORTED.  in_scale >= 1. */
int fp_attention_split(const void* qkv, int ld_qkv, void* out, int ld_out, int B, int n_tok, int dim, int heads, float in_scale, float out_scale,
                       int out_dtype, fp_stream_t stream);
/* LayerNorm whose output carries a scale: out_dtype FP_FP8 (e4m3(y * out_scale) bytes), FP_F16X3 (split row of y * out_scale) or FP_F16F8 (f16f8 row) */
int fp_layernorm_scaled(const float* x, int ld_x, const float* weight, const float* bias, float eps, void* out, int ld_out, int out_dtype, float out_scale,
                        int dim, int out_rows, fp_stream_t stream);
int fp_quantize_fp8(const void* in, int in_dtype, int64_t n, float scale, void* out, fp_stream_t stream);
/* exact-fp32 MFMA GEMM; epilogue: 0 store, 4 bias, 5 bias+gelu, 6 LayerScale residual, 8 SwiGLU (as above) */
int fp_gemm_f32(const float* A, int lda, const float* W, int ldw, int M, int N, int K, const float* bias,
                const float* gamma, float* out, int ldo, int epilogue, fp_stream_t stream);
/* qkv [B*N, 3D] (q | k | v column blocks, head-major inside) -> out [B*N, D].
 * dtype: FP_F32 / FP_BF16 / FP_F16 (IEEE fp16 q | k | v and output: the "f16" mode's kernel, variant 0 only), optionally OR-ed with FP_ATTN_VARIANT(v) to pick a
 * bf16 work split (bit-identical): 0 = 64 queries per wave, K/V by LDS-DMA (default), 1 = 32 queries per wave with register staging (the cross-check);
 * any other value is FP_ERR_INVALID.
 * FP_F32: 0 = flash attention on the fp32 MFMA (default), 1 = one thread per query with one fma chain per score (its cross-check;
 * the two agree to fp32 rounding, not bit for bit). */
#define FP_ATTN_VARIANT(v) ((v) << 8)
int fp_attention(const void* qkv, int ld_qkv, void* out, int ld_out, int B, int n_tok,
                 int dim, int heads, int dtype, fp_stream_t stream);
int fp_convert_f32_to_bf16(const float* in, void* out, int64_t n, fp_stream_t stream);

/* ---- crop producer (the step right before the path) ---------------------------------------------------
 * Batched misc.warp_image (utils/misc.py:458-519) as scripts/infer.py:433-450 calls it: every destination pixel of a
 * crop camera is mapped through the source camera in fp64 (window_to_eye -> eye_to_world -> world_to_eye ->
 * eye_to_window, points behind the source camera -> -1 when depth_check), cast to fp32 and resampled with cv2.remap
 * semantics (constant border 0).
 *   mode FP_WARP_LINEAR : src fp32 [n_src, src_h, src_w, channels] (HWC, [0,1]) -> out fp32 [batch, channels, out_h,
 *                         out_w] (CHW: array_to_tensor(...).permute(2,0,1), infer.py:466-468); INTER_LINEAR, which is
 *                         also what cv2.remap does for INTER_AREA
 *   mode FP_WARP_NEAREST: src u8 [n_src, src_h, src_w] -> out u8 [batch, out_h, out_w]   (the modal mask)
 * params [batch, 32] doubles per crop: crop camera f[2], c[2], R[9] (row-major rotation of T_world_from_eye), t[3],
 * then the same 16 for the source camera.  src_index [batch] picks the source image of each crop (null: crop b reads
 * image b).  map_out (may be null) receives the fp32 maps [batch, 2, out_h, out_w]. */
enum { FP_WARP_LINEAR = 0, FP_WARP_NEAREST = 1 };
int fp_warp_crops(const void* src, int n_src, int src_h, int src_w, int channels, int mode, const int32_t* src_index,
                  const double* params, int batch, int out_h, int out_w, int depth_check, void* out, float* map_out,
                  fp_stream_t stream);

/* Depth counterpart of fp_warp_crops (utils/misc.py:522-557 warp_depth_image): src fp32 [batch, src_h, src_w] (mm, 0 =
 * background; crop b reads image b), the same params and the same fp32 map, nearest source pixel; where recompute[b] is
 * non-zero (null: every crop) a positive source depth is replaced by the z of the same surface point in the crop camera,
 * computed in fp64 (the reference does this when the two extrinsics are not np.allclose).  out fp32 [batch, out_h, out_w]. */
int fp_warp_depth(const float* src, int src_h, int src_w, const double* params, const int32_t* recompute, int batch,
                  int out_h, int out_w, int depth_check, float* out, fp_stream_t stream);

/* ---- template renderer (scripts/gen_templates.py) ----------------------------------------------
 * One vertex-coloured triangle mesh seen by `batch` pinhole cameras.  Two calls with one host synchronisation between them:
 *   fp_render_setup   transforms and snaps every vertex, builds the triangle records and per-tile counts, scans them.
 *                     status [4] int64 afterwards: [1] flags (bit 0: a window coordinate beyond +-FP_RENDER_MAX_FIXED / 256
 *                     pixels or a NaN; bit 1: a face index outside the vertex range), [2] total tile-list entries,
 *                     [3] the smallest eye-space z of any vertex in any view (fp64 bits; the caller rejects <= 100 mm, the
 *                     reference's near plane -- nothing is clipped).  [0] is internal.
 *   fp_render_raster  fills the tile lists (lists: int32 [status[2]]) and rasterizes: color fp32 [batch, height, width, 3]
 *                     (k / 255), depth fp32 [batch, height, width] (eye-space z, mm, 0 = background), mask u8 (255 / 0),
 *                     tri_id int32 (face index, -1 = background; may be null), boxes int32 [batch, 4] (min x, min y,
 *                     max x, max y of the covered pixels; INT_MAX / INT_MIN when nothing is covered).
 * verts / normals fp32 [num_verts, 3] (mm / unit), colors fp32 [num_verts, 3] in [0, 1], faces int32 [num_faces, 3],
 * cams [batch, 16] doubles: f[2], c[2], R[9] (row-major rotation of T_world_from_eye), t[3] (mm).
 * Caller-owned workspaces: vert_ws batch * num_verts * FP_RENDER_VERT_BYTES, tri_ws batch * num_faces * FP_RENDER_TRI_BYTES,
 * tile_counts int32 [batch * tiles], tile_offsets int64 [batch * tiles + 1], tiles = ceil(width / 32) * ceil(height / 32).
 * Both calls take the same arguments; the outputs are ignored by fp_render_setup and the lists by neither. */
#define FP_RENDER_TILE 32
#define FP_RENDER_VERT_BYTES 40
#define FP_RENDER_TRI_BYTES 144
#define FP_RENDER_MAX_FIXED 536870912.0 /* 2^29: |window coordinate| x 256, keeps every edge function exact in int64 */
#define FP_RENDER_MAX_SIDE 8192
int fp_render_setup(const float* verts, const float* normals, const float* colors, int num_verts, const int32_t* faces,
                    int num_faces, const double* cams, int batch, int width, int height, void* vert_ws, void* tri_ws,
                    int32_t* tile_counts, int64_t* tile_offsets, int32_t* lists, int64_t* status, float* color,
                    float* depth, uint8_t* mask, int32_t* tri_id, int32_t* boxes, fp_stream_t stream);
int fp_render_raster(const float* verts, const float* normals, const float* colors, int num_verts, const int32_t* faces,
                     int num_faces, const double* cams, int batch, int width, int height, void* vert_ws, void* tri_ws,
                     int32_t* tile_counts, int64_t* tile_offsets, int32_t* lists, int64_t* status, float* color,
                     float* depth, uint8_t* mask, int32_t* tri_id, int32_t* boxes, fp_stream_t stream);

/* ---- textured models ("Textured models") ------------------------------------------------------
 * fp_texture_mips  rgb u8 [height, width, 3] (device; row 0 is the top of the image) -> pyramid: packed RGBA8 uint32 texels
 *                  (byte 0 red, 1 green, 2 blue, 3 = 255), every level row-major and the levels back to back.  Level 0 is
 *                  the image; level l + 1 is max(1, w_l >> 1) x max(1, h_l >> 1) and its texel (x, y) is, per channel,
 *                  (sum over i, j in {0, 1} of level_l(min(2x + i, w_l - 1), min(2y + j, h_l - 1)) + 2) >> 2; the levels
 *                  run down to 1 x 1.  Level l starts at texel offset sum_{k < l} w_k h_k; the total is that sum over all
 *                  levels (at most FP_TEXTURE_MAX_LEVELS).  Sides in [1, FP_TEXTURE_MAX_SIDE].
 * fp_render_raster_textured  fp_render_raster (after the same fp_render_setup) for a textured model: coverage, depth, mask,
 *                  tri_id and boxes are fp_render_raster's bit for bit; the colour samples the pyramid at the perspective-
 *                  correct uv (uv fp32 [num_verts, 2], device; v = 1 is row 0 of the image) with trilinear filtering (GL
 *                  LINEAR / LINEAR_MIPMAP_LINEAR, REPEAT wrap, analytic level of detail) and shades it with `material`
 *                  (HOST float[6]: metallic, roughness, base factor r, g, b, sRGB decode flag 0 / 1; every entry in [0, 1]).
 *                  tex_width x tex_height is level 0 of `pyramid`.  The colours argument is not read. */
#define FP_TEXTURE_MAX_SIDE 16384
#define FP_TEXTURE_MAX_LEVELS 15
int fp_texture_mips(const uint8_t* rgb, int width, int height, uint32_t* pyramid, fp_stream_t stream);
int fp_render_raster_textured(const float* verts, const float* normals, const float* colors, int num_verts, const int32_t* faces,
                              int num_faces, const double* cams, int batch, int width, int height, void* vert_ws, void* tri_ws,
                              int32_t* tile_counts, int64_t* tile_offsets, int32_t* lists, int64_t* status, float* color,
                              float* depth, uint8_t* mask, int32_t* tri_id, int32_t* boxes, const float* uv,
                              const uint32_t* pyramid, int tex_width, int tex_height, const float* material, fp_stream_t stream);

/* SSAA downsample by an integer factor (gen_templates.py:373-386 with the output casts of :389-480): color fp32
 * [batch, 3, out_h * factor, out_w * factor] (fp_warp_crops' layout), depth fp32 and mask u8 [batch, out_h * factor,
 * out_w * factor] -> rgb u8 [batch, 3, out_h, out_w] = trunc(255 * block mean), depth_u16 = round-half-even of the block's
 * top-left sample (clamped to [0, 65535]), mask_out = the top-left sample; boxes int32 [batch, 4] (may be null): the box of
 * the non-zero output mask pixels as in fp_render_raster. */
int fp_template_downsample(const float* color, const float* depth, const uint8_t* mask, int batch, int out_h, int out_w,
                           int factor, uint8_t* rgb, uint16_t* depth_u16, uint8_t* mask_out, int32_t* boxes,
                           fp_stream_t stream);

/* ---- pose evaluation (utils/eval_errors.py:12-68) -----------------------------------------------
 * Symmetry-aware BOP pose errors of num_hyp hypotheses, fp64 in and out.  Hypothesis h uses the vertices
 * pts[pt_off .. pt_off + pt_cnt) and the symmetries [sym_off .. sym_off + sym_cnt) given by ranges[h] = (pt_off, pt_cnt,
 * sym_off, sym_cnt) -- HOST memory, int32 [num_hyp, 4]: the call validates every range and copies a derived table into
 * scratch on `stream`, waiting for that copy (and so for the work queued before it) before it returns.  Device arrays:
 *   pts     [total_pts, 3]    model vertices (mm), objects concatenated
 *   est     [num_hyp, 12]     R_est (row-major) | t_est, model -> camera
 *   p_est   [num_hyp, 12]     K [R_est | t_est], row-major 3x4
 *   gt_sym  [total_syms, 12]  R_gt S_R | R_gt S_t + t_gt  (composed by the caller)
 *   p_gt    [total_syms, 12]  K [R_gt_sym | t_gt_sym]
 *   err     [num_hyp, 2]      (mssd, mspd) = min over symmetries of the max over vertices of the 3D / projected distance
 *   idx     [num_hyp, 4]      (mssd vertex, mssd symmetry, mspd vertex, mspd symmetry), relative to the hypothesis' ranges
 * The vertex maximum compares squared distances (one sqrt per symmetry: same value, see csrc/pose_eval.hip); ties go to
 * the lowest vertex / symmetry, NaN as numpy's max / argmax and np.argmin, the value across symmetries as Python's min().
 * Results are bit-identical across runs and batch compositions.  scratch: at least
 * FP_POSE_ERR_SCRATCH_BYTES(num_hyp, max pt_cnt, max sym_cnt) bytes (scratch_bytes says how many there are).
 * num_hyp < 1, a count < 1, a range outside [0, total), a NULL pointer or too little scratch: FP_ERR_INVALID, nothing written. */
#define FP_POSE_ERR_VERTS_PER_LANE 8
#define FP_POSE_ERR_TILE (64 * FP_POSE_ERR_VERTS_PER_LANE)
#define FP_POSE_ERR_SCRATCH_BYTES(num_hyp, max_pts, max_syms) \
  (32 * (((size_t)(num_hyp) + 7) / 8) * 8 + 24 * (size_t)(num_hyp) * (size_t)(max_syms) * (((size_t)(max_pts) + FP_POSE_ERR_TILE - 1) / FP_POSE_ERR_TILE))
int fp_pose_errors(const double* pts, int total_pts, const double* est, const double* p_est, const double* gt_sym, const double* p_gt,
                   int total_syms, const int32_t* ranges, int num_hyp, void* scratch, size_t scratch_bytes, double* err, int32_t* idx,
                   fp_stream_t stream);

/* ---- ADD / ADI (bop_toolkit_lib pose_error.add / adi; DESIGN.md section 22, tests/pose_add_ref.py restates it) -----------
 * The average distance of model points (ADD) and to the closest model point (ADI, "ADD-S") of num_pairs (estimate, GT) pairs,
 * fp64 in and out.  Pair h uses the points pts[pt_off .. pt_off + pt_cnt) given by ranges[h] = (pt_off, pt_cnt) -- HOST memory,
 * int32 [num_pairs, 2]: the call validates every range and copies a derived table into scratch on `stream`, waiting for that
 * copy as fp_pose_errors does.  Device arrays:
 *   pts  [total_pts, 3]   model points (mm), objects concatenated
 *   est  [num_pairs, 12]  R_est (row-major) | t_est, model -> camera
 *   gt   [num_pairs, 12]  R_gt | t_gt
 *   err  [num_pairs, 2]   (add, adi)
 * With E_v = ((r0 x + r1 y) + r2 z) + t per row of the estimate and G_v the same with the GT pose:
 *   add = mean_v sqrt((dx dx + dy dy) + dz dz), d = G_v - E_v
 *   adi = mean_v sqrt(min_u ((dx dx + dy dy) + dz dz)), d = G_v - E_u, u over the pair's whole range (brute force): the minimum
 *         starts at +inf and takes a candidate only when it is strictly smaller (a NaN never wins)
 * every operation rounded on its own (no contraction, correctly rounded sqrt, IEEE division).  The means have one summation
 * order: tiles of FP_POSE_ADD_TILE consecutive points are summed in ascending point order, the tile sums in ascending tile order,
 * and the sum is divided by (double)pt_cnt.  Results are bit-identical across runs, batch compositions and batch orders.
 * scratch: at least FP_POSE_ADD_SCRATCH_BYTES(num_pairs, max pt_cnt) bytes.  num_pairs outside [1, 65535], a pt_cnt < 1, a range
 * outside [0, total_pts], a NULL pointer or too little scratch: FP_ERR_INVALID, nothing written. */
#define FP_POSE_ADD_TILE 256
#define FP_POSE_ADD_BLOCK (4 * FP_POSE_ADD_TILE) /* query points of one workgroup */
#define FP_POSE_ADD_SCRATCH_BYTES(num_pairs, max_pts) \
  (32 * (((size_t)(num_pairs) + 7) / 8) * 8 + 16 * (size_t)(num_pairs) * (((size_t)(max_pts) + FP_POSE_ADD_TILE - 1) / FP_POSE_ADD_TILE))
int fp_pose_add_errors(const double* pts, int total_pts, const double* est, const double* gt, const int32_t* ranges, int num_pairs,
                       void* scratch, size_t scratch_bytes, double* err, fp_stream_t stream);

/* ---- farthest pair and directed Hausdorff distance inside one point set (models_info.py; DESIGN.md section 26,
 * tests/models_info_ref.py restates it) ------------------------------------------------------------------------------------
 * fp64 in and out, brute force, every operation rounded on its own as in the ADD / ADI entry above: a squared distance is
 * (dx dx + dy dy) + dz dz, squared distances are compared and one correctly rounded sqrt follows the reduction.  Results are
 * bit-identical across runs and launch shapes.  Both calls are asynchronous on `stream`.
 *
 * The diameter: pts [V, 3] (device) -> out_d [1] = sqrt(max_{i<j} d2(p_i, p_j)), out_pair int32 [2] = the lexicographically
 * lowest pair (i, j), i < j, that attains it.  The maximum starts at 0 with the pair (0, 0) and a candidate replaces it only
 * when strictly greater: a NaN never wins, and V = 1 (or V coincident points) gives 0.0 and (0, 0).  Work is done for pairs of
 * FP_PTS_TILE-point tiles a <= b only.  1 <= V <= FP_PTS_DIAMETER_MAX_V; scratch: FP_PTS_DIAMETER_SCRATCH_BYTES(V) bytes.
 *
 * The directed Hausdorff distance of K transformed copies: transforms [K, 12] = R row-major | t (device).  For candidate k the
 * queries are the points v = 0, s, 2 s, ... < V (s = query_stride), q_v = ((r0 x + r1 y) + r2 z) + t per row,
 * m_v = min_u d2(q_v, p_u) over ALL V untransformed points (from +inf, strictly smaller only: a NaN never wins),
 * out_h[k] = sqrt(max_v m_v), out_arg[k] = the lowest v that attains the maximum.  1 <= K <= 65535, V >= 1, query_stride >= 1;
 * scratch: FP_PTS_HAUSDORFF_SCRATCH_BYTES(V, query_stride, K) bytes.
 *
 * A NULL pointer, an argument outside its limits or too little scratch: FP_ERR_INVALID, nothing written. */
#define FP_PTS_TILE 1024 /* queries of one workgroup = targets of one LDS tile */
#define FP_PTS_DIAMETER_MAX_V (65535 * FP_PTS_TILE)
#define FP_PTS_TILES(n) (((size_t)(n) + FP_PTS_TILE - 1) / FP_PTS_TILE)
#define FP_PTS_DIAMETER_SCRATCH_BYTES(V) (16 * (FP_PTS_TILES(V) * (FP_PTS_TILES(V) + 1) / 2))
#define FP_PTS_HAUSDORFF_SCRATCH_BYTES(V, query_stride, K) \
  (16 * (size_t)(K) * FP_PTS_TILES(((size_t)(V) + (size_t)(query_stride) - 1) / (size_t)(query_stride)))
int fp_pts_diameter(const double* pts, int V, void* scratch, size_t scratch_bytes, double* out_d, int32_t* out_pair, fp_stream_t stream);
int fp_directed_hausdorff(const double* pts, int V, int query_stride, const double* transforms, int K, void* scratch,
                          size_t scratch_bytes, double* out_h, int32_t* out_arg, fp_stream_t stream);

/* ---- VSD (bop_toolkit_lib pose_error.vsd, `bop19` visibility, `step` cost) ----------------------
 * Counts for the Visible Surface Discrepancy of num_pairs (estimate, GT) pairs.  Device arrays:
 *   depth_test [num_test, height, width]  fp32 mm, 0 = no measurement (the test images)
 *   depth_est  [num_est, height, width]   fp32 mm, 0 = background (renders of the estimates)
 *   depth_gt   [num_gt, height, width]    fp32 mm, 0 = background (renders of the GT instances)
 *   counts     [num_pairs, 2 + num_taus]  int64: |union|, |intersection|, then per tau the intersection pixels with
 *                                         dist >= tau.  The call zeroes it on `stream`.
 * HOST arrays (validated, then copied into scratch on `stream`; the call waits for that copy, as fp_pose_errors does):
 *   pairs  int32 [num_pairs, 7]  (test index, est index, gt index, x0, y0, x1, y1): the inclusive pixel box scanned, the
 *                                union of the two renders' boxes (x1 = x0 - 1 or y1 = y0 - 1: empty).  Every pixel outside it
 *                                must have depth_est = depth_gt = 0.
 *   params fp64 [num_pairs, 6]   (fx, fy, cx, cy, delta mm, diameter mm)
 *   taus   fp64 [num_taus]       1 <= num_taus <= FP_VSD_MAX_TAUS
 * Per pixel, fp64, every operation rounded on its own (no contraction, IEEE division, correctly rounded sqrt):
 *   xs = (col - cx) / fx, ys = (row - cy) / fy  (integer pixel indices); dist = sqrt(((xs d)^2 + (ys d)^2) + d^2) for the
 *   fp32 depth d of each image; visib(m) = ((float)dist_m - (float)dist_test <= (float)delta || dist_test == 0) && dist_m > 0
 *   with the difference in fp32; visib_gt = visib(gt); visib_est = visib(est) || (visib_gt && dist_est > 0); on the
 *   intersection e = |dist_gt - dist_est| / diameter, counted for each tau with e >= tau.
 * The VSD error for tau is (count_tau + (|union| - |inter|)) / |union|, and 1 for every tau when |union| = 0 (host side).
 * Results are bit-identical across runs and batch compositions (integer sums).  scratch: FP_VSD_SCRATCH_BYTES(num_pairs).
 * num_pairs < 1, num_taus outside [1, FP_VSD_MAX_TAUS], a NaN tau or delta, height / width / image counts < 1, an index
 * outside its stack, a box outside the image, fx, fy or diameter not > 0, a NULL pointer or too little scratch:
 * FP_ERR_INVALID, nothing written. */
#define FP_VSD_MAX_TAUS 16
#define FP_VSD_BLOCK_PIXELS 1024
#define FP_VSD_SCRATCH_BYTES(num_pairs) (96 * (size_t)(num_pairs))
int fp_vsd_counts(const float* depth_test, int num_test, const float* depth_est, int num_est, const float* depth_gt, int num_gt,
                  int height, int width, const int32_t* pairs, const double* params, int num_pairs, const double* taus,
                  int num_taus, void* scratch, size_t scratch_bytes, int64_t* counts, fp_stream_t stream);

/* ---- GT annotations from renders (bop_toolkit's calc_gt_info.py / calc_gt_masks.py, `bop19` visibility) ----
 * Pixel counts, boxes and masks of num_inst ground-truth instances.  Device arrays:
 *   depth_test [num_test, height, width]              fp32 mm, 0 = no measurement (the frames' depth images)
 *   depth_obj  [num_inst, render_height, render_width] fp32 mm, 0 = background: instance p rendered alone into a window that holds
 *                                                     the image at columns [ox, ox + width), rows [oy, oy + height)
 *   out        [num_inst, 11] int32: px_count_all, px_count_valid, px_count_visib, the silhouette box (min x, min y, max x, max y)
 *              and the visible box in the same form, both in IMAGE coordinates (render coordinate - offset: the silhouette box can
 *              be negative or reach past the image); an empty box is INT_MAX, INT_MAX, INT_MIN, INT_MIN
 *   mask, mask_visib [num_inst, height, width] uint8, 255 / 0
 * The call defines every byte of the three outputs: it zeroes the two mask stacks with a memset on `stream`, initialises `out` and
 * then writes the masks inside the scan boxes.
 * HOST arrays (validated, then copied into scratch on `stream`; the call waits for that copy, as the VSD entry does):
 *   inst   int32 [num_inst, 7]  (test index, x0, y0, x1, y1, ox, oy): the inclusive box scanned, in render coordinates (x1 = x0 - 1 or
 *                               y1 = y0 - 1: empty); every pixel outside it must have depth_obj = 0.  (ox, oy): the image's offset.
 *   params fp64 [num_inst, 5]   (fx, fy, cx, cy, delta mm) of the IMAGE (not of the shifted render camera)
 * Per box pixel: depth_obj > 0 counts into px_count_all and extends the silhouette box.  Inside the image window, with (col, row) the
 * image coordinates, fp64, every operation rounded on its own: xs = (col - cx) / fx, ys = (row - cy) / fy, dist = sqrt(((xs d)^2 +
 * (ys d)^2) + d^2); mask = dist_obj > 0; px_count_valid counts mask && dist_test > 0; visib = ((float)dist_obj - (float)dist_test <=
 * (float)delta || dist_test == 0) && dist_obj > 0 with the difference in fp32, counted into px_count_visib, extending the visible box.
 * Integer sums and extremes: bit-identical across runs, batch compositions and launch shapes.  scratch: FP_GT_VIS_SCRATCH_BYTES(num_inst).
 * A NULL pointer, num_inst < 1 or > FP_GT_VIS_MAX_INST, sizes < 1, render_width * render_height > 2^31 - 1, a test index outside the
 * stack, a box outside the render, a window outside the render, fx or fy not > 0, a NaN delta or too little scratch: FP_ERR_INVALID,
 * nothing written.  (Added without a change of FP_ABI_VERSION: no existing entry point changed.) */
#define FP_GT_VIS_BLOCK_PIXELS 1024
#define FP_GT_VIS_MAX_INST (1 << 24)
#define FP_GT_VIS_SCRATCH_BYTES(num_inst) (80 * (size_t)(num_inst))
int fp_gt_visibility(const float* depth_test, int num_test, int height, int width, const float* depth_obj, int render_height,
                     int render_width, const int32_t* inst, const double* params, int num_inst, void* scratch, size_t scratch_bytes,
                     int32_t* out, uint8_t* mask, uint8_t* mask_visib, fp_stream_t stream);

/* ---- mask proposals from depth: plane removal and connected components (tests/depth_proposals_ref.py restates
 *      it) ----
 * Four entry points, called in this order per batch of num_frames frames of one size.  Shared conventions:
 *   depth   fp32 [num_frames, height, width] on the device, mm, 0 = no measurement.  A pixel is VALID when depth > 0 and
 *           (max_depth_mm == 0 or depth <= max_depth_mm, compared in fp64).  Its point is ((u - cx) / fx z, (v - cy) / fy z, z) with
 *           integer pixel centres, in fp64, every operation rounded on its own; the height over a plane (n, d) is ((n0 x + n1 y) +
 *           n2 z) + d.
 *   cameras fp64 [num_frames, 4] (fx, fy, cx, cy): a HOST array, validated (fx, fy > 0, everything finite), then copied into scratch on
 *           `stream`; the call waits for that copy, as fp_gt_visibility does.
 *   planes  fp64 [num_frames, FP_DEPTH_MAX_PLANES, 4] rows (n0, n1, n2, d) on the device, with an int32 [num_frames] count beside it.
 * height * width <= 2^31 - 1 and num_frames <= FP_DEPTH_MAX_FRAMES.  Integer results (labels, counts, tables, events) and the planes
 * (fp64 sums in a fixed order, no float atomics) are bit-identical across runs and batch compositions: a frame gives the same result
 * alone and inside a batch.  Every byte of every output is defined by the call.  A NULL pointer (unless stated), a size or option
 * outside its range, a bad camera or too little scratch: FP_ERR_INVALID, nothing written.  (Added without a change of FP_ABI_VERSION:
 * no existing entry point changed.)
 *
 * fp_depth_plane_fit: one more plane per frame.  frame_keys: HOST uint64 [num_frames].  prior_planes / num_prior: the frame's earlier
 * planes; num_prior[f] = k in [0, FP_DEPTH_MAX_PLANES) makes this plane k of the frame, any other value skips the frame (info[6] = -1,
 * zeros elsewhere).  A valid pixel is ELIGIBLE when it is not within plane_thresh_mm (|height| <= threshold) of a prior plane.
 * Hypothesis h in [0, hypotheses) draws three distinct eligible pixels (linear index y * width + x below height * width) with the keyed
 * sampler of fp_pnp_ransac_keyed (pair key frame_key * 8 + k, at most 65 attempts per index; a draw that gives up is a dead hypothesis);
 * n = (X1 - X0) x (X2 - X0), dead when |n|^2 <= 1e-12 |X1 - X0|^2 |X2 - X0|^2 or the normalisation fails; d = -n . X0, both negated
 * when d < 0.  Its count: the eligible pixels with y % stride == 0 and x % stride == 0 and |height| <= plane_thresh_mm (0 when dead).
 * The winner is the first hypothesis of the highest count; it is refitted twice by least squares over ALL eligible pixels within the
 * threshold of the current plane (centroid, then the 3 x 3 scatter about it; per-workgroup partials of FP_DEPTH_PLANE_CHUNK pixels
 * folded in ascending order; the normal is the eigenvector of the smallest eigenvalue by cyclic Jacobi, re-oriented to d >= 0; a refit
 * with fewer than 3 pixels keeps the plane).  The support is the number of eligible pixels within the threshold of the final plane;
 * the plane is accepted when the winner is alive, support >= 3 and (double)support >= min_plane_share * (double)valid.
 *   plane_out  fp64 [num_frames, 4]   (n, d), zeros when the winner is dead or the frame is skipped
 *   info       int32 [num_frames, 8]  winner (-1: skipped), its sub-grid count, support, eligible pixels, valid pixels, accepted,
 *                                     plane index k (-1: skipped), 0
 *   hyp_counts int32 [num_frames, hypotheses] or NULL: the counts of all hypotheses
 * hypotheses in [1, FP_DEPTH_MAX_HYPOTHESES], stride in [1, 64], plane_thresh_mm > 0, max_depth_mm >= 0, min_plane_share in [0, 1].
 * scratch: FP_DEPTH_PLANE_SCRATCH_BYTES(num_frames, height * width, hypotheses).
 *
 * fp_depth_components: foreground and components of one level.  planes / num_planes: the frame's accepted planes (num_planes is
 * clamped to [0, FP_DEPTH_MAX_PLANES]).  A valid pixel is FOREGROUND when height > object_margin_mm over every one of them.  Two
 * 4-neighbours are connected when both are foreground and |za - zb| <= connect_mm + slope_fx[f] * min(za, zb) in fp32, each operation
 * rounded on its own (slope_fx: HOST fp32 [num_frames], connect_slope / fx, finite and >= 0).  labels int32 [num_frames, height,
 * width]: the smallest linear index y * width + x of the pixel's component, -1 for background.
 * scratch: FP_DEPTH_COMPONENTS_SCRATCH_BYTES(num_frames, height * width).
 *
 * fp_component_table: a level's components -> the kept ones.  A component is a candidate when min_pixels <= area <= max_area and no row
 * of the frame in `finer` (int32 [num_finer, num_frames, max_proposals, 7], tables this entry wrote for finer levels; NULL with
 * num_finer = 0) has its (label, area).  Candidates are ranked by area descending, then label ascending; at most max_proposals are kept.
 *   table    int32 [num_frames, max_proposals, 7]  (label, area, x0, y0, x1, y1, level) per rank (the box inclusive); unused rows
 *                                                  (-1, 0, 0, 0, 0, 0, 0)
 *   counts   int32 [num_frames, 4]                 components, those within the area limits, kept, dropped as a finer level's
 *   rank_map int32 [num_frames, height, width]     the rank of the pixel's component, -1: none
 * min_pixels >= 1, max_area >= min_pixels, max_proposals in [1, FP_DEPTH_MAX_PROPOSALS], level and num_finer in [0, 2].
 * scratch: FP_COMPONENT_TABLE_SCRATCH_BYTES(num_frames, height * width).
 *
 * fp_component_runs: the run-length events of num_maps rank maps (any stack of fp_component_table's, e.g. frames x levels).  In the
 * column-major scan of map m (position p = x * height + y) rank r(p) differs from r(p - 1) exactly where a run of r(p) starts and a
 * run of r(p - 1) ends; every rank below num_kept[m] (clamped to [0, max_proposals]; ranks at or above it count as -1) also gets the
 * terminal position height * width once.  Each event is the int64 ((m * max_proposals + rank) << 32) | position.  Sorted ascending, the
 * positions of one (m, rank), differenced from 0, are COCO's uncompressed counts: runs alternate 0 / 1 from a run of 0 that may be
 * empty, continue across column ends and add up to height * width.
 *   num_events int32 [1]         the number of events, whatever the capacity
 *   events     int64 [capacity]  the events in no particular order, the rest filled with 0x7f7f7f7f7f7f7f7f (sorts last); may be NULL
 *                                with capacity 0 (a counting call)
 * num_maps <= 65535 and num_maps * (height * width + 1 + max_proposals) <= 2^30; capacity >= 0. */
#define FP_DEPTH_MAX_FRAMES 4096
#define FP_DEPTH_MAX_PLANES 4
#define FP_DEPTH_MAX_HYPOTHESES 4096
#define FP_DEPTH_MAX_PROPOSALS 1024
#define FP_DEPTH_PLANE_CHUNK 4096
#define FP_DEPTH_PLANE_SCRATCH_BYTES(num_frames, pixels, hypotheses)                                                        \
  (256 * (size_t)(num_frames) + 16 * (((size_t)(num_frames) * (size_t)(pixels) + 15) / 16) +                                \
   8 * (((size_t)(num_frames) * (size_t)(hypotheses) + 1) / 2) +                                                            \
   64 * (size_t)(num_frames) * (((size_t)(pixels) + FP_DEPTH_PLANE_CHUNK - 1) / FP_DEPTH_PLANE_CHUNK))
#define FP_DEPTH_COMPONENTS_SCRATCH_BYTES(num_frames, pixels) (64 * (size_t)(num_frames) + 4 * (size_t)(num_frames) * (size_t)(pixels))
#define FP_COMPONENT_TABLE_SCRATCH_BYTES(num_frames, pixels) (16 * (size_t)(num_frames) + 28 * (size_t)(num_frames) * (size_t)(pixels))
int fp_depth_plane_fit(const float* depth, int num_frames, int height, int width, const double* cameras, const uint64_t* frame_keys,
                       const double* prior_planes, const int32_t* num_prior, int hypotheses, int stride, double plane_thresh_mm,
                       double max_depth_mm, double min_plane_share, uint64_t seed, void* scratch, size_t scratch_bytes,
                       double* plane_out, int32_t* info, int32_t* hyp_counts, fp_stream_t stream);
int fp_depth_components(const float* depth, int num_frames, int height, int width, const double* cameras, const float* slope_fx,
                        const double* planes, const int32_t* num_planes, double max_depth_mm, double object_margin_mm, float connect_mm,
                        void* scratch, size_t scratch_bytes, int32_t* labels, fp_stream_t stream);
int fp_component_table(const int32_t* labels, int num_frames, int height, int width, int min_pixels, int max_area, int max_proposals,
                       int level, const int32_t* finer, int num_finer, void* scratch, size_t scratch_bytes, int32_t* table,
                       int32_t* counts, int32_t* rank_map, fp_stream_t stream);
int fp_component_runs(const int32_t* rank_map, int num_maps, int height, int width, const int32_t* num_kept, int max_proposals,
                      int64_t capacity, int64_t* events, int32_t* num_events, fp_stream_t stream);

/* ---- TSDF fusion of posed RGB-D frames and surface extraction (reconstruct.py; tests/tsdf_ref.py restates
 *      both stages) ----
 * The volume is a box in the model frame, mm: `box` = HOST fp64 [4] (origin x, y, z, voxel size h), nx x ny x nz voxels, x fastest,
 * voxel (i, j, k) centred at origin + ((i, j, k) + 0.5) h.  1 <= each dimension <= FP_TSDF_MAX_DIM (>= 2 for the two extraction
 * entries) and nx ny nz <= FP_TSDF_MAX_VOXELS.  Its state is six device planes of nx ny nz entries each: sdf_sum fp32, sdf_cnt int32,
 * rgb_sum fp32 [3, nz, ny, nx] (three planes: r, g, b), rgb_cnt int32; a new volume is all zeros.  Sums and counts, never running
 * means: the state after frames 1 .. F is bit-identical however the frames are split into calls.
 *
 * fp_tsdf_integrate adds num_frames frames, in ascending order, to the state.  Device arrays: depth fp32 [F, height, width] mm (a value
 * that is not > 0 is no measurement), mask uint8 [F, height, width], rgb uint8 [F, height, width, 3].  HOST array: frames fp64
 * [F, FP_TSDF_FRAME_DOUBLES] rows (fx, fy, cx, cy, R row-major, t), the model -> camera pose; it is validated (everything finite, fx and
 * fy > 0), then copied into scratch on `stream`, and the call waits for that copy as fp_gt_visibility does.  Per voxel centre X and
 * frame, fp64, every operation rounded on its own:
 *   x, y, z = ((r0 X + r1 Y) + r2 Z) + t per row of R; the frame is skipped unless z > 1
 *   u = (fx x) / z + cx, v = (fy y) / z + cy (pixel centres at integers); the tap is (floor(u + 0.5), floor(v + 0.5)), and the frame is
 *   skipped when it lies outside the image (no tap outside the image is read) or its depth d is no measurement
 *   mask == 0: when d >= z, sdf_sum += 1 and sdf_cnt += 1 (seen through: empty space); otherwise nothing (hidden)
 *   mask != 0: s = d - z; nothing when s < -trunc_mm; otherwise sdf_sum += (float)min(1, s / trunc_mm), sdf_cnt += 1, and when also
 *   |s| <= trunc_mm, rgb_sum += (float)rgb / 255.0f per channel (fp32 division) and rgb_cnt += 1.  The fp32 sums add in frame order.
 * One thread per voxel, no atomics, no reduction across threads.  1 <= F <= FP_TSDF_MAX_FRAMES, height * width <= 2^31 - 1,
 * trunc_mm finite and > 0; scratch: FP_TSDF_SCRATCH_BYTES(F).
 *
 * Extraction is marching tetrahedra on the cells between voxel centres ((nx - 1)(ny - 1)(nz - 1) of them, x fastest).  A cell's
 * corners are numbered by bits (x = bit 0, y = bit 1, z = bit 2) and it is cut into the six tetrahedra (0, a, b, 7), (a, b) =
 * (1,3), (3,2), (2,6), (6,4), (4,5), (5,1), the same way in every cell, so neighbouring cells agree on every shared face.  A cell takes
 * part only when all eight corners have sdf_cnt >= min_count (>= 1).  A corner's value is f = (double)sdf_sum / (double)sdf_cnt; it is
 * inside when f < 0 (an exact 0 is outside).  A tetrahedron with 1 or 3 corners inside gives one triangle, with 2 inside two.
 * fp_tsdf_count_triangles writes counts int32 [cells], the triangles per cell.
 * fp_tsdf_emit_triangles takes offsets int64 [cells] (device), the exclusive scan of those counts, and num_triangles, their sum, and
 * writes per triangle corner keys int64 [3 T], positions fp32 [3 T, 3] and colors fp32 [3 T, 3]; a cell whose offset would leave
 * [0, num_triangles) writes nothing.  Every vertex lies on an edge of the split, which joins a lower corner to one with more bits set:
 *   key      = (linear voxel index of the lower corner) * 7 + direction, the direction indexing the corner offsets (1,0,0), (0,1,0),
 *              (0,0,1), (1,1,0), (0,1,1), (1,0,1), (1,1,1)
 *   position = (float)(p_lo + w (p_hi - p_lo)) per axis, w = f_lo / (f_lo - f_hi), fp64 from the lower corner: the same bits from
 *              whichever tetrahedron or cell reaches the edge
 *   color    = (float)(c_lo + w (c_hi - c_lo)), c = (double)rgb_sum / (double)rgb_cnt; a corner with rgb_cnt = 0 has no colour: the
 *              other corner's is used, or 0.5 when neither has one
 * The winding makes the face normal point from inside to outside, towards rising f.
 * A NULL pointer, a size or option outside its range or too little scratch: FP_ERR_INVALID, nothing written.  (Added without a
 * change of FP_ABI_VERSION: no existing entry point changed.) */
#define FP_TSDF_MAX_DIM 512
#define FP_TSDF_MAX_VOXELS (1ll << 27)
#define FP_TSDF_MAX_FRAMES 4096
#define FP_TSDF_MAX_TRIANGLES (12 * FP_TSDF_MAX_VOXELS)
#define FP_TSDF_FRAME_DOUBLES 16
#define FP_TSDF_SCRATCH_BYTES(num_frames) (8 * FP_TSDF_FRAME_DOUBLES * (size_t)(num_frames))
int fp_tsdf_integrate(const float* depth, const uint8_t* mask, const uint8_t* rgb, int num_frames, int height, int width,
                      const double* frames, const double* box, int nx, int ny, int nz, double trunc_mm, void* scratch,
                      size_t scratch_bytes, float* sdf_sum, int32_t* sdf_cnt, float* rgb_sum, int32_t* rgb_cnt, fp_stream_t stream);
int fp_tsdf_count_triangles(const float* sdf_sum, const int32_t* sdf_cnt, int nx, int ny, int nz, int min_count, int32_t* counts,
                            fp_stream_t stream);
int fp_tsdf_emit_triangles(const float* sdf_sum, const int32_t* sdf_cnt, const float* rgb_sum, const int32_t* rgb_cnt, const double* box,
                           int nx, int ny, int nz, int min_count, const int64_t* offsets, int64_t num_triangles, int64_t* keys,
                           float* positions, float* colors, fp_stream_t stream);

/* ---- diffusion over a TSDF volume's grid: the smoother of hole filling (reconstruct.py, fill "carve"; DESIGN.md section 34;
 *      tests/tsdf_fill_ref.py restates it) ----
 * Device arrays: val fp32 [channels, nz, ny, nx] (x fastest, channels 1 or 3), state uint8 [nz, ny, nx] with 0 UNKNOWN, 1 FIXED, 2 FREE
 * (any other value is the caller's error: the wrapper refuses it; the kernel reads it as FREE).  Dimensions 1 .. FP_TSDF_MAX_DIM each and
 * nx ny nz <= FP_TSDF_MAX_VOXELS.  fp_tsdf_diffuse runs `iters` (0 .. FP_TSDF_DIFFUSE_MAX_ITERS; 0 touches nothing) Jacobi iterations,
 * each reading only the iteration before it, and leaves the result in val / state; val_tmp / state_tmp are scratch of the same sizes,
 * distinct from them, and hold nothing the caller may rely on afterwards.  One iteration, per voxel:
 *   a FIXED voxel keeps its value and its state;
 *   any other voxel visits, in the order centre, -x, +x, -y, +y, -z, +z, those of the seven that lie inside the volume and are not
 *   UNKNOWN.  n is their number, the same for every channel; per channel acc starts at +0.0f and adds their values in that order in
 *   fp32.  n = 0: the voxel stays (or becomes) UNKNOWN and its value +0.0f.  Otherwise its value is acc / (float)n (IEEE division) and
 *   its state FREE.
 * The value stored in an UNKNOWN voxel is never an operand: it is selected away, not multiplied by a mask, so a NaN there does not
 * spread.  Every output is a pure function of the previous iteration's seven voxels, so the bits are the same for any tiling, vector
 * width or split of T iterations into calls.  A NULL pointer, aliased scratch or a size outside its range: FP_ERR_INVALID, nothing
 * written.  (Added without a change of FP_ABI_VERSION: no existing entry point changed.) */
#define FP_TSDF_DIFFUSE_MAX_ITERS 4096
int fp_tsdf_diffuse(float* val, uint8_t* state, float* val_tmp, uint8_t* state_tmp, int channels, int nx, int ny, int nz, int iters,
                    fp_stream_t stream);

/* ---- mesh simplification: vertex clustering with quadric error positions (simplify.py; tests/simplify_ref.py
 *      restates both kernels) ----
 * The grid: `grid` = HOST fp64 [4] (origin x, y, z, cell size c), all finite and c > 0, and nx x ny x nz cells, x fastest,
 * 1 <= each dimension <= FP_MESH_MAX_DIM.  vertices fp32 [V, 3] on the device, 0 <= V <= FP_MESH_MAX_ROWS.
 *
 * fp_mesh_cell_keys writes keys int64 [V], one thread per vertex.  Per axis, fp64, every operation rounded on its own:
 *   g = ((double)x - o) / c;  i = floor(g) clamped to [0, n - 1] (a NaN gives 0: no key leaves the grid);  key = (k ny + j) nx + i.
 * (Added without a change of FP_ABI_VERSION: no existing entry point changed.)
 *
 * fp_mesh_cluster places one vertex per occupied cell, one wave per cell.  Device arrays besides vertices: colors fp32 [V, 3], faces
 * int32 [F, 3] (0 <= 3 F <= FP_MESH_MAX_ROWS; may be NULL when F = 0), and the tables of the C occupied cells (1 <= C <= V), all int64:
 *   cell_keys    [C]      the cells' keys, as fp_mesh_cell_keys writes them (ascending in simplify.py; the kernel needs no order)
 *   vert_order   [V]      vertex ids grouped by cell;  vert_begin [C + 1]: cell c owns vert_order[vert_begin[c] .. vert_begin[c + 1])
 *   corner_order [3 F]    corner ids 3 f + k grouped by the cell of the corner's vertex;  corner_begin [C + 1] likewise
 * A range is clamped to its array and an id or a face index outside its array contributes nothing: nothing outside the arrays is read.
 * All in fp64, every operation rounded on its own, square roots IEEE.  A corner record 3 f + k adds its face's plane quadric, the face's
 * vertices p0, p1, p2 always in the face's own order (never rotated by k, so a face adds the same bits to every cell it touches):
 *   m = (p1 - p0) x (p2 - p0), L = sqrt(m . m); nothing is added unless L > 0;  n = m / L, w = L / 2, d = -((n0 p0x + n1 p0y) + n2 p0z)
 *   the ten terms, in output order: (w na) nb for ab = 00, 01, 02, 11, 12, 22;  (w na) d for a = 0, 1, 2;  (w d) d
 * A face with two or three corners in a cell adds that many times (Garland's per-vertex rule).  Order of every sum: lane l of the wave
 * starts from 0.0 and adds the cell's records begin + l, begin + l + 64, ... in ascending order; the 64 lanes are then combined by the
 * xor butterfly at distances 32, 16, ..., 1.  Vertex records are summed the same way, positions and colours widened to fp64.  Then:
 *   mean = sum p / count;  colour = (float)(sum colour / count)
 *   A (the six terms) is decomposed by cyclic Jacobi, pairs (0,1), (0,2), (1,2), at most 30 sweeps, stopping when the squared
 *   off-diagonal mass is not > 1e-30 of the whole; eigenvalue j is kept when lmax > 0 and l_j > eig_eps lmax
 *   x = mean + sum over kept j = 0, 1, 2 in order of u_j (u_j . g) / l_j, g = -(b + A mean)
 *   with lo = o + index c per axis: x is accepted when it is finite and lo - c / 2 <= x <= lo + 3 c / 2 on every axis; otherwise
 *   x = mean and the status is -1.  A cell without a non-degenerate face (or F = 0) has lmax = 0 and gets its mean, status 0.
 * Outputs per cell: positions fp32 [C, 3], out_colors fp32 [C, 3], quadrics fp64 [C, 10] (the ten sums), means fp64 [C, 3], err fp64 [C]
 * = x'Ax + 2 b'x + s at the fp64 x (reported, never a criterion), status int32 [C]: the number of kept eigenvalues, or -1.
 * No atomics; a cell's outputs depend on its own records only, so they are the same bits whatever else is in the call.
 * eig_eps finite and in [0, 1).  A NULL pointer or a size or option outside its range: FP_ERR_INVALID, nothing written.  (Added without
 * a change of FP_ABI_VERSION: no existing entry point changed.) */
#define FP_MESH_MAX_DIM (1 << 20)
#define FP_MESH_MAX_ROWS 0x7fffffffll
int fp_mesh_cell_keys(const float* vertices, int64_t num_vertices, const double* grid, int nx, int ny, int nz, int64_t* keys,
                      fp_stream_t stream);
int fp_mesh_cluster(const float* vertices, const float* colors, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                    const int64_t* cell_keys, int64_t num_cells, const int64_t* vert_order, const int64_t* vert_begin,
                    const int64_t* corner_order, const int64_t* corner_begin, const double* grid, int nx, int ny, int nz, double eig_eps,
                    float* positions, float* out_colors, double* quadrics, double* means, double* err, int32_t* status,
                    fp_stream_t stream);

/* ---- featuremetric refinement of the best coarse pose (tests/featuremetric_ref.py restates it) ----
 * Levenberg-Marquardt on the 6-DoF pose of each of num_det detections, aligning a template's per-point features with the
 * query's projected patch-feature map.  Device arrays:
 *   map        fp32 [num_det, gh, gw, C] at element strides (sb, sy, sx, sc): the projected query feature map (gh, gw >= 2)
 *   cameras    fp64 [num_det, 4]  (fx, fy, cx, cy) of the camera the pose lives in; W x H its image size (map x_m = u gw / W - 1/2)
 *   R_in, t_in fp64 [num_det, 9], [num_det, 3]  the input pose, model -> camera (mm)
 *   row_begin, row_end int32 [num_det]  the template's rows [row_begin, row_end) of feats [num_rows, C] fp32 and vertices
 *              [num_rows, 3] fp32; at most max_points rows.  A range outside [0, num_rows] or longer than max_points is never read:
 *              the call then returns FP_ERR_INVALID naming the detection (it waits for the work queued on `stream` to learn this)
 *   has_pose   int32 [num_det]  0: skipped (status 2)
 * Outputs: R_out [num_det, 9], t_out [num_det, 3], cost_in, cost_out fp64 [num_det], num_points (valid points), iters_used and
 * status int32 [num_det] (0 refined, 1 no step accepted, 2 skipped: no pose, empty range or < 6 valid points; for 1 and 2 the
 * pose is the input bit for bit); normal_eq fp64 [num_det, 28] may be null: H (upper triangle, row-major), g, E at the input pose.
 * Valid set frozen at the input pose (z > 1 mm, inside the map), Cauchy loss with sigma^2 = mean squared residual there,
 * lambda from 1e-3, at most `iters` (0..1000) iterations; all of them are enqueued at once.  Deterministic and bit-identical
 * across batch compositions; no float atomics.  scratch: FP_REFINE_SCRATCH_BYTES(num_det, max_points). */
#define FP_REFINE_CHUNK 32
#define FP_REFINE_RECORD 32
#define FP_REFINE_STATE_BYTES 512
#define FP_REFINE_SCRATCH_BYTES(num_det, max_points)                                                                   \
  ((size_t)FP_REFINE_STATE_BYTES * (size_t)(num_det) +                                                                  \
   8 * FP_REFINE_RECORD * (size_t)(num_det) * (((size_t)(max_points) + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK) +       \
   (((size_t)(num_det) * (size_t)(max_points) + 7) / 8) * 8 + 8)
int fp_featuremetric_refine(const float* map, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int gh, int gw, int C, int W, int H,
                            const double* cameras, const double* R_in, const double* t_in, const int32_t* row_begin,
                            const int32_t* row_end, const float* feats, const float* vertices, int64_t num_rows,
                            const int32_t* has_pose, int num_det, int max_points, int iters, void* scratch, size_t scratch_bytes,
                            double* R_out, double* t_out, double* cost_in, double* cost_out, int32_t* num_points,
                            int32_t* iters_used, int32_t* status, double* normal_eq, fp_stream_t stream);

/* ---- depth refinement of the final pose (tests/depth_refine_ref.py restates it) ----------------------------
 * Levenberg-Marquardt on the 6-DoF pose of each of num_det detections against the frame's measured depth, in the frame's own
 * camera (never a crop camera; the depth is not warped or resampled).  Device arrays:
 *   depth       fp32 [num_images, H, W] mm, 0 = no measurement (H, W >= 2); image_index int32 [num_det]: the image a detection reads.
 *               An index outside [0, num_images) is never used: the call then returns FP_ERR_INVALID naming the detection
 *   cameras     fp64 [num_det, 4]  (fx, fy, cx, cy) of the frame's camera; pixel centres lie at integer coordinates
 *   R_in, t_in  fp64 [num_det, 9], [num_det, 3]  the input pose, model -> camera (mm)
 *   row_begin, row_end int32 [num_det]  the template's rows [row_begin, row_end) of vertices [num_rows, 3] fp32, at most max_points
 *               rows; a bad range is reported like a bad image index, and the rows are never read
 *   has_pose    int32 [num_det]  0: skipped (status 2);  tau fp64 [num_det]: the truncation distance (mm).  tau is not validated: a NaN
 *               or a value <= 0 leaves no inlier, so that detection is skipped (status 2) with its pose untouched
 * Per point: Xc = R X + t, (u, v) its projection, d the bilinear depth at (u, v) from the taps (x0, y0) = floor(u, v) and their +1
 * neighbours, r = d - z.  Measurable: z > 1 mm, the four taps inside the image and > 0.  rho = r^2 for an inlier (measurable, |r| < tau),
 * tau^2 otherwise (no gradient); cost = sum rho / (row_end - row_begin); H, g over the inliers.  The LM loop, lambda schedule and
 * stopping rules are fp_featuremetric_refine's, at most `iters` (0..1000) iterations, all enqueued at once.
 * Outputs: R_out, t_out, cost_in, cost_out, num_points (inliers at the input pose), iters_used, status (0 refined, 1 no step
 * accepted, 2 skipped: no pose, empty range or < 6 inliers at the input pose; for 1 and 2 the pose is the input bit for bit);
 * normal_eq fp64 [num_det, 28] may be null: H (upper triangle, row-major), g, cost at the input pose.  cost_out <= cost_in always.
 * Deterministic and bit-identical across batch compositions; no float atomics.  scratch: FP_DEPTH_REFINE_SCRATCH_BYTES. */
#define FP_DEPTH_REFINE_SCRATCH_BYTES(num_det, max_points)                                                             \
  ((size_t)FP_REFINE_STATE_BYTES * (size_t)(num_det) +                                                                  \
   8 * FP_REFINE_RECORD * (size_t)(num_det) * (((size_t)(max_points) + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK) + 8)
int fp_depth_refine(const float* depth, int num_images, int H, int W, const int32_t* image_index, const double* cameras,
                    const double* R_in, const double* t_in, const int32_t* row_begin, const int32_t* row_end, const float* vertices,
                    int64_t num_rows, const int32_t* has_pose, const double* tau, int num_det, int max_points, int iters,
                    void* scratch, size_t scratch_bytes, double* R_out, double* t_out, double* cost_in, double* cost_out,
                    int32_t* num_points, int32_t* iters_used, int32_t* status, double* normal_eq, fp_stream_t stream);

/* ---- frame-to-model tracking against a TSDF volume (reconstruct.py, pose_source "track"; DESIGN.md section 30;
 *      tests/tsdf_track_ref.py restates it) ----
 * Levenberg-Marquardt on the model -> camera pose of each of num_det independent problems against ONE volume of fp_tsdf_integrate:
 * sdf_sum, sdf_cnt, box (HOST fp64 [4]) and nx, ny, nz as there, every dimension >= 2 as for extraction; min_count >= 1; trunc_mm the
 * truncation distance tau the volume was built with, finite and > 0.  Device arrays:
 *   points      fp32 [num_rows, 3]  camera-frame points (mm), e.g. a frame's masked depth pixels lifted through its camera
 *   row_begin, row_end int32 [num_det]  a problem's rows [row_begin, row_end) of points, at most max_points; a range outside
 *               [0, num_rows] or longer than max_points is never read: the call then returns FP_ERR_INVALID naming the problem (it waits
 *               for the work queued on `stream` to learn this)
 *   R_in, t_in  fp64 [num_det, 9], [num_det, 3]  the input pose, model -> camera (mm);  has_pose int32 [num_det]  0: skipped (status 2)
 *   max_dist    fp64 [num_det]  the inlier distance (mm).  Not validated: a NaN or a value <= 0 leaves no inlier, so that problem is
 *               skipped (status 2) with its pose untouched
 * Per point X_c, fp64: d = X_c - t, X_m[i] = R[0][i] d0 + R[1][i] d1 + R[2][i] d2; per axis the grid coordinate g = (X_m - origin) / h
 * - 0.5, i0 = floor(g), alpha = g - i0.  Measurable: g finite and 0 <= i0 <= n - 2 on every axis (decided in fp64 before any conversion
 * or read; no voxel outside the volume is ever read) and all eight corners of the cell have sdf_cnt >= min_count (a point that is not
 * measurable reads no sdf_sum).  A corner's value is f = (double)sdf_sum / (double)sdf_cnt; phi is the trilinear interpolant of the
 * eight (x first, then y, then z), grad phi its exact gradient (per axis the four differences along it, bilinear over the other two
 * axes, over h), r = trunc_mm phi (mm).  rho = r^2 for an inlier (measurable, |r| < max_dist), max_dist^2 otherwise (no gradient);
 * cost = sum rho / (row_end - row_begin); with q = trunc_mm R grad phi the Jacobian row for the left-multiplied twist (rotation,
 * translation) is [q x X_c | -q]; H, g over the inliers.  The LM loop, lambda schedule and stopping rules are fp_featuremetric_refine's,
 * at most `iters` (0..1000) iterations, all enqueued at once.
 * Outputs: those of fp_depth_refine -- R_out, t_out, cost_in, cost_out, num_points (inliers at the input pose), iters_used, status
 * (0 refined, 1 no step accepted, 2 skipped: no pose, empty range or < 6 inliers at the input pose; for 1 and 2 the pose is the input
 * bit for bit); normal_eq fp64 [num_det, 28] may be null: H (upper triangle, row-major), g, cost at the input pose.  cost_out <=
 * cost_in always.  Deterministic and bit-identical across batch compositions; no float atomics.  A NULL pointer, a size or option
 * outside its range or too little scratch: FP_ERR_INVALID, nothing written.  scratch: FP_TSDF_TRACK_SCRATCH_BYTES.  (Added without a
 * change of FP_ABI_VERSION: no existing entry point changed.) */
#define FP_TSDF_TRACK_SCRATCH_BYTES(num_det, max_points) FP_DEPTH_REFINE_SCRATCH_BYTES(num_det, max_points)
int fp_tsdf_track(const float* sdf_sum, const int32_t* sdf_cnt, const double* box, int nx, int ny, int nz, int min_count, double trunc_mm,
                  const float* points, int64_t num_rows, const int32_t* row_begin, const int32_t* row_end, const double* R_in,
                  const double* t_in, const int32_t* has_pose, const double* max_dist, int num_det, int max_points, int iters,
                  void* scratch, size_t scratch_bytes, double* R_out, double* t_out, double* cost_in, double* cost_out,
                  int32_t* num_points, int32_t* iters_used, int32_t* status, double* normal_eq, fp_stream_t stream);

/* ---- frame-to-model tracking on shape and colour (reconstruct.py, track_color_weight > 0; DESIGN.md section 31;
 *      tests/tsdf_track_rgb_ref.py restates it) ----
 * fp_tsdf_track with a second per-point term: every argument of fp_tsdf_track means what it means there, plus
 *   rgb_sum, rgb_cnt  fp32 [3, nz, ny, nx] (planar), int32 [nz, ny, nx]  the colour planes fp_tsdf_integrate wrote beside the distances
 *   colors      fp32 [num_rows, 3]  the colour of every row of points, in [0, 1] (uint8 / 255 as fp_tsdf_integrate adds it)
 *   color_weight  lambda, mm per unit of colour, finite and > 0;  color_max  the channel inlier bound, finite and > 0
 * The geometric part of a point is evaluated exactly as in fp_tsdf_track.  Then, fp64: the point is colour-measurable when it is a
 * geometric inlier and all eight corners of its cell have rgb_cnt >= min_count (rgb_cnt is read only for geometric inliers, rgb_sum
 * only where all eight pass).  Per channel ch a corner's colour is (double)rgb_sum[ch] / (double)rgb_cnt, C_ch the trilinear
 * interpolant (x, then y, then z), grad C_ch its exact gradient over h -- phi's formulas; e_ch = C_ch - (double)colors[ch]; a channel
 * is an inlier when the point is colour-measurable and |e_ch| < color_max.  rho = rho_geom + sum_ch rho_ch, rho_ch = (lambda e_ch)^2
 * for a channel inlier and (lambda color_max)^2 otherwise (a geometric outlier, a point that is not colour-measurable, a NaN); cost =
 * sum rho / (row_end - row_begin).  A channel inlier adds the row [q_ch x X_c | -q_ch], q_ch = lambda R grad C_ch, with the residual
 * lambda e_ch to H and g: geometry first, then channel 0, 1, 2.  num_points, the stop on fewer than 6 inliers and status 2 count
 * GEOMETRIC inliers, as in fp_tsdf_track; normal_eq holds the joint system.  Outputs, scratch (FP_TSDF_TRACK_SCRATCH_BYTES), determinism
 * and the rule that a refused call writes nothing are fp_tsdf_track's.  (Added without a change of FP_ABI_VERSION: no existing entry
 * point changed.) */
int fp_tsdf_track_rgb(const float* sdf_sum, const int32_t* sdf_cnt, const float* rgb_sum, const int32_t* rgb_cnt, const double* box, int nx,
                      int ny, int nz, int min_count, double trunc_mm, const float* points, const float* colors, int64_t num_rows,
                      const int32_t* row_begin, const int32_t* row_end, const double* R_in, const double* t_in, const int32_t* has_pose,
                      const double* max_dist, double color_weight, double color_max, int num_det, int max_points, int iters, void* scratch,
                      size_t scratch_bytes, double* R_out, double* t_out, double* cost_in, double* cost_out, int32_t* num_points,
                      int32_t* iters_used, int32_t* status, double* normal_eq, fp_stream_t stream);

/* ---- joint refinement on features and depth (tests/rgbd_refine_ref.py restates it) --------------------------
 * One Levenberg-Marquardt objective E = E_f + depth_weight E_d per detection.  The pose (R, t) is model -> FRAME camera (mm).
 *   map, strides, gh, gw, C, W, H, feature_cameras   the featuremetric call's map arguments: the projected feature map and the camera
 *               (fx, fy, cx, cy; image W x H) it belongs to, the crop camera
 *   A, a        fp64 [num_det, 9], [num_det, 3]  the rigid transform frame camera -> feature camera, X_f = A X_c + a
 *   depth, num_images, Hd, Wd, image_index, frame_cameras, tau   the depth call's arguments: the frames' depth images and cameras
 *   R_in, t_in, row_begin, row_end, feats, vertices, num_rows, has_pose   as in the two calls above; a bad row range or image index is
 *               reported by FP_ERR_INVALID naming the detection, and such rows and images are never read
 *   depth_weight  w_d >= 0 (a negative or NaN value: FP_ERR_INVALID before any device work)
 * Feature term: the featuremetric call's, evaluated at X_f: valid set V frozen at the input pose, sigma^2 the mean squared residual
 * over V there (floored at 1e-12), weight 1 / (1 + s / sigma^2), E_f = sum_V log(1 + s / sigma^2) / |V|; the Jacobian carries A, the
 * twist is left-multiplied on the frame-camera pose.  Depth term: the depth call's at X_c, and a point is measurable only if also
 * max(taps) - min(taps) <= tau; E_d = sum min(r^2, tau^2) / (N tau^2) over the N rows of the range.
 * H = H_f / (|V| sigma^2) + w_d H_d / (N tau^2), g likewise.  The LM loop is the featuremetric call's (a trial that puts a point of
 * V at z_f <= 1 mm is rejected).  A detection with w_d = 0 or fewer than 6 depth inliers at the input pose runs on E_f alone.
 * Outputs as above: num_points = |V|, num_depth_inliers = the inliers at the input pose, status 0 refined, 1 no step accepted,
 * 2 skipped (no pose, empty range, |V| < 6); for 1 and 2 the pose is the input bit for bit; cost_out <= cost_in always.
 * normal_eq fp64 [num_det, 57] may be null: H_f (21) | g_f (6) | E_f, H_d (21) | g_d (6) | E_d, E, at the input pose.
 * Deterministic and bit-identical across batch compositions; no float atomics.  scratch: FP_RGBD_REFINE_SCRATCH_BYTES. */
#define FP_RGBD_REFINE_SCRATCH_BYTES(num_det, max_points)                                                              \
  ((size_t)FP_REFINE_STATE_BYTES * (size_t)(num_det) +                                                                  \
   16 * FP_REFINE_RECORD * (size_t)(num_det) * (((size_t)(max_points) + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK) +      \
   (((size_t)(num_det) * (size_t)(max_points) + 7) / 8) * 8 + 8)
int fp_rgbd_refine(const float* map, int64_t sb, int64_t sy, int64_t sx, int64_t sc, int gh, int gw, int C, int W, int H,
                   const double* feature_cameras, const double* A, const double* a, const float* depth, int num_images, int Hd, int Wd,
                   const int32_t* image_index, const double* frame_cameras, const double* R_in, const double* t_in,
                   const int32_t* row_begin, const int32_t* row_end, const float* feats, const float* vertices, int64_t num_rows,
                   const int32_t* has_pose, const double* tau, double depth_weight, int num_det, int max_points, int iters,
                   void* scratch, size_t scratch_bytes, double* R_out, double* t_out, double* cost_in, double* cost_out,
                   int32_t* num_points, int32_t* num_depth_inliers, int32_t* iters_used, int32_t* status, double* normal_eq,
                   fp_stream_t stream);

/* ---- result pictures (utils/vis_util.py:179-687 vis_inference_results in its vis_for_paper layout; DESIGN.md section 12;
 * tests/vis_ref.py restates every entry) ---------------------------------------------------------------------------------
 * Images are uint8 HWC (3 channels), contiguous, with a leading batch dimension; sides lie in [1, FP_VIS_MAX_SIDE].  One thread
 * produces one output pixel from a gather in a fixed order (no atomics): a detection's picture is bit-identical across runs
 * and batch compositions.  cv2 and matplotlib are not restated: the contract is this project's own (edge pixels are not
 * Canny's, the anti-aliasing is not Agg's).  Bad sizes or NULL pointers: FP_ERR_INVALID, nothing written. */
#define FP_VIS_MAX_SIDE 16384
#define FP_VIS_MAX_MATCHES 1024
#define FP_VIS_MAX_DILATE 8
#define FP_VIS_MAX_LAYERS 4096
/* normalize_data (vis_base_util.py:26) + nearest upsampling: map fp32 [batch, gh, gw, C] (C >= 3, channels 0..2 are used);
 * lo / hi = min / max over the gh gw 3 values of a detection (ONE range for the three channels), written to range fp32
 * [batch, 2] (scratch and output); out [batch, out_h, out_w, 3] = trunc(255 ((x - lo) / (hi - lo))) in fp32, the quotient first so that hi maps to 255 (0 when hi == lo), of
 * the cell (floor(y gh / out_h), floor(x gw / out_w)), then dimmed in integers: (v dim_num) / dim_den with 0 <= dim_num <= dim_den
 * <= 255 (1 / 1: unchanged; 9 / 10 for the query side of the match picture, vis_util.py's 0.9 factor). */
int fp_vis_pca_colorize(const float* map, int batch, int gh, int gw, int C, int out_h, int out_w, int dim_num, int dim_den, float* range,
                        uint8_t* out, fp_stream_t stream);
/* vis_util.py:286-292 with the white accent colour: out = (img + 255) >> 1 per channel where mask [batch, h, w] != 0, img elsewhere. */
int fp_vis_mask_tint(const uint8_t* img, const uint8_t* mask, int batch, int h, int w, uint8_t* out, fp_stream_t stream);
/* Replaces add_contour_overlay (cv2.Canny + cv2.dilate; unpinned).  A pixel of mask [batch, h, w] is an edge when it is set and
 * one of its 4 neighbours inside the image is unset; the edge map is dilated dilate_iterations (0..FP_VIS_MAX_DILATE) times by a
 * 3 x 3 square; those pixels of img [batch, h, w, 3] are overwritten with (r, g, b), each in [0, 255].  In place. */
int fp_vis_contour(const uint8_t* mask, int batch, int h, int w, int dilate_iterations, int r, int g, int b, uint8_t* img,
                   fp_stream_t stream);
/* Area-average downscaling of src [batch, h, w, 3] to out [batch, out_h, out_w, 3] (out_h <= h, out_w <= w, else FP_ERR_INVALID):
 * the footprint of output pixel x is [x w / out_w, (x + 1) w / out_w), likewise in y; the value is the footprint-area-weighted mean,
 * computed exactly in integers and rounded to nearest (half up). */
int fp_vis_resize_area(const uint8_t* src, int batch, int h, int w, int out_h, int out_w, uint8_t* out, fp_stream_t stream);
/* plot_matches: counts[b] <= max_matches <= FP_VIS_MAX_MATCHES segments (x0, y0, x1, y1) fp32 [batch, max_matches, 4] with a disc at both
 * ends, drawn in place onto tile [batch, h, w, 3].  Per pixel, centre p = (x + 1/2, y + 1/2), the matches in input order, for each its
 * segment (coverage clamp(1/2 + lw / 2 - dist(p, segment), 0, 1)) and then its two discs (clamp(1/2 + radius - |p - c|, 0, 1)):
 * out = out (1 - alpha cov) + colour alpha cov in fp32, rounded to nearest once at the end.  colour: HOST fp32 [3] in [0, 255]. */
int fp_vis_draw_matches(const float* segments, const int32_t* counts, int batch, int max_matches, int h, int w, const float* colour,
                        float alpha, float lw, float radius, uint8_t* tile, fp_stream_t stream);
/* One frame with several posed objects: depth fp32 [layers, h, w] in mm, 0 = background (fp_render_raster's output), colours uint8
 * [layers, 3].  ids int32 [h, w] = the layer with the smallest positive depth (ties: the lowest layer), -1 where none;
 * out [h, w, 3] = (img + colours[id]) >> 1 where a layer covers the pixel, img elsewhere.  1 <= layers <= FP_VIS_MAX_LAYERS. */
int fp_vis_scene_composite(const float* depth, const uint8_t* colours, int layers, int h, int w, const uint8_t* img, uint8_t* out,
                           int32_t* ids, fp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FOUNDPOSE_AMD_H */
