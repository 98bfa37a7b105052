/* libfoundpose_amd.so: the entry points of the silhouette refinement, declared in a header of their own beside include/foundpose_amd.h.
 * The types, status codes, fp_stream_t, fp_last_error and the FP_REFINE_* constants are that header's; the library is the same one.
 * Added without a change of FP_ABI_VERSION: no existing entry point changed. */
#ifndef FOUNDPOSE_AMD_MASK_REFINE_H
#define FOUNDPOSE_AMD_MASK_REFINE_H

#include "foundpose_amd.h"

#if FP_ABI_VERSION != 20
#error "foundpose_amd_mask_refine.h was written against FP_ABI_VERSION 20"
#endif

#define FP_MASK_MAX_SIDE 16384         /* the largest height / width of a mask */
#define FP_MASK_D2_EMPTY (1 << 30)     /* fp_mask_distance's value everywhere in a mask without a set pixel (the largest real value is 2 x 16383^2 < 5.4e8) */
#define FP_MASK_REFINE_TILE 256        /* projected points a workgroup of the contour pass holds in LDS at a time */
/* fp_mask_refine's scratch: states | forward records | err | backward records | (u, v) fp64 and the in-front flag int32 of every point */
#define FP_MASK_REFINE_SCRATCH_BYTES(num_det, max_points, max_contour)                                                                      \
  ((size_t)FP_REFINE_STATE_BYTES * (size_t)(num_det) +                                                                                      \
   8 * (size_t)FP_REFINE_RECORD * (size_t)(num_det) * (((size_t)(max_points) + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK) + 8 +                \
   8 * (size_t)FP_REFINE_RECORD * (size_t)(num_det) * (((size_t)(max_contour) + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK) +                   \
   16 * (size_t)(num_det) * (size_t)(max_points) + (((size_t)(num_det) * (size_t)(max_points) + 1) / 2) * 8)

#ifdef __cplusplus
extern "C" {
#endif

/* ---- squared distance field of binary masks (tests/mask_refine_ref.py restates it) ----
 * masks uint8 [num_masks, H, W] on the device, non-zero = set; d2 int32 [num_masks, H, W]: d2[b, y, x] = the minimum over the set
 * pixels (x', y') of mask b of (x - x')^2 + (y - y')^2, 0 on a set pixel, FP_MASK_D2_EMPTY everywhere in a mask without a set pixel.
 * Exact, in integers, over the whole frame; nothing outside [0, W) x [0, H) is read.  1 <= H, W <= FP_MASK_MAX_SIDE, 1 <= num_masks <=
 * 65535.  A NULL pointer or a size outside its range: FP_ERR_INVALID, nothing written. */
int fp_mask_distance(const uint8_t* masks, int num_masks, int H, int W, int32_t* d2, fp_stream_t stream);

/* ---- silhouette refinement of the final pose (foundpose_amd/refine_util.py; tests/mask_refine_ref.py) ----
 * Levenberg-Marquardt on the 6-DoF pose, model -> the FRAME's own camera (mm), of each of num_det detections against the detection's
 * mask at frame resolution.  Device arrays:
 *   d2          int32 [num_det, H, W]   fp_mask_distance of the detections' masks, one map per detection
 *   contour     int32 [num_contour, 2]  contour pixels (x, y) of the masks; contour_begin, contour_end int32 [num_det]: a detection's rows
 *               [begin, end), at most max_contour.  A range outside [0, num_contour] or longer than max_contour is never read:
 *               FP_ERR_INVALID naming the detection.  The values are used in arithmetic only, never as an index
 *   cameras     fp64 [num_det, 4]  fx, fy, cx, cy;  R_in, t_in fp64 [num_det, 9], [num_det, 3];  has_pose int32 [num_det]  0: skipped
 *   vertices    fp32 [num_rows, 3]; row_begin, row_end int32 [num_det]: the detection's N model points, at most max_points; a bad range is
 *               never read: FP_ERR_INVALID naming the detection (the call waits for the work queued on `stream` to learn either)
 * huber_px is the Huber delta in pixels, finite and > 0; iters 0..1000; 1 <= H, W <= FP_MASK_MAX_SIDE.
 * All arithmetic is fp64.  Xc = R X + t, u = fx Xc.x / Xc.z + cx, v = fy Xc.y / Xc.z + cy; a point is in front iff Xc.z > 1.
 * Forward rows, one per point: measurable iff in front and the taps x0 = floor(u), x0 + 1, y0 = floor(v), y0 + 1 lie inside the image;
 *   r = the bilinear value of sqrt((double) d2) at the four taps; Huber: |r| <= delta: rho = r^2, w = 1, else rho = 2 delta |r| -
 *   delta^2, w = delta / |r|; J = (dr/du, dr/dv) d(u, v)/dXc [-[Xc]x | I].  A row that is not measurable: rho = 0, no gradient.
 * Backward rows, one per contour row q: j = argmin over the in-front points of (u_j - q.x)^2 + (v_j - q.y)^2 (strict <, ties to the
 *   lowest j; no image-bounds test), e = (u_j - q.x, v_j - q.y), Huber on |e|, the two Jacobian rows d(u, v)/dXc [-[Xc]x | I] at X_j.  A
 *   pose at which no point is in front has cost +inf.  A point whose squared distance to q is not finite (a projection beyond about
 *   1e154 pixels, just past z > 1) is no candidate: a row all of whose in-front points are such costs +inf as well.
 * cost E = 1/2 sum_fwd rho / N + 1/2 sum_bwd rho / K (N = row_end - row_begin, K = contour_end - contour_begin); H and g are the same
 * weighted sums of w J^T J and w J^T r.  The LM loop, lambda schedule and stopping rules are fp_featuremetric_refine's, all
 * iterations enqueued at once.
 * Outputs: those of fp_depth_refine -- R_out, t_out, cost_in, cost_out, num_points (measurable forward rows at the input pose),
 * iters_used, status (0 refined, 1 no step accepted, 2 skipped: no pose, empty point range, K < 6, fewer than 6 measurable forward
 * rows at the input pose, or an input cost that is not finite; for 1 and 2 the pose is the input bit for bit); normal_eq fp64
 * [num_det, 28] may be null: H (upper triangle, row-major), g, E at the input pose.  cost_out <= cost_in always.  Deterministic and
 * bit-identical across batch compositions; no float atomics.  A NULL pointer, a size or option outside its range or too little
 * scratch: FP_ERR_INVALID, nothing written.  scratch: FP_MASK_REFINE_SCRATCH_BYTES(num_det, max_points, max_contour). */
int fp_mask_refine(const int32_t* d2, int H, int W, const int32_t* contour, int64_t num_contour, const int32_t* contour_begin,
                   const int32_t* contour_end, const double* cameras, const double* R_in, const double* t_in, const int32_t* row_begin,
                   const int32_t* row_end, const float* vertices, int64_t num_rows, const int32_t* has_pose, double huber_px, int num_det,
                   int max_points, int max_contour, int iters, void* scratch, size_t scratch_bytes, double* R_out, double* t_out,
                   double* cost_in, double* cost_out, int32_t* num_points, int32_t* iters_used, int32_t* status, double* normal_eq,
                   fp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FOUNDPOSE_AMD_MASK_REFINE_H */
