/* libfoundpose_amd.so: the multi-view entry point, declared in a header of its own beside include/foundpose_amd.h.
 * The types, status codes, fp_stream_t, fp_last_error and FP_DEPTH_REFINE_SCRATCH_BYTES are that header's; the library is the same one.
 * Added without a change of FP_ABI_VERSION: no existing entry point changed. */
#ifndef FOUNDPOSE_AMD_MULTIVIEW_H
#define FOUNDPOSE_AMD_MULTIVIEW_H

#include "foundpose_amd.h"

#if FP_ABI_VERSION != 20
#error "foundpose_amd_multiview.h was written against FP_ABI_VERSION 20"
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- multi-view pose consensus (foundpose_amd/multiview.py; tests/multiview_ref.py restates it) ----
 * Levenberg-Marquardt on the model -> WORLD pose (mm) of each of num_det independent problems (one scene object each) whose rows are
 * (member view, model point) pairs: the pixel a member view's own estimate projects the point to is a virtual observation of the point
 * in that view.  No image is read.  Device arrays:
 *   points      fp32 [num_rows, 3]  a row's model point y (mm)
 *   targets     fp64 [num_rows, 2]  a row's target pixel (u*, v*).  Not validated: a value that is not finite makes the problem's cost
 *               NaN, no step is then accepted and its pose stays the input
 *   view_index  int32 [num_rows]    a row's view, an index into the two tables; a value outside [0, num_views) in a claimed row is never
 *               used: the call then returns FP_ERR_INVALID naming the problem
 *   view_cam    fp64 [num_views, 4]   fx, fy, cx, cy;   view_T  fp64 [num_views, 12]  R_v row-major | t_v, world -> camera (mm)
 *   row_begin, row_end int32 [num_det]  a problem's rows [row_begin, row_end), at most max_points (the cap the scratch is sized for); a
 *               range outside [0, num_rows] or longer than max_points is never read: FP_ERR_INVALID naming the problem (the call waits
 *               for the work queued on `stream` to learn either)
 *   R_in, t_in  fp64 [num_det, 9], [num_det, 3]  the input pose, model -> world;  has_pose int32 [num_det]  0: skipped (status 2)
 * huber_px is the Huber delta in pixels, finite and > 0; num_views >= 1; iters 0..1000.
 * Per row, fp64: Xw = R y + t, Xc = R_v Xw + t_v, e = (fx Xc.x / Xc.z + cx - u*, fy Xc.y / Xc.z + cy - v*), s = e . e.  Where Xc.z > 1 is
 * false the row is not measurable: rho = delta^2, no gradient, not an inlier.  Otherwise Huber: sqrt(s) <= delta: rho = s, w = 1, an
 * inlier; else rho = 2 delta sqrt(s) - delta^2, w = delta / sqrt(s), not an inlier.  There is no image-bounds test.  H += w J^T J, g +=
 * w J^T e with, for each row p of d(u, v)/dXc and q = R_v^T p, the Jacobian row [Xw x q | q] of the left-multiplied twist (rotation,
 * translation) in the world frame.  cost = sum rho / (row_end - row_begin).  The LM loop, lambda schedule and stopping rules are
 * fp_featuremetric_refine's, all iterations enqueued at once.
 * Outputs: those of fp_depth_refine -- R_out, t_out, cost_in, cost_out, num_points (inliers at the input pose), iters_used, status
 * (0 refined, 1 no step accepted, 2 skipped: no pose, empty range or < 6 inliers at the input pose; for 1 and 2 the pose is the input
 * bit for bit); normal_eq fp64 [num_det, 28] may be null: H (upper triangle, row-major), g, cost at the input pose.  cost_out <=
 * cost_in always.  Deterministic and bit-identical across batch compositions; no float atomics.  A NULL pointer, a size or option
 * outside its range or too little scratch: FP_ERR_INVALID, nothing written.  scratch: FP_DEPTH_REFINE_SCRATCH_BYTES(num_det,
 * max_points), the same layout.  (Added without a change of FP_ABI_VERSION: no existing entry point changed.) */
int fp_multiview_refine(const float* points, const double* targets, const int32_t* view_index, int64_t num_rows, const double* view_cam,
                        const double* view_T, int num_views, const int32_t* row_begin, const int32_t* row_end, const double* R_in,
                        const double* t_in, const int32_t* has_pose, double huber_px, int num_det, int max_points, int iters, void* scratch,
                        size_t scratch_bytes, double* R_out, double* t_out, double* cost_in, double* cost_out, int32_t* num_points,
                        int32_t* iters_used, int32_t* status, double* normal_eq, fp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FOUNDPOSE_AMD_MULTIVIEW_H */
