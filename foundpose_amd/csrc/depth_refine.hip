// Depth refinement of the final pose: Levenberg-Marquardt on the truncated-quadratic residual between the
// frame's measured depth, sampled bilinearly at the projections of a template's 3D points, and those points' own depth under the
// pose.  It runs in the frame's own camera on the unwarped depth image.  tests/depth_refine_ref.py restates the contract in numpy fp64.
//
// Kernels, all enqueued by fp_depth_refine without a host round trip between them:
//   depth_refine_setup     one thread per detection: validates the bank row range and the image index, initialises the LM state (lm_setup)
//   depth_refine_pass      (chunk of FP_REFINE_CHUNK points, detection), one wave: ONE POINT PER LANE -- projection, four taps, residual,
//                          Jacobian row (fp64; depth_point) -- then a butterfly over the chunk's lanes for the 29 terms, one partial record
//                          per workgroup (lm_lane_pass)
//   depth_refine_solve     one wave per detection: folds the partials in chunk order, then accepts / rejects the trial pose and
//                          solves the damped 6x6 system for the next one (lm_lane_solve)
//   depth_refine_finalize  one thread per detection: the outputs (lm_finalize)
// The parts named in brackets and the order of the launches (lm_enqueue) live in refine_terms.hpp: the term is shared with
// rgbd_refine.hip, the one-point-per-lane pass and its solve (the cost normalised by the point count, the stop on fewer than 6 inliers,
// no z-bad count) with tsdf_track.hip, the rest with all four solvers.  This file names its kernels and says which term they run.
// The pass/solve pair runs 1 + `iters` times.  Detections that have stopped leave both kernels at their first instruction.
// Every sum has a fixed order (lanes: butterfly; chunks: ascending), no atomics, and a detection's chunk decomposition depends
// only on its own point count: results are bit-identical across runs and batch compositions.
#include "common.hpp"
#include "kernels.hpp"
#include "refine_terms.hpp"

namespace {

__global__ void __launch_bounds__(64) depth_refine_setup_kernel(DepthRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < a.lm.num_det) lm_setup(a.lm, &a.d, a.state[b], b, 28);
}

__global__ void __launch_bounds__(64) depth_refine_pass_kernel(DepthRefineArgs a) {
  const int b = blockIdx.y;
  lm_lane_pass(a.lm, a.state[b], b,
               [&](const double* R, const double* t, const float* Xv, double (&acc)[FP_DEPTH_TERMS]) { depth_point<false>(a.d, a.lm.cam, b, R, t, Xv, acc); });
}

__global__ void __launch_bounds__(64) depth_refine_solve_kernel(DepthRefineArgs a, int mode) {
  __shared__ double tot[FP_REFINE_RECORD];
  lm_lane_solve(a.lm, a.state[blockIdx.x], blockIdx.x, mode, tot);
}

__global__ void __launch_bounds__(64) depth_refine_finalize_kernel(DepthRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < a.lm.num_det) lm_finalize(a.lm, a.state[b], b);
}

}  // namespace

int launch_depth_refine(const DepthRefineArgs& a, hipStream_t st) {
  return lm_enqueue(a.lm, 64, false,   // no sigma stage
                    [&](dim3 g, dim3 blk) { return lm_launch("depth_refine_setup", depth_refine_setup_kernel, g, blk, st, a); },
                    [&](dim3 g, dim3 blk, int) { return lm_launch("depth_refine_pass", depth_refine_pass_kernel, g, blk, st, a); },
                    [&](dim3 g, dim3 blk, int mode) { return lm_launch("depth_refine_solve", depth_refine_solve_kernel, g, blk, st, a, mode); },
                    [&](dim3 g, dim3 blk) { return lm_launch("depth_refine_finalize", depth_refine_finalize_kernel, g, blk, st, a); });
}
