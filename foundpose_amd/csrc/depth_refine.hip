// Depth refinement of the final pose: Levenberg-Marquardt on the truncated-quadratic residual between the
// frame's measured depth, sampled bilinearly at the projections of a template's 3D points, and those points' own depth under the
// pose.  It runs in the frame's own camera on the unwarped depth image.  tests/depth_refine_ref.py restates the contract in numpy fp64.
//
// Kernels, all enqueued by fp_depth_refine without a host round trip between them:
//   depth_refine_setup     one thread per detection: validates the bank row range and the image index, initialises the LM state (lm_setup)
//   depth_refine_pass      (chunk of FP_REFINE_CHUNK points, detection), one wave: ONE POINT PER LANE -- projection, four taps, residual,
//                          Jacobian row (fp64; depth_point) -- then a butterfly over the chunk's lanes for the 29 terms, one partial record per workgroup
//   depth_refine_solve     one wave per detection: folds the partials in chunk order, then accepts / rejects the trial pose and
//                          solves the damped 6x6 system for the next one
//   depth_refine_finalize  one thread per detection: the outputs (lm_finalize)
// The parts named in brackets, the fold and the accept / reject / propose steps of the solve live in refine_terms.hpp, shared with
// refine.hip and rgbd_refine.hip; this file keeps its one-point-per-lane butterfly, the cost normalised by the point count, the stop on
// fewer than 6 inliers and its rejection test (there is no z-bad count: a point behind the camera is an outlier like any other).
// The pass/solve pair runs 1 + `iters` times.  Detections that have stopped leave both kernels at their first instruction.
// Every sum has a fixed order (lanes: butterfly; chunks: ascending), no atomics, and a detection's chunk decomposition depends
// only on its own point count: results are bit-identical across runs and batch compositions.
#include "common.hpp"
#include "kernels.hpp"
#include "refine_terms.hpp"

namespace {

constexpr int DR_REC = FP_REFINE_RECORD;   // doubles per partial: H (21, upper triangle row-major), g (6), sum rho [27], pad, inliers [29], pad
static_assert(FP_REFINE_CHUNK == 32, "one half-wave per chunk");

__global__ void __launch_bounds__(64) depth_refine_setup_kernel(DepthRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < a.lm.num_det) lm_setup(a.lm, &a.d, a.state[b], b, 28);
}

// A chunk is FP_REFINE_CHUNK = 32 points, so lanes 32..63 of the wave idle by construction.  A 64-point chunk would fill the wave, but
// FP_REFINE_CHUNK is shared with refine.hip (scratch layout, chunk order of its sums): changing it changes that kernel's output bits.
// At these sizes the call is bound by its launches, not by the pass.
__global__ void __launch_bounds__(64) depth_refine_pass_kernel(DepthRefineArgs a) {
  const int b = blockIdx.y;
  const RefineState& s = a.state[b];
  if (!s.active || !s.pending) return;
  const int np = s.np, chunk0 = blockIdx.x * FP_REFINE_CHUNK;
  if (chunk0 >= np) return;
  const int lane = threadIdx.x;
  const int p = chunk0 + lane;
  double acc[FP_DEPTH_TERMS];
#pragma unroll
  for (int k = 0; k < FP_DEPTH_TERMS; ++k) acc[k] = 0.0;
  if (lane < FP_REFINE_CHUNK && p < np) depth_point<false>(a.d, a.lm.cam, b, s.Rt, s.tt, a.lm.verts + 3 * ((long long)s.p0 + p), acc);
  // lanes 32..63 carry zeros and fold among themselves: lane 0 ends with the sum of lanes 0..31 in butterfly order
#pragma unroll
  for (int k = 0; k < FP_DEPTH_TERMS; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = FP_REFINE_CHUNK / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    acc[k] = v;
  }
  if (lane == 0) {
    double* out = a.lm.part + ((long long)b * a.lm.chunks + blockIdx.x) * DR_REC;
#pragma unroll
    for (int k = 0; k < 28; ++k) out[k] = acc[k];
    out[28] = 0.0;
    out[29] = acc[28];
    out[30] = out[31] = 0.0;
  }
}

__global__ void __launch_bounds__(64) depth_refine_solve_kernel(DepthRefineArgs a, int mode) {
  __shared__ double tot[DR_REC];
  const int b = blockIdx.x;
  RefineState& s = a.state[b];
  if (!s.active || !s.pending) return;
  lm_fold(a.lm, b, s.np, DR_REC, threadIdx.x, tot);
  if (threadIdx.x != 0) return;
  s.pending = 0;
  const double Et = tot[27] / s.np;   // the point set is every row of the range: costs at different poses are comparable
  if (mode == SOLVE_STEP && !(Et < s.E)) {
    lm_reject(s, a.lm.iters);
    return;
  }
  if (mode == SOLVE_FIRST) {
    s.E = s.E_in = Et;
    s.nvalid = (int)tot[29];
    if (a.lm.normal_eq) {
      for (int i = 0; i < 27; ++i) a.lm.normal_eq[28 * b + i] = tot[i];
      a.lm.normal_eq[28 * b + 27] = Et;
    }
  } else if (!lm_accept(s, Et)) {
    return;
  }
  lm_set_system(s, tot);
  if (mode == SOLVE_FIRST) {
    if (s.nvalid < 6) { lm_stop(s); return; }
    s.skipped = 0;
  }
  lm_propose(s, a.lm.iters);
}

__global__ void __launch_bounds__(64) depth_refine_finalize_kernel(DepthRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < a.lm.num_det) lm_finalize(a.lm, a.state[b], b);
}

}  // namespace

int launch_depth_refine(const DepthRefineArgs& a, hipStream_t st) {
  const dim3 pgrid(a.lm.chunks, a.lm.num_det), sgrid(a.lm.num_det);
  const int tgrid = cdiv(a.lm.num_det, 64);
  hipLaunchKernelGGL(depth_refine_setup_kernel, dim3(tgrid), dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("depth_refine_setup");
  hipLaunchKernelGGL(depth_refine_pass_kernel, pgrid, dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("depth_refine_pass");
  hipLaunchKernelGGL(depth_refine_solve_kernel, sgrid, dim3(64), 0, st, a, (int)SOLVE_FIRST);
  FP_CHECK_LAUNCH("depth_refine_solve");
  for (int k = 0; k < a.lm.iters; ++k) {
    hipLaunchKernelGGL(depth_refine_pass_kernel, pgrid, dim3(64), 0, st, a);
    FP_CHECK_LAUNCH("depth_refine_pass");
    hipLaunchKernelGGL(depth_refine_solve_kernel, sgrid, dim3(64), 0, st, a, (int)SOLVE_STEP);
    FP_CHECK_LAUNCH("depth_refine_solve");
  }
  hipLaunchKernelGGL(depth_refine_finalize_kernel, dim3(tgrid), dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("depth_refine_finalize");
  return FP_OK;
}
