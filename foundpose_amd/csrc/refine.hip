// Featuremetric refinement of the best coarse pose: Levenberg-Marquardt on the Cauchy-robust residual
// between the query's projected patch-feature map, sampled bilinearly at the projections of a template's 3D points, and
// those points' own features.  tests/featuremetric_ref.py restates the contract in numpy fp64.
//
// Kernels, all enqueued by fp_featuremetric_refine without a host round trip between them:
//   refine_setup     one thread per detection: validates the bank row range, initialises the LM state (lm_setup)
//   refine_pass      (chunk of FP_REFINE_CHUNK points, detection): bilinear taps + six C-length dot products per point (fp32), the
//                    per-point Jacobian, cost and normal-equation terms (fp64; feat_point), one partial record per workgroup
//   refine_solve     one wave per detection: folds the partials in chunk order, then accepts / rejects the trial pose and
//                    solves the damped 6x6 system for the next one (fp64 Cholesky)
//   refine_finalize  one thread per detection: the outputs (lm_finalize)
// The parts named in brackets, the fold, the sigma stage (lm_sigma), the accept / reject / propose steps of the solve and the order of
// the launches (lm_enqueue) live in refine_terms.hpp, shared with depth_refine.hip, rgbd_refine.hip and tsdf_track.hip; this file keeps
// the reduction of its pass and its unnormalised H, g, E.
// The pass/solve pair runs `iters` times.  Detections that have stopped leave both kernels at their first instruction.
// Every sum has a fixed order (lanes: butterfly; waves: 0..3; chunks: ascending), no atomics, and a detection's chunk
// decomposition depends only on its own point count: results are bit-identical across runs and batch compositions.
#include "common.hpp"
#include "kernels.hpp"
#include "refine_terms.hpp"

namespace {

constexpr int RF_WAVES = 4;
constexpr int RF_PTS_PER_WAVE = FP_REFINE_CHUNK / RF_WAVES;
constexpr int RF_REC = FP_REFINE_RECORD;  // doubles per partial: H (21, upper triangle row-major), g (6), E, sum s, valid, z-bad, pad

__global__ void __launch_bounds__(64) refine_setup_kernel(RefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < a.lm.num_det) lm_setup(a.lm, nullptr, a.state[b], b, 28);
}

__global__ void __launch_bounds__(64 * RF_WAVES) refine_pass_kernel(RefineArgs a, int mode) {
  __shared__ double red[RF_WAVES][RF_REC];
  const int b = blockIdx.y;
  const RefineState& s = a.state[b];
  if (!s.active || (mode == MODE_EVAL && !s.pending)) return;
  const int np = s.np, chunk0 = blockIdx.x * FP_REFINE_CHUNK;
  if (chunk0 >= np) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const FeatFrame c = feat_frame(a.f, a.lm.cam, b, a.lm.max_points, s.sigma2);
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = s.Rt[i];
  for (int i = 0; i < 3; ++i) t[i] = s.tt[i];
  double acc[RF_REC];
#pragma unroll
  for (int k = 0; k < RF_REC; ++k) acc[k] = 0.0;
  // the pose's own camera: no (A, a); slot 27 carries sigma^2 log1p(q)
  if (mode == MODE_INIT) {
    for (int k = 0, p = chunk0 + wave * RF_PTS_PER_WAVE; k < RF_PTS_PER_WAVE && p < np; ++k, ++p)
      feat_point<MODE_INIT, false, true>(a.f, c, R, t, nullptr, nullptr, a.lm.verts, s.p0, p, lane, acc);
  } else {
    for (int k = 0, p = chunk0 + wave * RF_PTS_PER_WAVE; k < RF_PTS_PER_WAVE && p < np; ++k, ++p)
      feat_point<MODE_EVAL, false, true>(a.f, c, R, t, nullptr, nullptr, a.lm.verts, s.p0, p, lane, acc);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < RF_REC; ++k) red[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < RF_REC) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < RF_WAVES; ++w) v += red[w][threadIdx.x];
    a.lm.part[((long long)b * a.lm.chunks + blockIdx.x) * RF_REC + threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(64) refine_solve_kernel(RefineArgs a, int mode) {
  __shared__ double tot[RF_REC];
  const int b = blockIdx.x;
  RefineState& s = a.state[b];
  if (!s.active || !s.pending) return;
  lm_fold(a.lm, b, s.np, RF_REC, threadIdx.x, tot);
  if (threadIdx.x != 0) return;
  if (mode == SOLVE_SIGMA) {
    lm_sigma(s, tot);
    return;
  }
  s.pending = 0;
  const double Et = tot[27];
  if (mode == SOLVE_STEP && !(tot[30] == 0.0 && Et < s.E)) {
    lm_reject(s, a.lm.iters);
    return;
  }
  if (mode == SOLVE_FIRST) {
    s.E = s.E_in = Et;
    if (a.lm.normal_eq)
      for (int i = 0; i < 28; ++i) a.lm.normal_eq[28 * b + i] = tot[i];
  } else if (!lm_accept(s, Et)) {
    return;
  }
  lm_set_system(s, tot);   // H, g, E stay unnormalised
  lm_propose(s, a.lm.iters);
}

__global__ void __launch_bounds__(64) refine_finalize_kernel(RefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < a.lm.num_det) lm_finalize(a.lm, a.state[b], b);
}

}  // namespace

int launch_featuremetric_refine(const RefineArgs& a, hipStream_t st) {
  return lm_enqueue(a.lm, 64 * RF_WAVES, true,   // with the sigma stage
                    [&](dim3 g, dim3 blk) { return lm_launch("refine_setup", refine_setup_kernel, g, blk, st, a); },
                    [&](dim3 g, dim3 blk, int mode) { return lm_launch("refine_pass", refine_pass_kernel, g, blk, st, a, mode); },
                    [&](dim3 g, dim3 blk, int mode) { return lm_launch("refine_solve", refine_solve_kernel, g, blk, st, a, mode); },
                    [&](dim3 g, dim3 blk) { return lm_launch("refine_finalize", refine_finalize_kernel, g, blk, st, a); });
}
