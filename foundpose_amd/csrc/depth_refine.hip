// Depth refinement of the final pose: Levenberg-Marquardt on the truncated-quadratic residual between the
// frame's measured depth, sampled bilinearly at the projections of a template's 3D points, and those points' own depth under the
// pose.  It runs in the frame's own camera on the unwarped depth image.  tests/depth_refine_ref.py restates the contract in numpy fp64.
//
// Kernels, all enqueued by fp_depth_refine without a host round trip between them:
//   depth_refine_setup     one thread per detection: validates the bank row range and the image index, initialises the LM state
//   depth_refine_pass      (chunk of FP_REFINE_CHUNK points, detection), one wave: ONE POINT PER LANE -- projection, four taps, residual,
//                          Jacobian row (fp64) -- then a butterfly over the chunk's lanes for the 29 terms, one partial record per workgroup
//   depth_refine_solve     one wave per detection: folds the partials in chunk order, then accepts / rejects the trial pose and
//                          solves the damped 6x6 system for the next one (lm_step.hpp, shared with refine.hip)
//   depth_refine_finalize  one thread per detection: the outputs
// The pass/solve pair runs 1 + `iters` times.  Detections that have stopped leave both kernels at their first instruction.
// Every sum has a fixed order (lanes: butterfly; chunks: ascending), no atomics, and a detection's chunk decomposition depends
// only on its own point count: results are bit-identical across runs and batch compositions.
#include "common.hpp"
#include "kernels.hpp"
#include "lm_step.hpp"
#include "rot.hpp"

namespace {

constexpr int DR_REC = FP_REFINE_RECORD;   // doubles per partial: H (21, upper triangle row-major), g (6), sum rho [27], pad, inliers [29], pad
constexpr int DR_TERMS = 29;               // what the butterfly carries: 0..27 and the inlier count
static_assert(FP_REFINE_CHUNK == 32, "one half-wave per chunk");

enum { DSOLVE_FIRST = 0, DSOLVE_STEP = 1 };

__global__ void __launch_bounds__(64) depth_refine_setup_kernel(DepthRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.num_det) return;
  RefineState& s = a.state[b];
  for (int i = 0; i < 9; ++i) s.R[i] = s.Rt[i] = a.R_in[9 * b + i];
  for (int i = 0; i < 3; ++i) s.t[i] = s.tt[i] = a.t_in[3 * b + i];
  for (int i = 0; i < 21; ++i) s.H[i] = 0.0;
  for (int i = 0; i < 6; ++i) s.g[i] = 0.0;
  s.E = s.E_in = s.sigma2 = 0.0;
  s.lam = 1e-3;
  s.it = s.accepted = s.nvalid = s.pending = 0;
  s.skipped = 1;
  s.active = 0;
  s.p0 = s.np = 0;
  if (a.normal_eq)
    for (int i = 0; i < 28; ++i) a.normal_eq[28 * b + i] = 0.0;
  if (!a.has_pose[b]) return;
  const int r0 = a.row_begin[b], r1 = a.row_end[b], im = a.image_index[b];
  if (r0 < 0 || r1 < r0 || (long long)r1 > a.num_rows || r1 - r0 > a.max_points) {
    a.err[0] = b + 1;      // reported by the host through fp_last_error; neither the rows nor the image are ever read
    return;
  }
  if (im < 0 || im >= a.num_images) {
    a.err[0] = -(b + 1);
    return;
  }
  s.p0 = r0;
  s.np = r1 - r0;
  s.active = s.pending = s.np > 0;
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
  double acc[DR_TERMS];
#pragma unroll
  for (int k = 0; k < DR_TERMS; ++k) acc[k] = 0.0;
  if (lane < FP_REFINE_CHUNK && p < np) {
    const double fx = a.cam[4 * b + 0], fy = a.cam[4 * b + 1], cx = a.cam[4 * b + 2], cy = a.cam[4 * b + 3];
    const double tau = a.tau[b];
    const float* Xf = a.verts + 3 * ((long long)s.p0 + p);
    const double X[3] = {Xf[0], Xf[1], Xf[2]};
    double Xc[3];
    for (int i = 0; i < 3; ++i) Xc[i] = s.Rt[3 * i] * X[0] + s.Rt[3 * i + 1] * X[1] + s.Rt[3 * i + 2] * X[2] + s.tt[i];
    const double z = Xc[2], iz = 1.0 / z;
    const double u = fx * Xc[0] / z + cx, v = fy * Xc[1] / z + cy;
    // measurable: z > 1 mm and the four taps x0, x0 + 1, y0, y0 + 1 inside the image (NaN compares false), all of them > 0
    bool ok = z > 1.0 && u >= 0.0 && u < (double)(a.W - 1) && v >= 0.0 && v < (double)(a.H - 1);
    double rho = tau * tau;
    if (ok) {
      const int x0 = (int)floor(u), y0 = (int)floor(v);
      const double al = u - x0, be = v - y0;
      const float* d0 = a.depth + ((long long)a.image_index[b] * a.H + y0) * a.W + x0;
      const double D00 = d0[0], D10 = d0[1], D01 = d0[a.W], D11 = d0[a.W + 1];
      ok = D00 > 0.0 && D10 > 0.0 && D01 > 0.0 && D11 > 0.0;
      const double d = (1.0 - be) * ((1.0 - al) * D00 + al * D10) + be * ((1.0 - al) * D01 + al * D11);
      const double r = d - z;
      if (ok && fabs(r) < tau) {   // an inlier: the only points with a gradient
        const double du = (1.0 - be) * (D10 - D00) + be * (D11 - D01), dv = (1.0 - al) * (D01 - D00) + al * (D11 - D10);
        // dr/dXc = (dd/du, dd/dv) d(u, v)/dXc - e_z; J = dr/dXc [-[Xc]x | I]: the rotation part is Xc x (dr/dXc)
        const double q[3] = {du * fx * iz, dv * fy * iz, -(du * fx * Xc[0] + dv * fy * Xc[1]) * iz * iz - 1.0};
        double J[6];
        cross3(Xc, q, J);
        for (int i = 0; i < 3; ++i) J[3 + i] = q[i];
        int k2 = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = i; j < 6; ++j, ++k2) acc[k2] = J[i] * J[j];
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[21 + i] = J[i] * r;
        rho = r * r;
        acc[28] = 1.0;
      }
    }
    acc[27] = rho;
  }
  // lanes 32..63 carry zeros and fold among themselves: lane 0 ends with the sum of lanes 0..31 in butterfly order
#pragma unroll
  for (int k = 0; k < DR_TERMS; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = FP_REFINE_CHUNK / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    acc[k] = v;
  }
  if (lane == 0) {
    double* out = a.part + ((long long)b * a.chunks + blockIdx.x) * DR_REC;
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
  const int lane = threadIdx.x;
  const int nch = (s.np + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK;
  if (lane < DR_REC) {
    const double* p = a.part + (long long)b * a.chunks * DR_REC + lane;
    double v = 0.0;
    for (int c = 0; c < nch; ++c) v += p[(long long)c * DR_REC];
    tot[lane] = v;
  }
  __syncthreads();
  if (lane != 0) return;
  s.pending = 0;
  const double Et = tot[27] / s.np;   // the point set is every row of the range: costs at different poses are comparable
  if (mode == DSOLVE_FIRST) {
    for (int i = 0; i < 21; ++i) s.H[i] = tot[i];
    for (int i = 0; i < 6; ++i) s.g[i] = tot[21 + i];
    s.E = s.E_in = Et;
    s.nvalid = (int)tot[29];
    if (a.normal_eq) {
      for (int i = 0; i < 27; ++i) a.normal_eq[28 * b + i] = tot[i];
      a.normal_eq[28 * b + 27] = Et;
    }
    if (s.nvalid < 6) { lm_stop(s); return; }
    s.skipped = 0;
    lm_propose(s, a.iters);
    return;
  }
  // DSOLVE_STEP: the pass evaluated the trial pose
  if (Et < s.E) {
    const double rel = (s.E - Et) / s.E;
    for (int i = 0; i < 9; ++i) s.R[i] = s.Rt[i];
    for (int i = 0; i < 3; ++i) s.t[i] = s.tt[i];
    for (int i = 0; i < 21; ++i) s.H[i] = tot[i];
    for (int i = 0; i < 6; ++i) s.g[i] = tot[21 + i];
    s.E = Et;
    s.lam = fmax(s.lam / 10.0, 1e-12);
    s.accepted = 1;
    if (rel < 1e-10) { lm_stop(s); return; }
  } else {
    s.lam *= 10.0;
    if (s.lam > 1e12) { lm_stop(s); return; }
  }
  lm_propose(s, a.iters);
}

__global__ void __launch_bounds__(64) depth_refine_finalize_kernel(DepthRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.num_det) return;
  const RefineState& s = a.state[b];
  for (int i = 0; i < 9; ++i) a.R_out[9 * b + i] = s.R[i];
  for (int i = 0; i < 3; ++i) a.t_out[3 * b + i] = s.t[i];
  a.cost_in[b] = s.E_in;
  a.cost_out[b] = s.E;
  a.num_points[b] = s.nvalid;
  a.iters_used[b] = s.it;
  a.status[b] = s.skipped ? 2 : (s.accepted ? 0 : 1);
}

}  // namespace

int launch_depth_refine(const DepthRefineArgs& a, hipStream_t st) {
  const dim3 pgrid(a.chunks, a.num_det), sgrid(a.num_det);
  const int tgrid = cdiv(a.num_det, 64);
  hipLaunchKernelGGL(depth_refine_setup_kernel, dim3(tgrid), dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("depth_refine_setup");
  hipLaunchKernelGGL(depth_refine_pass_kernel, pgrid, dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("depth_refine_pass");
  hipLaunchKernelGGL(depth_refine_solve_kernel, sgrid, dim3(64), 0, st, a, (int)DSOLVE_FIRST);
  FP_CHECK_LAUNCH("depth_refine_solve");
  for (int k = 0; k < a.iters; ++k) {
    hipLaunchKernelGGL(depth_refine_pass_kernel, pgrid, dim3(64), 0, st, a);
    FP_CHECK_LAUNCH("depth_refine_pass");
    hipLaunchKernelGGL(depth_refine_solve_kernel, sgrid, dim3(64), 0, st, a, (int)DSOLVE_STEP);
    FP_CHECK_LAUNCH("depth_refine_solve");
  }
  hipLaunchKernelGGL(depth_refine_finalize_kernel, dim3(tgrid), dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("depth_refine_finalize");
  return FP_OK;
}
