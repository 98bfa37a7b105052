// Featuremetric refinement of the best coarse pose: Levenberg-Marquardt on the Cauchy-robust residual
// between the query's projected patch-feature map, sampled bilinearly at the projections of a template's 3D points, and
// those points' own features.  tests/featuremetric_ref.py restates the contract in numpy fp64.
//
// Kernels, all enqueued by fp_featuremetric_refine without a host round trip between them:
//   refine_setup     one thread per detection: validates the bank row range, initialises the LM state
//   refine_pass      (chunk of FP_REFINE_CHUNK points, detection): bilinear taps + six C-length dot products per point (fp32), the
//                    per-point Jacobian, cost and normal-equation terms (fp64), one partial record per workgroup
//   refine_solve     one wave per detection: folds the partials in chunk order, then accepts / rejects the trial pose and
//                    solves the damped 6x6 system for the next one (fp64 Cholesky; lm_step.hpp)
//   refine_finalize  one thread per detection: the outputs
// The pass/solve pair runs `iters` times.  Detections that have stopped leave both kernels at their first instruction.
// Every sum has a fixed order (lanes: butterfly; waves: 0..3; chunks: ascending), no atomics, and a detection's chunk
// decomposition depends only on its own point count: results are bit-identical across runs and batch compositions.
#include "common.hpp"
#include "kernels.hpp"
#include "lm_step.hpp"
#include "rot.hpp"

namespace {

constexpr int RF_WAVES = 4;
constexpr int RF_PTS_PER_WAVE = FP_REFINE_CHUNK / RF_WAVES;
constexpr int RF_REC = FP_REFINE_RECORD;  // doubles per partial: H (21, upper triangle row-major), g (6), E, sum s, valid, z-bad, pad

enum { MODE_INIT = 0, MODE_EVAL = 1 };
enum { SOLVE_SIGMA = 0, SOLVE_FIRST = 1, SOLVE_STEP = 2 };

FP_DEVICE float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(64) refine_setup_kernel(RefineArgs a) {
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
  const int r0 = a.row_begin[b], r1 = a.row_end[b];
  if (r0 < 0 || r1 < r0 || (long long)r1 > a.num_rows || r1 - r0 > a.max_points) {
    a.err[0] = b + 1;   // reported by the host through fp_last_error; the rows are never read
    return;
  }
  s.p0 = r0;
  s.np = r1 - r0;
  s.active = s.pending = s.np > 0;
}

__global__ void __launch_bounds__(64 * RF_WAVES) refine_pass_kernel(RefineArgs a, int mode) {
  __shared__ double red[RF_WAVES][RF_REC];
  const int b = blockIdx.y;
  const RefineState& s = a.state[b];
  if (!s.active || (mode == MODE_EVAL && !s.pending)) return;
  const int np = s.np, chunk0 = blockIdx.x * FP_REFINE_CHUNK;
  if (chunk0 >= np) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double fx = a.cam[4 * b + 0], fy = a.cam[4 * b + 1], cx = a.cam[4 * b + 2], cy = a.cam[4 * b + 3];
  const double sx = (double)a.gw / a.W, sy = (double)a.gh / a.H;
  const double xmax = a.gw - 1, ymax = a.gh - 1;
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = s.Rt[i];
  for (int i = 0; i < 3; ++i) t[i] = s.tt[i];
  const double sig2 = s.sigma2;
  const float* map = a.map + (long long)b * a.sb;
  uint8_t* valid = a.valid + (long long)b * a.max_points;
  double acc[RF_REC];
#pragma unroll
  for (int k = 0; k < RF_REC; ++k) acc[k] = 0.0;
  for (int k = 0; k < RF_PTS_PER_WAVE; ++k) {
    const int p = chunk0 + wave * RF_PTS_PER_WAVE + k;
    if (p >= np) break;
    if (mode == MODE_EVAL && !valid[p]) continue;
    const long long row = (long long)s.p0 + p;
    const float* Xf = a.verts + 3 * row;
    const double X[3] = {Xf[0], Xf[1], Xf[2]};
    double Xc[3];
    for (int i = 0; i < 3; ++i) Xc[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
    const double z = Xc[2];
    if (mode == MODE_EVAL && !(z > 1.0)) { acc[30] += 1.0; continue; }
    double xm = (fx * Xc[0] / z + cx) * sx - 0.5, ym = (fy * Xc[1] / z + cy) * sy - 0.5;
    if (mode == MODE_INIT) {
      const bool ok = z > 1.0 && xm >= 0.0 && xm <= xmax && ym >= 0.0 && ym <= ymax;
      if (lane == 0) valid[p] = ok ? 1 : 0;
      if (!ok) continue;
    }
    const bool clx = !(xm >= 0.0 && xm <= xmax), cly = !(ym >= 0.0 && ym <= ymax);
    xm = fmin(fmax(xm, 0.0), xmax);
    ym = fmin(fmax(ym, 0.0), ymax);
    const int x0 = min((int)floor(xm), a.gw - 2), y0 = min((int)floor(ym), a.gh - 2);
    const float al = (float)(xm - x0), be = (float)(ym - y0);
    const float* m00 = map + (long long)y0 * a.sy + (long long)x0 * a.sx;
    const float* m10 = m00 + a.sx;
    const float* m01 = m00 + a.sy;
    const float* m11 = m01 + a.sx;
    const float* f = a.feats + row * a.C;
    float gxx = 0.f, gxy = 0.f, gyy = 0.f, gxr = 0.f, gyr = 0.f, rr = 0.f;
    for (int c = lane; c < a.C; c += 64) {
      const long long o = (long long)c * a.sc;
      const float v00 = m00[o], v10 = m10[o], v01 = m01[o], v11 = m11[o];
      const float F = (1.f - be) * ((1.f - al) * v00 + al * v10) + be * ((1.f - al) * v01 + al * v11);
      const float r = F - f[c];
      const float gx = (1.f - be) * (v10 - v00) + be * (v11 - v01);
      const float gy = (1.f - al) * (v01 - v00) + al * (v11 - v10);
      gxx += gx * gx; gxy += gx * gy; gyy += gy * gy; gxr += gx * r; gyr += gy * r; rr += r * r;
    }
    gxx = wave_sum(gxx); gxy = wave_sum(gxy); gyy = wave_sum(gyy); gxr = wave_sum(gxr); gyr = wave_sum(gyr); rr = wave_sum(rr);
    const double si = rr;
    if (mode == MODE_INIT) {
      acc[28] += si;
      acc[29] += 1.0;
      continue;
    }
    // d(x_m, y_m)/d xi: rows ax, ay = diag(gw/W, gh/H) d(u, v)/dXc [-[Xc]x | I]; the rotation part is Xc x p
    const double iz = 1.0 / z;
    double px[3] = {sx * fx * iz, 0.0, -sx * fx * Xc[0] * iz * iz};
    double py[3] = {0.0, sy * fy * iz, -sy * fy * Xc[1] * iz * iz};
    double ax[6], ay[6];
    cross3(Xc, px, ax);
    cross3(Xc, py, ay);
    for (int i = 0; i < 3; ++i) { ax[3 + i] = px[i]; ay[3 + i] = py[i]; }
    if (clx) for (int i = 0; i < 6; ++i) ax[i] = 0.0;
    if (cly) for (int i = 0; i < 6; ++i) ay[i] = 0.0;
    const double q = si / sig2;
    const double w = 1.0 / (1.0 + q);
    const double dxx = w * (double)gxx, dxy = w * (double)gxy, dyy = w * (double)gyy;
    int k2 = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++k2) acc[k2] += dxx * ax[i] * ax[j] + dxy * (ax[i] * ay[j] + ay[i] * ax[j]) + dyy * ay[i] * ay[j];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += w * ((double)gxr * ax[i] + (double)gyr * ay[i]);
    acc[27] += sig2 * log1p(q);
    acc[29] += 1.0;
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < RF_REC; ++k) red[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < RF_REC) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < RF_WAVES; ++w) v += red[w][threadIdx.x];
    a.part[((long long)b * a.chunks + blockIdx.x) * RF_REC + threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(64) refine_solve_kernel(RefineArgs a, int mode) {
  __shared__ double tot[RF_REC];
  const int b = blockIdx.x;
  RefineState& s = a.state[b];
  if (!s.active || !s.pending) return;
  const int lane = threadIdx.x;
  const int nch = (s.np + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK;
  if (lane < RF_REC) {
    const double* p = a.part + (long long)b * a.chunks * RF_REC + lane;
    double v = 0.0;
    for (int c = 0; c < nch; ++c) v += p[(long long)c * RF_REC];
    tot[lane] = v;
  }
  __syncthreads();
  if (lane != 0) return;
  if (mode == SOLVE_SIGMA) {
    s.nvalid = (int)tot[29];
    if (s.nvalid < 6) { lm_stop(s); return; }
    s.skipped = 0;
    s.sigma2 = fmax(tot[28] / s.nvalid, 1e-12);
    return;   // pending stays 1: the next pass evaluates the input pose
  }
  if (mode == SOLVE_FIRST) {
    for (int i = 0; i < 21; ++i) s.H[i] = tot[i];
    for (int i = 0; i < 6; ++i) s.g[i] = tot[21 + i];
    s.E = s.E_in = tot[27];
    if (a.normal_eq)
      for (int i = 0; i < 28; ++i) a.normal_eq[28 * b + i] = tot[i];
    s.pending = 0;
    lm_propose(s, a.iters);
    return;
  }
  // SOLVE_STEP: the pass evaluated the trial pose
  s.pending = 0;
  const double Et = tot[27];
  if (tot[30] == 0.0 && Et < s.E) {
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

__global__ void __launch_bounds__(64) refine_finalize_kernel(RefineArgs a) {
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

int launch_featuremetric_refine(const RefineArgs& a, hipStream_t st) {
  const dim3 pgrid(a.chunks, a.num_det), sgrid(a.num_det);
  const int tgrid = cdiv(a.num_det, 64);
  hipLaunchKernelGGL(refine_setup_kernel, dim3(tgrid), dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("refine_setup");
  hipLaunchKernelGGL(refine_pass_kernel, pgrid, dim3(64 * RF_WAVES), 0, st, a, (int)MODE_INIT);
  FP_CHECK_LAUNCH("refine_pass");
  hipLaunchKernelGGL(refine_solve_kernel, sgrid, dim3(64), 0, st, a, (int)SOLVE_SIGMA);
  FP_CHECK_LAUNCH("refine_solve");
  hipLaunchKernelGGL(refine_pass_kernel, pgrid, dim3(64 * RF_WAVES), 0, st, a, (int)MODE_EVAL);
  FP_CHECK_LAUNCH("refine_pass");
  hipLaunchKernelGGL(refine_solve_kernel, sgrid, dim3(64), 0, st, a, (int)SOLVE_FIRST);
  FP_CHECK_LAUNCH("refine_solve");
  for (int k = 0; k < a.iters; ++k) {
    hipLaunchKernelGGL(refine_pass_kernel, pgrid, dim3(64 * RF_WAVES), 0, st, a, (int)MODE_EVAL);
    FP_CHECK_LAUNCH("refine_pass");
    hipLaunchKernelGGL(refine_solve_kernel, sgrid, dim3(64), 0, st, a, (int)SOLVE_STEP);
    FP_CHECK_LAUNCH("refine_solve");
  }
  hipLaunchKernelGGL(refine_finalize_kernel, dim3(tgrid), dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("refine_finalize");
  return FP_OK;
}
