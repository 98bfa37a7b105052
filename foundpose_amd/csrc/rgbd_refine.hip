// Joint refinement of the final pose on features and depth: Levenberg-Marquardt on
//   E = E_f + w_d E_d,   E_f = sum_V log(1 + s_i / sigma^2) / |V| (section 11's term),   E_d = sum min(r^2, tau^2) / (N tau^2) (section 14's)
// The pose lives in the frame's camera; the feature term is evaluated in the feature (crop) camera, X_f = A X_c + a, and its Jacobian
// carries A.  The depth term adds a tap-consistency test to section 14's: a point whose four taps spread over more than tau is not
// measurable.  tests/rgbd_refine_ref.py restates the contract in numpy fp64.
//
// Kernels, all enqueued by fp_rgbd_refine without a host round trip between them:
//   rgbd_setup     one thread per detection: validates the bank row range and the image index, initialises the LM state
//   rgbd_pass      (chunk of FP_REFINE_CHUNK points, detection), four waves of 8 points: refine.hip's channel loop and six shuffle-reduced
//                  fp32 dot products per point with all 64 lanes; then lane p of a wave takes the wave's point p for the depth row (fp64).
//                  The two terms stay apart: one record of 64 doubles per workgroup, feature half | depth half, no normalisation
//   rgbd_solve     one wave per detection: folds the partials in chunk order, mixes the halves with 1 / (|V| sigma^2) and
//                  w_d / (N tau^2), accepts / rejects the trial pose and solves for the next one (lm_step.hpp)
//   rgbd_finalize  one thread per detection: the outputs
// 2 + 2 iters launches after the setup chain, as refine.hip alone.  Detections that have stopped leave pass and solve at their first
// instruction.  Every sum has a fixed order (lanes: butterfly; points of a wave: ascending; waves: 0..3; the 32 depth rows of a chunk:
// ascending; chunks: ascending), no atomics, and a detection's chunk decomposition depends only on its own point count: results are
// bit-identical across runs and batch compositions.
#include "common.hpp"
#include "kernels.hpp"
#include "lm_step.hpp"
#include "rot.hpp"

namespace {

constexpr int RG_WAVES = 4;
constexpr int RG_PTS_PER_WAVE = FP_REFINE_CHUNK / RG_WAVES;
constexpr int RG_HALF = FP_REFINE_RECORD;   // feature half: H (21, upper triangle row-major), g (6), sum log1p [27], sum s [28], valid [29], z-bad [30], pad
constexpr int RG_REC = 2 * RG_HALF;         // depth half at +32: H (21), g (6), sum rho [27], pad, inliers [29], pad
constexpr int RG_DTERMS = 29;               // what a depth row carries: 0..27 and the inlier flag
constexpr int RG_DSTRIDE = RG_DTERMS + 4;   // odd number of doubles per row: the 8 lanes of a wave write different banks
static_assert(RG_PTS_PER_WAVE == 8 && FP_REFINE_CHUNK == 32, "lane p of a wave takes the wave's point p");

enum { MODE_INIT = 0, MODE_EVAL = 1 };
enum { SOLVE_SIGMA = 0, SOLVE_FIRST = 1, SOLVE_STEP = 2 };

FP_DEVICE float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(64) rgbd_setup_kernel(RgbdRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.num_det) return;
  RgbdState& rs = a.state[b];
  RefineState& s = rs.s;
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
  rs.ninl = 0;
  rs.use_depth = 1;        // the pass at the input pose always evaluates the depth rows: the solve then decides
  if (a.normal_eq)
    for (int i = 0; i < 57; ++i) a.normal_eq[57 * b + i] = 0.0;
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

__global__ void __launch_bounds__(64 * RG_WAVES) rgbd_pass_kernel(RgbdRefineArgs a, int mode) {
  __shared__ double red[RG_WAVES][RG_HALF];
  __shared__ double drow[FP_REFINE_CHUNK][RG_DSTRIDE];
  const int b = blockIdx.y;
  const RgbdState& rs = a.state[b];
  const RefineState& s = rs.s;
  if (!s.active || (mode == MODE_EVAL && !s.pending)) return;
  const int np = s.np, chunk0 = blockIdx.x * FP_REFINE_CHUNK;
  if (chunk0 >= np) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool with_depth = mode == MODE_EVAL && rs.use_depth;
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = s.Rt[i];
  for (int i = 0; i < 3; ++i) t[i] = s.tt[i];
  {
    // ---- the feature term: refine.hip's pass at X_f = A X_c + a; every lane carries the same fp64 values
    const double fx = a.fcam[4 * b + 0], fy = a.fcam[4 * b + 1], cx = a.fcam[4 * b + 2], cy = a.fcam[4 * b + 3];
    const double sx = (double)a.gw / a.W, sy = (double)a.gh / a.H;
    const double xmax = a.gw - 1, ymax = a.gh - 1;
    double A[9], av[3];
    for (int i = 0; i < 9; ++i) A[i] = a.A[9 * b + i];
    for (int i = 0; i < 3; ++i) av[i] = a.a[3 * b + i];
    const double sig2 = s.sigma2;
    const float* map = a.map + (long long)b * a.sb;
    uint8_t* valid = a.valid + (long long)b * a.max_points;
    double acc[RG_HALF];
#pragma unroll
    for (int k = 0; k < RG_HALF; ++k) acc[k] = 0.0;
    for (int k = 0; k < RG_PTS_PER_WAVE; ++k) {
      const int p = chunk0 + wave * RG_PTS_PER_WAVE + k;
      if (p >= np) break;
      if (mode == MODE_EVAL && !valid[p]) continue;
      const long long row = (long long)s.p0 + p;
      const float* Xv = a.verts + 3 * row;
      const double X[3] = {Xv[0], Xv[1], Xv[2]};
      double Xc[3], Xf[3];
      for (int i = 0; i < 3; ++i) Xc[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
      for (int i = 0; i < 3; ++i) Xf[i] = A[3 * i] * Xc[0] + A[3 * i + 1] * Xc[1] + A[3 * i + 2] * Xc[2] + av[i];
      const double z = Xf[2];
      if (mode == MODE_EVAL && !(z > 1.0)) { acc[30] += 1.0; continue; }
      double xm = (fx * Xf[0] / z + cx) * sx - 0.5, ym = (fy * Xf[1] / z + cy) * sy - 0.5;
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
      // d(x_m, y_m)/d xi: rows ax, ay = diag(gw/W, gh/H) d(u, v)/dXf A [-[Xc]x | I]; with p' = A^T p the rotation part is Xc x p'
      const double iz = 1.0 / z;
      const double qx[3] = {sx * fx * iz, 0.0, -sx * fx * Xf[0] * iz * iz};
      const double qy[3] = {0.0, sy * fy * iz, -sy * fy * Xf[1] * iz * iz};
      double px[3], py[3];
      for (int i = 0; i < 3; ++i) {
        px[i] = A[i] * qx[0] + A[3 + i] * qx[1] + A[6 + i] * qx[2];
        py[i] = A[i] * qy[0] + A[3 + i] * qy[1] + A[6 + i] * qy[2];
      }
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
      acc[27] += log1p(q);
      acc[29] += 1.0;
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < RG_HALF; ++k) red[wave][k] = acc[k];
    }
  }
  // ---- the depth term: lane p of a wave takes the wave's point p (every row of the range, valid for the feature term or not)
  if (with_depth && lane < RG_PTS_PER_WAVE) {
    const int slot = wave * RG_PTS_PER_WAVE + lane, p = chunk0 + slot;
    double d[RG_DTERMS];
#pragma unroll
    for (int k = 0; k < RG_DTERMS; ++k) d[k] = 0.0;
    if (p < np) {
      const double fx = a.cam[4 * b + 0], fy = a.cam[4 * b + 1], cx = a.cam[4 * b + 2], cy = a.cam[4 * b + 3];
      const double tau = a.tau[b];
      const float* Xv = a.verts + 3 * ((long long)s.p0 + p);
      const double X[3] = {Xv[0], Xv[1], Xv[2]};
      double Xc[3];
      for (int i = 0; i < 3; ++i) Xc[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
      const double z = Xc[2], iz = 1.0 / z;
      const double u = fx * Xc[0] / z + cx, v = fy * Xc[1] / z + cy;
      // measurable: z > 1 mm, the four taps x0, x0 + 1, y0, y0 + 1 inside the image (NaN compares false), all of them > 0 and within tau of each other
      bool ok = z > 1.0 && u >= 0.0 && u < (double)(a.Wd - 1) && v >= 0.0 && v < (double)(a.Hd - 1);
      double rho = tau * tau;
      if (ok) {
        const int x0 = (int)floor(u), y0 = (int)floor(v);
        const double al = u - x0, be = v - y0;
        const float* d0 = a.depth + ((long long)a.image_index[b] * a.Hd + y0) * a.Wd + x0;
        const double D00 = d0[0], D10 = d0[1], D01 = d0[a.Wd], D11 = d0[a.Wd + 1];
        const double hi = fmax(fmax(D00, D10), fmax(D01, D11)), lo = fmin(fmin(D00, D10), fmin(D01, D11));
        ok = D00 > 0.0 && D10 > 0.0 && D01 > 0.0 && D11 > 0.0 && hi - lo <= tau;
        const double dd = (1.0 - be) * ((1.0 - al) * D00 + al * D10) + be * ((1.0 - al) * D01 + al * D11);
        const double r = dd - z;
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
            for (int j = i; j < 6; ++j, ++k2) d[k2] = J[i] * J[j];
#pragma unroll
          for (int i = 0; i < 6; ++i) d[21 + i] = J[i] * r;
          rho = r * r;
          d[28] = 1.0;
        }
      }
      d[27] = rho;
    }
#pragma unroll
    for (int k = 0; k < RG_DTERMS; ++k) drow[slot][k] = d[k];
  }
  __syncthreads();
  double* out = a.part + ((long long)b * a.chunks + blockIdx.x) * RG_REC;
  if (threadIdx.x < RG_HALF) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < RG_WAVES; ++w) v += red[w][threadIdx.x];
    out[threadIdx.x] = v;
  } else if (threadIdx.x < RG_REC) {
    // depth half: column j of the chunk's 32 rows in ascending order; 28 is a pad, the inlier count sits at 29 as in depth_refine.hip
    const int j = threadIdx.x - RG_HALF, col = j < 28 ? j : (j == 29 ? 28 : -1);
    double v = 0.0;
    if (with_depth && col >= 0)
      for (int r = 0; r < FP_REFINE_CHUNK; ++r) v += drow[r][col];
    out[threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(64) rgbd_solve_kernel(RgbdRefineArgs a, int mode) {
  __shared__ double tot[RG_REC];
  const int b = blockIdx.x;
  RgbdState& rs = a.state[b];
  RefineState& s = rs.s;
  if (!s.active || !s.pending) return;
  const int lane = threadIdx.x;
  const int nch = (s.np + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK;
  {
    const double* p = a.part + (long long)b * a.chunks * RG_REC + lane;
    double v = 0.0;
    for (int c = 0; c < nch; ++c) v += p[(long long)c * RG_REC];
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
  const double* td = tot + RG_HALF;
  const double tau = a.tau[b];
  const double nf = (double)s.nvalid * s.sigma2, nd = (double)s.np * (tau * tau);
  const double Ef = tot[27] / s.nvalid, Ed = td[27] / nd;
  if (mode == SOLVE_FIRST) {
    rs.ninl = (int)td[29];
    rs.use_depth = a.wd > 0.0 && rs.ninl >= 6;
  }
  const bool dep = rs.use_depth;
  const double Et = dep ? Ef + a.wd * Ed : Ef;
  if (mode == SOLVE_FIRST) {
    if (a.normal_eq) {
      double* ne = a.normal_eq + 57 * b;
      for (int i = 0; i < 27; ++i) { ne[i] = tot[i]; ne[28 + i] = td[i]; }
      ne[27] = Ef;
      ne[55] = Ed;
      ne[56] = Et;
    }
    s.E_in = Et;
  } else if (!(tot[30] == 0.0 && Et < s.E)) {
    // SOLVE_STEP, the trial pose is rejected
    s.pending = 0;
    s.lam *= 10.0;
    if (s.lam > 1e12) { lm_stop(s); return; }
    lm_propose(s, a.iters);
    return;
  }
  // the system at the (new) current pose: H = H_f / (|V| sigma^2) + w_d H_d / (N tau^2), g likewise
  const double rel = mode == SOLVE_FIRST ? 1.0 : (s.E - Et) / s.E;
  for (int i = 0; i < 21; ++i) s.H[i] = dep ? tot[i] / nf + a.wd * td[i] / nd : tot[i] / nf;
  for (int i = 0; i < 6; ++i) s.g[i] = dep ? tot[21 + i] / nf + a.wd * td[21 + i] / nd : tot[21 + i] / nf;
  s.E = Et;
  s.pending = 0;
  if (mode == SOLVE_STEP) {
    for (int i = 0; i < 9; ++i) s.R[i] = s.Rt[i];
    for (int i = 0; i < 3; ++i) s.t[i] = s.tt[i];
    s.lam = fmax(s.lam / 10.0, 1e-12);
    s.accepted = 1;
    if (rel < 1e-10) { lm_stop(s); return; }
  }
  lm_propose(s, a.iters);
}

__global__ void __launch_bounds__(64) rgbd_finalize_kernel(RgbdRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.num_det) return;
  const RgbdState& rs = a.state[b];
  const RefineState& s = rs.s;
  for (int i = 0; i < 9; ++i) a.R_out[9 * b + i] = s.R[i];
  for (int i = 0; i < 3; ++i) a.t_out[3 * b + i] = s.t[i];
  a.cost_in[b] = s.E_in;
  a.cost_out[b] = s.E;
  a.num_points[b] = s.nvalid;
  a.num_depth_inliers[b] = rs.ninl;
  a.iters_used[b] = s.it;
  a.status[b] = s.skipped ? 2 : (s.accepted ? 0 : 1);
}

}  // namespace

int launch_rgbd_refine(const RgbdRefineArgs& a, hipStream_t st) {
  const dim3 pgrid(a.chunks, a.num_det), sgrid(a.num_det);
  const int tgrid = cdiv(a.num_det, 64);
  hipLaunchKernelGGL(rgbd_setup_kernel, dim3(tgrid), dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("rgbd_setup");
  hipLaunchKernelGGL(rgbd_pass_kernel, pgrid, dim3(64 * RG_WAVES), 0, st, a, (int)MODE_INIT);
  FP_CHECK_LAUNCH("rgbd_pass");
  hipLaunchKernelGGL(rgbd_solve_kernel, sgrid, dim3(64), 0, st, a, (int)SOLVE_SIGMA);
  FP_CHECK_LAUNCH("rgbd_solve");
  hipLaunchKernelGGL(rgbd_pass_kernel, pgrid, dim3(64 * RG_WAVES), 0, st, a, (int)MODE_EVAL);
  FP_CHECK_LAUNCH("rgbd_pass");
  hipLaunchKernelGGL(rgbd_solve_kernel, sgrid, dim3(64), 0, st, a, (int)SOLVE_FIRST);
  FP_CHECK_LAUNCH("rgbd_solve");
  for (int k = 0; k < a.iters; ++k) {
    hipLaunchKernelGGL(rgbd_pass_kernel, pgrid, dim3(64 * RG_WAVES), 0, st, a, (int)MODE_EVAL);
    FP_CHECK_LAUNCH("rgbd_pass");
    hipLaunchKernelGGL(rgbd_solve_kernel, sgrid, dim3(64), 0, st, a, (int)SOLVE_STEP);
    FP_CHECK_LAUNCH("rgbd_solve");
  }
  hipLaunchKernelGGL(rgbd_finalize_kernel, dim3(tgrid), dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("rgbd_finalize");
  return FP_OK;
}
