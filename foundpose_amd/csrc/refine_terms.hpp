// The parts shared by the four Levenberg-Marquardt solvers -- the three pose refinements (refine.hip, depth_refine.hip, rgbd_refine.hip;
// DESIGN.md sections 11, 14 and 15) and the frame-to-model tracker (tsdf_track.hip; section 30): state initialisation and row claim, the
// outputs, the fold of the partial records, the damped 6x6 solve, the proposal / acceptance / rejection of a trial pose on a RefineState,
// the sigma stage of the two feature solves, the whole one-point-per-lane pass and its solve (depth_refine.hip and tsdf_track.hip: only
// the per-point term differs), the two per-point terms -- features and depth -- of the refiners' passes, and, on the host, the order in
// which a call enqueues its kernels.
// What differs between the solvers (the camera of the feature term, its cost slot, the tap-spread test, the reduction of a feature
// pass, the normalisation and stopping rule of a feature solve, the tracker's per-point term and its rule for a failed call) is a
// template parameter here or stays in the caller.
// The device functions are defined here, at global scope, without `static`: that is safe only because FP_DEVICE is
// __device__ __forceinline__ (every use is inlined, no symbol is emitted twice).  Keep them FP_DEVICE.
// Every floating-point statement stands as one source expression: the library is built with -ffp-contract=on, so splitting or merging
// one changes which multiplies fuse with which adds, and with that the output bits.
#pragma once
#include "common.hpp"
#include "kernels.hpp"
#include "rot.hpp"

enum { MODE_INIT = 0, MODE_EVAL = 1 };                        // a feature pass: mark the valid points and sum s_i for sigma | build the system
enum { SOLVE_SIGMA = 0, SOLVE_FIRST = 1, SOLVE_STEP = 2 };    // a solve: after MODE_INIT | at the input pose | at a trial pose
constexpr int FP_DEPTH_TERMS = 29;                            // what depth_point produces: H (21), g (6), rho [27], the inlier flag [28]

// ---- setup / finalize: one thread per detection
// Initialises the state and claims the bank rows; a bad row range sets err to b + 1, a bad image index (checked where `da` is given)
// to -(b + 1): the host reports either through fp_last_error, and neither the rows nor the image are ever read.
FP_DEVICE void lm_setup(const RefineLmArgs& a, const RefineDepthArgs* da, RefineState& s, int b, int neq_width) {
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
    for (int i = 0; i < neq_width; ++i) a.normal_eq[neq_width * b + i] = 0.0;
  if (!a.has_pose[b]) return;
  const int r0 = a.row_begin[b], r1 = a.row_end[b];
  if (r0 < 0 || r1 < r0 || (long long)r1 > a.num_rows || r1 - r0 > a.max_points) {
    a.err[0] = b + 1;
    return;
  }
  if (da) {
    const int im = da->image_index[b];
    if (im < 0 || im >= da->num_images) {
      a.err[0] = -(b + 1);
      return;
    }
  }
  s.p0 = r0;
  s.np = r1 - r0;
  s.active = s.pending = s.np > 0;
}

FP_DEVICE void lm_finalize(const RefineLmArgs& a, const RefineState& s, int b) {
  for (int i = 0; i < 9; ++i) a.R_out[9 * b + i] = s.R[i];
  for (int i = 0; i < 3; ++i) a.t_out[3 * b + i] = s.t[i];
  a.cost_in[b] = s.E_in;
  a.cost_out[b] = s.E;
  a.num_points[b] = s.nvalid;
  a.iters_used[b] = s.it;
  a.status[b] = s.skipped ? 2 : (s.accepted ? 0 : 1);
}

// ---- solve: one wave per detection
// tot[0..n) = the detection's partial records of n doubles, summed in ascending chunk order; every thread of the workgroup calls it
FP_DEVICE void lm_fold(const RefineLmArgs& a, int b, int np, int n, int lane, double* tot) {
  const int nch = (np + FP_REFINE_CHUNK - 1) / FP_REFINE_CHUNK;
  if (lane < n) {
    const double* p = a.part + (long long)b * a.chunks * n + lane;
    double v = 0.0;
    for (int c = 0; c < nch; ++c) v += p[(long long)c * n];
    tot[lane] = v;
  }
  __syncthreads();
}

// (H + lam diag(H)) d = -g by Cholesky; false if a pivot is not > 0 (or not finite)
FP_DEVICE bool lm_solve(const double* H, const double* g, double lam, double* d) {
  double L[6][6];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++k) { L[j][i] = H[k]; L[i][j] = H[k]; }
  for (int i = 0; i < 6; ++i) L[i][i] = L[i][i] + lam * L[i][i];
  for (int j = 0; j < 6; ++j) {
    double dj = L[j][j];
    for (int m = 0; m < j; ++m) dj -= L[j][m] * L[j][m];
    if (!(dj > 0.0) || !(dj < INFINITY)) return false;
    const double ljj = sqrt(dj);
    L[j][j] = ljj;
    for (int i = j + 1; i < 6; ++i) {
      double v = L[i][j];
      for (int m = 0; m < j; ++m) v -= L[i][m] * L[j][m];
      L[i][j] = v / ljj;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double v = -g[i];
    for (int m = 0; m < i; ++m) v -= L[i][m] * y[m];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int m = i + 1; m < 6; ++m) v -= L[m][i] * d[m];
    d[i] = v / L[i][i];
  }
  return true;
}

FP_DEVICE void lm_stop(RefineState& s) { s.active = 0; s.pending = 0; }

// next trial pose from the current system; a failed factorisation is a rejected step (one iteration, lam x 10)
FP_DEVICE void lm_propose(RefineState& s, int iters) {
  for (int k = 0; k <= iters && s.active; ++k) {
    if (s.it >= iters) { lm_stop(s); return; }
    double d[6];
    const bool ok = lm_solve(s.H, s.g, s.lam, d);
    s.it += 1;
    if (ok) {
      double E[9];
      rot_exp(d, E);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) s.Rt[i * 3 + j] = E[i * 3 + 0] * s.R[0 * 3 + j] + E[i * 3 + 1] * s.R[1 * 3 + j] + E[i * 3 + 2] * s.R[2 * 3 + j];
      for (int i = 0; i < 3; ++i) s.tt[i] = E[i * 3 + 0] * s.t[0] + E[i * 3 + 1] * s.t[1] + E[i * 3 + 2] * s.t[2] + d[3 + i];
      s.pending = 1;
      return;
    }
    s.lam *= 10.0;
    if (s.lam > 1e12) { lm_stop(s); return; }
  }
}

FP_DEVICE void lm_set_system(RefineState& s, const double* tot) {   // H | g as a partial record lays them out
  for (int i = 0; i < 21; ++i) s.H[i] = tot[i];
  for (int i = 0; i < 6; ++i) s.g[i] = tot[21 + i];
}

// the trial pose, of cost Et < s.E, becomes the current one; false: converged, the detection has stopped.  Otherwise the caller puts
// the pose's system into s.H, s.g and proposes the next one -- as it does at the input pose, so that lm_propose is inlined once for both
FP_DEVICE bool lm_accept(RefineState& s, double Et) {
  const double rel = (s.E - Et) / s.E;
  for (int i = 0; i < 9; ++i) s.R[i] = s.Rt[i];
  for (int i = 0; i < 3; ++i) s.t[i] = s.tt[i];
  s.E = Et;
  s.lam = fmax(s.lam / 10.0, 1e-12);
  s.accepted = 1;
  if (rel < 1e-10) { lm_stop(s); return false; }
  return true;
}

FP_DEVICE void lm_reject(RefineState& s, int iters) {
  s.lam *= 10.0;
  if (s.lam > 1e12) { lm_stop(s); return; }
  lm_propose(s, iters);
}

// the sigma stage of a feature solve (SOLVE_SIGMA, lane 0): tot = the fold of a MODE_INIT pass, sum s [28] over the valid points [29]
FP_DEVICE void lm_sigma(RefineState& s, const double* tot) {
  s.nvalid = (int)tot[29];
  if (s.nvalid < 6) { lm_stop(s); return; }
  s.skipped = 0;
  s.sigma2 = fmax(tot[28] / s.nvalid, 1e-12);
  // pending stays 1: the next pass evaluates the input pose
}

// ---- one point per lane (depth_refine.hip, tsdf_track.hip, and multiview.hip with one (view, point) row per lane): the pass, one wave per (chunk, problem) = (blockIdx.x, b), and its solve,
// one wave per problem.  The record is FP_REFINE_RECORD doubles: H (21, upper triangle row-major), g (6), sum rho [27], pad, inliers [29],
// pad.  The cost is normalised by the point count, a problem with fewer than 6 inliers at the input pose stops (there is no z-bad count:
// a point that cannot be measured is an outlier like any other).
static_assert(FP_REFINE_CHUNK == 32, "one half-wave per chunk");
// point(R, t, Xv, acc) is the caller's term: acc arrives zeroed and leaves with the point's FP_DEPTH_TERMS values (see depth_point).
// A chunk is FP_REFINE_CHUNK = 32 points, so lanes 32..63 of the wave idle by construction.  A 64-point chunk would fill the wave, but
// FP_REFINE_CHUNK is shared with the feature passes (scratch layout, chunk order of their sums, lm_fold): changing it changes the
// output bits of all four solvers.  At these sizes a call is bound by its launches, not by the pass.
template <class Point>
FP_DEVICE void lm_lane_pass(const RefineLmArgs& a, const RefineState& s, int b, Point point) {
  if (!s.active || !s.pending) return;
  const int np = s.np, chunk0 = blockIdx.x * FP_REFINE_CHUNK;
  if (chunk0 >= np) return;
  const int lane = threadIdx.x;
  const int p = chunk0 + lane;
  double acc[FP_DEPTH_TERMS];
#pragma unroll
  for (int k = 0; k < FP_DEPTH_TERMS; ++k) acc[k] = 0.0;
  if (lane < FP_REFINE_CHUNK && p < np) point(s.Rt, s.tt, a.verts + 3 * ((long long)s.p0 + p), acc);
  // lanes 32..63 carry zeros and fold among themselves: lane 0 ends with the sum of lanes 0..31 in butterfly order
#pragma unroll
  for (int k = 0; k < FP_DEPTH_TERMS; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = FP_REFINE_CHUNK / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    acc[k] = v;
  }
  if (lane == 0) {
    double* out = a.part + ((long long)b * a.chunks + blockIdx.x) * FP_REFINE_RECORD;
#pragma unroll
    for (int k = 0; k < 28; ++k) out[k] = acc[k];
    out[28] = 0.0;
    out[29] = acc[28];
    out[30] = out[31] = 0.0;
  }
}

// tot: FP_REFINE_RECORD doubles of LDS; every thread of the workgroup calls it
FP_DEVICE void lm_lane_solve(const RefineLmArgs& a, RefineState& s, int b, int mode, double* tot) {
  if (!s.active || !s.pending) return;
  lm_fold(a, b, s.np, FP_REFINE_RECORD, threadIdx.x, tot);
  if (threadIdx.x != 0) return;
  s.pending = 0;
  const double Et = tot[27] / s.np;   // the point set is every row of the range: costs at different poses are comparable
  if (mode == SOLVE_STEP && !(Et < s.E)) {
    lm_reject(s, a.iters);
    return;
  }
  if (mode == SOLVE_FIRST) {
    s.E = s.E_in = Et;
    s.nvalid = (int)tot[29];
    if (a.normal_eq) {
      for (int i = 0; i < 27; ++i) a.normal_eq[28 * b + i] = tot[i];
      a.normal_eq[28 * b + 27] = Et;
    }
  } else if (!lm_accept(s, Et)) {
    return;
  }
  lm_set_system(s, tot);
  if (mode == SOLVE_FIRST) {
    if (s.nvalid < 6) { lm_stop(s); return; }
    s.skipped = 0;
  }
  lm_propose(s, a.iters);
}

// ---- the feature term of one point (sections 11 and 15), run by a whole wave: the 64 lanes split the channels, every lane carries the
// same fp64 values.  acc: H (21, upper triangle row-major), g (6), the cost [27], sum s [28], valid [29], z-bad [30].
struct FeatFrame {         // a detection's constants of the term
  double fx, fy, cx, cy, sx, sy, xmax, ymax, sig2;
  const float* map; uint8_t* valid;
};
FP_DEVICE FeatFrame feat_frame(const RefineMapArgs& a, const double* cam, int b, int max_points, double sig2) {
  FeatFrame c;
  c.fx = cam[4 * b + 0]; c.fy = cam[4 * b + 1]; c.cx = cam[4 * b + 2]; c.cy = cam[4 * b + 3];
  c.sx = (double)a.gw / a.W; c.sy = (double)a.gh / a.H;
  c.xmax = a.gw - 1; c.ymax = a.gh - 1;
  c.sig2 = sig2;
  c.map = a.map + (long long)b * a.sb;
  c.valid = a.valid + (long long)b * max_points;
  return c;
}
// Point p of the detection (bank row p0 + p) under the pose (R, t).  VIA_A: the map's camera is reached through X_f = A X_c + av and the
// Jacobian carries A^T (rgbd_refine.hip); otherwise it is the pose's own camera and A, av are not read (refine.hip).
// SIG2_COST: slot 27 takes sigma^2 log1p(q) (refine.hip) instead of log1p(q).
template <int MODE, bool VIA_A, bool SIG2_COST>
FP_DEVICE void feat_point(const RefineMapArgs& a, const FeatFrame& c, const double* R, const double* t, const double* A, const double* av,
                          const float* verts, int p0, int p, int lane, double (&acc)[FP_REFINE_RECORD]) {
  const double fx = c.fx, fy = c.fy, cx = c.cx, cy = c.cy, sx = c.sx, sy = c.sy, xmax = c.xmax, ymax = c.ymax, sig2 = c.sig2;
  if (MODE == MODE_EVAL && !c.valid[p]) return;
  const long long row = (long long)p0 + p;
  const float* Xv = verts + 3 * row;
  const double X[3] = {Xv[0], Xv[1], Xv[2]};
  double Xc[3], Xf[3];
  for (int i = 0; i < 3; ++i) Xc[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
  if constexpr (VIA_A) {
    for (int i = 0; i < 3; ++i) Xf[i] = A[3 * i] * Xc[0] + A[3 * i + 1] * Xc[1] + A[3 * i + 2] * Xc[2] + av[i];
  } else {
    for (int i = 0; i < 3; ++i) Xf[i] = Xc[i];
  }
  const double z = Xf[2];
  if (MODE == MODE_EVAL && !(z > 1.0)) { acc[30] += 1.0; return; }
  double xm = (fx * Xf[0] / z + cx) * sx - 0.5, ym = (fy * Xf[1] / z + cy) * sy - 0.5;
  if (MODE == MODE_INIT) {
    const bool ok = z > 1.0 && xm >= 0.0 && xm <= xmax && ym >= 0.0 && ym <= ymax;
    if (lane == 0) c.valid[p] = ok ? 1 : 0;
    if (!ok) return;
  }
  const bool clx = !(xm >= 0.0 && xm <= xmax), cly = !(ym >= 0.0 && ym <= ymax);
  xm = fmin(fmax(xm, 0.0), xmax);
  ym = fmin(fmax(ym, 0.0), ymax);
  const int x0 = min((int)floor(xm), a.gw - 2), y0 = min((int)floor(ym), a.gh - 2);
  const float al = (float)(xm - x0), be = (float)(ym - y0);
  const float* m00 = c.map + (long long)y0 * a.sy + (long long)x0 * a.sx;
  const float* m10 = m00 + a.sx;
  const float* m01 = m00 + a.sy;
  const float* m11 = m01 + a.sx;
  const float* f = a.feats + row * a.C;
  float gxx = 0.f, gxy = 0.f, gyy = 0.f, gxr = 0.f, gyr = 0.f, rr = 0.f;
  for (int ch = lane; ch < a.C; ch += 64) {
    const long long o = (long long)ch * a.sc;
    const float v00 = m00[o], v10 = m10[o], v01 = m01[o], v11 = m11[o];
    const float F = (1.f - be) * ((1.f - al) * v00 + al * v10) + be * ((1.f - al) * v01 + al * v11);
    const float r = F - f[ch];
    const float gx = (1.f - be) * (v10 - v00) + be * (v11 - v01);
    const float gy = (1.f - al) * (v01 - v00) + al * (v11 - v10);
    gxx += gx * gx; gxy += gx * gy; gyy += gy * gy; gxr += gx * r; gyr += gy * r; rr += r * r;
  }
  gxx = wave_sum(gxx); gxy = wave_sum(gxy); gyy = wave_sum(gyy); gxr = wave_sum(gxr); gyr = wave_sum(gyr); rr = wave_sum(rr);
  const double si = rr;
  if (MODE == MODE_INIT) {
    acc[28] += si;
    acc[29] += 1.0;
    return;
  }
  // d(x_m, y_m)/d xi: rows ax, ay = diag(gw/W, gh/H) d(u, v)/dXf [A] [-[Xc]x | I]; with p the row of d(u, v)/dXf (VIA_A: A^T times
  // it) the rotation part is Xc x p
  const double iz = 1.0 / z;
  double px[3] = {sx * fx * iz, 0.0, -sx * fx * Xf[0] * iz * iz};
  double py[3] = {0.0, sy * fy * iz, -sy * fy * Xf[1] * iz * iz};
  if constexpr (VIA_A) {
    const double qx[3] = {px[0], px[1], px[2]}, qy[3] = {py[0], py[1], py[2]};
    for (int i = 0; i < 3; ++i) {
      px[i] = A[i] * qx[0] + A[3 + i] * qx[1] + A[6 + i] * qx[2];
      py[i] = A[i] * qy[0] + A[3 + i] * qy[1] + A[6 + i] * qy[2];
    }
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
  acc[29] += 1.0;   // not the last statement: as the tail it is merged with the z-bad return's `acc[30] += 1.0` into one store with a
                    // variable index, and acc[28..31] leave the registers for scratch
  if constexpr (SIG2_COST) acc[27] += sig2 * log1p(q);
  else acc[27] += log1p(q);
}

// ---- the depth term of one point (sections 14 and 15), run by one lane: the vertex Xv under the pose (R, t) in detection b's frame
// camera.  acc arrives zeroed and leaves with the point's FP_DEPTH_TERMS values.  TAP_SPREAD: a point whose four taps spread over more
// than tau is not measurable (rgbd_refine.hip).
template <bool TAP_SPREAD>
FP_DEVICE void depth_point(const RefineDepthArgs& a, const double* cam, int b, const double* R, const double* t, const float* Xv,
                           double (&acc)[FP_DEPTH_TERMS]) {
  const double fx = cam[4 * b + 0], fy = cam[4 * b + 1], cx = cam[4 * b + 2], cy = cam[4 * b + 3];
  const double tau = a.tau[b];
  const double X[3] = {Xv[0], Xv[1], Xv[2]};
  double Xc[3];
  for (int i = 0; i < 3; ++i) Xc[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
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
    if constexpr (TAP_SPREAD) {
      const double hi = fmax(fmax(D00, D10), fmax(D01, D11)), lo = fmin(fmin(D00, D10), fmin(D01, D11));
      ok = ok && hi - lo <= tau;
    }
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

// ---- the host side: what a call enqueues, without a round trip between the launches
// one launch under the name its failure is reported by; `mode` goes to the kernels that take one
template <class Args, class... Mode>
int lm_launch(const char* name, void (*kernel)(Args, Mode...), dim3 grid, dim3 block, hipStream_t st, const Args& a, Mode... mode) {
  hipLaunchKernelGGL(kernel, grid, block, 0, st, a, mode...);
  FP_CHECK_LAUNCH(name);
  return FP_OK;
}
// setup, [init pass, sigma solve,] pass, first solve, iters x (pass, step solve), finalize: 3 + 2 iters + 1 launches, 5 + 2 iters + 1 with
// the sigma stage.  setup / finalize (grid, block) run one thread per problem, pass (grid, block, mode) a workgroup of pass_block threads
// per (chunk, problem), solve (grid, block, mode) one wave per problem; each returns its lm_launch.
template <class Setup, class Pass, class Solve, class Finalize>
int lm_enqueue(const RefineLmArgs& lm, int pass_block, bool sigma, Setup setup, Pass pass, Solve solve, Finalize finalize) {
  const dim3 pgrid(lm.chunks, lm.num_det), sgrid(lm.num_det), tgrid(cdiv(lm.num_det, 64)), wave(64), pblock(pass_block);
  if (int rc = setup(tgrid, wave)) return rc;
  if (sigma) {
    if (int rc = pass(pgrid, pblock, (int)MODE_INIT)) return rc;
    if (int rc = solve(sgrid, wave, (int)SOLVE_SIGMA)) return rc;
  }
  if (int rc = pass(pgrid, pblock, (int)MODE_EVAL)) return rc;
  if (int rc = solve(sgrid, wave, (int)SOLVE_FIRST)) return rc;
  for (int k = 0; k < lm.iters; ++k) {
    if (int rc = pass(pgrid, pblock, (int)MODE_EVAL)) return rc;
    if (int rc = solve(sgrid, wave, (int)SOLVE_STEP)) return rc;
  }
  return finalize(tgrid, wave);
}
