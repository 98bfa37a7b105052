// Frame-to-model tracking against a TSDF volume (reconstruct.py with pose_source "track"): Levenberg-Marquardt on
// the model -> camera pose that lays a frame's camera-frame depth points onto the zero level of the volume fp_tsdf_integrate has built
// so far.  The residual of a point is the trilinear sample of the volume at X_m = R^T (X_c - t), in mm (r = tau phi); the objective is
// section 14's truncated quadratic.  tests/tsdf_track_ref.py restates the contract in numpy fp64.
//
// Kernels, all enqueued by fp_tsdf_track without a host round trip between them:
//   tsdf_track_setup     one thread per problem: validates the row range, initialises the LM state (lm_setup, no image index)
//   tsdf_track_pass      (chunk of FP_REFINE_CHUNK points, problem), one wave: ONE POINT PER LANE -- the point into the model frame, the
//                        cell it falls into, eight sdf_cnt taps, then (only where all eight were seen min_count times) eight sdf_sum taps,
//                        the sample, its gradient and the Jacobian row (fp64; track_point) -- then a butterfly over the chunk's lanes for
//                        the 29 terms, one partial record per workgroup (lm_lane_pass).  The two x-neighbours of a tap pair are adjacent
//                        in memory.
//   tsdf_track_rgb_pass  fp_tsdf_track_rgb's pass (section 31; tests/tsdf_track_rgb_ref.py): the same point, and for a geometric inlier the
//                        colour term -- eight rgb_cnt taps once, then per channel eight rgb_sum taps of its plane, the sample, its gradient
//                        and the row, added to the same 29 terms.  Setup, solve and finalize are shared with fp_tsdf_track.
//   tsdf_track_solve     one wave per problem: folds the partials in chunk order, accepts / rejects the trial pose, solves for the next
//                        (lm_lane_solve)
//   tsdf_track_finalize  one thread per problem: the outputs (lm_finalize)
// A bad row range anywhere in the batch fails the whole call, as in the refiners; here the pass, the solve and the finalize then leave
// at their first instruction, so that such a call writes none of its outputs.
// The parts named in brackets and the order of the launches (lm_enqueue) live in refine_terms.hpp; the one-point-per-lane pass and its
// solve are the ones depth_refine.hip runs (same record layout, same cost normalisation, same stop on fewer than 6 inliers).  This file
// keeps what is the tracker's own: the per-point term, and the rule for a failed call -- the leading err test of its kernels, the
// setup that hides normal_eq from lm_setup and the finalize that zeroes the rows no solve has written.  Every floating-point statement
// of the term stands as one source expression (the library is built with -ffp-contract=on).  Every sum has a fixed order (lanes:
// butterfly; chunks: ascending), no atomics, and a problem's chunk decomposition depends only on its own point count: results are
// bit-identical across runs and batch compositions.
#include "common.hpp"
#include "kernels.hpp"
#include "refine_terms.hpp"

namespace {

// One camera-frame point Xv under the pose (R, t) against the volume.  acc arrives zeroed and leaves with the point's FP_DEPTH_TERMS
// values: H (21), g (6), rho [27], the inlier flag [28].  RGB: the colour term of section 31 follows the geometric part of an inlier (c
// is read with RGB only); without it the function is the geometric term, statement for statement.
template <bool RGB>
FP_DEVICE void track_point(const TsdfTrackArgs& a, const TsdfTrackRgbArgs* c, int b, const double* R, const double* t, const float* Xv,
                           double (&acc)[FP_DEPTH_TERMS]) {
  const double md = a.max_dist[b], tau = a.tau, h = a.vol.h;
  const double Xc[3] = {Xv[0], Xv[1], Xv[2]};
  const double d0 = Xc[0] - t[0], d1 = Xc[1] - t[1], d2 = Xc[2] - t[2];
  double Xm[3];
  for (int i = 0; i < 3; ++i) Xm[i] = R[i] * d0 + R[3 + i] * d1 + R[6 + i] * d2;
  const double gx = (Xm[0] - a.vol.ox) / h - 0.5, gy = (Xm[1] - a.vol.oy) / h - 0.5, gz = (Xm[2] - a.vol.oz) / h - 0.5;
  // measurable: the cell's lower corner floor(g) lies in [0, n - 2] on every axis (a NaN or an infinity compares false), decided in fp64
  // before any conversion or read, and all eight corners were seen min_count times
  bool ok = gx >= 0.0 && gx < (double)(a.vol.nx - 1) && gy >= 0.0 && gy < (double)(a.vol.ny - 1) && gz >= 0.0 && gz < (double)(a.vol.nz - 1);
  double rho = md * md;
  double rc[3];   // RGB: rho per channel, (lambda color_max)^2 until the channel proves an inlier
  if constexpr (RGB) {
    const double lc = c->color_weight * c->color_max;
    rc[0] = rc[1] = rc[2] = lc * lc;
  }
  if (ok) {
    const int i0 = (int)floor(gx), j0 = (int)floor(gy), k0 = (int)floor(gz);
    const double ax = gx - i0, ay = gy - j0, az = gz - k0;
    const long long sy = a.vol.nx, sz = (long long)a.vol.nx * a.vol.ny;
    const long long base = (long long)k0 * sz + (long long)j0 * sy + i0;
    const int* c0 = a.sdf_cnt + base;
    const int n0 = c0[0], n1 = c0[1], n2 = c0[sy], n3 = c0[sy + 1], n4 = c0[sz], n5 = c0[sz + 1], n6 = c0[sz + sy], n7 = c0[sz + sy + 1];
    const int mc = a.min_count;
    ok = n0 >= mc && n1 >= mc && n2 >= mc && n3 >= mc && n4 >= mc && n5 >= mc && n6 >= mc && n7 >= mc;
    if (ok) {   // only now is sdf_sum read
      const float* s0 = a.sdf_sum + base;
      const double f0 = (double)s0[0] / (double)n0, f1 = (double)s0[1] / (double)n1, f2 = (double)s0[sy] / (double)n2, f3 = (double)s0[sy + 1] / (double)n3;
      const double f4 = (double)s0[sz] / (double)n4, f5 = (double)s0[sz + 1] / (double)n5, f6 = (double)s0[sz + sy] / (double)n6, f7 = (double)s0[sz + sy + 1] / (double)n7;
      // x first, then y, then z
      const double c00 = (1.0 - ax) * f0 + ax * f1, c10 = (1.0 - ax) * f2 + ax * f3, c01 = (1.0 - ax) * f4 + ax * f5, c11 = (1.0 - ax) * f6 + ax * f7;
      const double phi = (1.0 - az) * ((1.0 - ay) * c00 + ay * c10) + az * ((1.0 - ay) * c01 + ay * c11);
      const double r = tau * phi;
      if (fabs(r) < md) {   // an inlier: the only points with a gradient
        // the exact gradient of the interpolant: the four differences along an axis, bilinear over the other two, over h
        const double px = ((1.0 - az) * ((1.0 - ay) * (f1 - f0) + ay * (f3 - f2)) + az * ((1.0 - ay) * (f5 - f4) + ay * (f7 - f6))) / h;
        const double py = ((1.0 - az) * ((1.0 - ax) * (f2 - f0) + ax * (f3 - f1)) + az * ((1.0 - ax) * (f6 - f4) + ax * (f7 - f5))) / h;
        const double pz = ((1.0 - ay) * ((1.0 - ax) * (f4 - f0) + ax * (f5 - f1)) + ay * ((1.0 - ax) * (f6 - f2) + ax * (f7 - f3))) / h;
        // q = tau R grad phi, the gradient in the camera frame.  Under the left twist (w, v) of lm_propose the model point moves by
        // R^T (X_c x w - v), so dr = w . (q x X_c) - q . v
        double q[3], J[6];
        for (int i = 0; i < 3; ++i) q[i] = tau * (R[3 * i] * px + R[3 * i + 1] * py + R[3 * i + 2] * pz);
        cross3(q, Xc, J);
        for (int i = 0; i < 3; ++i) J[3 + i] = -q[i];
        int k2 = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = i; j < 6; ++j, ++k2) acc[k2] = J[i] * J[j];
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[21 + i] = J[i] * r;
        rho = r * r;
        acc[28] = 1.0;
        if constexpr (RGB) {
          // the colour term: eight rgb_cnt taps once, then one channel after the other -- eight rgb_sum taps of its plane, the sample,
          // its gradient, the row -- so that one channel's corner values are live at a time
          const int* w0 = c->rgb_cnt + base;
          const int m0 = w0[0], m1 = w0[1], m2 = w0[sy], m3 = w0[sy + 1], m4 = w0[sz], m5 = w0[sz + 1], m6 = w0[sz + sy], m7 = w0[sz + sy + 1];
          if (m0 >= mc && m1 >= mc && m2 >= mc && m3 >= mc && m4 >= mc && m5 >= mc && m6 >= mc && m7 >= mc) {   // only now is rgb_sum read
            const double lam = c->color_weight, cmax = c->color_max;
            const float* cp = c->colors + (Xv - a.lm.verts);   // the row of colors that belongs to this row of points
            const long long plane = sz * a.vol.nz;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const float* u0 = c->rgb_sum + ch * plane + base;
              const double e0 = (double)u0[0] / (double)m0, e1 = (double)u0[1] / (double)m1, e2 = (double)u0[sy] / (double)m2, e3 = (double)u0[sy + 1] / (double)m3;
              const double e4 = (double)u0[sz] / (double)m4, e5 = (double)u0[sz + 1] / (double)m5, e6 = (double)u0[sz + sy] / (double)m6, e7 = (double)u0[sz + sy + 1] / (double)m7;
              const double d00 = (1.0 - ax) * e0 + ax * e1, d10 = (1.0 - ax) * e2 + ax * e3, d01 = (1.0 - ax) * e4 + ax * e5, d11 = (1.0 - ax) * e6 + ax * e7;
              const double C = (1.0 - az) * ((1.0 - ay) * d00 + ay * d10) + az * ((1.0 - ay) * d01 + ay * d11);
              const double e = C - (double)cp[ch];
              if (fabs(e) < cmax) {   // a channel inlier (a NaN compares false)
                const double ux = ((1.0 - az) * ((1.0 - ay) * (e1 - e0) + ay * (e3 - e2)) + az * ((1.0 - ay) * (e5 - e4) + ay * (e7 - e6))) / h;
                const double uy = ((1.0 - az) * ((1.0 - ax) * (e2 - e0) + ax * (e3 - e1)) + az * ((1.0 - ax) * (e6 - e4) + ax * (e7 - e5))) / h;
                const double uz = ((1.0 - ay) * ((1.0 - ax) * (e4 - e0) + ax * (e5 - e1)) + ay * ((1.0 - ax) * (e6 - e2) + ax * (e7 - e3))) / h;
                // q = lambda R grad C: the point carries its own colour, only the volume sample moves with the pose -- the geometric row's form
                double qc[3], Jc[6];
                for (int i = 0; i < 3; ++i) qc[i] = lam * (R[3 * i] * ux + R[3 * i + 1] * uy + R[3 * i + 2] * uz);
                cross3(qc, Xc, Jc);
                for (int i = 0; i < 3; ++i) Jc[3 + i] = -qc[i];
                const double rl = lam * e;
                int k3 = 0;
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                  for (int j = i; j < 6; ++j, ++k3) acc[k3] += Jc[i] * Jc[j];
#pragma unroll
                for (int i = 0; i < 6; ++i) acc[21 + i] += Jc[i] * rl;
                rc[ch] = rl * rl;
              }
            }
          }
        }
      }
    }
  }
  if constexpr (RGB) acc[27] = ((rho + rc[0]) + rc[1]) + rc[2];
  else acc[27] = rho;
}

__global__ void __launch_bounds__(64) tsdf_track_setup_kernel(TsdfTrackArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  RefineLmArgs lm = a.lm;
  lm.normal_eq = nullptr;   // a call with a bad row range writes none of its outputs: the finalize zeroes the rows no solve has written
  if (b < lm.num_det) lm_setup(lm, nullptr, a.state[b], b, 28);
}

// The leading test of the three kernels below: a bad row range somewhere in the batch (err, set by the setup a launch ago) fails the
// call, and nothing is computed.
__global__ void __launch_bounds__(64) tsdf_track_pass_kernel(TsdfTrackArgs a) {
  if (a.lm.err[0] != 0) return;
  const int b = blockIdx.y;
  lm_lane_pass(a.lm, a.state[b], b,
               [&](const double* R, const double* t, const float* Xv, double (&acc)[FP_DEPTH_TERMS]) { track_point<false>(a, nullptr, b, R, t, Xv, acc); });
}

// the same pass with the colour term; setup, solve and finalize are the geometric call's
__global__ void __launch_bounds__(64) tsdf_track_rgb_pass_kernel(TsdfTrackRgbArgs a) {
  if (a.g.lm.err[0] != 0) return;
  const int b = blockIdx.y;
  lm_lane_pass(a.g.lm, a.g.state[b], b,
               [&](const double* R, const double* t, const float* Xv, double (&acc)[FP_DEPTH_TERMS]) { track_point<true>(a.g, &a, b, R, t, Xv, acc); });
}

__global__ void __launch_bounds__(64) tsdf_track_solve_kernel(TsdfTrackArgs a, int mode) {
  __shared__ double tot[FP_REFINE_RECORD];
  if (a.lm.err[0] != 0) return;
  lm_lane_solve(a.lm, a.state[blockIdx.x], blockIdx.x, mode, tot);
}

__global__ void __launch_bounds__(64) tsdf_track_finalize_kernel(TsdfTrackArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (a.lm.err[0] != 0 || b >= a.lm.num_det) return;
  if (a.lm.normal_eq && a.state[b].np == 0)   // no pose or an empty range: no solve ran
    for (int i = 0; i < 28; ++i) a.lm.normal_eq[28 * b + i] = 0.0;
  lm_finalize(a.lm, a.state[b], b);
}

}  // namespace

int launch_tsdf_track(const TsdfTrackArgs& a, hipStream_t st) {
  return lm_enqueue(a.lm, 64, false,   // no sigma stage
                    [&](dim3 g, dim3 blk) { return lm_launch("tsdf_track_setup", tsdf_track_setup_kernel, g, blk, st, a); },
                    [&](dim3 g, dim3 blk, int) { return lm_launch("tsdf_track_pass", tsdf_track_pass_kernel, g, blk, st, a); },
                    [&](dim3 g, dim3 blk, int mode) { return lm_launch("tsdf_track_solve", tsdf_track_solve_kernel, g, blk, st, a, mode); },
                    [&](dim3 g, dim3 blk) { return lm_launch("tsdf_track_finalize", tsdf_track_finalize_kernel, g, blk, st, a); });
}

int launch_tsdf_track_rgb(const TsdfTrackRgbArgs& a, hipStream_t st) {
  return lm_enqueue(a.g.lm, 64, false,
                    [&](dim3 g, dim3 blk) { return lm_launch("tsdf_track_setup", tsdf_track_setup_kernel, g, blk, st, a.g); },
                    [&](dim3 g, dim3 blk, int) { return lm_launch("tsdf_track_rgb_pass", tsdf_track_rgb_pass_kernel, g, blk, st, a); },
                    [&](dim3 g, dim3 blk, int mode) { return lm_launch("tsdf_track_solve", tsdf_track_solve_kernel, g, blk, st, a.g, mode); },
                    [&](dim3 g, dim3 blk) { return lm_launch("tsdf_track_finalize", tsdf_track_finalize_kernel, g, blk, st, a.g); });
}
