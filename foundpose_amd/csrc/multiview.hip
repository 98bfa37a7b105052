// Multi-view pose consensus (foundpose_amd/multiview.py): Levenberg-Marquardt on the model -> WORLD pose of a scene
// object that several calibrated views have estimated.  A row is a (member view, model point) pair: the pixel the member's own estimate
// projects the point to is a virtual observation of the point in that view, and the objective is the Huber-robust reprojection error of
// the world pose over all rows.  No image is read.  tests/multiview_ref.py restates the contract in numpy fp64.
//
// Kernels, all enqueued by fp_multiview_refine without a host round trip between them:
//   multiview_setup     one wave per problem: lane 0 validates the row range and initialises the LM state (lm_setup, no image index), then
//                       the wave checks the view index of every row of the range
//   multiview_pass      (chunk of FP_REFINE_CHUNK rows, problem), one wave: ONE ROW PER LANE -- the point into the world, into its view's
//                       camera, the residual against the target pixel, the Huber weight and the two Jacobian rows (fp64; view_point) --
//                       then a butterfly over the chunk's lanes for the 29 terms, one partial record per workgroup (lm_lane_pass)
//   multiview_solve     one wave per problem: folds the partials in chunk order, accepts / rejects the trial pose, solves for the next
//                       (lm_lane_solve)
//   multiview_finalize  one thread per problem: the outputs (lm_finalize)
// A bad row range or view index anywhere in the batch fails the whole call, as in tsdf_track.hip: the pass, the solve and the finalize
// then leave at their first instruction, so that such a call writes none of its outputs and reads no table row that does not exist.
// The parts named in brackets and the order of the launches (lm_enqueue) live in refine_terms.hpp; the pass and its solve are the ones
// depth_refine.hip and tsdf_track.hip run (same record layout, same cost normalisation, same stop on fewer than 6 inliers).  This file
// keeps what is its own: the per-row term and the view check.  Every floating-point statement of the term stands as one source
// expression (the library is built with -ffp-contract=on).  Every sum has a fixed order (lanes: butterfly; chunks: ascending), no
// atomics, and a problem's chunk decomposition depends only on its own row count: results are bit-identical across runs and batch
// compositions.
#include "common.hpp"
#include "kernels.hpp"
#include "refine_terms.hpp"

namespace {

// One row -- the model point Xv, its view and target -- under the world pose (R, t).  acc arrives zeroed and leaves with the row's
// FP_DEPTH_TERMS values: H (21), g (6), rho [27], the inlier flag [28].
FP_DEVICE void view_point(const MultiviewArgs& a, const double* R, const double* t, const float* Xv, double (&acc)[FP_DEPTH_TERMS]) {
  const long long row = (Xv - a.lm.verts) / 3;
  const double* cam = a.view_cam + 4 * (long long)a.view[row];
  const double* T = a.view_T + 12 * (long long)a.view[row];
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
  const double delta = a.delta;
  const double X[3] = {Xv[0], Xv[1], Xv[2]};
  double Xw[3], Xc[3];
  for (int i = 0; i < 3; ++i) Xw[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
  for (int i = 0; i < 3; ++i) Xc[i] = T[3 * i] * Xw[0] + T[3 * i + 1] * Xw[1] + T[3 * i + 2] * Xw[2] + T[9 + i];
  const double z = Xc[2], iz = 1.0 / z;
  const double e0 = fx * Xc[0] / z + cx - a.target[2 * row], e1 = fy * Xc[1] / z + cy - a.target[2 * row + 1];
  const double s = e0 * e0 + e1 * e1;
  double rho = delta * delta;
  if (z > 1.0) {   // measurable (a NaN compares false); there is no image-bounds test: a target outside the picture is a valid observation
    const double rs = sqrt(s);
    const bool inl = rs <= delta;
    const double w = inl ? 1.0 : delta / rs;
    // d(u, v)/dXw: the rows px, py of d(u, v)/dXc times R_v, i.e. R_v^T p; J = q^T [-[Xw]x | I]: the rotation part is Xw x q
    const double px[3] = {fx * iz, 0.0, -fx * Xc[0] * iz * iz}, py[3] = {0.0, fy * iz, -fy * Xc[1] * iz * iz};
    double Jx[6], Jy[6];
    for (int i = 0; i < 3; ++i) {
      Jx[3 + i] = T[i] * px[0] + T[3 + i] * px[1] + T[6 + i] * px[2];
      Jy[3 + i] = T[i] * py[0] + T[3 + i] * py[1] + T[6 + i] * py[2];
    }
    cross3(Xw, Jx + 3, Jx);
    cross3(Xw, Jy + 3, Jy);
    int k2 = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++k2) acc[k2] = w * (Jx[i] * Jx[j] + Jy[i] * Jy[j]);
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] = w * (Jx[i] * e0 + Jy[i] * e1);
    rho = inl ? s : 2.0 * delta * rs - delta * delta;
    acc[28] = inl ? 1.0 : 0.0;
  }
  acc[27] = rho;
}

// grid: one wave per problem.  A view index outside the tables sets err to -(b + 1), as a bad image index does in the refiners.
__global__ void __launch_bounds__(64) multiview_setup_kernel(MultiviewArgs a) {
  __shared__ int range[2];
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    RefineLmArgs lm = a.lm;
    lm.normal_eq = nullptr;   // a refused call writes none of its outputs: the finalize zeroes the rows no solve has written
    lm_setup(lm, nullptr, a.state[b], b, 28);
    range[0] = a.state[b].p0;
    range[1] = a.state[b].np;   // 0 for a problem without a pose or with a bad range: none of its rows is read
  }
  __syncthreads();
  bool bad = false;
  for (int p = threadIdx.x; p < range[1]; p += 64) {
    const int v = a.view[(long long)range[0] + p];
    bad = bad || v < 0 || v >= a.num_views;
  }
  if (bad) a.lm.err[0] = -(b + 1);
}

// The leading test of the three kernels below: a bad row range or view index somewhere in the batch (err, set by the setup a launch
// ago) fails the call, and nothing is computed.
__global__ void __launch_bounds__(64) multiview_pass_kernel(MultiviewArgs a) {
  if (a.lm.err[0] != 0) return;
  const int b = blockIdx.y;
  lm_lane_pass(a.lm, a.state[b], b,
               [&](const double* R, const double* t, const float* Xv, double (&acc)[FP_DEPTH_TERMS]) { view_point(a, R, t, Xv, acc); });
}

__global__ void __launch_bounds__(64) multiview_solve_kernel(MultiviewArgs a, int mode) {
  __shared__ double tot[FP_REFINE_RECORD];
  if (a.lm.err[0] != 0) return;
  lm_lane_solve(a.lm, a.state[blockIdx.x], blockIdx.x, mode, tot);
}

__global__ void __launch_bounds__(64) multiview_finalize_kernel(MultiviewArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (a.lm.err[0] != 0 || b >= a.lm.num_det) return;
  if (a.lm.normal_eq && a.state[b].np == 0)   // no pose or an empty range: no solve ran
    for (int i = 0; i < 28; ++i) a.lm.normal_eq[28 * b + i] = 0.0;
  lm_finalize(a.lm, a.state[b], b);
}

}  // namespace

int launch_multiview_refine(const MultiviewArgs& a, hipStream_t st) {
  return lm_enqueue(a.lm, 64, false,   // no sigma stage
                    [&](dim3, dim3 blk) { return lm_launch("multiview_setup", multiview_setup_kernel, dim3(a.lm.num_det), blk, st, a); },
                    [&](dim3 g, dim3 blk, int) { return lm_launch("multiview_pass", multiview_pass_kernel, g, blk, st, a); },
                    [&](dim3 g, dim3 blk, int mode) { return lm_launch("multiview_solve", multiview_solve_kernel, g, blk, st, a, mode); },
                    [&](dim3 g, dim3 blk) { return lm_launch("multiview_finalize", multiview_finalize_kernel, g, blk, st, a); });
}
