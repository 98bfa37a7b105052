// Hypothesis verification against depth (coarse_select_type "depth_verify"): the whole model's point sample placed at
// the coarse pose of a (detection, template slot) pair, its visibility decided by a coarse z-buffer of the sample itself, and every visible
// point classified against the frame's depth image.  This stage is the project's own; the reference keeps the hypothesis with the most
// correspondence inliers.
//   set-up  R_f = A R, t_f = A t (solve camera -> frame camera); the model's bounding sphere (c, rho) projected to a square of side
//           2 r_px around (u_c, v_c), divided into G x G cells;
//   pass 1  every sampled point -> its cell; zbuf[cell] = min(zbuf[cell], fl32(z)) by an LDS integer atomic-min on the fp32 bits (positive
//           floats order like their bit patterns: the minimum does not depend on the order of arrival);
//   pass 2  the transform again (no projections are stored); visible iff z <= zbuf[cell] + tau; a visible point is outside the image, on a
//           hole, an inlier (|D - z| <= tau), occluded (D - z < -tau) or in free space (D - z > tau).
// One 256-thread workgroup per pair; fp64, every step one rounded operation in the order section 17 states (FMA contraction off), points
// stored as fp32.  The outputs are integer counts and one quotient of two of them: a pair's result depends on its own data only.
#include "common.hpp"
#include "kernels.hpp"
#include "verify_grid.hpp"  // FramePose, CellGrid, to_camera, project: shared with mask_verify.hip

namespace {

constexpr int PV_COUNTS = 6;  // n_vis, n_in, n_occ, n_free, n_hole, n_out

__global__ __launch_bounds__(PV_THREADS) void pose_verify_depth_kernel(VerifyArgs a) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* zbuf = reinterpret_cast<unsigned*>(smem);        // [G * G] fp32 bits of the nearest z per cell
  int* total = reinterpret_cast<int*>(zbuf + a.grid * a.grid);  // [8] the six counts of the pair

  const int pair = blockIdx.x, tid = threadIdx.x;
  const int det = pair / a.n_slots;
  auto finish = [&](int status) {  // block-uniform: zero counts, zero score
    if (tid == 0) {
      for (int k = 0; k < PV_COUNTS; ++k) a.counts[(size_t)pair * PV_COUNTS + k] = 0;
      a.score[pair] = 0.0;
      a.status[pair] = status;
    }
  };
  const int image = a.image_index[det];
  const double tau = a.tau[det];
  if (image < 0 || image >= a.num_images || !(tau > 0.0 && tau < __builtin_inf())) { finish(-1); return; }  // the image is never read
  const int begin = min(max(a.ranges[det * 2 + 0], 0), a.m_total), end = min(max(a.ranges[det * 2 + 1], 0), a.m_total);
  if (a.success[pair] <= 0 || begin >= end) { finish(2); return; }

  // ---- set-up (every thread, from block-uniform data)
  FramePose P;
  {
    const double* A = a.A + (size_t)det * 9;
    const double* R = a.R + (size_t)pair * 9;
    const double* t = a.t + (size_t)pair * 3;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) P.R[i * 3 + j] = (A[i * 3 + 0] * R[0 * 3 + j] + A[i * 3 + 1] * R[1 * 3 + j]) + A[i * 3 + 2] * R[2 * 3 + j];
      P.t[i] = (A[i * 3 + 0] * t[0] + A[i * 3 + 1] * t[1]) + A[i * 3 + 2] * t[2];
    }
  }
  CellGrid g;
  g.fx = a.cam[det * 4 + 0]; g.fy = a.cam[det * 4 + 1]; g.cx = a.cam[det * 4 + 2]; g.cy = a.cam[det * 4 + 3];
  g.G = a.grid;
  {
    const double c[3] = {a.center[det * 3 + 0], a.center[det * 3 + 1], a.center[det * 3 + 2]};
    const double rho = a.radius[det];
    double C[3];
    to_camera(P, c, C);
    if (!(C[2] > rho + 1.0)) { finish(2); return; }  // (a NaN pose ends here too)
    const double uc = g.fx * C[0] / C[2] + g.cx, vc = g.fy * C[1] / C[2] + g.cy;
    const double rpx = fmax(g.fx, g.fy) * rho / (C[2] - rho);
    g.u0 = uc - rpx;
    g.v0 = vc - rpx;
    g.h = 2.0 * rpx / (double)g.G;
  }

  for (int i = tid; i < g.G * g.G; i += PV_THREADS) zbuf[i] = 0x7f800000u;  // +inf
  if (tid < 8) total[tid] = 0;
  __syncthreads();

  // ---- pass 1: the z-buffer of the sample
  for (int p = begin + tid; p < end; p += PV_THREADS) {
    const double X[3] = {(double)a.points[(size_t)p * 3 + 0], (double)a.points[(size_t)p * 3 + 1], (double)a.points[(size_t)p * 3 + 2]};
    double Xc[3], u, v;
    to_camera(P, X, Xc);
    if (!(Xc[2] > 1.0)) continue;
    const int cell = project(g, Xc, &u, &v);
    atomicMin(&zbuf[cell], __float_as_uint((float)Xc[2]));
  }
  __syncthreads();

  // ---- pass 2: visibility and the depth test
  const float* img = a.depth + (size_t)image * a.H * a.W;
  int n[PV_COUNTS] = {0, 0, 0, 0, 0, 0};
  for (int p = begin + tid; p < end; p += PV_THREADS) {
    const double X[3] = {(double)a.points[(size_t)p * 3 + 0], (double)a.points[(size_t)p * 3 + 1], (double)a.points[(size_t)p * 3 + 2]};
    double Xc[3], u, v;
    to_camera(P, X, Xc);
    if (!(Xc[2] > 1.0)) continue;
    const int cell = project(g, Xc, &u, &v);
    if (!(Xc[2] <= (double)__uint_as_float(zbuf[cell]) + tau)) continue;
    n[0] += 1;
    const double px = rint(u), py = rint(v);  // half to even
    if (!(px >= 0.0 && px <= (double)(a.W - 1) && py >= 0.0 && py <= (double)(a.H - 1))) { n[5] += 1; continue; }  // no tap outside the image
    const float D = img[(size_t)(int)py * a.W + (int)px];
    if (!(D > 0.f)) { n[4] += 1; continue; }
    const double r = (double)D - Xc[2];
    if (fabs(r) <= tau) n[1] += 1;
    else if (r < 0.0) n[2] += 1;
    else n[3] += 1;
  }
#pragma unroll
  for (int k = 0; k < PV_COUNTS; ++k) {
    int s = n[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) atomicAdd(&total[k], s);
  }
  __syncthreads();
  if (tid == 0) {
    const int n_vis = total[0];
    for (int k = 0; k < PV_COUNTS; ++k) a.counts[(size_t)pair * PV_COUNTS + k] = total[k];
    const bool scored = n_vis >= a.min_visible;
    a.score[pair] = scored ? (double)total[1] / (double)n_vis : 0.0;
    a.status[pair] = scored ? 0 : 1;
  }
}

}  // namespace

int launch_pose_verify_depth(const VerifyArgs& a, int num_pairs, hipStream_t st) {
  FP_REQUIRE(a.grid >= PV_MIN_GRID && a.grid <= PV_MAX_GRID, "pose_verify_depth: grid must be in [%d, %d] (got %d)", PV_MIN_GRID, PV_MAX_GRID, a.grid);
  FP_REQUIRE(a.n_slots >= 1 && a.min_visible >= 1, "pose_verify_depth: bad n_slots / min_visible");
  FP_REQUIRE(a.m_total >= 0 && a.m_total <= (1 << 30), "pose_verify_depth: %d sampled points (at most 2^30: the point loops count in int)", a.m_total);
  FP_REQUIRE(a.num_images >= 1 && a.H >= 1 && a.W >= 1, "pose_verify_depth: %d depth images of %d x %d", a.num_images, a.W, a.H);
  if (num_pairs == 0) return FP_OK;
  const size_t lds = ((size_t)a.grid * a.grid + 8) * 4;
  static FpDeviceOnce attr;  // G = 128 asks for 64 KB + 32 B, above the default limit of dynamic LDS: raised once per device, and checked
  if (fp_first_on_device(attr)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pose_verify_depth_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (PV_MAX_GRID * PV_MAX_GRID + 8) * 4);
    FP_REQUIRE(e == hipSuccess, "pose_verify_depth: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(pose_verify_depth_kernel, dim3(num_pairs), dim3(PV_THREADS), lds, st, a);
  FP_CHECK_LAUNCH("pose_verify_depth");
  return FP_OK;
}
