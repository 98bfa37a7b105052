// Hypothesis verification against the detection's mask (coarse_select_type "mask_verify"): the whole model's point
// sample placed at the coarse pose of a (detection, template slot) pair, the cells of a G x G grid it projects into taken as the model's
// silhouette, and that silhouette compared pixel by pixel with the detection's segmentation mask.  This stage is the project's own; the
// reference keeps the hypothesis with the most correspondence inliers.
//   set-up  section 17's: R_f = A R, t_f = A t; the model's bounding sphere (c, rho) projected to a square of side 2 r_px around (u_c, v_c),
//           divided into G x G cells (verify_grid.hpp);
//   pass 1  every sampled point with z > 1 -> its cell; bit `cell` of an occupancy bitmap in LDS is set by an integer atomic-or (the result
//           does not depend on the order of arrival).  No z-buffer: every point of the model projects inside its silhouette;
//   pass 2  every pixel of a rectangle that contains the square's part of the image: a pixel whose (unclamped) cell lies in the grid and has
//           its bit set is a model pixel, counted in n_both (mask set) or n_model_only (mask clear).
// One 256-thread workgroup per pair; fp64, every step one rounded operation in the order section 18 states (FMA contraction off), points
// stored as fp32.  The outputs are integer counts and one quotient of two of them: a pair's result depends on its own data only.
#include "common.hpp"
#include "kernels.hpp"
#include "verify_grid.hpp"

namespace {

constexpr int MV_COUNTS = 4;                                        // n_both, n_model_only, n_mask_only, n_cells
constexpr int MV_MAX_WORDS = (PV_MAX_GRID * PV_MAX_GRID + 31) / 32;  // 512 words = 2 KB

// the integer range [lo, hi] of pixel coordinates that contains every pixel p in [0, size) with 0 <= floor((p - e0) / h) < G, where
// side = 2 r_px = G h up to rounding.  Such a pixel has e0 <= p < e0 + side up to the rounding of three operations (a few 2^-53 of
// |e0| + side); the range is widened by pad = 2 + 2^-40 (|e0| + side), a million times that, and clamped to the image in fp64 before it
// becomes integers (fmax / fmin drop a NaN: the range is then empty or the whole image, and pass 2's own test decides every pixel).
FP_DEVICE void pixel_range(double e0, double side, int size, int* lo, int* hi) {
#pragma clang fp contract(off)
  const double pad = 2.0 + 0x1p-40 * (fabs(e0) + side);
  *lo = (int)fmin(fmax(floor(e0 - pad), 0.0), (double)size);
  *hi = (int)fmin(fmax(ceil((e0 + side) + pad), -1.0), (double)(size - 1));
}

__global__ __launch_bounds__(PV_THREADS) void pose_verify_mask_kernel(MaskVerifyArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned bits[MV_MAX_WORDS];  // bit (cell & 31) of word (cell >> 5): a sampled point projects into the cell
  __shared__ int total[4];                 // n_both, n_model_only, n_cells

  const int pair = blockIdx.x, tid = threadIdx.x;
  const int det = pair / a.n_slots;
  auto finish = [&](int status) {  // block-uniform: zero counts, zero score
    if (tid == 0) {
      for (int k = 0; k < MV_COUNTS; ++k) a.counts[(size_t)pair * MV_COUNTS + k] = 0;
      a.score[pair] = 0.0;
      a.status[pair] = status;
    }
  };
  const int begin = min(max(a.ranges[det * 2 + 0], 0), a.m_total), end = min(max(a.ranges[det * 2 + 1], 0), a.m_total);
  if (a.success[pair] <= 0 || begin >= end) { finish(2); return; }

  // ---- set-up (every thread, from block-uniform data)
  FramePose P;
  frame_pose(a.A + (size_t)det * 9, a.R + (size_t)pair * 9, a.t + (size_t)pair * 3, P);
  CellGrid g;
  double rpx;
  {
    const double c[3] = {a.center[det * 3 + 0], a.center[det * 3 + 1], a.center[det * 3 + 2]};
    if (!sphere_grid(P, a.cam + (size_t)det * 4, c, a.radius[det], a.grid, g, &rpx)) { finish(2); return; }  // (a NaN pose ends here too)
  }
  const int G = g.G, words = (G * G + 31) >> 5;

  for (int i = tid; i < words; i += PV_THREADS) bits[i] = 0u;
  if (tid < 4) total[tid] = 0;
  __syncthreads();

  // ---- pass 1: the occupancy bitmap of the sample
  for (int p = begin + tid; p < end; p += PV_THREADS) {
    const double X[3] = {(double)a.points[(size_t)p * 3 + 0], (double)a.points[(size_t)p * 3 + 1], (double)a.points[(size_t)p * 3 + 2]};
    double Xc[3], u, v;
    to_camera(P, X, Xc);
    if (!(Xc[2] > 1.0)) continue;
    const int cell = project(g, Xc, &u, &v);  // in [0, G * G): clamped
    atomicOr(&bits[cell >> 5], 1u << (cell & 31));
  }
  __syncthreads();

  // ---- pass 2: the pixels of the square against the mask, lanes along px
  int x_lo, x_hi, y_lo, y_hi;
  pixel_range(g.u0, 2.0 * rpx, a.W, &x_lo, &x_hi);
  pixel_range(g.v0, 2.0 * rpx, a.H, &y_lo, &y_hi);
  const int nx = x_hi - x_lo + 1, ny = y_hi - y_lo + 1;  // each at most W / H: the product fits (the host bounds H * W)
  const int npix = (nx > 0 && ny > 0) ? nx * ny : 0;
  const unsigned char* mask = a.masks + (size_t)det * a.H * a.W;
  const double dG = (double)G;
  int n[3] = {0, 0, 0};
  for (int i = tid; i < npix; i += PV_THREADS) {
    const int row = i / nx;
    const int px = x_lo + (i - row * nx), py = y_lo + row;  // inside [0, W) x [0, H) by the clamps of pixel_range
    const double qx = floor(((double)px - g.u0) / g.h), qy = floor(((double)py - g.v0) / g.h);
    if (!(qx >= 0.0 && qx < dG && qy >= 0.0 && qy < dG)) continue;  // not in the square (a NaN is not)
    const int cell = (int)qy * G + (int)qx;
    if (!((bits[cell >> 5] >> (cell & 31)) & 1u)) continue;
    if (mask[(size_t)py * a.W + px] != 0) n[0] += 1;
    else n[1] += 1;
  }
  for (int i = tid; i < words; i += PV_THREADS) n[2] += __popc(bits[i]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int s = n[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) atomicAdd(&total[k], s);
  }
  __syncthreads();
  if (tid == 0) {
    const int n_both = total[0], n_model_only = total[1];
    const int n_mask_only = a.area[det] - n_both;
    a.counts[(size_t)pair * MV_COUNTS + 0] = n_both;
    a.counts[(size_t)pair * MV_COUNTS + 1] = n_model_only;
    a.counts[(size_t)pair * MV_COUNTS + 2] = n_mask_only;
    a.counts[(size_t)pair * MV_COUNTS + 3] = total[2];
    const bool scored = n_both + n_model_only >= a.min_pixels;
    const long long uni = (long long)n_both + n_model_only + n_mask_only;
    a.score[pair] = scored ? (double)n_both / (double)uni : 0.0;
    a.status[pair] = scored ? 0 : 1;
  }
}

}  // namespace

int launch_pose_verify_mask(const MaskVerifyArgs& a, int num_pairs, hipStream_t st) {
  FP_REQUIRE(a.grid >= PV_MIN_GRID && a.grid <= PV_MAX_GRID, "pose_verify_mask: grid must be in [%d, %d] (got %d)", PV_MIN_GRID, PV_MAX_GRID, a.grid);
  FP_REQUIRE(a.n_slots >= 1 && a.min_pixels >= 1, "pose_verify_mask: bad n_slots / min_pixels");
  FP_REQUIRE(a.m_total >= 0 && a.m_total <= (1 << 30), "pose_verify_mask: %d sampled points (at most 2^30: the point loop counts in int)", a.m_total);
  FP_REQUIRE(a.H >= 1 && a.W >= 1 && (long long)a.H * a.W <= (1ll << 30), "pose_verify_mask: masks of %d x %d (at least 1 x 1, at most 2^30 pixels: the pixel loop counts in int)", a.W, a.H);
  if (num_pairs == 0) return FP_OK;
  hipLaunchKernelGGL(pose_verify_mask_kernel, dim3(num_pairs), dim3(PV_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("pose_verify_mask");
  return FP_OK;
}
