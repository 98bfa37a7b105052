// Ground-truth annotations from renders (bop_toolkit's calc_gt_info.py and calc_gt_masks.py with
// visibility.estimate_visib_mask_gt(..., visib_mode='bop19') and misc.depth_im_to_dist_im_fast), a batch of instances per call.
//
// An instance is rendered into a window of render_width x render_height that holds the image at offset (ox, oy); per pixel
// (cr, rr) of its scan box, in render coordinates:
//   obj_large = depth_obj > 0                     -> px_count_all, the silhouette box in IMAGE coordinates (cr - ox, rr - oy)
//   inside the image window, col = cr - ox, row = rr - oy, fp64, every operation rounded on its own (bop_dist.hpp):
//     xs = (col - cx) / fx, ys = (row - cy) / fy, dist(d) = sqrt(((xs d)^2 + (ys d)^2) + d^2)
//     mask  = dist_obj > 0                                                                  -> mask, 255 / 0
//     valid = mask && dist_test > 0                                                         -> px_count_valid
//     visib = ((float)dist_obj - (float)dist_test <= (float)delta || dist_test == 0) && dist_obj > 0
//                                                                                           -> px_count_visib, the visible box, mask_visib
// A render depth of +-0 has dist 0 exactly and is in no mask: its two bytes are stored without any arithmetic.
//
// Two kernels.  gt_vis_init_kernel writes the neutral element of every output row (0 for the counts, INT_MAX / INT_MIN for
// the boxes); the host zeroes the two mask stacks with hipMemsetAsync in front of it.  gt_visibility_kernel: one 256-thread
// workgroup per GT_BLOCK_PIX consecutive box pixels of an instance (a flat block table, the workgroup finds its instance by a
// binary search over the first blocks, as vsd_counts_kernel does); a thread keeps 3 sums, 4 minima and 4 maxima in registers,
// the wave folds them by shuffles, the workgroup through LDS, and one 32-bit integer atomic per non-neutral entry goes to the
// output row.  Integer sums and extremes only: bit-identical across runs, batch compositions and launch shapes.
#include <climits>

#include "common.hpp"
#include "group_parts.hpp"  // last_at_or_before
#include "bop_dist.hpp"   // dadd, dist, visib: the same functions vsd.hip uses
#include "../../include/foundpose_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int GT_THREADS = 256;
constexpr int GT_PPT = 4;                           // pixels per thread
constexpr int GT_BLOCK_PIX = GT_THREADS * GT_PPT;   // = FP_GT_VIS_BLOCK_PIXELS
constexpr int GT_NO = 11;                           // entries of an output row: 3 sums, then per box 2 minima and 2 maxima
static_assert(GT_BLOCK_PIX == FP_GT_VIS_BLOCK_PIXELS, "block size of the header");

enum { GT_SUM = 0, GT_MIN = 1, GT_MAX = 2 };
FP_DEVICE int entry_kind(int c) { return c < 3 ? GT_SUM : (((c - 3) & 3) < 2 ? GT_MIN : GT_MAX); }
FP_DEVICE int neutral(int kind) { return kind == GT_SUM ? 0 : (kind == GT_MIN ? INT_MAX : INT_MIN); }
FP_DEVICE int fold(int kind, int a, int b) { return kind == GT_SUM ? a + b : (kind == GT_MIN ? min(a, b) : max(a, b)); }

__global__ __launch_bounds__(GT_THREADS) void gt_vis_init_kernel(int* out, int n) {
  const int i = blockIdx.x * GT_THREADS + threadIdx.x;
  if (i < n) out[i] = neutral(entry_kind(i % GT_NO));
}

__global__ __launch_bounds__(GT_THREADS) void gt_visibility_kernel(GtVisArgs a) {
  const long long blk = blockIdx.x;
  const int lo = last_at_or_before(a.num_inst, blk, [&](int i) { return a.inst[i].blk0; });  // the instance that owns the block
  const GtVisInst in = a.inst[lo];
  const int npix = in.bw * in.bh;
  const int base = (int)(blk - in.blk0) * GT_BLOCK_PIX;
  const float* dobj = a.depth_obj + (long long)lo * a.render_h * a.render_w;
  const long long img = (long long)lo * a.height * a.width;
  int v[GT_NO];
#pragma unroll
  for (int c = 0; c < GT_NO; ++c) v[c] = neutral(entry_kind(c));
#pragma unroll
  for (int k = 0; k < GT_PPT; ++k) {
    const int q = base + k * GT_THREADS + (int)threadIdx.x;
    if (q >= npix) continue;
    const int rr = in.y0 + q / in.bw, cr = in.x0 + q % in.bw;      // inside the render: the host checked the box
    const float d = dobj[rr * a.render_w + cr];                    // render_w * render_h <= INT_MAX
    const int row = rr - in.oy, col = cr - in.ox;
    if (d > 0.f) {
      v[0] += 1;
      v[3] = min(v[3], col), v[4] = min(v[4], row), v[5] = max(v[5], col), v[6] = max(v[6], row);
    }
    if (row < 0 || row >= a.height || col < 0 || col >= a.width) continue;
    const long long pix = (long long)row * a.width + col;
    bool m = false, vis = false;
    if (d != 0.f) {   // +-0 has dist 0; a negative or NaN depth goes through the arithmetic as numpy's would
      const float dt = a.depth_test[in.test_off + pix];
      const double xs = __ddiv_rn(dadd((double)col, -in.cx), in.fx), ys = __ddiv_rn(dadd((double)row, -in.cy), in.fy);
      const double dist_t = dist(xs, ys, dt), dist_o = dist(xs, ys, d);
      m = dist_o > 0.0;
      vis = visib(dist_o, dist_t, in.delta);
      v[1] += m && dist_t > 0.0;
      if (vis) {
        v[2] += 1;
        v[7] = min(v[7], col), v[8] = min(v[8], row), v[9] = max(v[9], col), v[10] = max(v[10], row);
      }
    }
    a.mask[img + pix] = m ? 255 : 0;
    a.mask_visib[img + pix] = vis ? 255 : 0;
  }
  __shared__ int red[GT_THREADS / 64][GT_NO];
#pragma unroll
  for (int c = 0; c < GT_NO; ++c) {
    const int kind = entry_kind(c);
    int s = v[c];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = fold(kind, s, __shfl_xor(s, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < GT_NO) {
    const int kind = entry_kind(threadIdx.x);
    int s = neutral(kind);
#pragma unroll
    for (int w = 0; w < GT_THREADS / 64; ++w) s = fold(kind, s, red[w][threadIdx.x]);
    int* dst = a.out + (size_t)lo * GT_NO + threadIdx.x;
    if (s != neutral(kind)) {
      if (kind == GT_SUM) atomicAdd(dst, s);
      else if (kind == GT_MIN) atomicMin(dst, s);
      else atomicMax(dst, s);
    }
  }
}

}  // namespace

int launch_gt_visibility(const GtVisArgs& a, long long num_blocks, hipStream_t st) {
  const int n = a.num_inst * GT_NO;
  hipLaunchKernelGGL(gt_vis_init_kernel, dim3((unsigned)cdiv(n, GT_THREADS)), dim3(GT_THREADS), 0, st, a.out, n);
  FP_CHECK_LAUNCH("gt_vis_init");
  if (num_blocks == 0) return FP_OK;
  hipLaunchKernelGGL(gt_visibility_kernel, dim3((unsigned)num_blocks), dim3(GT_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("gt_visibility");
  return FP_OK;
}
