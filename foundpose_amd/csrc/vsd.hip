// Visible Surface Discrepancy counts (bop_toolkit_lib pose_error.vsd with visibility._estimate_visib_mask in `bop19` mode,
// misc.depth_im_to_dist_im_fast and the `step` cost), a batch of (estimate, GT) pairs per call.
//
// Per pixel (col, row) of a pair's box, all in fp64 unless said otherwise, every operation rounded on its own:
//   xs = (col - cx) / fx,  ys = (row - cy) / fy                   (integer pixel indices, IEEE division)
//   dist(d) = sqrt(((xs d)^2 + (ys d)^2) + d^2)                    for the fp32 depths of the test, GT and estimate images
//   visib(m) = ((float)dist_m - (float)dist_test <= (float)delta  ||  dist_test == 0)  &&  dist_m > 0     (fp32 difference)
//   visib_gt = visib(gt),  visib_est = visib(est) || (visib_gt && dist_est > 0)
//   union = visib_gt || visib_est,  inter = visib_gt && visib_est
//   on inter pixels: e = |dist_gt - dist_est| / diameter, counted once for every tau with e >= tau.
// A pixel where both renders are 0 is in neither mask (visib needs dist_model > 0), so it is skipped before any arithmetic;
// the box (the union of the two renders' boxes) bounds every pixel that can count.
//
// One kernel.  vsd_counts_kernel: one 256-thread workgroup per VSD_BLOCK_PIX consecutive box pixels of a pair (a flat
// block table: the workgroup finds its pair by a binary search over the pairs' first blocks); each thread counts its
// pixels in registers, the wave sums by shuffles, the workgroup through LDS, and one 64-bit integer atomic per non-zero
// counter goes into the output the host zeroed on the stream.  Integer sums: bit-identical across runs and batches.
#include "common.hpp"
#include "group_parts.hpp"  // last_at_or_before
#include "bop_dist.hpp"   // dmul, dadd, dist, visib
#include "../../include/foundpose_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int VSD_THREADS = 256;
constexpr int VSD_PPT = 4;                          // pixels per thread
constexpr int VSD_BLOCK_PIX = VSD_THREADS * VSD_PPT;  // = FP_VSD_BLOCK_PIXELS
constexpr int VSD_NC = 2 + FP_VSD_MAX_TAUS;         // counters per pair, at most
static_assert(VSD_BLOCK_PIX == FP_VSD_BLOCK_PIXELS, "block size of the header");

__global__ __launch_bounds__(VSD_THREADS) void vsd_counts_kernel(VsdArgs a) {
  const long long blk = blockIdx.x;
  const int lo = last_at_or_before(a.num_pairs, blk, [&](int i) { return a.pairs[i].blk0; });  // the pair that owns the block
  const VsdPair pr = a.pairs[lo];
  const int npix = pr.bw * pr.bh;
  const int base = (int)(blk - pr.blk0) * VSD_BLOCK_PIX;
  int cnt[VSD_NC];
#pragma unroll
  for (int c = 0; c < VSD_NC; ++c) cnt[c] = 0;
#pragma unroll
  for (int k = 0; k < VSD_PPT; ++k) {
    const int q = base + k * VSD_THREADS + (int)threadIdx.x;
    if (q >= npix) continue;
    const int row = pr.y0 + q / pr.bw, col = pr.x0 + q % pr.bw;
    const long long pix = (long long)row * a.width + col;
    const float dg = a.depth_gt[pr.gt_off + pix], de = a.depth_est[pr.est_off + pix];
    if (dg == 0.f && de == 0.f) continue;  // in neither mask
    const float dt = a.depth_test[pr.test_off + pix];
    const double xs = __ddiv_rn(dadd((double)col, -pr.cx), pr.fx), ys = __ddiv_rn(dadd((double)row, -pr.cy), pr.fy);
    const double dist_t = dist(xs, ys, dt), dist_g = dist(xs, ys, dg), dist_e = dist(xs, ys, de);
    const bool vg = visib(dist_g, dist_t, pr.delta);
    const bool ve = visib(dist_e, dist_t, pr.delta) || (vg && dist_e > 0.0);
    if (!(vg || ve)) continue;
    cnt[0] += 1;
    if (!(vg && ve)) continue;
    cnt[1] += 1;
    const double e = __ddiv_rn(fabs(dadd(dist_g, -dist_e)), pr.diameter);
#pragma unroll
    for (int t = 0; t < FP_VSD_MAX_TAUS; ++t)
      if (t < a.num_taus) cnt[2 + t] += e >= a.taus[t];
  }
  __shared__ int red[VSD_THREADS / 64][VSD_NC];
  const int nc = 2 + a.num_taus;
#pragma unroll
  for (int c = 0; c < VSD_NC; ++c) {
    if (c < nc) {  // uniform
      int s = cnt[c];
      s = wave_sum(s);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = s;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < nc) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < VSD_THREADS / 64; ++w) s += red[w][threadIdx.x];
    if (s) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts + (size_t)lo * nc + threadIdx.x), (unsigned long long)s);
  }
}

}  // namespace

int launch_vsd_counts(const VsdArgs& a, long long num_blocks, hipStream_t st) {
  hipLaunchKernelGGL(vsd_counts_kernel, dim3((unsigned)num_blocks), dim3(VSD_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("vsd_counts");
  return FP_OK;
}
