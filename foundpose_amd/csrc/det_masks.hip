// Detection masks on the device (infer_batched's device_masks path): the COCO run lengths of N detections in, the
// opened, centre-cropped uint8 [N, H, W] masks and their areas out -- the bits of infer_pose_util.rle_to_binary_mask, open_mask_3x3 and the
// [dy : hc - dy, dx : wc - dx] slice of the host path.
//   scan    one workgroup per detection: the inclusive prefix sums s_i of its runs, in chunks of 256 (group_parts.hpp's block scan) with a
//           running carry; a negative count counts as 0 and the sums saturate at 2^31 - 1, so the sums never decrease whatever the input;
//   masks   one workgroup per 64 x 16 tile of the OUTPUT image.  Canvas pixel (x, y) has the column-major index p = x hc + y; with k = the
//           number of s_i <= p (a binary search over the detection's sums) it is set iff k < R and k is odd.  With the opening the tile's
//           pixels and a halo of 2 are decoded into LDS, eroded into LDS with a halo of 1 and dilated into the output: a pixel outside the
//           CANVAS never vetoes an erosion and never wins a dilation (cv2's border rule, open_mask_3x3), and the crop comes last.  Every
//           output byte is written exactly once; the tile's count goes through the wave butterfly and one integer atomicAdd per workgroup.
// Integers only: a detection's result depends on its own runs and on nothing else.
#include "common.hpp"
#include "group_parts.hpp"

namespace {

constexpr int DM_THREADS = 256, DM_WAVES = DM_THREADS / 64;
static_assert(DM_THREADS == BS_THREADS, "rle_scan_kernel scans with block_scan_inclusive");
constexpr int DM_RW = DM_TILE_W + 4, DM_RH = DM_TILE_H + 4;  // decoded pixels: the tile and a halo of 2
constexpr int DM_EW = DM_TILE_W + 2, DM_EH = DM_TILE_H + 2;  // eroded pixels: the tile and a halo of 1

// the detection's runs in counts / prefix, clamped to the arrays: no read outside them whatever run_off holds
FP_DEVICE OffsetRange det_runs(const DetMaskArgs& a, int n) { return offset_range(a.run_off, n, a.num_runs); }

__global__ __launch_bounds__(DM_THREADS) void rle_scan_kernel(DetMaskArgs a) {
  __shared__ long long slots[BS_WAVES];
  const int tid = threadIdx.x;
  const OffsetRange r = det_runs(a, blockIdx.x);
  const int e = r.begin + r.n;
  long long carry = 0;
  for (int i0 = r.begin; i0 < e; i0 += DM_THREADS) {  // block-uniform trip count
    const int i = i0 + tid;
    long long all;
    const long long v = block_scan_inclusive(i < e ? (long long)max(a.counts[i], 0) : 0ll, slots, all);
    if (i < e) a.prefix[i] = (int)min(carry + v, (long long)INT32_MAX);
    carry += all;  // at most 2^31 per run and 2^31 runs: no overflow
    __syncthreads();  // slots are written again in the next round
  }
}

// 1 iff canvas index p lies in an odd run of the detection whose R inclusive prefix sums are s[0 .. R)
FP_DEVICE int decode_pixel(const int* __restrict__ s, int R, int p) {
  int lo = 0, hi = R;  // -> the number of s_i <= p
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] <= p) lo = mid + 1;
    else hi = mid;
  }
  return (lo < R) & lo & 1;
}

template <bool OPEN>
__global__ __launch_bounds__(DM_THREADS) void det_mask_kernel(DetMaskArgs a) {
  __shared__ unsigned char raw[DM_RH * DM_RW];
  __shared__ unsigned char ero[DM_EH * DM_EW];
  __shared__ int wave_count[DM_WAVES];
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  const int tx = blk % a.tiles_x;
  blk /= a.tiles_x;
  const int ty = blk % a.tiles_y, n = blk / a.tiles_y;
  const OffsetRange runs = det_runs(a, n);
  const int* __restrict__ s = a.prefix + runs.begin;
  const int R = runs.n;
  const int dx = (a.wc - a.W) / 2, dy = (a.hc - a.H) / 2;
  const int ox0 = tx * DM_TILE_W, oy0 = ty * DM_TILE_H;  // the tile's origin in the output image; + (dx, dy) on the canvas

  if constexpr (OPEN) {
    for (int i = tid; i < DM_RH * DM_RW; i += DM_THREADS) {  // consecutive lanes on consecutive x
      const int ry = i / DM_RW, rx = i - ry * DM_RW;
      const int x = ox0 + dx - 2 + rx, y = oy0 + dy - 2 + ry;
      int v = 1;  // outside the canvas: never vetoes an erosion
      if (x >= 0 && x < a.wc && y >= 0 && y < a.hc) v = decode_pixel(s, R, x * a.hc + y);
      raw[i] = (unsigned char)v;
    }
    __syncthreads();
    for (int i = tid; i < DM_EH * DM_EW; i += DM_THREADS) {
      const int ey = i / DM_EW, ex = i - ey * DM_EW;
      const int x = ox0 + dx - 1 + ex, y = oy0 + dy - 1 + ey;
      int v = 0;  // outside the canvas: never wins a dilation
      if (x >= 0 && x < a.wc && y >= 0 && y < a.hc) {
        v = 1;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int k = 0; k < 3; ++k) v &= raw[(ey + j) * DM_RW + ex + k];
      }
      ero[i] = (unsigned char)v;
    }
    __syncthreads();
  }

  int count = 0;
  for (int i = tid; i < DM_TILE_H * DM_TILE_W; i += DM_THREADS) {
    const int ly = i / DM_TILE_W, lx = i - ly * DM_TILE_W;
    const int ox = ox0 + lx, oy = oy0 + ly;
    if (ox < a.W && oy < a.H) {
      int v = 0;
      if constexpr (OPEN) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int k = 0; k < 3; ++k) v |= ero[(ly + j) * DM_EW + lx + k];
      } else {
        v = decode_pixel(s, R, (ox + dx) * a.hc + (oy + dy));
      }
      a.masks[((size_t)n * a.H + oy) * a.W + ox] = (unsigned char)v;
      count += v;
    }
  }
  count = wave_sum(count);
  if ((tid & 63) == 0) wave_count[tid >> 6] = count;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < DM_WAVES; ++w) total += wave_count[w];
    if (total) atomicAdd(&a.area[n], total);
  }
}

}  // namespace

int launch_detection_masks(DetMaskArgs a, int num_det, int open3x3, hipStream_t st) {
  a.tiles_x = cdiv(a.W, DM_TILE_W);
  a.tiles_y = cdiv(a.H, DM_TILE_H);
  const long long blocks = (long long)num_det * a.tiles_x * a.tiles_y;
  FP_REQUIRE(blocks <= INT32_MAX, "detection_masks: %d detections of %d x %d tiles (at most 2^31 - 1 workgroups in one call)", num_det, a.tiles_x, a.tiles_y);
  if (hipMemsetAsync(a.area, 0, (size_t)num_det * sizeof(int), st) != hipSuccess) {
    fp_set_error("detection_masks: cannot zero the areas: %s", hipGetErrorString(hipGetLastError()));
    return FP_ERR_HIP;
  }
  if (a.num_runs > 0) {
    hipLaunchKernelGGL(rle_scan_kernel, dim3(num_det), dim3(DM_THREADS), 0, st, a);
    FP_CHECK_LAUNCH("detection_masks (scan)");
  }
  if (open3x3) hipLaunchKernelGGL(det_mask_kernel<true>, dim3((unsigned)blocks), dim3(DM_THREADS), 0, st, a);
  else hipLaunchKernelGGL(det_mask_kernel<false>, dim3((unsigned)blocks), dim3(DM_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("detection_masks");
  return FP_OK;
}
