// Result pictures: the compositing kernels behind foundpose_amd/vis_util.py.
//
// Replaces the cv2 / matplotlib / pyrender drawing of utils/vis_util.py:179-687 (vis_inference_results, vis_for_paper layout) and
// utils/vis_base_util.py (normalize_data, add_contour_overlay, plot_matches) by an exact pixel contract of this project's own --
// tests/vis_ref.py restates it in numpy.  Images are uint8 HWC with a leading batch dimension; one launch covers the batch.
// Every output pixel is produced by exactly one thread from a gather over its inputs, in a fixed order: no atomics, so a
// detection's picture is bit-identical whatever else is in the batch.
//   mask_tint        (img + 255) >> 1 where the mask is set                                  (integer, exact)
//   contour          4-neighbour edge of a mask, dilated by a 3 x 3 square n times, painted   (integer, exact)
//   scene_composite  nearest positive depth layer per pixel, (img + colour[k]) >> 1, id map   (integer, exact)
//   resize_area      footprint-area-weighted mean, in integer arithmetic (exact rational, round half up)
//   pca_colorize     one (lo, hi) per detection over channels 0..2, trunc(255 (x - lo) / (hi - lo)), nearest upsampling (fp32),
//                    optionally dimmed by an integer ratio ((9 v) / 10 for the query side of the match picture)
//   draw_matches     anti-aliased segments with end discs, sequential fp32 blend per pixel, rounded once at the end
#include "common.hpp"
#include "kernels.hpp"
#include "../../include/foundpose_amd.h"

namespace {

// ---------------------------------------------------------------- mask_tint: 4 pixels (12 bytes) per thread over the flat pixel index
FP_DEVICE unsigned tint_byte(unsigned v, bool on) { return on ? (v + 255u) >> 1 : v; }

__global__ __launch_bounds__(256) void mask_tint_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, long long pixels,
                                                        bool aligned, uint8_t* __restrict__ out) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x, p0 = g * 4;
  if (p0 >= pixels) return;
  if (aligned && p0 + 4 <= pixels) {   // all three pointers are dword-aligned
    const unsigned m = reinterpret_cast<const unsigned*>(mask)[g];
    const unsigned* src = reinterpret_cast<const unsigned*>(img) + g * 3;
    unsigned* dst = reinterpret_cast<unsigned*>(out) + g * 3;
#pragma unroll
    for (int wd = 0; wd < 3; ++wd) {
      const unsigned v = src[wd];
      unsigned r = 0;
#pragma unroll
      for (int by = 0; by < 4; ++by) {
        const int pix = (wd * 4 + by) / 3;   // which of the 4 pixels byte (wd, by) belongs to
        r |= tint_byte((v >> (8 * by)) & 255u, ((m >> (8 * pix)) & 255u) != 0) << (8 * by);
      }
      dst[wd] = r;
    }
    return;
  }
  for (long long p = p0; p < min(p0 + 4, pixels); ++p)   // the last 1..3 pixels; everything when a pointer is not dword-aligned
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = (uint8_t)tint_byte(img[p * 3 + c], mask[p] != 0);
}

// ---------------------------------------------------------------- contour
FP_DEVICE bool mask_edge(const uint8_t* m, int x, int y, int w, int h) {
  if (m[(size_t)y * w + x] == 0) return false;
  return (x > 0 && m[(size_t)y * w + x - 1] == 0) || (x + 1 < w && m[(size_t)y * w + x + 1] == 0) ||
         (y > 0 && m[(size_t)(y - 1) * w + x] == 0) || (y + 1 < h && m[(size_t)(y + 1) * w + x] == 0);
}

// n dilations by a 3 x 3 square = one by a (2n + 1)-square: the pixel is painted when an edge pixel lies within Chebyshev distance n
__global__ __launch_bounds__(256) void contour_kernel(const uint8_t* __restrict__ mask, int h, int w, int dil, uchar4 colour,
                                                      uint8_t* __restrict__ img) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (x >= w || y >= h) return;
  const uint8_t* m = mask + (size_t)b * h * w;
  bool hit = false;
  const int y0 = max(y - dil, 0), y1 = min(y + dil, h - 1), x0 = max(x - dil, 0), x1 = min(x + dil, w - 1);
  for (int yy = y0; yy <= y1 && !hit; ++yy)
    for (int xx = x0; xx <= x1 && !hit; ++xx) hit = mask_edge(m, xx, yy, w, h);
  if (!hit) return;
  uint8_t* px = img + (((size_t)b * h + y) * w + x) * 3;
  px[0] = colour.x, px[1] = colour.y, px[2] = colour.z;
}

// ---------------------------------------------------------------- scene_composite
__global__ __launch_bounds__(256) void scene_composite_kernel(const float* __restrict__ depth, const uint8_t* __restrict__ colours, int layers,
                                                              int h, int w, const uint8_t* __restrict__ img, uint8_t* __restrict__ out,
                                                              int* __restrict__ ids) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const size_t pix = (size_t)y * w + x, plane = (size_t)h * w;
  int best = -1;
  float zbest = 0.f;
  for (int k = 0; k < layers; ++k) {
    const float z = depth[k * plane + pix];
    if (z > 0.f && (best < 0 || z < zbest)) best = k, zbest = z;   // strict <: a tie keeps the lowest k
  }
  ids[pix] = best;
  for (int c = 0; c < 3; ++c) {
    const unsigned v = img[pix * 3 + c];
    out[pix * 3 + c] = (uint8_t)(best < 0 ? v : (v + colours[best * 3 + c]) >> 1);
  }
}

// ---------------------------------------------------------------- resize_area (downscaling): exact integer footprint weights
// In units of 1 / out_w source pixels the footprint of output column x is [x w, (x + 1) w) and source column s covers [s out_w, (s + 1) out_w):
// the overlap is an integer, likewise in y, and the weights of a footprint sum to w h.
__global__ __launch_bounds__(256) void resize_area_kernel(const uint8_t* __restrict__ src, int h, int w, int oh, int ow, uint8_t* __restrict__ out) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (x >= ow || y >= oh) return;
  const uint8_t* s = src + (size_t)b * h * w * 3;
  const long long fx0 = (long long)x * w, fx1 = fx0 + w, fy0 = (long long)y * h, fy1 = fy0 + h;
  const int sx0 = (int)(fx0 / ow), sx1 = (int)((fx1 - 1) / ow), sy0 = (int)(fy0 / oh), sy1 = (int)((fy1 - 1) / oh);
  unsigned long long acc[3] = {0, 0, 0};
  for (int sy = sy0; sy <= sy1; ++sy) {
    const long long wy = min(fy1, (long long)(sy + 1) * oh) - max(fy0, (long long)sy * oh);
    for (int sx = sx0; sx <= sx1; ++sx) {
      const long long wx = min(fx1, (long long)(sx + 1) * ow) - max(fx0, (long long)sx * ow);
      const unsigned long long wgt = (unsigned long long)(wx * wy);
      const uint8_t* p = s + ((size_t)sy * w + sx) * 3;
      acc[0] += wgt * p[0], acc[1] += wgt * p[1], acc[2] += wgt * p[2];
    }
  }
  const unsigned long long area = (unsigned long long)w * h;
  uint8_t* o = out + (((size_t)b * oh + y) * ow + x) * 3;
  for (int c = 0; c < 3; ++c) o[c] = (uint8_t)((2 * acc[c] + area) / (2 * area));
}

// ---------------------------------------------------------------- pca_colorize
// (lo, hi) of channels 0..2 of one detection: one workgroup, a strided scan and an LDS tree (min / max do not depend on the order).
__global__ __launch_bounds__(256) void pca_range_kernel(const float* __restrict__ map, int cells, int C, float* __restrict__ range) {
  __shared__ float slo[256], shi[256];
  const float* m = map + (size_t)blockIdx.x * cells * C;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < cells * 3; i += 256) {
    const float v = m[(size_t)(i / 3) * C + i % 3];
    lo = fminf(lo, v), hi = fmaxf(hi, v);
  }
  slo[threadIdx.x] = lo, shi[threadIdx.x] = hi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      slo[threadIdx.x] = fminf(slo[threadIdx.x], slo[threadIdx.x + s]);
      shi[threadIdx.x] = fmaxf(shi[threadIdx.x], shi[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) range[blockIdx.x * 2] = slo[0], range[blockIdx.x * 2 + 1] = shi[0];
}

__global__ __launch_bounds__(256) void pca_colorize_kernel(const float* __restrict__ map, int gh, int gw, int C, int h, int w,
                                                           int num, int den, const float* __restrict__ range, uint8_t* __restrict__ out) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (x >= w || y >= h) return;
  const int sy = (int)((long long)y * gh / h), sx = (int)((long long)x * gw / w);   // F.interpolate(mode="nearest")
  const float* m = map + (((size_t)b * gh + sy) * gw + sx) * C;
  const float lo = range[b * 2], hi = range[b * 2 + 1], span = hi - lo;
  uint8_t* o = out + (((size_t)b * h + y) * w + x) * 3;
  for (int c = 0; c < 3; ++c) {
    float v = 0.f;
    if (hi > lo) v = fminf(fmaxf(255.f * __fdiv_rn(m[c] - lo, span), 0.f), 255.f);   // the quotient first: exactly 1 at hi, so hi maps to 255
    o[c] = (uint8_t)((int)v * num / den);   // trunc, then the integer dimming (num <= den)
  }
}

// ---------------------------------------------------------------- draw_matches
// A 32 x 8 pixel workgroup stages the detection's segments in LDS and walks them in input order; a segment whose reach
// (its box grown by max(lw / 2, radius) + 1/2) misses the workgroup's pixels is skipped by the whole workgroup at once.
__global__ __launch_bounds__(256) void draw_matches_kernel(const float* __restrict__ segs, const int* __restrict__ counts, int max_matches,
                                                           int h, int w, float cr, float cg, float cb, float alpha, float lw, float radius,
                                                           uint8_t* __restrict__ tile) {
  __shared__ float4 sseg[FP_VIS_MAX_MATCHES];
  const int b = blockIdx.z;
  const int n = min(max(counts[b], 0), max_matches);
  for (int i = threadIdx.x; i < n; i += 256) sseg[i] = reinterpret_cast<const float4*>(segs)[(size_t)b * max_matches + i];
  __syncthreads();
  const int bx = blockIdx.x * 32, by = blockIdx.y * 8;
  const int x = bx + (threadIdx.x & 31), y = by + (threadIdx.x >> 5);
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  const float reach = fmaxf(0.5f * lw, radius) + 0.5f;
  const float rx0 = (float)bx - reach, rx1 = (float)(bx + 32) + reach, ry0 = (float)by - reach, ry1 = (float)(by + 8) + reach;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f;
  bool loaded = false, inside = x < w && y < h;
  uint8_t* p = tile + (((size_t)b * h + (inside ? y : 0)) * w + (inside ? x : 0)) * 3;
  auto blend = [&](float cov) {
    if (cov <= 0.f || !inside) return;
    if (!loaded) o0 = p[0], o1 = p[1], o2 = p[2], loaded = true;
    const float a = alpha * cov;
    o0 = o0 * (1.f - a) + cr * a, o1 = o1 * (1.f - a) + cg * a, o2 = o2 * (1.f - a) + cb * a;
  };
  auto clamp01 = [](float v) { return fminf(fmaxf(v, 0.f), 1.f); };
  for (int i = 0; i < n; ++i) {
    const float4 s = sseg[i];
    if (fmaxf(s.x, s.z) < rx0 || fminf(s.x, s.z) > rx1 || fmaxf(s.y, s.w) < ry0 || fminf(s.y, s.w) > ry1) continue;   // workgroup-uniform
    const float dx = s.z - s.x, dy = s.w - s.y, len2 = dx * dx + dy * dy;
    float t = len2 > 0.f ? ((px - s.x) * dx + (py - s.y) * dy) / len2 : 0.f;
    t = clamp01(t);
    const float ex = px - (s.x + t * dx), ey = py - (s.y + t * dy);
    blend(clamp01(0.5f + 0.5f * lw - sqrtf(ex * ex + ey * ey)));
    const float ax = px - s.x, ay = py - s.y, qx = px - s.z, qy = py - s.w;
    blend(clamp01(0.5f + radius - sqrtf(ax * ax + ay * ay)));
    blend(clamp01(0.5f + radius - sqrtf(qx * qx + qy * qy)));
  }
  if (loaded) {
    p[0] = (uint8_t)__float2int_rn(fminf(fmaxf(o0, 0.f), 255.f));
    p[1] = (uint8_t)__float2int_rn(fminf(fmaxf(o1, 0.f), 255.f));
    p[2] = (uint8_t)__float2int_rn(fminf(fmaxf(o2, 0.f), 255.f));
  }
}

dim3 pixel_grid(int w, int h, int batch) { return dim3(cdiv(w, 64), cdiv(h, 4), batch); }

}  // namespace

int launch_vis_mask_tint(const uint8_t* img, const uint8_t* mask, long long pixels, uint8_t* out, hipStream_t st) {
  hipLaunchKernelGGL(mask_tint_kernel, dim3((unsigned)((pixels + 1023) / 1024)), dim3(256), 0, st, img, mask, pixels,
                     ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(out)) & 3) == 0, out);
  FP_CHECK_LAUNCH("vis_mask_tint");
  return FP_OK;
}

int launch_vis_contour(const uint8_t* mask, int batch, int h, int w, int dil, int r, int g, int b, uint8_t* img, hipStream_t st) {
  hipLaunchKernelGGL(contour_kernel, pixel_grid(w, h, batch), dim3(256), 0, st, mask, h, w, dil,
                     make_uchar4((unsigned char)r, (unsigned char)g, (unsigned char)b, 0), img);
  FP_CHECK_LAUNCH("vis_contour");
  return FP_OK;
}

int launch_vis_scene_composite(const float* depth, const uint8_t* colours, int layers, int h, int w, const uint8_t* img, uint8_t* out,
                               int* ids, hipStream_t st) {
  hipLaunchKernelGGL(scene_composite_kernel, pixel_grid(w, h, 1), dim3(256), 0, st, depth, colours, layers, h, w, img, out, ids);
  FP_CHECK_LAUNCH("vis_scene_composite");
  return FP_OK;
}

int launch_vis_resize_area(const uint8_t* src, int batch, int h, int w, int oh, int ow, uint8_t* out, hipStream_t st) {
  hipLaunchKernelGGL(resize_area_kernel, pixel_grid(ow, oh, batch), dim3(256), 0, st, src, h, w, oh, ow, out);
  FP_CHECK_LAUNCH("vis_resize_area");
  return FP_OK;
}

int launch_vis_pca_colorize(const float* map, int batch, int gh, int gw, int C, int h, int w, int num, int den, float* range, uint8_t* out,
                            hipStream_t st) {
  hipLaunchKernelGGL(pca_range_kernel, dim3(batch), dim3(256), 0, st, map, gh * gw, C, range);
  FP_CHECK_LAUNCH("vis_pca_range");
  hipLaunchKernelGGL(pca_colorize_kernel, pixel_grid(w, h, batch), dim3(256), 0, st, map, gh, gw, C, h, w, num, den, range, out);
  FP_CHECK_LAUNCH("vis_pca_colorize");
  return FP_OK;
}

int launch_vis_draw_matches(const float* segs, const int* counts, int batch, int max_matches, int h, int w, const float* colour, float alpha,
                            float lw, float radius, uint8_t* tile, hipStream_t st) {
  hipLaunchKernelGGL(draw_matches_kernel, dim3(cdiv(w, 32), cdiv(h, 8), batch), dim3(256), 0, st, segs, counts, max_matches, h, w,
                     colour[0], colour[1], colour[2], alpha, lw, radius, tile);
  FP_CHECK_LAUNCH("vis_draw_matches");
  return FP_OK;
}
