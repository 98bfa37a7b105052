// TSDF fusion of posed RGB-D frames and marching-tetrahedra extraction (reconstruct.py; DESIGN.md section 29, tests/tsdf_ref.py
// restates both stages).
//
// The volume: nx x ny x nz voxels, x fastest, voxel (i, j, k) centred at origin + ((i, j, k) + 0.5) h, in the model frame, mm.  Its
// state is six planes of nx ny nz entries: sdf_sum fp32, sdf_cnt int32, rgb_sum 3 x fp32 (planar), rgb_cnt int32.  Sums and counts,
// never running means: a voxel's state after frames 1 .. F is the same bits however the frames are split into calls.
//
// tsdf_integrate_kernel   one thread per voxel, by linear index: a wave holds 64 consecutive voxels of an x-row (whole rows when
//                         nx % 64 == 0, else it runs on into the next row; the loads and stores of the six planes are contiguous
//                         either way).  The voxel's six values sit in registers while the frames of the call are visited in
//                         ascending order; the frame table (camera, pose) is read through wave-uniform addresses, the three image
//                         taps are gathers into images that fit in L2.  No atomics, no reduction across threads.  The geometry
//                         is fp64, every operation rounded on its own (rounded.hpp).
// tsdf_count_kernel       one thread per cell (the cube between 8 voxel centres, (nx - 1)(ny - 1)(nz - 1) of them, x fastest):
//                         the triangles its six tetrahedra give, 0 unless all eight corners have sdf_cnt >= min_count.
// tsdf_emit_kernel        the same walk; a cell writes its triangles at the offset the host's exclusive scan gave it: per corner an
//                         int64 edge key, a position and a colour.
//
// The six tetrahedra of a cell share its main diagonal 0-7 (corners numbered by bits, x = bit 0): (0, a, b, 7) for (a, b) in (1,3),
// (3,2), (2,6), (6,4), (4,5), (5,1), all positively oriented.  The split is the same in every cell, so two cells cut their shared
// face along the same diagonal and the surface has no cracks.  Every edge of the split joins a corner to one with MORE bits set:
// a vertex is named by (linear index of the lower corner) * 7 + direction and computed from the lower corner, so it has the same
// bits from whichever tetrahedron or cell reaches it.
#include "common.hpp"
#include "kernels.hpp"
#include "rounded.hpp"
#include "../../include/foundpose_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int TSDF_THREADS = 256;

FP_DEVICE double voxel_centre(double o, int i, double h) { return dadd(o, dmul(dadd((double)i, 0.5), h)); }

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_integrate_kernel(TsdfIntegrateArgs a) {
  const long long n = (long long)a.vol.nx * a.vol.ny * a.vol.nz;   // <= 2^27
  const long long v = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (v >= n) return;
  const int i = (int)(v % a.vol.nx), j = (int)((v / a.vol.nx) % a.vol.ny), k = (int)(v / ((long long)a.vol.nx * a.vol.ny));
  const double X = voxel_centre(a.vol.ox, i, a.vol.h), Y = voxel_centre(a.vol.oy, j, a.vol.h), Z = voxel_centre(a.vol.oz, k, a.vol.h);
  float sum = a.sdf_sum[v], cr = a.rgb_sum[v], cg = a.rgb_sum[n + v], cb = a.rgb_sum[2 * n + v];
  int cnt = a.sdf_cnt[v], ccnt = a.rgb_cnt[v];
  const long long pixels = (long long)a.height * a.width;
  for (int f = 0; f < a.num_frames; ++f) {
    const TsdfFrame& fr = a.frames[f];                              // wave-uniform: scalar loads
    const double z = affine(fr.R + 6, fr.t[2], X, Y, Z);
    if (!(z > 1.0)) continue;                                       // behind or within 1 mm of the camera (a NaN too)
    const double x = affine(fr.R, fr.t[0], X, Y, Z), y = affine(fr.R + 3, fr.t[1], X, Y, Z);
    const double pu = floor(dadd(dadd(ddiv(dmul(fr.fx, x), z), fr.cx), 0.5));
    const double pv = floor(dadd(dadd(ddiv(dmul(fr.fy, y), z), fr.cy), 0.5));
    if (!(pu >= 0.0 && pu < (double)a.width && pv >= 0.0 && pv < (double)a.height)) continue;   // no tap outside the image is read
    const long long pix = (long long)f * pixels + (long long)pv * a.width + (long long)pu;
    const float d = a.depth[pix];
    if (!(d > 0.f)) continue;                                       // 0 = no measurement (a negative or NaN depth is none either)
    if (a.mask[pix] == 0) {
      if ((double)d >= z) sum = __fadd_rn(sum, 1.f), ++cnt;         // seen through: empty space
      continue;                                                     // else hidden behind something that is not the object
    }
    const double s = dsub((double)d, z);
    if (s < -a.tau) continue;
    sum = __fadd_rn(sum, (float)fmin(1.0, ddiv(s, a.tau)));
    ++cnt;
    if (fabs(s) <= a.tau) {
      const uint8_t* c = a.rgb + 3 * pix;
      cr = __fadd_rn(cr, __fdiv_rn((float)c[0], 255.f));
      cg = __fadd_rn(cg, __fdiv_rn((float)c[1], 255.f));
      cb = __fadd_rn(cb, __fdiv_rn((float)c[2], 255.f));
      ++ccnt;
    }
  }
  a.sdf_sum[v] = sum, a.sdf_cnt[v] = cnt;
  a.rgb_sum[v] = cr, a.rgb_sum[n + v] = cg, a.rgb_sum[2 * n + v] = cb, a.rgb_cnt[v] = ccnt;
}

// ---- extraction
// Per inside mask of a tetrahedron (bit q = vertex q inside): the triangle count, then per triangle corner the edge it lies on as
// 4 * inside vertex + outside vertex.  Made for a positively oriented tetrahedron: the normal points from inside to outside.
__constant__ unsigned char TET_TRI[16][7] = {
    {0, 0, 0, 0, 0, 0, 0},    {1, 1, 2, 3, 0, 0, 0},    {1, 4, 7, 6, 0, 0, 0},    {2, 2, 3, 7, 2, 7, 6},
    {1, 8, 9, 11, 0, 0, 0},   {2, 3, 1, 9, 3, 9, 11},   {2, 4, 7, 11, 4, 11, 8},  {1, 3, 7, 11, 0, 0, 0},
    {1, 12, 14, 13, 0, 0, 0}, {2, 1, 2, 14, 1, 14, 13}, {2, 6, 4, 12, 6, 12, 14}, {1, 2, 14, 6, 0, 0, 0},
    {2, 8, 9, 13, 8, 13, 12}, {1, 1, 9, 13, 0, 0, 0},   {1, 4, 12, 8, 0, 0, 0},   {0, 0, 0, 0, 0, 0, 0}};
__constant__ unsigned char TET_MID[6][2] = {{1, 3}, {3, 2}, {2, 6}, {6, 4}, {4, 5}, {5, 1}};
__constant__ unsigned char EDGE_DIR[8] = {0, 0, 1, 3, 2, 5, 4, 6};   // corner offset bits -> direction: 100 010 001 110 011 101 111 (x y z)

struct Cell {
  int i, j, k;
  long long base;      // linear voxel index of corner 0
  double f[8];
  bool live;
};

FP_DEVICE long long corner_index(const TsdfVolume& vol, const Cell& c, int q) {
  return c.base + (q & 1) + (long long)((q >> 1) & 1) * vol.nx + (long long)(q >> 2) * vol.nx * vol.ny;
}

// the cell of thread `cell` (below the cell count): its corner values, live when all eight corners were seen min_count times
FP_DEVICE Cell load_cell(const TsdfVolume& vol, const float* sdf_sum, const int* sdf_cnt, int min_count, long long cell) {
  Cell c;
  const int cx = vol.nx - 1, cy = vol.ny - 1;
  c.i = (int)(cell % cx), c.j = (int)((cell / cx) % cy), c.k = (int)(cell / ((long long)cx * cy));
  c.base = ((long long)c.k * vol.ny + c.j) * vol.nx + c.i;
  c.live = true;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const long long v = corner_index(vol, c, q);
    const int n = sdf_cnt[v];
    c.live = c.live && n >= min_count;
    c.f[q] = n > 0 ? ddiv((double)sdf_sum[v], (double)n) : 0.0;
  }
  return c;
}

FP_DEVICE int tet_mask(const Cell& c, int t) {   // inside = f < 0; an exact 0 is outside
  return (int)(c.f[0] < 0.0) | ((int)(c.f[TET_MID[t][0]] < 0.0) << 1) | ((int)(c.f[TET_MID[t][1]] < 0.0) << 2) | ((int)(c.f[7] < 0.0) << 3);
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_count_kernel(TsdfExtractArgs a, long long cells) {
  const long long cell = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (cell >= cells) return;
  const Cell c = load_cell(a.vol, a.sdf_sum, a.sdf_cnt, a.min_count, cell);
  int n = 0;
  if (c.live) {
#pragma unroll
    for (int t = 0; t < 6; ++t) n += TET_TRI[tet_mask(c, t)][0];
  }
  a.counts[cell] = n;
}

__global__ __launch_bounds__(TSDF_THREADS) void tsdf_emit_kernel(TsdfExtractArgs a, long long cells) {
  const long long cell = (long long)blockIdx.x * TSDF_THREADS + threadIdx.x;
  if (cell >= cells) return;
  const Cell c = load_cell(a.vol, a.sdf_sum, a.sdf_cnt, a.min_count, cell);
  if (!c.live) return;
  long long tri = a.offsets[cell];
  const long long n = (long long)a.vol.nx * a.vol.ny * a.vol.nz;
  for (int t = 0; t < 6; ++t) {
    const int m = tet_mask(c, t);
    const int corner[4] = {0, TET_MID[t][0], TET_MID[t][1], 7};
    for (int e = 0; e < 3 * TET_TRI[m][0]; ++e) {
      if (e % 3 == 0 && (tri < 0 || tri >= a.num_triangles)) return;   // offsets that do not belong to this volume: nothing past the arrays
      const int code = TET_TRI[m][1 + e];
      const int qa = corner[code >> 2], qb = corner[code & 3];
      const int lo = qa < qb ? qa : qb, hi = qa < qb ? qb : qa;        // every edge of the split: lo's bits are a subset of hi's
      const long long vlo = corner_index(a.vol, c, lo), vhi = corner_index(a.vol, c, hi);
      const double w = ddiv(c.f[lo], dsub(c.f[lo], c.f[hi]));
      const long long out = 3 * tri + e % 3;
      a.keys[out] = vlo * 7 + EDGE_DIR[hi ^ lo];
      const int li[3] = {c.i + (lo & 1), c.j + ((lo >> 1) & 1), c.k + (lo >> 2)};
      const int hi3[3] = {c.i + (hi & 1), c.j + ((hi >> 1) & 1), c.k + (hi >> 2)};
      const double o[3] = {a.vol.ox, a.vol.oy, a.vol.oz};
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const double plo = voxel_centre(o[x], li[x], a.vol.h), phi = voxel_centre(o[x], hi3[x], a.vol.h);
        a.pos[3 * out + x] = (float)dadd(plo, dmul(w, dsub(phi, plo)));
      }
      const int nlo = a.rgb_cnt[vlo], nhi = a.rgb_cnt[vhi];
#pragma unroll
      for (int x = 0; x < 3; ++x) {
        const double clo = nlo > 0 ? ddiv((double)a.rgb_sum[x * n + vlo], (double)nlo) : 0.5;
        const double chi = nhi > 0 ? ddiv((double)a.rgb_sum[x * n + vhi], (double)nhi) : 0.5;
        const double col = nlo > 0 && nhi > 0 ? dadd(clo, dmul(w, dsub(chi, clo))) : (nlo > 0 ? clo : chi);
        a.col[3 * out + x] = (float)col;
      }
      if (e % 3 == 2) ++tri;
    }
  }
}

}  // namespace

int launch_tsdf_integrate(const TsdfIntegrateArgs& a, hipStream_t st) {
  const long long n = (long long)a.vol.nx * a.vol.ny * a.vol.nz;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)((n + TSDF_THREADS - 1) / TSDF_THREADS)), dim3(TSDF_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("tsdf_integrate");
  return FP_OK;
}

int launch_tsdf_extract(const TsdfExtractArgs& a, bool emit, hipStream_t st) {
  const long long cells = (long long)(a.vol.nx - 1) * (a.vol.ny - 1) * (a.vol.nz - 1);
  const dim3 grid((unsigned)((cells + TSDF_THREADS - 1) / TSDF_THREADS));
  if (emit) hipLaunchKernelGGL(tsdf_emit_kernel, grid, dim3(TSDF_THREADS), 0, st, a, cells);
  else hipLaunchKernelGGL(tsdf_count_kernel, grid, dim3(TSDF_THREADS), 0, st, a, cells);
  FP_CHECK_LAUNCH(emit ? "tsdf_emit" : "tsdf_count");
  return FP_OK;
}
