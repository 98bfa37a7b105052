// ADD and ADI (ADD-S) pose errors of a ragged batch of (estimate, GT) pairs, fp64 throughout (bop_toolkit_lib.pose_error.add / adi;
// DESIGN.md section 22, tests/pose_add_ref.py restates it).
//
// Per pair with model points p_v (its point range, M of them), E_v = R_est p_v + t_est and G_v = R_gt p_v + t_gt:
//   ADD  mean_v |G_v - E_v|
//   ADI  mean_v min_u |G_v - E_u|       (the tree of the toolkit is built on the estimate's points and queried with the GT's)
// Arithmetic as in pose_eval.hip: every product / sum individually rounded, no contraction; R p + t as ((r0 x + r1 y) + r2 z) + t;
// a squared distance as (dx dx + dy dy) + dz dz.  The nearest neighbour compares SQUARED distances and the root is taken once per
// point after the minimum (sqrt is monotone: the minimum of the roots).  The minimum starts at +inf and takes a candidate only when it
// is strictly smaller, so a NaN never wins (np.fmin.reduce(..., initial=inf)); v_min_f64 computes exactly that here -- the running
// minimum is never a NaN, a NaN candidate is quiet (it comes out of arithmetic) and is dropped, and no -0 occurs among sums of squares.
//
// The means have ONE summation order, whatever the grid: points are cut into tiles of FP_POSE_ADD_TILE = 256 consecutive indices, a
// tile's sum adds its values in ascending v (one rounded add each), a pair's sum adds its tile sums in ascending tile order, and the
// sum is divided by (double)M.  A pair's two numbers therefore depend on its own data only.
//
// Two kernels.  pose_add_nn: one 256-thread workgroup per (pair, block of PA_Q * 256 query points); thread k holds the GT placement
// and the running minimum of queries 256 j + k (j < PA_Q) in registers.  The estimate's points stream through LDS in tiles of
// PA_LDS_PTS points, placed from pts by the workgroup as it loads them (one affine triple per point against 256 * PA_Q distance
// evaluations); in the inner loop every lane reads the same LDS address (a broadcast, no bank conflicts) and the three reads of a
// point serve the PA_Q queries of the lane: nine fp64 VALU operations per (query, point), none an FMA.  The ragged last tile is
// padded with NaN points, which never win.  Then each thread takes its roots, the values go to LDS and 2 * PA_Q threads walk one
// sum tile each in ascending order; one (sum_a, sum_n) partial per tile goes to scratch.  pose_add_fold: one wave per pair adds the
// tile partials in tile order and divides.
#include "common.hpp"
#include "kernels.hpp"
#include "rounded.hpp"
#include "../../include/foundpose_amd.h"

namespace {

constexpr int PA_TILE = FP_POSE_ADD_TILE;   // points per sum tile = threads per workgroup
constexpr int PA_Q = 4;                     // queries per thread
constexpr int PA_BLOCK = PA_TILE * PA_Q;    // query points per workgroup
constexpr int PA_LDS_PTS = 1024;            // estimate points per LDS tile (24 KB)
static_assert(PA_BLOCK == FP_POSE_ADD_BLOCK, "FP_POSE_ADD_BLOCK of the header");
static_assert(PA_LDS_PTS % PA_TILE == 0 && PA_LDS_PTS % 4 == 0 && 2 * PA_BLOCK <= 3 * PA_LDS_PTS, "the value tiles reuse the point tile's LDS");

__global__ __launch_bounds__(PA_TILE) void pose_add_nn_kernel(PoseAddArgs a) {
  const PoseAddPair pd = a.pairs[blockIdx.y];
  // the host validated the table; clamped again so that no entry can reach outside pts or parts
  const int off = min(max(pd.pt_off, 0), a.total_pts);
  const int cnt = min(max(pd.pt_cnt, 0), a.total_pts - off);
  const int tiles = min(pd.tiles, (cnt + PA_TILE - 1) / PA_TILE);
  const int q0 = blockIdx.x * PA_BLOCK;
  if (q0 >= cnt || blockIdx.x * PA_Q >= tiles) return;  // workgroup-uniform, before any barrier
  const int k = threadIdx.x;
  const double* P = a.pts + 3 * (size_t)off;
  double E[12], G[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) E[i] = a.est[(size_t)blockIdx.y * 12 + i], G[i] = a.gt[(size_t)blockIdx.y * 12 + i];

  __shared__ double lds[3 * PA_LDS_PTS];
  double* const sx = lds;
  double* const sy = lds + PA_LDS_PTS;
  double* const sz = lds + 2 * PA_LDS_PTS;

  double gx[PA_Q], gy[PA_Q], gz[PA_Q], av[PA_Q], best[PA_Q];
#pragma unroll
  for (int j = 0; j < PA_Q; ++j) {
    const int v = q0 + PA_TILE * j + k;
    const double* p = P + 3 * (size_t)(v < cnt ? v : 0);  // a slot past the range computes on point 0 and is never summed
    const double x = p[0], y = p[1], z = p[2];
    gx[j] = affine(G + 0, G[9], x, y, z);
    gy[j] = affine(G + 3, G[10], x, y, z);
    gz[j] = affine(G + 6, G[11], x, y, z);
    const double dx = dsub(gx[j], affine(E + 0, E[9], x, y, z));
    const double dy = dsub(gy[j], affine(E + 3, E[10], x, y, z));
    const double dz = dsub(gz[j], affine(E + 6, E[11], x, y, z));
    av[j] = __dsqrt_rn(sqdist(dx, dy, dz));
    best[j] = __longlong_as_double(0x7ff0000000000000ll);
  }

  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int t0 = 0; t0 < cnt; t0 += PA_LDS_PTS) {
    __syncthreads();  // the previous tile has been read
#pragma unroll
    for (int i = k; i < PA_LDS_PTS; i += PA_TILE) {
      const int u = t0 + i;
      double ex = nan, ey = nan, ez = nan;  // padding of the ragged last tile: a NaN distance never wins
      if (u < cnt) {
        const double x = P[3 * (size_t)u], y = P[3 * (size_t)u + 1], z = P[3 * (size_t)u + 2];
        ex = affine(E + 0, E[9], x, y, z);
        ey = affine(E + 3, E[10], x, y, z);
        ez = affine(E + 6, E[11], x, y, z);
      }
      sx[i] = ex, sy[i] = ey, sz[i] = ez;
    }
    __syncthreads();
    const int n = (min(PA_LDS_PTS, cnt - t0) + 3) & ~3;  // workgroup-uniform, padded to the unroll
    for (int i = 0; i < n; i += 4) {
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const double ex = sx[i + ii], ey = sy[i + ii], ez = sz[i + ii];
#pragma unroll
        for (int j = 0; j < PA_Q; ++j) best[j] = fmin(best[j], sqdist(dsub(gx[j], ex), dsub(gy[j], ey), dsub(gz[j], ez)));
      }
    }
  }

  // the values of the block's PA_Q sum tiles -> LDS: va[j][k], vn[j][k]
  __syncthreads();
  double* const va = lds;
  double* const vn = lds + PA_BLOCK;
#pragma unroll
  for (int j = 0; j < PA_Q; ++j) {
    va[PA_TILE * j + k] = av[j];
    vn[PA_TILE * j + k] = __dsqrt_rn(best[j]);
  }
  __syncthreads();
  if (k < 2 * PA_Q) {  // thread 2 j + w walks sum tile j of metric w in ascending point order
    const int j = k >> 1, tile = blockIdx.x * PA_Q + j;
    if (tile < tiles) {
      const double* val = (k & 1 ? vn : va) + PA_TILE * j;
      const int m = min(PA_TILE, cnt - (q0 + PA_TILE * j));
      double s = val[0];
      for (int i = 1; i < m; ++i) s = dadd(s, val[i]);
      a.parts[2 * ((size_t)pd.part_base + tile) + (k & 1)] = s;
    }
  }
}

__global__ __launch_bounds__(64) void pose_add_fold_kernel(PoseAddArgs a) {
  const PoseAddPair pd = a.pairs[blockIdx.x];
  const int off = min(max(pd.pt_off, 0), a.total_pts);
  const int cnt = min(max(pd.pt_cnt, 0), a.total_pts - off);
  const int tiles = min(pd.tiles, (cnt + PA_TILE - 1) / PA_TILE);
  if (tiles < 1) return;  // wave-uniform
  const double* part = a.parts + 2 * (size_t)pd.part_base;
  __shared__ double sh[2 * 64];
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int t0 = 0; t0 < tiles; t0 += 64) {
    __syncthreads();
    if (t0 + lane < tiles) sh[2 * lane] = part[2 * (size_t)(t0 + lane)], sh[2 * lane + 1] = part[2 * (size_t)(t0 + lane) + 1];
    __syncthreads();
    if (lane < 2) {  // lane w adds the tile sums of metric w in tile order
      const int m = min(64, tiles - t0);
      for (int i = 0; i < m; ++i) s = (t0 + i == 0) ? sh[2 * i + lane] : dadd(s, sh[2 * i + lane]);
    }
  }
  if (lane < 2) a.err[2 * (size_t)blockIdx.x + lane] = __ddiv_rn(s, (double)cnt);
}

}  // namespace

int launch_pose_add_errors(const PoseAddArgs& a, int num_pairs, int max_blocks, hipStream_t st) {
  hipLaunchKernelGGL(pose_add_nn_kernel, dim3(max_blocks, num_pairs), dim3(PA_TILE), 0, st, a);
  FP_CHECK_LAUNCH("pose_add_nn");
  hipLaunchKernelGGL(pose_add_fold_kernel, dim3(num_pairs), dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("pose_add_fold");
  return FP_OK;
}
