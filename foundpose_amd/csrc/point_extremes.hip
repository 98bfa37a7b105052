// Farthest pair and directed Hausdorff distances inside one point set, fp64 throughout (models_info.py: an object's diameter and its
// symmetry candidates; DESIGN.md section 26, tests/models_info_ref.py restates it).
//
//   fp_pts_diameter        sqrt(max_{i<j} d2(p_i, p_j)) and the lexicographically lowest pair (i, j) that attains it
//   fp_directed_hausdorff  per candidate k with q_v = R_k p_v + t_k:  sqrt(max_v min_u d2(q_v, p_u)), v = 0, s, 2s, ..., u over all V
//                          points, and the lowest v that attains it
// Arithmetic as in pose_add.hip: every product / sum individually rounded, no contraction; R p + t as ((r0 x + r1 y) + r2 z) + t; a
// squared distance as (dx dx + dy dy) + dz dz; SQUARED distances are compared and one correctly rounded root is taken after the
// reduction (sqrt is monotone).  The minimum starts at +inf and takes a candidate only when it is strictly smaller, the maximum of the
// diameter starts at 0 with the pair (0, 0) and takes a candidate only when it is strictly greater: a NaN never wins (v_min_f64 /
// v_max_f64 drop a quiet NaN operand; the running value is never a NaN).  Maxima with their lowest index are associative, so the result
// does not depend on the launch shape.
//
// Both searches are pose_add_nn_kernel's loop: 256 threads, PE_Q = 4 queries per thread in registers, 1 024 targets per LDS tile read
// as broadcasts, nine fp64 VALU operations per point pair.  The targets are the untransformed points, so a tile is loaded as it is.
//   pts_hausdorff_kernel  one workgroup per (block of 1 024 queries, candidate), all V targets streamed; one (max, v) partial per
//                         workgroup -> scratch; pts_hausdorff_fold_kernel: one wave per candidate.
//   pts_diameter_kernel   one workgroup per pair of 1 024-point tiles (a, b), a <= b: the queries are tile a, the targets tile b.  The
//                         inner loop keeps, per query, the maximum and the GROUP of four targets it came from (three v_max_f64, one
//                         compare and three selects per four pairs); afterwards the thread finds the first target of that group that
//                         gives the same bits.  In the diagonal tile pair a query also meets targets u <= i: d2 is symmetric bit for
//                         bit and d2(i, i) is 0 or NaN, so with the pair stored as (min, max) the lowest pair still wins (the lowest
//                         pair (i*, j*) is reported by query i*: no u < i* attains the maximum, or (u, i*) would be lower).
//                         pts_diameter_fold_kernel: one workgroup folds the partials and takes the root.
#include "common.hpp"
#include "kernels.hpp"
#include "rounded.hpp"
#include "../../include/foundpose_amd.h"

namespace {

constexpr int PE_THREADS = 256;
constexpr int PE_Q = 4;                     // queries per thread
constexpr int PE_TILE = PE_THREADS * PE_Q;  // queries per workgroup = targets per LDS tile (24 KB)
static_assert(PE_TILE == FP_PTS_TILE, "FP_PTS_TILE of the header");

// a maximum with the index pair it came from; v is never a NaN.  `wins`: greater, or equal with the lexicographically lower pair.
struct Cand { double v; int a, b; };
FP_DEVICE bool wins(const Cand& x, const Cand& y) { return x.v > y.v || (x.v == y.v && (x.a < y.a || (x.a == y.a && x.b < y.b))); }
FP_DEVICE Cand wave_best(Cand c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const Cand t{__shfl_xor(c.v, o, 64), __shfl_xor(c.a, o, 64), __shfl_xor(c.b, o, 64)};
    if (wins(t, c)) c = t;
  }
  return c;
}
// the best of a 256-thread workgroup, valid in thread 0; `sh` holds 4 entries
FP_DEVICE Cand block_best(Cand c, Cand* sh) {
  c = wave_best(c);
  __syncthreads();  // sh may alias memory the workgroup has been reading
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < PE_THREADS / 64; ++w)
      if (wins(sh[w], c)) c = sh[w];
  }
  return c;
}

// the workgroup loads targets [t0, t0 + PE_TILE) of P (V points) into the three LDS arrays; the ragged end is padded with NaN points
FP_DEVICE void load_tile(const double* P, int V, int t0, double* sx, double* sy, double* sz) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
  for (int i = threadIdx.x; i < PE_TILE; i += PE_THREADS) {
    const long long u = (long long)t0 + i;
    double x = nan, y = nan, z = nan;
    if (u < V) x = P[3 * u], y = P[3 * u + 1], z = P[3 * u + 2];
    sx[i] = x, sy[i] = y, sz[i] = z;
  }
}

__global__ __launch_bounds__(PE_THREADS) void pts_hausdorff_kernel(PtsHausdorffArgs a) {
  const int k = threadIdx.x;
  const int q0 = blockIdx.x * PE_TILE;  // first query of the block; the host sized the grid: q0 < nq
  const double* P = a.pts;
  double T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = a.tf[(size_t)blockIdx.y * 12 + i];

  __shared__ double lds[3 * PE_TILE];
  double* const sx = lds;
  double* const sy = lds + PE_TILE;
  double* const sz = lds + 2 * PE_TILE;

  double gx[PE_Q], gy[PE_Q], gz[PE_Q], best[PE_Q];
#pragma unroll
  for (int j = 0; j < PE_Q; ++j) {
    const int qi = q0 + PE_THREADS * j + k;
    const long long v = qi < a.nq ? (long long)qi * a.stride : 0;  // a slot past the last query computes on point 0 and is never reported
    const double x = P[3 * v], y = P[3 * v + 1], z = P[3 * v + 2];
    gx[j] = affine(T + 0, T[9], x, y, z);
    gy[j] = affine(T + 3, T[10], x, y, z);
    gz[j] = affine(T + 6, T[11], x, y, z);
    best[j] = __longlong_as_double(0x7ff0000000000000ll);
  }

  for (int t0 = 0; t0 < a.V; t0 += PE_TILE) {
    __syncthreads();  // the previous tile has been read
    load_tile(P, a.V, t0, sx, sy, sz);
    __syncthreads();
    const int n = (min(PE_TILE, a.V - t0) + 3) & ~3;  // workgroup-uniform, padded to the unroll
    for (int i = 0; i < n; i += 4) {
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const double ex = sx[i + ii], ey = sy[i + ii], ez = sz[i + ii];
#pragma unroll
        for (int j = 0; j < PE_Q; ++j) best[j] = fmin(best[j], sqdist(dsub(gx[j], ex), dsub(gy[j], ey), dsub(gz[j], ez)));
      }
    }
  }

  Cand c{-1.0, 0x7fffffff, 0};  // every m_v is >= 0 or +inf
#pragma unroll
  for (int j = 0; j < PE_Q; ++j) {  // ascending v within the thread: strictly greater keeps the lowest
    const int qi = q0 + PE_THREADS * j + k;
    if (qi < a.nq && best[j] > c.v) c = Cand{best[j], (int)((long long)qi * a.stride), 0};
  }
  c = block_best(c, reinterpret_cast<Cand*>(lds));
  if (k == 0) a.parts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = PtsPart{c.v, c.a, c.b};
}

__global__ __launch_bounds__(64) void pts_hausdorff_fold_kernel(PtsHausdorffArgs a, int blocks) {
  const PtsPart* part = a.parts + (size_t)blockIdx.x * blocks;
  Cand c{-1.0, 0x7fffffff, 0};
  for (int i = threadIdx.x; i < blocks; i += 64) {
    const Cand t{part[i].v, part[i].a, part[i].b};
    if (wins(t, c)) c = t;
  }
  c = wave_best(c);
  if (threadIdx.x == 0) a.out_h[blockIdx.x] = __dsqrt_rn(c.v), a.out_arg[blockIdx.x] = c.a;
}

__global__ __launch_bounds__(PE_THREADS) void pts_diameter_kernel(PtsDiameterArgs a) {
  // blockIdx.x = the tile pair's position in the row-major upper triangle: row ta starts at ta (2 T - ta + 1) / 2
  const long long T = a.tiles, p = blockIdx.x;
  int ta = (int)((((double)(2 * T + 1)) - sqrt((double)((2 * T + 1) * (2 * T + 1) - 8 * p))) * 0.5);
  ta = min(max(ta, 0), (int)T - 1);
  while (ta > 0 && (long long)ta * (2 * T - ta + 1) / 2 > p) --ta;
  while (ta + 1 < T && (long long)(ta + 1) * (2 * T - ta) / 2 <= p) ++ta;
  const int tb = ta + (int)(p - (long long)ta * (2 * T - ta + 1) / 2);  // ta <= tb < T
  const int k = threadIdx.x;
  const double* P = a.pts;

  __shared__ double lds[3 * PE_TILE];
  double* const sx = lds;
  double* const sy = lds + PE_TILE;
  double* const sz = lds + 2 * PE_TILE;

  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double gx[PE_Q], gy[PE_Q], gz[PE_Q], best[PE_Q];
  int grp[PE_Q];
#pragma unroll
  for (int j = 0; j < PE_Q; ++j) {
    const long long i = (long long)ta * PE_TILE + PE_THREADS * j + k;
    gx[j] = gy[j] = gz[j] = nan;  // a slot past the last point never wins
    if (i < a.V) gx[j] = P[3 * i], gy[j] = P[3 * i + 1], gz[j] = P[3 * i + 2];
    best[j] = 0.0;
    grp[j] = -1;
  }

  const int t0 = tb * PE_TILE;
  load_tile(P, a.V, t0, sx, sy, sz);
  __syncthreads();
  const int n = (min(PE_TILE, a.V - t0) + 3) & ~3;  // workgroup-uniform
  for (int i = 0; i < n; i += 4) {
    double ex[4], ey[4], ez[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) ex[ii] = sx[i + ii], ey[ii] = sy[i + ii], ez[ii] = sz[i + ii];
#pragma unroll
    for (int j = 0; j < PE_Q; ++j) {
      double d[4];
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) d[ii] = sqdist(dsub(gx[j], ex[ii]), dsub(gy[j], ey[ii]), dsub(gz[j], ez[ii]));
      const double m = fmax(fmax(d[0], d[1]), fmax(d[2], d[3]));  // a NaN operand is dropped
      if (m > best[j]) best[j] = m, grp[j] = i;
    }
  }

  Cand c{0.0, 0, 0};  // the maximum starts at 0 with the pair (0, 0)
#pragma unroll
  for (int j = 0; j < PE_Q; ++j) {
    if (grp[j] < 0) continue;
    int u = -1;  // the first target of the group that gives the maximum's bits (the tile is still in LDS)
#pragma unroll
    for (int ii = 3; ii >= 0; --ii) {
      const int g = grp[j] + ii;
      if (sqdist(dsub(gx[j], sx[g]), dsub(gy[j], sy[g]), dsub(gz[j], sz[g])) == best[j]) u = t0 + g;
    }
    const int i = ta * PE_TILE + PE_THREADS * j + k;
    const Cand t{best[j], min(i, u), max(i, u)};
    if (u >= 0 && wins(t, c)) c = t;  // best[j] > 0 here
  }
  c = block_best(c, reinterpret_cast<Cand*>(lds));
  if (k == 0) a.parts[blockIdx.x] = PtsPart{c.v, c.a, c.b};
}

__global__ __launch_bounds__(PE_THREADS) void pts_diameter_fold_kernel(PtsDiameterArgs a, long long pairs) {
  __shared__ Cand sh[PE_THREADS / 64];
  Cand c{0.0, 0, 0};
  for (long long i = threadIdx.x; i < pairs; i += PE_THREADS) {
    const Cand t{a.parts[i].v, a.parts[i].a, a.parts[i].b};
    if (wins(t, c)) c = t;  // a workgroup that found nothing above 0 wrote (0, (0, 0)), the start itself
  }
  c = block_best(c, sh);
  if (threadIdx.x == 0) a.out_d[0] = __dsqrt_rn(c.v), a.out_pair[0] = c.a, a.out_pair[1] = c.b;
}

}  // namespace

int launch_pts_hausdorff(const PtsHausdorffArgs& a, int K, hipStream_t st) {
  const int blocks = (a.nq + PE_TILE - 1) / PE_TILE;
  hipLaunchKernelGGL(pts_hausdorff_kernel, dim3(blocks, K), dim3(PE_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("pts_hausdorff");
  hipLaunchKernelGGL(pts_hausdorff_fold_kernel, dim3(K), dim3(64), 0, st, a, blocks);
  FP_CHECK_LAUNCH("pts_hausdorff_fold");
  return FP_OK;
}

int launch_pts_diameter(const PtsDiameterArgs& a, hipStream_t st) {
  const long long pairs = (long long)a.tiles * (a.tiles + 1) / 2;
  hipLaunchKernelGGL(pts_diameter_kernel, dim3((unsigned)pairs), dim3(PE_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("pts_diameter");
  hipLaunchKernelGGL(pts_diameter_fold_kernel, dim3(1), dim3(PE_THREADS), 0, st, a, pairs);
  FP_CHECK_LAUNCH("pts_diameter_fold");
  return FP_OK;
}
