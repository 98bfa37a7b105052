// Class-agnostic mask proposals from an organised depth image: the supporting planes by RANSAC, the pixels that
// stand on them, their connected components along depth discontinuities, the components' table and COCO run lengths.
//
//   planes      dp_eligible_kernel marks the frame's valid pixels that no earlier plane took and counts both; dp_hypothesis_kernel, one
//               256-thread workgroup per (frame, hypothesis): three distinct eligible pixels from the keyed sampler of ransac.hpp (pair key
//               frame key * 8 + plane index), the plane through their points, the eligible sub-grid pixels within the threshold (an
//               integer block reduction); dp_winner_kernel: the first hypothesis of the highest count; then two least-squares refits
//               over ALL eligible pixels within the threshold, each a centroid pass and a scatter pass of dp_refit_partial_kernel
//               (per-workgroup fp64 partials in a fixed order) folded in ascending order by one lane (dp_refit_fold_kernel), which also
//               takes the eigenvector of the smallest eigenvalue by cyclic Jacobi; a last count pass gives the support.
//   components  dp_tile_kernel: foreground test (fp64) and a union-find over a 32 x 32 tile in LDS; dp_merge_kernel: unions across the
//               tile borders in global memory; dp_flatten_kernel: every pixel to its root.  Three launches: no kernel relies on a plain
//               load seeing another workgroup's store.  In the merge every parent word is read by an agent-scope atomic load and
//               written by atomicMin only, whose RETURNED value drives the union; parents only decrease, so every loop ends on its
//               own and none waits for another workgroup.  A component's label is the smallest linear index of its pixels.
//   table       dp_slot_init / dp_stats (integer atomics on the root's slot, aggregated per wave), dp_candidates (area filter, drop of
//               components a finer level kept), dp_select (one workgroup per frame picks by area descending, label ascending),
//               dp_rank_map.
//   runs        dp_run_events_kernel: one thread per column-major position; where the rank changes a run starts and a run ends.
// Floating point: fp64 with every operation rounded on its own (no contraction in this file), fp32 _rn intrinsics for the connectivity.
#include <climits>

#include "common.hpp"
#pragma clang fp contract(off)   // in front of rot.hpp / ransac.hpp: cross3, dot3 and normalize3 are compiled here without FMAs
#include "kernels.hpp"
#include "ransac.hpp"
#include "rounded.hpp"
#include "../../include/foundpose_amd.h"

namespace {

constexpr int DP_THREADS = 256;
constexpr int DP_PPT = 4;                        // pixels per thread of the per-pixel kernels
constexpr int DP_LAST_ATTEMPT = 64;              // an index is drawn at most 65 times
constexpr double DP_THIN2 = 1e-12;               // a triangle is too thin when |e1 x e2|^2 <= 1e-12 |e1|^2 |e2|^2 (sine of the angle <= 1e-6)
constexpr int DP_CHUNK = FP_DEPTH_PLANE_CHUNK;   // pixels per workgroup of the refit passes
constexpr int DP_TILE = 32;                      // side of a components tile
constexpr int DP_JACOBI_SWEEPS = 30;
enum { ST_PLANE = 0, ST_CENTROID = 4, ST_COUNT = 7, ST_ALIVE = 8, ST_SIZE = 16 };   // a frame's refit state, in doubles
enum { SL_AREA = 0, SL_X0, SL_Y0, SL_X1, SL_Y1, SL_RANK, SL_SIZE };                  // a label's slot, in ints

FP_DEVICE bool dp_valid(float D, double max_depth) { return D > 0.f && (max_depth == 0.0 || (double)D <= max_depth); }
// the point of pixel (u, v): ((u - cx) / fx z, (v - cy) / fy z, z)
FP_DEVICE void dp_point(const DpFrame& c, int u, int v, float D, double* X) {
  const double z = (double)D;
  X[0] = dmul(ddiv(dsub((double)u, c.cx), c.fx), z);
  X[1] = dmul(ddiv(dsub((double)v, c.cy), c.fy), z);
  X[2] = z;
}
// height over the plane (n, d): ((n0 x + n1 y) + n2 z) + d
FP_DEVICE double dp_height(const double* pl, const double* X) { return dadd(dot3(pl[0], pl[1], pl[2], X[0], X[1], X[2]), pl[3]); }
FP_DEVICE int dp_plane_index(const int* num_prior, int f) {   // -1: the frame is skipped
  const int k = num_prior[f];
  return (k < 0 || k >= FP_DEPTH_MAX_PLANES) ? -1 : k;
}
FP_DEVICE int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------------------------------------ planes
__global__ __launch_bounds__(DP_THREADS) void dp_eligible_kernel(DpPlaneArgs a) {
  const int f = blockIdx.y, tid = threadIdx.x;
  const long long hw = (long long)a.h * a.w;
  const DpFrame fr = a.frames[f];
  const int k = dp_plane_index(a.num_prior, f);
  const float* D = a.depth + f * hw;
  int nv = 0, ne = 0;
#pragma unroll
  for (int j = 0; j < DP_PPT; ++j) {
    const long long p = ((long long)blockIdx.x * DP_PPT + j) * DP_THREADS + tid;
    if (p >= hw) continue;
    const float d = D[p];
    const bool valid = dp_valid(d, a.max_depth);
    bool el = valid && k >= 0;
    if (el) {
      double X[3];
      dp_point(fr, (int)(p % a.w), (int)(p / a.w), d, X);
      for (int q = 0; q < k; ++q) el = el && !(fabs(dp_height(a.prior + ((size_t)f * FP_DEPTH_MAX_PLANES + q) * 4, X)) <= a.thresh);
    }
    a.elig[f * hw + p] = el ? 1 : 0;
    nv += valid, ne += el;
  }
  __shared__ int red[DP_THREADS / 64][2];
  nv = wave_sum_int(nv), ne = wave_sum_int(ne);
  if ((tid & 63) == 0) red[tid >> 6][0] = nv, red[tid >> 6][1] = ne;
  __syncthreads();
  if (tid < 2) {
    const int s = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    if (s) atomicAdd(a.cnt2 + f * 2 + tid, s);
  }
}

// hypothesis h of a frame -> its plane (n, d) with d >= 0; false: dead
FP_DEVICE bool dp_hypothesis(const DpPlaneArgs& a, const DpFrame& fr, int f, int k, int h, double* pl) {
  const long long hw = (long long)a.h * a.w;
  const unsigned char* el = a.elig + f * hw;
  const unsigned long long pk = fr.key * 8ull + (unsigned long long)k;
  const unsigned long long base = ransac_pair_base(a.seed, &pk, 0);
  int id[3];
  if (!ransac_draw<3, DP_LAST_ATTEMPT>(ransac_hypothesis_key(base, h), (int)hw, id, [&](int c) -> bool { return el[c] != 0; })) return false;
  double X[3][3];
  for (int j = 0; j < 3; ++j) dp_point(fr, id[j] % a.w, id[j] / a.w, a.depth[f * hw + id[j]], X[j]);
  const double e1[3] = {X[1][0] - X[0][0], X[1][1] - X[0][1], X[1][2] - X[0][2]};
  const double e2[3] = {X[2][0] - X[0][0], X[2][1] - X[0][1], X[2][2] - X[0][2]};
  double n[3];
  cross3(e1, e2, n);
  const double nn = dot3(n, n), l1 = dot3(e1, e1), l2 = dot3(e2, e2);
  if (!(nn > DP_THIN2 * (l1 * l2))) return false;
  if (!normalize3(n)) return false;
  double d = -dot3(n, X[0]);
  if (d < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; d = -d; }
  pl[0] = n[0], pl[1] = n[1], pl[2] = n[2], pl[3] = d;
  return true;
}

__global__ __launch_bounds__(DP_THREADS) void dp_hypothesis_kernel(DpPlaneArgs a) {
  const int h = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const int k = dp_plane_index(a.num_prior, f);
  __shared__ double s_pl[4];
  __shared__ int s_alive, s_red[DP_THREADS / 64];
  const DpFrame fr = a.frames[f];
  if (tid == 0) {
    double pl[4] = {0.0, 0.0, 0.0, 0.0};
    s_alive = (k >= 0 && dp_hypothesis(a, fr, f, k, h, pl)) ? 1 : 0;
    for (int i = 0; i < 4; ++i) s_pl[i] = pl[i];
  }
  __syncthreads();
  int c = 0;
  if (s_alive) {   // block-uniform
    const double pl[4] = {s_pl[0], s_pl[1], s_pl[2], s_pl[3]};
    const long long hw = (long long)a.h * a.w;
    const int gx = (a.w + a.stride - 1) / a.stride, gy = (a.h + a.stride - 1) / a.stride;
    for (int i = tid; i < gx * gy; i += DP_THREADS) {
      const int y = (i / gx) * a.stride, x = (i % gx) * a.stride;
      const long long p = (long long)y * a.w + x;
      if (!a.elig[f * hw + p]) continue;
      double X[3];
      dp_point(fr, x, y, a.depth[f * hw + p], X);
      c += fabs(dp_height(pl, X)) <= a.thresh;
    }
  }
  c = wave_sum_int(c);
  if ((tid & 63) == 0) s_red[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) a.hyp_cnt[(size_t)f * a.hyp + h] = s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// the first hypothesis of the highest count; its plane into the frame's state
__global__ __launch_bounds__(DP_THREADS) void dp_winner_kernel(DpPlaneArgs a) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const int k = dp_plane_index(a.num_prior, f);
  unsigned long long best = 0;   // (count << 32) | (0xffffffff - h): the maximum is the first of the highest count
  for (int h = tid; h < a.hyp; h += DP_THREADS) {
    const unsigned long long key = ((unsigned long long)(unsigned)a.hyp_cnt[(size_t)f * a.hyp + h] << 32) | (0xffffffffu - (unsigned)h);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(best, o, 64);
    best = t > best ? t : best;
  }
  __shared__ unsigned long long s_best[DP_THREADS / 64];
  if ((tid & 63) == 0) s_best[tid >> 6] = best;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 0; w < DP_THREADS / 64; ++w) best = s_best[w] > best ? s_best[w] : best;
  const int win = (int)(0xffffffffu - (unsigned)(best & 0xffffffffu)), cnt = (int)(best >> 32);
  double* st = a.state + (size_t)f * ST_SIZE;
  double pl[4] = {0.0, 0.0, 0.0, 0.0};
  const bool alive = k >= 0 && dp_hypothesis(a, a.frames[f], f, k, win, pl);
  for (int i = 0; i < ST_SIZE; ++i) st[i] = 0.0;
  for (int i = 0; i < 4; ++i) st[ST_PLANE + i] = pl[i];
  st[ST_ALIVE] = alive ? 1.0 : 0.0;
  int* info = a.info + (size_t)f * 8;
  info[0] = k >= 0 ? win : -1;
  info[1] = k >= 0 ? cnt : 0;
  info[2] = 0;
  info[3] = a.cnt2[f * 2 + 1];
  info[4] = a.cnt2[f * 2 + 0];
  info[5] = 0;
  info[6] = k;
  info[7] = 0;
}

// MODE 0: (count, sum x, sum y, sum z) of the eligible pixels within the threshold of the state's plane; MODE 1: their scatter about
// the state's centroid (xx, xy, xz, yy, yz, zz).  One partial row of 8 doubles per workgroup.
template <int MODE>
__global__ __launch_bounds__(DP_THREADS) void dp_refit_partial_kernel(DpPlaneArgs a) {
  const int f = blockIdx.y, tid = threadIdx.x;
  const long long hw = (long long)a.h * a.w;
  const double* st = a.state + (size_t)f * ST_SIZE;
  const DpFrame fr = a.frames[f];
  constexpr int NV = MODE == 0 ? 4 : 6;
  double v[NV];
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  if (st[ST_ALIVE] != 0.0) {   // block-uniform
    const double pl[4] = {st[0], st[1], st[2], st[3]}, c[3] = {st[ST_CENTROID], st[ST_CENTROID + 1], st[ST_CENTROID + 2]};
    for (int j = 0; j < DP_CHUNK / DP_THREADS; ++j) {
      const long long p = (long long)blockIdx.x * DP_CHUNK + j * DP_THREADS + tid;
      if (p >= hw || !a.elig[f * hw + p]) continue;
      double X[3];
      dp_point(fr, (int)(p % a.w), (int)(p / a.w), a.depth[f * hw + p], X);
      if (!(fabs(dp_height(pl, X)) <= a.thresh)) continue;
      if constexpr (MODE == 0) {
        v[0] += 1.0, v[1] += X[0], v[2] += X[1], v[3] += X[2];
      } else {
        const double x = X[0] - c[0], y = X[1] - c[1], z = X[2] - c[2];
        v[0] += x * x, v[1] += x * y, v[2] += x * z, v[3] += y * y, v[4] += y * z, v[5] += z * z;
      }
    }
  }
  __shared__ double acc[4][8];
  block_partials<NV>(v, acc, tid);
  if (tid < 8) a.part[((size_t)f * a.chunks + blockIdx.x) * 8 + tid] = tid < NV ? block_total(acc, tid) : 0.0;
}

// Eigenvector of the smallest eigenvalue of the symmetric 3x3 M (row-major, destroyed) by cyclic Jacobi, the scheme of kabsch.hip's
// jacobi4_largest: pairs (0,1) (0,2) (1,2); the first of equal eigenvalues.
FP_DEVICE void jacobi3_smallest(double* M, double* q) {
  double V[9];
  for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < DP_JACOBI_SWEEPS; ++sweep) {
    double off = 0.0, all = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        all += M[i * 3 + j] * M[i * 3 + j];
        if (i != j) off += M[i * 3 + j] * M[i * 3 + j];
      }
    if (!(off > 1e-30 * all)) break;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int r = p + 1; r < 3; ++r) {
        const double apr = M[p * 3 + r];
        if (apr == 0.0) continue;
        const double theta = (M[r * 3 + r] - M[p * 3 + p]) / (2.0 * apr);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 3; ++k) {
          const double mkp = M[k * 3 + p], mkr = M[k * 3 + r];
          M[k * 3 + p] = c * mkp - s * mkr;
          M[k * 3 + r] = s * mkp + c * mkr;
        }
        for (int k = 0; k < 3; ++k) {
          const double mpk = M[p * 3 + k], mrk = M[r * 3 + k];
          M[p * 3 + k] = c * mpk - s * mrk;
          M[r * 3 + k] = s * mpk + c * mrk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k * 3 + p], vkr = V[k * 3 + r];
          V[k * 3 + p] = c * vkp - s * vkr;
          V[k * 3 + r] = s * vkp + c * vkr;
        }
      }
  }
  int best = 0;
  for (int i = 1; i < 3; ++i)
    if (M[i * 4] < M[best * 4]) best = i;
  for (int k = 0; k < 3; ++k) q[k] = V[k * 3 + best];
}

// One lane per frame folds the partial rows in ascending order.  MODE 0: the centroid into the state; MODE 1: the scatter's normal
// becomes the state's plane (kept as it is with fewer than 3 pixels); MODE 2: after a MODE-0 pass on the final plane, the outputs.
template <int MODE>
__global__ void dp_refit_fold_kernel(DpPlaneArgs a) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.n) return;
  double* st = a.state + (size_t)f * ST_SIZE;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int c = 0; c < a.chunks; ++c)
    for (int i = 0; i < 8; ++i) s[i] += a.part[((size_t)f * a.chunks + c) * 8 + i];
  if constexpr (MODE == 0 || MODE == 2) {
    st[ST_COUNT] = s[0];
    if (s[0] > 0.0)
      for (int r = 0; r < 3; ++r) st[ST_CENTROID + r] = s[1 + r] / s[0];
  }
  if constexpr (MODE == 1) {
    if (st[ST_ALIVE] != 0.0 && st[ST_COUNT] >= 3.0) {
      double M[9] = {s[0], s[1], s[2], s[1], s[3], s[4], s[2], s[4], s[5]}, n[3];
      jacobi3_smallest(M, n);
      double d = -(n[0] * st[ST_CENTROID] + n[1] * st[ST_CENTROID + 1] + n[2] * st[ST_CENTROID + 2]);
      if (d < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; d = -d; }
      st[0] = n[0], st[1] = n[1], st[2] = n[2], st[3] = d;
    }
  }
  if constexpr (MODE == 2) {
    int* info = a.info + (size_t)f * 8;
    const bool alive = st[ST_ALIVE] != 0.0;
    const int support = alive ? (int)s[0] : 0;
    const bool accepted = alive && support >= 3 && (double)support >= a.min_share * (double)info[4];
    info[2] = support;
    info[5] = accepted ? 1 : 0;
    for (int i = 0; i < 4; ++i) a.plane_out[(size_t)f * 4 + i] = alive ? st[i] : 0.0;
  }
}

// -------------------------------------------------------------------------------------------------------------------------- components
FP_DEVICE bool dp_connected(float za, float zb, float connect_mm, float slope_fx) {   // 0: not foreground
  if (!(za > 0.f) || !(zb > 0.f)) return false;
  return fabsf(__fsub_rn(za, zb)) <= __fadd_rn(connect_mm, __fmul_rn(slope_fx, fminf(za, zb)));
}

// union-find on parent words that only ever decrease: SCOPE is the memory scope of the loads (workgroup for LDS, agent for global)
template <int SCOPE>
FP_DEVICE int uf_find(int* p, int i) {
  for (;;) {
    const int q = __hip_atomic_load(p + i, __ATOMIC_RELAXED, SCOPE);
    if (q == i) return i;
    i = q;
  }
}
template <int SCOPE>
FP_DEVICE void uf_union(int* p, int a, int b) {
  for (;;) {
    a = uf_find<SCOPE>(p, a);
    b = uf_find<SCOPE>(p, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(p + a, b);   // hook the larger root under the smaller; the returned value tells whether a was still a root
    if (old == a) return;
    a = old;                               // a had a parent `old` < a already: unite that with b
  }
}

__global__ __launch_bounds__(DP_THREADS) void dp_tile_kernel(DpCompArgs a) {
  __shared__ float z[DP_TILE * DP_TILE];
  __shared__ int par[DP_TILE * DP_TILE];
  const int f = blockIdx.z, tid = threadIdx.x;
  const int tx0 = blockIdx.x * DP_TILE, ty0 = blockIdx.y * DP_TILE;
  const long long hw = (long long)a.h * a.w;
  const DpFrame fr = a.frames[f];
  int np = a.num_planes[f];
  np = np < 0 ? 0 : (np > FP_DEPTH_MAX_PLANES ? FP_DEPTH_MAX_PLANES : np);
#pragma unroll
  for (int j = 0; j < DP_PPT; ++j) {
    const int l = j * DP_THREADS + tid, x = tx0 + (l % DP_TILE), y = ty0 + (l / DP_TILE);
    float zz = 0.f;
    if (x < a.w && y < a.h) {
      const float d = a.depth[f * hw + (long long)y * a.w + x];
      bool fg = dp_valid(d, a.max_depth);
      if (fg) {
        double X[3];
        dp_point(fr, x, y, d, X);
        for (int q = 0; q < np; ++q) fg = fg && dp_height(a.planes + ((size_t)f * FP_DEPTH_MAX_PLANES + q) * 4, X) > a.margin;
      }
      zz = fg ? d : 0.f;
    }
    z[l] = zz;
    par[l] = l;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < DP_PPT; ++j) {
    const int l = j * DP_THREADS + tid;
    if (!(z[l] > 0.f)) continue;
    if ((l % DP_TILE) > 0 && dp_connected(z[l], z[l - 1], a.connect_mm, fr.slope_fx)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, l - 1);
    if (l >= DP_TILE && dp_connected(z[l], z[l - DP_TILE], a.connect_mm, fr.slope_fx)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, l - DP_TILE);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < DP_PPT; ++j) {
    const int l = j * DP_THREADS + tid, x = tx0 + (l % DP_TILE), y = ty0 + (l / DP_TILE);
    if (x >= a.w || y >= a.h) continue;
    int out = -1;
    if (z[l] > 0.f) {
      const int r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l);   // local order = global order inside a tile
      out = (ty0 + r / DP_TILE) * a.w + tx0 + (r % DP_TILE);
    }
    a.parent[f * hw + (long long)y * a.w + x] = out;
  }
}

// one thread per pixel on the first column / row of a tile that has a neighbour tile to the left / above
__global__ __launch_bounds__(DP_THREADS) void dp_merge_kernel(DpCompArgs a) {
  const int f = blockIdx.y;
  const long long hw = (long long)a.h * a.w;
  const int nbx = (a.w - 1) / DP_TILE, nby = (a.h - 1) / DP_TILE;
  const long long t = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  int x, y, dx, dy;
  if (t < (long long)nbx * a.h) { x = ((int)(t / a.h) + 1) * DP_TILE; y = (int)(t % a.h); dx = 1; dy = 0; }
  else {
    const long long u = t - (long long)nbx * a.h;
    if (u >= (long long)nby * a.w) return;
    y = ((int)(u / a.w) + 1) * DP_TILE; x = (int)(u % a.w); dx = 0; dy = 1;
  }
  const int p = y * a.w + x, q = (y - dy) * a.w + (x - dx);
  int* par = a.parent + f * hw;
  // whether a pixel is foreground never changes in this launch (a foreground parent word stays >= 0), only which root it points to
  const float slope = a.frames[f].slope_fx;
  const float zp = __hip_atomic_load(par + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0 ? a.depth[f * hw + p] : 0.f;
  const float zq = __hip_atomic_load(par + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0 ? a.depth[f * hw + q] : 0.f;
  if (dp_connected(zp, zq, a.connect_mm, slope)) uf_union<__HIP_MEMORY_SCOPE_AGENT>(par, p, q);
}

__global__ __launch_bounds__(DP_THREADS) void dp_flatten_kernel(DpCompArgs a) {
  const int f = blockIdx.y;
  const long long hw = (long long)a.h * a.w;
  const long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (p >= hw) return;
  const int* par = a.parent + f * hw;   // final since the merge launch ended: plain loads
  int i = par[p];
  if (i >= 0)
    for (int q = par[i]; q != i; q = par[i]) i = q;
  a.labels[f * hw + p] = i;
}

// ------------------------------------------------------------------------------------------------------------------------------- table
__global__ __launch_bounds__(DP_THREADS) void dp_slot_init_kernel(DpTableArgs a) {
  const int f = blockIdx.y;
  const long long hw = (long long)a.h * a.w;
  const long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 4) a.counts[f * 4 + threadIdx.x] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 4) a.ncand[f] = 0;
  if (p >= hw || a.labels[f * hw + p] != (int)p) return;
  int* s = a.slots + (f * hw + p) * SL_SIZE;
  s[SL_AREA] = 0, s[SL_X0] = INT_MAX, s[SL_Y0] = INT_MAX, s[SL_X1] = INT_MIN, s[SL_Y1] = INT_MIN, s[SL_RANK] = -1;
}

FP_DEVICE int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
FP_DEVICE int wave_max_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// area and box per label: a wave folds the lanes that share a label, then one lane issues the five atomics
__global__ __launch_bounds__(DP_THREADS) void dp_stats_kernel(DpTableArgs a) {
  const int f = blockIdx.y, lane = threadIdx.x & 63;
  const long long hw = (long long)a.h * a.w;
  const long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  const int L = p < hw ? a.labels[f * hw + p] : -1;
  const int x = (int)(p % a.w), y = (int)(p / a.w);
  bool pending = L >= 0 && L < hw;   // a label outside the frame (not one of fp_depth_components') is background
  for (;;) {   // every lane of the wave runs the same number of rounds
    const unsigned long long m = __ballot(pending);
    if (!m) break;
    const int lead = __ffsll((long long)m) - 1;
    const int Ll = __shfl(L, lead, 64);
    const bool mine = pending && L == Ll;
    const int cnt = __popcll(__ballot(mine));
    const int x0 = wave_min_int(mine ? x : INT_MAX), y0 = wave_min_int(mine ? y : INT_MAX);
    const int x1 = wave_max_int(mine ? x : INT_MIN), y1 = wave_max_int(mine ? y : INT_MIN);
    if (lane == lead) {
      int* s = a.slots + (f * hw + Ll) * SL_SIZE;
      atomicAdd(s + SL_AREA, cnt);
      atomicMin(s + SL_X0, x0), atomicMin(s + SL_Y0, y0);
      atomicMax(s + SL_X1, x1), atomicMax(s + SL_Y1, y1);
    }
    pending = pending && !mine;
  }
}

// roots that pass the area filter and that no finer level kept -> the frame's candidate list (in any order: dp_select orders by key)
__global__ __launch_bounds__(DP_THREADS) void dp_candidates_kernel(DpTableArgs a) {
  const int f = blockIdx.y;
  const long long hw = (long long)a.h * a.w;
  const long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (p >= hw || a.labels[f * hw + p] != (int)p) return;
  atomicAdd(a.counts + f * 4 + 0, 1);
  const int area = a.slots[(f * hw + p) * SL_SIZE + SL_AREA];
  if (area < a.min_pixels || area > a.max_area) return;
  atomicAdd(a.counts + f * 4 + 1, 1);
  for (int l = 0; l < a.num_finer; ++l) {
    const int* t = a.finer + ((size_t)l * a.n + f) * a.max_prop * 7;
    for (int r = 0; r < a.max_prop && t[r * 7] >= 0; ++r)
      if (t[r * 7] == (int)p && t[r * 7 + 1] == area) {
        atomicAdd(a.counts + f * 4 + 3, 1);
        return;
      }
  }
  a.cand[f * hw + atomicAdd(a.ncand + f, 1)] = (int)p;
}

// one workgroup per frame: max_prop rounds, each the largest key (area << 32 | ~label) below the previous round's
__global__ __launch_bounds__(DP_THREADS) void dp_select_kernel(DpTableArgs a) {
  const int f = blockIdx.x, tid = threadIdx.x;
  const long long hw = (long long)a.h * a.w;
  const int nc = a.ncand[f];
  __shared__ unsigned long long s_w[DP_THREADS / 64], s_prev;
  if (tid == 0) s_prev = ~0ull;
  __syncthreads();
  int kept = 0;
  for (int r = 0; r < a.max_prop; ++r) {
    const unsigned long long prev = s_prev;
    unsigned long long best = 0;
    for (int c = tid; c < nc; c += DP_THREADS) {
      const int L = a.cand[f * hw + c];
      const unsigned long long key = ((unsigned long long)(unsigned)a.slots[(f * hw + L) * SL_SIZE + SL_AREA] << 32) | (0xffffffffu - (unsigned)L);
      if (key < prev && key > best) best = key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long t = __shfl_xor(best, o, 64);
      best = t > best ? t : best;
    }
    if ((tid & 63) == 0) s_w[tid >> 6] = best;
    __syncthreads();
    for (int w = 0; w < DP_THREADS / 64; ++w) best = s_w[w] > best ? s_w[w] : best;
    __syncthreads();   // s_w and s_prev are read by every thread before thread 0 writes again
    if (best == 0) break;   // block-uniform
    if (tid == 0) {
      const int L = (int)(0xffffffffu - (unsigned)(best & 0xffffffffu));
      int* s = a.slots + (f * hw + L) * SL_SIZE;
      int* row = a.table + ((size_t)f * a.max_prop + r) * 7;
      row[0] = L, row[1] = s[SL_AREA], row[2] = s[SL_X0], row[3] = s[SL_Y0], row[4] = s[SL_X1], row[5] = s[SL_Y1], row[6] = a.level;
      s[SL_RANK] = r;
      s_prev = best;
    }
    __syncthreads();
    kept = r + 1;
  }
  for (int i = kept * 7 + tid; i < a.max_prop * 7; i += DP_THREADS) a.table[(size_t)f * a.max_prop * 7 + i] = (i % 7 == 0) ? -1 : 0;
  if (tid == 0) a.counts[f * 4 + 2] = kept;
}

__global__ __launch_bounds__(DP_THREADS) void dp_rank_map_kernel(DpTableArgs a) {
  const int f = blockIdx.y;
  const long long hw = (long long)a.h * a.w;
  const long long p = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  if (p >= hw) return;
  const int L = a.labels[f * hw + p];
  a.rank_map[f * hw + p] = (L >= 0 && L < hw && a.labels[f * hw + L] == L) ? a.slots[(f * hw + L) * SL_SIZE + SL_RANK] : -1;
}

// -------------------------------------------------------------------------------------------------------------------------------- runs
// the lanes of a wave that hold an event take consecutive places behind one atomic add
FP_DEVICE void dp_append(const DpRunsArgs& a, bool has, long long key) {
  const unsigned long long m = __ballot(has);
  if (!m) return;
  const int lane = threadIdx.x & 63, lead = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == lead) base = atomicAdd(a.count, __popcll(m));
  base = __shfl(base, lead, 64);
  if (has) {
    const long long idx = (long long)base + __popcll(m & ((1ull << lane) - 1ull));
    if (idx < a.capacity) a.events[idx] = key;
  }
}

// thread t of a map: t <= H W is column-major position t (H W: the end of the scan); t = H W + 1 + r closes rank r's list
__global__ __launch_bounds__(DP_THREADS) void dp_run_events_kernel(DpRunsArgs a) {
  const int m = blockIdx.y;
  const long long hw = (long long)a.h * a.w;
  const long long t = (long long)blockIdx.x * DP_THREADS + threadIdx.x;
  const int* rk = a.rank_map + m * hw;
  const int kept = min(max(a.num_kept[m], 0), a.max_prop);
  auto rank_at = [&](long long p) -> int {   // ranks at or past num_kept are no proposal
    if (p < 0 || p >= hw) return -1;
    const int r = rk[(p % a.h) * a.w + p / a.h];
    return (r >= 0 && r < kept) ? r : -1;
  };
  int r0 = -1, r1 = -1;
  bool e_start = false, e_end = false;
  if (t <= hw) {
    r1 = rank_at(t), r0 = rank_at(t - 1);
    e_start = r1 >= 0 && r1 != r0;
    e_end = r0 >= 0 && r1 != r0;
  } else if (t - hw - 1 < kept) {
    r0 = (int)(t - hw - 1);
    e_end = r0 != rank_at(hw - 1);   // the list of the rank that holds the last pixel is closed by its own end event
  }
  const long long pos = t <= hw ? t : hw;
  dp_append(a, e_start, ((long long)m * a.max_prop + r1) << 32 | pos);
  dp_append(a, e_end, ((long long)m * a.max_prop + r0) << 32 | pos);
}

}  // namespace

int launch_depth_plane_fit(const DpPlaneArgs& a, hipStream_t st) {
  const long long hw = (long long)a.h * a.w;
  const dim3 per_pixel((unsigned)((hw + DP_THREADS * DP_PPT - 1) / (DP_THREADS * DP_PPT)), a.n), chunks(a.chunks, a.n);
  const unsigned fold = (unsigned)cdiv(a.n, 64);
  hipLaunchKernelGGL(dp_eligible_kernel, per_pixel, dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_eligible");
  hipLaunchKernelGGL(dp_hypothesis_kernel, dim3(a.hyp, a.n), dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_hypothesis");
  hipLaunchKernelGGL(dp_winner_kernel, dim3(a.n), dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_winner");
  for (int it = 0; it < 2; ++it) {
    hipLaunchKernelGGL(dp_refit_partial_kernel<0>, chunks, dim3(DP_THREADS), 0, st, a);
    hipLaunchKernelGGL(dp_refit_fold_kernel<0>, dim3(fold), dim3(64), 0, st, a);
    hipLaunchKernelGGL(dp_refit_partial_kernel<1>, chunks, dim3(DP_THREADS), 0, st, a);
    hipLaunchKernelGGL(dp_refit_fold_kernel<1>, dim3(fold), dim3(64), 0, st, a);
    FP_CHECK_LAUNCH("dp_refit");
  }
  hipLaunchKernelGGL(dp_refit_partial_kernel<0>, chunks, dim3(DP_THREADS), 0, st, a);
  hipLaunchKernelGGL(dp_refit_fold_kernel<2>, dim3(fold), dim3(64), 0, st, a);
  FP_CHECK_LAUNCH("dp_refit_final");
  return FP_OK;
}

int launch_depth_components(const DpCompArgs& a, hipStream_t st) {
  const long long hw = (long long)a.h * a.w;
  hipLaunchKernelGGL(dp_tile_kernel, dim3(cdiv(a.w, DP_TILE), cdiv(a.h, DP_TILE), a.n), dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_tile");
  const long long border = (long long)((a.w - 1) / DP_TILE) * a.h + (long long)((a.h - 1) / DP_TILE) * a.w;
  if (border > 0) {
    hipLaunchKernelGGL(dp_merge_kernel, dim3((unsigned)((border + DP_THREADS - 1) / DP_THREADS), a.n), dim3(DP_THREADS), 0, st, a);
    FP_CHECK_LAUNCH("dp_merge");
  }
  hipLaunchKernelGGL(dp_flatten_kernel, dim3((unsigned)((hw + DP_THREADS - 1) / DP_THREADS), a.n), dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_flatten");
  return FP_OK;
}

int launch_component_table(const DpTableArgs& a, hipStream_t st) {
  const long long hw = (long long)a.h * a.w;
  const dim3 grid((unsigned)((hw + DP_THREADS - 1) / DP_THREADS), a.n);
  hipLaunchKernelGGL(dp_slot_init_kernel, grid, dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_slot_init");
  hipLaunchKernelGGL(dp_stats_kernel, grid, dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_stats");
  hipLaunchKernelGGL(dp_candidates_kernel, grid, dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_candidates");
  hipLaunchKernelGGL(dp_select_kernel, dim3(a.n), dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_select");
  hipLaunchKernelGGL(dp_rank_map_kernel, grid, dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_rank_map");
  return FP_OK;
}

int launch_component_runs(const DpRunsArgs& a, hipStream_t st) {
  const long long threads = (long long)a.h * a.w + 1 + a.max_prop;
  hipLaunchKernelGGL(dp_run_events_kernel, dim3((unsigned)((threads + DP_THREADS - 1) / DP_THREADS), a.m), dim3(DP_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("dp_run_events");
  return FP_OK;
}
