// Symmetry-aware BOP pose errors: MSSD and MSPD (utils/eval_errors.py:12-68 with bop_toolkit_lib.misc.transform_pts_Rt /
// project_pts), a ragged batch of hypotheses per call, fp64 throughout.
//
// Per hypothesis h with vertices p_v (its vertex range) and symmetries s (its symmetry range):
//   MSSD  e_s = max_v |gt_sym_s(p_v) - est(p_v)|            result min_s e_s
//   MSPD  e_s = max_v |proj(P_est, p_v) - proj(P_gt_s, p_v)|  result min_s e_s
// Arithmetic follows the reference operation by operation, every product / sum / quotient individually rounded (no
// contraction): R.dot(pts.T) + t as ((r0 x + r1 y) + r2 z) + t_i (numpy hands the product to BLAS, whose summation order
// is not specified); P.dot([p; 1]) as (((p0 x + p1 y) + p2 z) + p3), then x and y divided by the third row (IEEE
// division); norm(axis=1) as sqrt((d0 d0 + d1 d1) + d2 d2).
//
// The maximum over vertices compares SQUARED distances and the winner's square root is taken once per symmetry: sqrt is
// monotone, so the value equals the reference's err.max(); the vertex index can differ from err.argmax() only when two
// distinct squares round to the same root.  Ties go to the lowest vertex; a NaN wins over every number and the first NaN
// wins (np.max / np.argmax).  Across symmetries the value follows Python's sequential min(es) -- NaN if es[0] is NaN,
// else the smallest non-NaN e_s -- and the chosen symmetry follows np.argmin(es): the first NaN if there is one, else the
// first minimum.  Every reduction is a total order on (value, index), so results do not depend on the reduction tree,
// the grid or the neighbours of a hypothesis in the batch.
//
// Two kernels.  pose_err_partial: one wave per (hypothesis, tile of 64 * PE_V vertices, chunk of PE_SYM_CHUNK symmetries);
// each lane owns PE_V consecutive vertices, transforms and projects them by the estimate once, then loops over the
// chunk's symmetries (their 24 coefficients are wave-uniform loads), keeps its own best (square, vertex) and reduces the
// wave with a shuffle max + ballot; lane 0 writes one partial per (h, tile, s).  pose_err_fold: one workgroup per
// hypothesis folds the tiles of every symmetry in tile order, takes the roots and reduces over symmetries in LDS.
#include <limits.h>

#include "common.hpp"
#include "kernels.hpp"
#include "rounded.hpp"
#include "../../include/foundpose_amd.h"

namespace {

constexpr int PE_V = FP_POSE_ERR_VERTS_PER_LANE;  // vertices per lane
constexpr int PE_TILE = FP_POSE_ERR_TILE;         // vertices per wave = 64 * PE_V
constexpr int PE_SYM_CHUNK = 16;                  // symmetries per wave
constexpr int PE_WAVES = 4;                       // waves per workgroup (partial kernel)
constexpr int PE_FOLD_THREADS = 256;

FP_DEVICE bool isnan_d(double a) { return a != a; }

// (a, ia) preferred to (b, ib) for a maximum with np.argmax's rules: a NaN beats every number, ties -> lower index
FP_DEVICE bool max_beats(double a, int ia, double b, int ib) {
  const bool an = isnan_d(a), bn = isnan_d(b);
  if (an || bn) return an && (!bn || ia < ib);
  return a > b || (a == b && ia < ib);
}
// ... and for a minimum with np.argmin's rules: a NaN beats every number, ties -> lower index
FP_DEVICE bool min_beats(double a, int ia, double b, int ib) {
  const bool an = isnan_d(a), bn = isnan_d(b);
  if (an || bn) return an && (!bn || ia < ib);
  return a < b || (a == b && ia < ib);
}

// The wave's (max, first argmax) of the per-lane bests.  Lane l owns vertices [l * PE_V, (l + 1) * PE_V) of the tile and
// its best is the first of its own maxima, so the lowest lane holding the wave maximum holds the lowest vertex index.
FP_DEVICE void wave_argmax(double v, int iv, double& out, int& iout) {
  const unsigned long long nan_lanes = __ballot(isnan_d(v));
  if (nan_lanes) {  // the first NaN
    iout = __shfl(iv, __ffsll((long long)nan_lanes) - 1);
    out = __shfl(v, __ffsll((long long)nan_lanes) - 1);
    return;
  }
  double m = v;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off));
  const unsigned long long at = __ballot(v == m);
  out = m;
  iout = __shfl(iv, __ffsll((long long)at) - 1);
}

__global__ __launch_bounds__(64 * PE_WAVES) void pose_err_partial_kernel(PoseErrArgs a) {
  const PoseErrHyp hd = a.hyps[blockIdx.z];
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * PE_WAVES + (threadIdx.x >> 6);
  const int s0 = blockIdx.y * PE_SYM_CHUNK;
  if (tile >= hd.tiles || s0 >= hd.sym_cnt) return;  // wave-uniform
  const int s1 = min(s0 + PE_SYM_CHUNK, hd.sym_cnt);
  const double* E = a.est + (size_t)blockIdx.z * 12;
  const double* PE = a.p_est + (size_t)blockIdx.z * 12;
  const int v0 = tile * PE_TILE + lane * PE_V;  // vertex index (within the hypothesis' range) of this lane's first slot
  double px[PE_V], py[PE_V], pz[PE_V], ex[PE_V], ey[PE_V], ez[PE_V], eu[PE_V], ev[PE_V];
  bool valid[PE_V];
#pragma unroll
  for (int j = 0; j < PE_V; ++j) {
    valid[j] = v0 + j < hd.pt_cnt;
    const double* p = a.pts + 3 * ((size_t)hd.pt_off + (valid[j] ? v0 + j : 0));
    px[j] = p[0], py[j] = p[1], pz[j] = p[2];
    // transform_pts_Rt(pts, R_est, t_est)
    ex[j] = affine(E + 0, E[9], px[j], py[j], pz[j]);
    ey[j] = affine(E + 3, E[10], px[j], py[j], pz[j]);
    ez[j] = affine(E + 6, E[11], px[j], py[j], pz[j]);
    // project_pts(pts, K, R_est, t_est) with P_est = K [R_est | t_est]
    const double w = affine(PE + 8, PE[11], px[j], py[j], pz[j]);
    eu[j] = __ddiv_rn(affine(PE + 0, PE[3], px[j], py[j], pz[j]), w);
    ev[j] = __ddiv_rn(affine(PE + 4, PE[7], px[j], py[j], pz[j]), w);
  }
  PoseErrPart* part = a.parts + hd.part_base + (size_t)tile * hd.sym_cnt;
  for (int s = s0; s < s1; ++s) {
    const double* G = a.gt_sym + ((size_t)hd.sym_off + s) * 12;  // R_gt S_R | R_gt S_t + t_gt
    const double* PG = a.p_gt + ((size_t)hd.sym_off + s) * 12;   // K [R_gt_sym | t_gt_sym]
    double bsd = -1.0, bpd = -1.0;  // below every distance: a lane with no valid slot never wins
    int isd = INT_MAX, ipd = INT_MAX;
#pragma unroll
    for (int j = 0; j < PE_V; ++j) {
      const double dx = dsub(affine(G + 0, G[9], px[j], py[j], pz[j]), ex[j]);
      const double dy = dsub(affine(G + 3, G[10], px[j], py[j], pz[j]), ey[j]);
      const double dz = dsub(affine(G + 6, G[11], px[j], py[j], pz[j]), ez[j]);
      double sd = dadd(dadd(dmul(dx, dx), dmul(dy, dy)), dmul(dz, dz));
      const double w = affine(PG + 8, PG[11], px[j], py[j], pz[j]);
      const double du = dsub(eu[j], __ddiv_rn(affine(PG + 0, PG[3], px[j], py[j], pz[j]), w));
      const double dv = dsub(ev[j], __ddiv_rn(affine(PG + 4, PG[7], px[j], py[j], pz[j]), w));
      double pd = dadd(dmul(du, du), dmul(dv, dv));
      if (!valid[j]) sd = pd = -1.0;
      // slots run in vertex order: a later slot replaces the lane's best only when strictly better
      if (!isnan_d(bsd) && (isnan_d(sd) || sd > bsd)) bsd = sd, isd = v0 + j;
      if (!isnan_d(bpd) && (isnan_d(pd) || pd > bpd)) bpd = pd, ipd = v0 + j;
    }
    double wsd, wpd;
    int iwsd, iwpd;
    wave_argmax(bsd, isd, wsd, iwsd);
    wave_argmax(bpd, ipd, wpd, iwpd);
    if (lane == 0) part[s] = PoseErrPart{wsd, wpd, iwsd, iwpd};
  }
}

struct FoldSlot {
  double val[2];   // np.argmin candidate per metric
  int sym[2], vtx[2];
  double vmin[2];  // smallest non-NaN e_s per metric (NaN: none yet)
};

__global__ __launch_bounds__(PE_FOLD_THREADS) void pose_err_fold_kernel(PoseErrArgs a) {
  const int h = blockIdx.x;
  const PoseErrHyp hd = a.hyps[h];
  const PoseErrPart* part = a.parts + hd.part_base;
  __shared__ FoldSlot slots[PE_FOLD_THREADS];
  __shared__ int first_is_nan[2];
  FoldSlot me;
  for (int m = 0; m < 2; ++m) me.val[m] = __longlong_as_double(0x7ff0000000000000ll), me.sym[m] = INT_MAX, me.vtx[m] = 0,
                              me.vmin[m] = __longlong_as_double(0x7ff8000000000000ll);
  for (int s = threadIdx.x; s < hd.sym_cnt; s += PE_FOLD_THREADS) {
    // max over the tiles of symmetry s, tiles in order (the order does not matter: max_beats is a total order)
    PoseErrPart b = part[s];
    for (int t = 1; t < hd.tiles; ++t) {
      const PoseErrPart c = part[(size_t)t * hd.sym_cnt + s];
      if (max_beats(c.sd, c.vsd, b.sd, b.vsd)) b.sd = c.sd, b.vsd = c.vsd;
      if (max_beats(c.pd, c.vpd, b.pd, b.vpd)) b.pd = c.pd, b.vpd = c.vpd;
    }
    const double e[2] = {__dsqrt_rn(b.sd), __dsqrt_rn(b.pd)};
    const int ve[2] = {b.vsd, b.vpd};
    for (int m = 0; m < 2; ++m) {
      if (s == 0) first_is_nan[m] = isnan_d(e[m]);
      if (min_beats(e[m], s, me.val[m], me.sym[m])) me.val[m] = e[m], me.sym[m] = s, me.vtx[m] = ve[m];
      me.vmin[m] = fmin(me.vmin[m], e[m]);  // fmin skips NaN
    }
  }
  slots[threadIdx.x] = me;
  __syncthreads();
  for (int n = PE_FOLD_THREADS / 2; n >= 1; n >>= 1) {
    if ((int)threadIdx.x < n) {
      FoldSlot& x = slots[threadIdx.x];
      const FoldSlot& y = slots[threadIdx.x + n];
      for (int m = 0; m < 2; ++m) {
        if (min_beats(y.val[m], y.sym[m], x.val[m], x.sym[m])) x.val[m] = y.val[m], x.sym[m] = y.sym[m], x.vtx[m] = y.vtx[m];
        x.vmin[m] = fmin(x.vmin[m], y.vmin[m]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const FoldSlot& r = slots[0];
    for (int m = 0; m < 2; ++m) {
      // min(es): NaN when es[0] is NaN (no later value compares below it), else the smallest non-NaN value
      a.err[(size_t)h * 2 + m] = first_is_nan[m] ? __longlong_as_double(0x7ff8000000000000ll) : r.vmin[m];
      a.idx[(size_t)h * 4 + 2 * m] = r.vtx[m];  // es_ind[np.argmin(es)]
      a.idx[(size_t)h * 4 + 2 * m + 1] = r.sym[m];
    }
  }
}

}  // namespace

int launch_pose_errors(const PoseErrArgs& a, int num_hyp, int max_tiles, int max_syms, hipStream_t st) {
  dim3 grid(cdiv(max_tiles, PE_WAVES), cdiv(max_syms, PE_SYM_CHUNK), num_hyp);
  hipLaunchKernelGGL(pose_err_partial_kernel, grid, dim3(64 * PE_WAVES), 0, st, a);
  FP_CHECK_LAUNCH("pose_err_partial");
  hipLaunchKernelGGL(pose_err_fold_kernel, dim3(num_hyp), dim3(PE_FOLD_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("pose_err_fold");
  return FP_OK;
}
