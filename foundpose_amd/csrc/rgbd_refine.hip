// Joint refinement of the final pose on features and depth: Levenberg-Marquardt on
//   E = E_f + w_d E_d,   E_f = sum_V log(1 + s_i / sigma^2) / |V| (section 11's term),   E_d = sum min(r^2, tau^2) / (N tau^2) (section 14's)
// The pose lives in the frame's camera; the feature term is evaluated in the feature (crop) camera, X_f = A X_c + a, and its Jacobian
// carries A.  The depth term adds a tap-consistency test to section 14's: a point whose four taps spread over more than tau is not
// measurable.  tests/rgbd_refine_ref.py restates the contract in numpy fp64.
//
// Kernels, all enqueued by fp_rgbd_refine without a host round trip between them:
//   rgbd_setup     one thread per detection: validates the bank row range and the image index, initialises the LM state (lm_setup)
//   rgbd_pass      (chunk of FP_REFINE_CHUNK points, detection), four waves of 8 points: refine.hip's channel loop and six shuffle-reduced
//                  fp32 dot products per point with all 64 lanes (feat_point); then lane p of a wave takes the wave's point p for the
//                  depth row (fp64; depth_point).
//                  The two terms stay apart: one record of 64 doubles per workgroup, feature half | depth half, no normalisation
//   rgbd_solve     one wave per detection: folds the partials in chunk order, mixes the halves with 1 / (|V| sigma^2) and
//                  w_d / (N tau^2), accepts / rejects the trial pose and solves for the next one
//   rgbd_finalize  one thread per detection: the outputs (lm_finalize, and the depth inliers)
// The parts named in brackets, the fold, the sigma stage (lm_sigma), the accept / reject / propose steps of the solve and the order of
// the launches (lm_enqueue) live in refine_terms.hpp, shared with refine.hip, depth_refine.hip and tsdf_track.hip; this file keeps the
// (A, a) camera of its feature term, the tap-spread test, the LDS rows of its depth reduction, the mixing of the two halves and the
// use_depth decision.
// 2 + 2 iters launches after the setup chain, as refine.hip alone.  Detections that have stopped leave pass and solve at their first
// instruction.  Every sum has a fixed order (lanes: butterfly; points of a wave: ascending; waves: 0..3; the 32 depth rows of a chunk:
// ascending; chunks: ascending), no atomics, and a detection's chunk decomposition depends only on its own point count: results are
// bit-identical across runs and batch compositions.
#include "common.hpp"
#include "kernels.hpp"
#include "refine_terms.hpp"

namespace {

constexpr int RG_WAVES = 4;
constexpr int RG_PTS_PER_WAVE = FP_REFINE_CHUNK / RG_WAVES;
constexpr int RG_HALF = FP_REFINE_RECORD;   // feature half: H (21, upper triangle row-major), g (6), sum log1p [27], sum s [28], valid [29], z-bad [30], pad
constexpr int RG_REC = 2 * RG_HALF;         // depth half at +32: H (21), g (6), sum rho [27], pad, inliers [29], pad
constexpr int RG_DSTRIDE = FP_DEPTH_TERMS + 4;   // odd number of doubles per row: the 8 lanes of a wave write different banks
static_assert(RG_PTS_PER_WAVE == 8 && FP_REFINE_CHUNK == 32, "lane p of a wave takes the wave's point p");

__global__ void __launch_bounds__(64) rgbd_setup_kernel(RgbdRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.lm.num_det) return;
  RgbdState& rs = a.state[b];
  rs.ninl = 0;
  rs.use_depth = 1;        // the pass at the input pose always evaluates the depth rows: the solve then decides
  lm_setup(a.lm, &a.d, rs.s, b, 57);
}

__global__ void __launch_bounds__(64 * RG_WAVES) rgbd_pass_kernel(RgbdRefineArgs a, int mode) {
  __shared__ double red[RG_WAVES][RG_HALF];
  __shared__ double drow[FP_REFINE_CHUNK][RG_DSTRIDE];
  const int b = blockIdx.y;
  const RgbdState& rs = a.state[b];
  const RefineState& s = rs.s;
  if (!s.active || (mode == MODE_EVAL && !s.pending)) return;
  const int np = s.np, chunk0 = blockIdx.x * FP_REFINE_CHUNK;
  if (chunk0 >= np) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool with_depth = mode == MODE_EVAL && rs.use_depth;
  double R[9], t[3];
  for (int i = 0; i < 9; ++i) R[i] = s.Rt[i];
  for (int i = 0; i < 3; ++i) t[i] = s.tt[i];
  {
    // ---- the feature term at X_f = A X_c + a, in the feature camera; slot 27 carries log1p(q), the solve divides by sigma^2
    const FeatFrame c = feat_frame(a.f, a.fcam, b, a.lm.max_points, s.sigma2);
    double A[9], av[3];
    for (int i = 0; i < 9; ++i) A[i] = a.A[9 * b + i];
    for (int i = 0; i < 3; ++i) av[i] = a.a[3 * b + i];
    double acc[RG_HALF];
#pragma unroll
    for (int k = 0; k < RG_HALF; ++k) acc[k] = 0.0;
    if (mode == MODE_INIT) {
      for (int k = 0, p = chunk0 + wave * RG_PTS_PER_WAVE; k < RG_PTS_PER_WAVE && p < np; ++k, ++p)
        feat_point<MODE_INIT, true, false>(a.f, c, R, t, A, av, a.lm.verts, s.p0, p, lane, acc);
    } else {
      for (int k = 0, p = chunk0 + wave * RG_PTS_PER_WAVE; k < RG_PTS_PER_WAVE && p < np; ++k, ++p)
        feat_point<MODE_EVAL, true, false>(a.f, c, R, t, A, av, a.lm.verts, s.p0, p, lane, acc);
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < RG_HALF; ++k) red[wave][k] = acc[k];
    }
  }
  // ---- the depth term: lane p of a wave takes the wave's point p (every row of the range, valid for the feature term or not)
  if (with_depth && lane < RG_PTS_PER_WAVE) {
    const int slot = wave * RG_PTS_PER_WAVE + lane, p = chunk0 + slot;
    double d[FP_DEPTH_TERMS];
#pragma unroll
    for (int k = 0; k < FP_DEPTH_TERMS; ++k) d[k] = 0.0;
    if (p < np) depth_point<true>(a.d, a.lm.cam, b, R, t, a.lm.verts + 3 * ((long long)s.p0 + p), d);
#pragma unroll
    for (int k = 0; k < FP_DEPTH_TERMS; ++k) drow[slot][k] = d[k];
  }
  __syncthreads();
  double* out = a.lm.part + ((long long)b * a.lm.chunks + blockIdx.x) * RG_REC;
  if (threadIdx.x < RG_HALF) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < RG_WAVES; ++w) v += red[w][threadIdx.x];
    out[threadIdx.x] = v;
  } else if (threadIdx.x < RG_REC) {
    // depth half: column j of the chunk's 32 rows in ascending order; 28 is a pad, the inlier count sits at 29 as in depth_refine.hip
    const int j = threadIdx.x - RG_HALF, col = j < 28 ? j : (j == 29 ? 28 : -1);
    double v = 0.0;
    if (with_depth && col >= 0)
      for (int r = 0; r < FP_REFINE_CHUNK; ++r) v += drow[r][col];
    out[threadIdx.x] = v;
  }
}

__global__ void __launch_bounds__(64) rgbd_solve_kernel(RgbdRefineArgs a, int mode) {
  __shared__ double tot[RG_REC];
  const int b = blockIdx.x;
  RgbdState& rs = a.state[b];
  RefineState& s = rs.s;
  if (!s.active || !s.pending) return;
  lm_fold(a.lm, b, s.np, RG_REC, threadIdx.x, tot);
  if (threadIdx.x != 0) return;
  if (mode == SOLVE_SIGMA) {
    lm_sigma(s, tot);
    return;
  }
  s.pending = 0;
  const double* td = tot + RG_HALF;
  const double tau = a.d.tau[b];
  const double nf = (double)s.nvalid * s.sigma2, nd = (double)s.np * (tau * tau);
  const double Ef = tot[27] / s.nvalid, Ed = td[27] / nd;
  if (mode == SOLVE_FIRST) {
    rs.ninl = (int)td[29];
    rs.use_depth = a.wd > 0.0 && rs.ninl >= 6;
  }
  const bool dep = rs.use_depth;
  const double Et = dep ? Ef + a.wd * Ed : Ef;
  if (mode == SOLVE_STEP && !(tot[30] == 0.0 && Et < s.E)) {
    lm_reject(s, a.lm.iters);
    return;
  }
  // the system at the (new) current pose: H = H_f / (|V| sigma^2) + w_d H_d / (N tau^2), g likewise
  for (int i = 0; i < 21; ++i) s.H[i] = dep ? tot[i] / nf + a.wd * td[i] / nd : tot[i] / nf;
  for (int i = 0; i < 6; ++i) s.g[i] = dep ? tot[21 + i] / nf + a.wd * td[21 + i] / nd : tot[21 + i] / nf;
  if (mode == SOLVE_FIRST) {
    if (a.lm.normal_eq) {
      double* ne = a.lm.normal_eq + 57 * b;
      for (int i = 0; i < 27; ++i) { ne[i] = tot[i]; ne[28 + i] = td[i]; }
      ne[27] = Ef;
      ne[55] = Ed;
      ne[56] = Et;
    }
    s.E = s.E_in = Et;
  } else if (!lm_accept(s, Et)) {
    return;
  }
  lm_propose(s, a.lm.iters);
}

__global__ void __launch_bounds__(64) rgbd_finalize_kernel(RgbdRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.lm.num_det) return;
  lm_finalize(a.lm, a.state[b].s, b);
  a.num_depth_inliers[b] = a.state[b].ninl;
}

}  // namespace

int launch_rgbd_refine(const RgbdRefineArgs& a, hipStream_t st) {
  return lm_enqueue(a.lm, 64 * RG_WAVES, true,   // with the sigma stage
                    [&](dim3 g, dim3 blk) { return lm_launch("rgbd_setup", rgbd_setup_kernel, g, blk, st, a); },
                    [&](dim3 g, dim3 blk, int mode) { return lm_launch("rgbd_pass", rgbd_pass_kernel, g, blk, st, a, mode); },
                    [&](dim3 g, dim3 blk, int mode) { return lm_launch("rgbd_solve", rgbd_solve_kernel, g, blk, st, a, mode); },
                    [&](dim3 g, dim3 blk) { return lm_launch("rgbd_finalize", rgbd_finalize_kernel, g, blk, st, a); });
}
