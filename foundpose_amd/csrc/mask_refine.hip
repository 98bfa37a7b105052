// Silhouette refinement of the final pose: the exact squared distance field of the detections' masks
// (fp_mask_distance) and Levenberg-Marquardt on the pose against it and against the masks' contours (fp_mask_refine).  It runs in the
// frame's own camera on the masks at frame resolution.  tests/mask_refine_ref.py restates the contract in numpy fp64.
//
// fp_mask_distance, two kernels:
//   mask_distance_columns  one thread per (column, mask): two sweeps leave g[y][x] = the distance in rows to the nearest set pixel of the
//                          column, FP_MASK_FAR = 32768 where the column has none (32768^2 = FP_MASK_D2_EMPTY)
//   mask_distance_rows     one workgroup per (row, mask): the row's g in LDS (uint16), then per pixel the row minimum
//                          min_x' (x - x')^2 + g[x']^2 by a scan outwards from x that stops once dx^2 reaches the best value so far
// fp_mask_refine, all kernels enqueued without a host round trip between them:
//   mask_refine_setup      one thread per detection: validates the bank row range and the contour row range, initialises the LM state
//   mask_refine_forward    (chunk of FP_REFINE_CHUNK points, detection), one wave: ONE POINT PER LANE -- projection, written to scratch
//                          with the in-front flag for the contour pass, the four taps of the distance field, the Huber weight and the
//                          Jacobian row (forward_point) -- then lm_lane_pass's butterfly and partial record
//   mask_refine_contour    (chunk of FP_REFINE_CHUNK contour rows, detection), four waves: the detection's projected points stream through
//                          LDS in tiles of FP_MASK_REFINE_TILE; eight groups of 32 lanes search one contour row per lane in an eighth
//                          of each tile and keep (best s, j); wave 0 takes the lexicographic minimum over the groups, ONE CONTOUR ROW
//                          PER LANE, builds the two Jacobian rows at X_j (contour_row); the same butterfly, one partial record per workgroup
//   mask_refine_solve      one wave per detection: folds both record sets in chunk order (forward, then backward), weighs them into one
//                          system, accepts / rejects the trial pose and solves for the next one
//   mask_refine_finalize   one thread per detection: the outputs (lm_finalize)
// The LM parts and the order of the launches (lm_enqueue) live in refine_terms.hpp.  Every floating-point statement stands as one
// source expression (the library is built with -ffp-contract=on).  Every sum has a fixed order (lanes: butterfly; chunks: ascending;
// forward before backward), no atomics, and a detection's decomposition depends only on its own N and K: results are bit-identical
// across runs and batch compositions.
#include "../../include/foundpose_amd_mask_refine.h"
#include "common.hpp"
#include "kernels.hpp"
#include "refine_terms.hpp"

namespace {

constexpr int FP_MASK_FAR = 32768;   // "no set pixel in this column": above every real distance, and its square is FP_MASK_D2_EMPTY
static_assert(FP_MASK_FAR > FP_MASK_MAX_SIDE && FP_MASK_FAR * FP_MASK_FAR == FP_MASK_D2_EMPTY, "the sentinel is the square of the far value");
static_assert(FP_MASK_FAR <= 65535, "a row's column distances are staged as uint16");

// grid: (ceil(W / 256), masks)
__global__ void __launch_bounds__(256) mask_distance_columns_kernel(MaskDistanceArgs a) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= a.W) return;
  const long long base = (long long)blockIdx.y * a.H * a.W + x;
  int d = FP_MASK_FAR;
  for (int y = 0; y < a.H; ++y) {
    const long long i = base + (long long)y * a.W;
    d = a.masks[i] ? 0 : min(d + 1, FP_MASK_FAR);
    a.d2[i] = d;
  }
  d = FP_MASK_FAR;
  for (int y = a.H - 1; y >= 0; --y) {
    const long long i = base + (long long)y * a.W;
    const int g = a.d2[i];
    d = g == 0 ? 0 : min(d + 1, FP_MASK_FAR);
    if (d < g) a.d2[i] = d;
  }
}

// grid: (H, masks).  In place: a row's column distances are read into LDS before any of its pixels is written.  The LDS is sized for the
// widest row (32 KB), which caps the workgroups of a CU at five whatever W is; sizing it by W is not done.
__global__ void __launch_bounds__(256) mask_distance_rows_kernel(MaskDistanceArgs a) {
  __shared__ uint16_t g[FP_MASK_MAX_SIDE];
  __shared__ int any;
  int32_t* row = a.d2 + ((long long)blockIdx.y * a.H + blockIdx.x) * a.W;
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  bool mine = false;
  for (int x = threadIdx.x; x < a.W; x += 256) {
    const int v = row[x];
    g[x] = (uint16_t)v;
    mine = mine || v < FP_MASK_FAR;
  }
  if (mine) any = 1;
  __syncthreads();
  const bool some = any != 0;   // false: no column of the mask has a set pixel (a column distance is finite in every row or in none)
  for (int x = threadIdx.x; x < a.W; x += 256) {
    int best = (int)g[x] * (int)g[x];
    for (int dx = 1; some && dx * dx < best; ++dx) {   // a column further than sqrt(best) away cannot lower it
      const int xl = x - dx, xr = x + dx;
      if (xl < 0 && xr >= a.W) break;
      if (xl >= 0) best = min(best, (int)g[xl] * (int)g[xl] + dx * dx);
      if (xr < a.W) best = min(best, (int)g[xr] * (int)g[xr] + dx * dx);
    }
    row[x] = best;
  }
}

// ---- the forward term of one point (model -> mask), run by one lane: the vertex Xv under the pose (R, t) in detection b's frame camera.
// The projection and the in-front flag go to scratch for the contour pass.  acc arrives zeroed and leaves with the point's
// FP_DEPTH_TERMS values: H (21), g (6), rho [27], the measurable flag [28].
FP_DEVICE void forward_point(const MaskRefineArgs& a, int b, int p0, const double* R, const double* t, const float* Xv, double (&acc)[FP_DEPTH_TERMS]) {
  const double* cam = a.lm.cam;
  const double fx = cam[4 * b + 0], fy = cam[4 * b + 1], cx = cam[4 * b + 2], cy = cam[4 * b + 3];
  const double delta = a.delta;
  const double X[3] = {Xv[0], Xv[1], Xv[2]};
  double Xc[3];
  for (int i = 0; i < 3; ++i) Xc[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
  const double z = Xc[2], iz = 1.0 / z;
  const double u = fx * Xc[0] / z + cx, v = fy * Xc[1] / z + cy;
  const bool front = z > 1.0;   // a NaN compares false
  // the point's index within the detection, from its address: lm_lane_pass hands the term Xv = a.lm.verts + 3 (p0 + p) and no index, so
  // this line depends on how that function forms Xv
  const long long slot = (long long)b * a.lm.max_points + ((Xv - a.lm.verts) / 3 - p0);
  a.pu[slot] = u;
  a.pv[slot] = v;
  a.pf[slot] = front ? 1 : 0;
  // measurable: in front and the four taps x0, x0 + 1, y0, y0 + 1 inside the image
  if (front && u >= 0.0 && u < (double)(a.W - 1) && v >= 0.0 && v < (double)(a.H - 1)) {
    const int x0 = (int)floor(u), y0 = (int)floor(v);
    const double al = u - x0, be = v - y0;
    const int32_t* d0 = a.d2 + ((long long)b * a.H + y0) * a.W + x0;
    const double D00 = sqrt((double)d0[0]), D10 = sqrt((double)d0[1]), D01 = sqrt((double)d0[a.W]), D11 = sqrt((double)d0[a.W + 1]);
    const double r = (1.0 - be) * ((1.0 - al) * D00 + al * D10) + be * ((1.0 - al) * D01 + al * D11);
    const double du = (1.0 - be) * (D10 - D00) + be * (D11 - D01), dv = (1.0 - al) * (D01 - D00) + al * (D11 - D10);
    const bool inl = r <= delta;
    const double w = inl ? 1.0 : delta / r;
    // dr/dXc = (dr/du, dr/dv) d(u, v)/dXc; J = dr/dXc [-[Xc]x | I]: the rotation part is Xc x (dr/dXc)
    const double q[3] = {du * fx * iz, dv * fy * iz, -(du * fx * Xc[0] + dv * fy * Xc[1]) * iz * iz};
    double J[6];
    cross3(Xc, q, J);
    for (int i = 0; i < 3; ++i) J[3 + i] = q[i];
    int k2 = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j, ++k2) acc[k2] = w * (J[i] * J[j]);
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] = w * (J[i] * r);
    acc[27] = inl ? r * r : 2.0 * delta * r - delta * delta;
    acc[28] = 1.0;
  }
}

// ---- the backward term of one contour row (mask contour -> model), run by one lane: the row q against its nearest projected point,
// the vertex Xv, under the pose (R, t).  The two Jacobian rows are multiview.hip's with the view transform the identity.
FP_DEVICE void contour_row(const MaskRefineArgs& a, int b, const double* R, const double* t, const float* Xv, double qx, double qy,
                           double (&acc)[FP_DEPTH_TERMS]) {
  const double* cam = a.lm.cam;
  const double fx = cam[4 * b + 0], fy = cam[4 * b + 1], cx = cam[4 * b + 2], cy = cam[4 * b + 3];
  const double delta = a.delta;
  const double X[3] = {Xv[0], Xv[1], Xv[2]};
  double Xc[3];
  for (int i = 0; i < 3; ++i) Xc[i] = R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2] + t[i];
  const double z = Xc[2], iz = 1.0 / z;
  const double e0 = fx * Xc[0] / z + cx - qx, e1 = fy * Xc[1] / z + cy - qy;
  const double s = e0 * e0 + e1 * e1;
  const double rs = sqrt(s);
  const bool inl = rs <= delta;
  const double w = inl ? 1.0 : delta / rs;
  const double px[3] = {fx * iz, 0.0, -fx * Xc[0] * iz * iz}, py[3] = {0.0, fy * iz, -fy * Xc[1] * iz * iz};
  double Jx[6], Jy[6];
  cross3(Xc, px, Jx);
  cross3(Xc, py, Jy);
  for (int i = 0; i < 3; ++i) { Jx[3 + i] = px[i]; Jy[3 + i] = py[i]; }
  int k2 = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j, ++k2) acc[k2] = w * (Jx[i] * Jx[j] + Jy[i] * Jy[j]);
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] = w * (Jx[i] * e0 + Jy[i] * e1);
  acc[27] = inl ? s : 2.0 * delta * rs - delta * delta;
  acc[28] = inl ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(64) mask_refine_setup_kernel(MaskRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.lm.num_det) return;
  MaskRefineState& ms = a.state[b];
  lm_setup(a.lm, nullptr, ms.s, b, 28);
  ms.k0 = ms.nk = 0;
  if (!a.lm.has_pose[b]) return;
  const int k0 = a.cbegin[b], k1 = a.cend[b];
  if (k0 < 0 || k1 < k0 || (long long)k1 > a.num_contour || k1 - k0 > a.max_contour) {   // never read: the host reports it
    a.lm.err[0] = -(b + 1);
    ms.s.active = ms.s.pending = 0;
    return;
  }
  ms.k0 = k0;
  ms.nk = k1 - k0;
  if (ms.nk < 6) ms.s.active = ms.s.pending = 0;   // skipped: too few contour rows (an empty mask, a mask without a contour)
}

__global__ void __launch_bounds__(64) mask_refine_forward_kernel(MaskRefineArgs a) {
  const int b = blockIdx.y;
  const RefineState& s = a.state[b].s;
  lm_lane_pass(a.lm, s, b,
               [&](const double* R, const double* t, const float* Xv, double (&acc)[FP_DEPTH_TERMS]) { forward_point(a, b, s.p0, R, t, Xv, acc); });
}

// grid: (bchunks, detections), block FP_MASK_SEARCH_GROUPS x FP_REFINE_CHUNK.  Reads the projections the forward pass of the same
// iteration left in scratch.  Thread (group g, row r) searches contour row chunk0 + r among the candidates g, g + GROUPS, ... of every
// tile, in ascending order; the groups' (best s, j) meet in LDS and the lexicographic minimum wins -- the lowest s, of equal s the lowest
// j -- which is the argmin of one ascending scan whatever the number of groups.  Wave 0 then builds the rows and the record.
constexpr int FP_MASK_SEARCH_GROUPS = 8;
__global__ void __launch_bounds__(FP_MASK_SEARCH_GROUPS * FP_REFINE_CHUNK) mask_refine_contour_kernel(MaskRefineArgs a) {
  constexpr int THREADS = FP_MASK_SEARCH_GROUPS * FP_REFINE_CHUNK;
  __shared__ double su[FP_MASK_REFINE_TILE], sv[FP_MASK_REFINE_TILE];
  __shared__ int sf[FP_MASK_REFINE_TILE];
  __shared__ double gs[FP_MASK_SEARCH_GROUPS][FP_REFINE_CHUNK];
  __shared__ int gj[FP_MASK_SEARCH_GROUPS][FP_REFINE_CHUNK];
  const int b = blockIdx.y;
  const MaskRefineState& ms = a.state[b];
  const RefineState& s = ms.s;
  if (!s.active || !s.pending) return;
  const int nk = ms.nk, np = s.np, chunk0 = blockIdx.x * FP_REFINE_CHUNK;
  if (chunk0 >= nk) return;
  const int lane = threadIdx.x, grp = threadIdx.x / FP_REFINE_CHUNK, r = threadIdx.x % FP_REFINE_CHUNK;
  const int k = chunk0 + r;
  double qx = 0.0, qy = 0.0;
  if (k < nk) {
    const int32_t* q = a.contour + 2 * ((long long)ms.k0 + k);
    qx = q[0];
    qy = q[1];
  }
  const long long base = (long long)b * a.lm.max_points;
  double best = INFINITY;
  int bj = -1;
  for (int tile0 = 0; tile0 < np; tile0 += FP_MASK_REFINE_TILE) {
    const int n = min(FP_MASK_REFINE_TILE, np - tile0);
    __syncthreads();
    for (int i = lane; i < n; i += THREADS) {
      su[i] = a.pu[base + tile0 + i];
      sv[i] = a.pv[base + tile0 + i];
      sf[i] = a.pf[base + tile0 + i];
    }
    __syncthreads();
    if (k < nk) {
      for (int i = grp; i < n; i += FP_MASK_SEARCH_GROUPS) {
        const double du = su[i] - qx, dv = sv[i] - qy;
        const double sd = du * du + dv * dv;
        if (sf[i] && sd < best) {   // strict: within a group ties go to the lowest j; a distance that is not finite never wins
          best = sd;
          bj = tile0 + i;
        }
      }
    }
  }
  gs[grp][r] = best;
  gj[grp][r] = bj;
  __syncthreads();
  if (lane >= 64) return;   // wave 0 goes on; no barrier follows
  const bool have = lane < FP_REFINE_CHUNK && k < nk;
  if (have) {
    for (int g = 1; g < FP_MASK_SEARCH_GROUPS; ++g) {
      const double sg = gs[g][r];
      const int jg = gj[g][r];
      if (jg >= 0 && (sg < best || (sg == best && jg < bj))) {
        best = sg;
        bj = jg;
      }
    }
  }
  double acc[FP_DEPTH_TERMS];
#pragma unroll
  for (int i = 0; i < FP_DEPTH_TERMS; ++i) acc[i] = 0.0;
  if (have) {
    if (bj < 0) acc[27] = INFINITY;   // no point in front: the pose costs +inf
    else contour_row(a, b, s.Rt, s.tt, a.lm.verts + 3 * ((long long)s.p0 + bj), qx, qy, acc);
  }
  // as lm_lane_pass: lanes 32..63 carry zeros and fold among themselves, lane 0 ends with the sum of lanes 0..31 in butterfly order
#pragma unroll
  for (int i = 0; i < FP_DEPTH_TERMS; ++i) {
    double v = acc[i];
#pragma unroll
    for (int o = FP_REFINE_CHUNK / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    acc[i] = v;
  }
  if (lane == 0) {
    double* out = a.bpart + ((long long)b * a.bchunks + blockIdx.x) * FP_REFINE_RECORD;
#pragma unroll
    for (int i = 0; i < 28; ++i) out[i] = acc[i];
    out[28] = 0.0;
    out[29] = acc[28];
    out[30] = out[31] = 0.0;
  }
}

__global__ void __launch_bounds__(64) mask_refine_solve_kernel(MaskRefineArgs a, int mode) {
  __shared__ double totf[FP_REFINE_RECORD], totb[FP_REFINE_RECORD];
  const int b = blockIdx.x;
  MaskRefineState& ms = a.state[b];
  RefineState& s = ms.s;
  if (!s.active || !s.pending) return;
  RefineLmArgs back = a.lm;
  back.part = a.bpart;
  back.chunks = a.bchunks;
  lm_fold(a.lm, b, s.np, FP_REFINE_RECORD, threadIdx.x, totf);
  lm_fold(back, b, ms.nk, FP_REFINE_RECORD, threadIdx.x, totb);
  if (threadIdx.x != 0) return;
  s.pending = 0;
  double tot[28];
  for (int i = 0; i < 28; ++i) tot[i] = 0.5 * (totf[i] / s.np) + 0.5 * (totb[i] / ms.nk);   // N and K count every row: costs at different poses are comparable
  const double Et = tot[27];
  if (mode == SOLVE_STEP && !(Et < s.E)) {
    lm_reject(s, a.lm.iters);
    return;
  }
  if (mode == SOLVE_FIRST) {
    s.E = s.E_in = Et;
    s.nvalid = (int)totf[29];
    if (a.lm.normal_eq)
      for (int i = 0; i < 28; ++i) a.lm.normal_eq[28 * b + i] = tot[i];
  } else if (!lm_accept(s, Et)) {
    return;
  }
  lm_set_system(s, tot);
  if (mode == SOLVE_FIRST) {
    if (s.nvalid < 6 || !(Et < INFINITY)) { lm_stop(s); return; }   // too few measurable forward rows, or a cost that is not finite
    s.skipped = 0;
  }
  lm_propose(s, a.lm.iters);
}

__global__ void __launch_bounds__(64) mask_refine_finalize_kernel(MaskRefineArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < a.lm.num_det) lm_finalize(a.lm, a.state[b].s, b);
}

}  // namespace

int launch_mask_distance(const MaskDistanceArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(mask_distance_columns_kernel, dim3(cdiv(a.W, 256), a.B), dim3(256), 0, st, a);
  FP_CHECK_LAUNCH("mask_distance_columns");
  hipLaunchKernelGGL(mask_distance_rows_kernel, dim3(a.H, a.B), dim3(256), 0, st, a);
  FP_CHECK_LAUNCH("mask_distance_rows");
  return FP_OK;
}

int launch_mask_refine(const MaskRefineArgs& a, hipStream_t st) {
  return lm_enqueue(a.lm, 64, false,   // no sigma stage; a pass is the forward kernel, then the contour kernel on its projections
                    [&](dim3 g, dim3 blk) { return lm_launch("mask_refine_setup", mask_refine_setup_kernel, g, blk, st, a); },
                    [&](dim3 g, dim3 blk, int) {
                      if (int rc = lm_launch("mask_refine_forward", mask_refine_forward_kernel, g, blk, st, a)) return rc;
                      return lm_launch("mask_refine_contour", mask_refine_contour_kernel, dim3(a.bchunks, a.lm.num_det), dim3(FP_MASK_SEARCH_GROUPS * FP_REFINE_CHUNK), st, a);
                    },
                    [&](dim3 g, dim3 blk, int mode) { return lm_launch("mask_refine_solve", mask_refine_solve_kernel, g, blk, st, a, mode); },
                    [&](dim3 g, dim3 blk) { return lm_launch("mask_refine_finalize", mask_refine_finalize_kernel, g, blk, st, a); });
}
