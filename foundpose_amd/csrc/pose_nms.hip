// Duplicate suppression between the poses of one frame (frame_select_type "pose_nms").  This stage is the project's
// own; the reference never looks at two poses of a frame together.
//
// pose_overlap_kernel: for an ordered pair (i, j) of poses in one common coordinate frame, the fraction of i's model sample that lies in
// space occupied by j's model.
//   skip       an invalid pose, an empty sample or rho_j not > 0: status 2;
//   prefilter  the bounding spheres placed at the poses; disjoint (or NaN): status 1, no point read -- block-uniform, before any barrier;
//   pass 1     j's sample in j's OWN model frame -> the cells of a G x G x G grid over the cube of its bounding sphere; bit `cell` of an
//              occupancy bitmap in LDS is set by an integer atomic-or (the result does not depend on the order of arrival);
//   pass 2     i's sample placed at i's pose and taken back into j's model frame (R_j^T (X - t_j)); a point whose (unclamped) cell lies in
//              the cube and has its bit set counts into n_in.
// One 256-thread workgroup per pair; fp64, every step one rounded operation in the order section 20 states (FMA contraction off), points
// stored as fp32.  The outputs are integer counts and one quotient of two of them: a pair's result depends on its own data only.
//
// pose_nms_greedy_kernel: one workgroup per frame (at most 256 poses, in rank order).  The pairs whose overlap reaches the threshold in
// either direction become a symmetric conflict bit matrix in LDS; then rank by rank, a pose that is still alive suppresses the later
// poses it conflicts with.
#include "common.hpp"
#include "group_parts.hpp"
#include "verify_grid.hpp"  // FramePose, to_camera, PV_THREADS

namespace {

constexpr int PN_MAX_WORDS = (PN_MAX_GRID * PN_MAX_GRID * PN_MAX_GRID + 31) / 32;  // 1024 words = 4 KB
constexpr int PN_ROW_WORDS = PN_MAX_GROUP / 32;                                    // a row of the conflict matrix: 8 words

// the cell of x along one axis of j's grid, clamped into [0, G - 1] (a NaN lands in cell 0: fmax / fmin drop it)
FP_DEVICE int clamped_cell(double x, double x0, double h, double top) {
#pragma clang fp contract(off)
  return (int)fmin(fmax(floor((x - x0) / h), 0.0), top);
}

__global__ __launch_bounds__(PV_THREADS) void pose_overlap_kernel(PoseOverlapArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned bits[PN_MAX_WORDS];  // bit (cell & 31) of word (cell >> 5): a point of j's sample lies in the cell
  __shared__ int total[2];                 // n_in, n_cells

  const int pair = blockIdx.x, tid = threadIdx.x;
  auto finish = [&](int status) {  // block-uniform: zero counts, zero overlap
    if (tid == 0) {
      a.counts[(size_t)pair * 2 + 0] = 0;
      a.counts[(size_t)pair * 2 + 1] = 0;
      a.overlap[pair] = 0.0;
      a.status[pair] = status;
    }
  };
  // (the host validates the indices; a bad one that reaches the kernel all the same is skipped and nothing is read through it)
  const int pi = a.pairs[(size_t)pair * 2 + 0], pj = a.pairs[(size_t)pair * 2 + 1];
  if (pi < 0 || pi >= a.n_poses || pj < 0 || pj >= a.n_poses) { finish(2); return; }
  const int oi = a.pose_obj[pi], oj = a.pose_obj[pj];
  if (oi < 0 || oi >= a.n_objects || oj < 0 || oj >= a.n_objects) { finish(2); return; }
  const int bi = min(max(a.ranges[oi * 2 + 0], 0), a.m_total), ei = min(max(a.ranges[oi * 2 + 1], 0), a.m_total);
  const int bj = min(max(a.ranges[oj * 2 + 0], 0), a.m_total), ej = min(max(a.ranges[oj * 2 + 1], 0), a.m_total);
  const double rho_i = a.radius[oi], rho_j = a.radius[oj];
  if (a.valid[pi] <= 0 || a.valid[pj] <= 0 || bi >= ei || bj >= ej || !(rho_j > 0.0)) { finish(2); return; }

  // ---- set-up (every thread, from block-uniform data)
  FramePose Pi, Pj;
  for (int k = 0; k < 9; ++k) { Pi.R[k] = a.R[(size_t)pi * 9 + k]; Pj.R[k] = a.R[(size_t)pj * 9 + k]; }
  for (int k = 0; k < 3; ++k) { Pi.t[k] = a.t[(size_t)pi * 3 + k]; Pj.t[k] = a.t[(size_t)pj * 3 + k]; }
  const double cj[3] = {a.center[oj * 3 + 0], a.center[oj * 3 + 1], a.center[oj * 3 + 2]};
  {
    const double ci[3] = {a.center[oi * 3 + 0], a.center[oi * 3 + 1], a.center[oi * 3 + 2]};
    double Ci[3], Cj[3];
    to_camera(Pi, ci, Ci);
    to_camera(Pj, cj, Cj);
    const double dx = Ci[0] - Cj[0], dy = Ci[1] - Cj[1], dz = Ci[2] - Cj[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const double s = rho_i + rho_j;
    if (!(d2 <= s * s)) { finish(1); return; }  // disjoint spheres (a NaN pose ends here too)
  }
  const int G = a.grid, words = (G * G * G + 31) >> 5;
  const double dG = (double)G, top = (double)(G - 1);
  const double x0[3] = {cj[0] - rho_j, cj[1] - rho_j, cj[2] - rho_j};
  const double h = 2.0 * rho_j / dG;

  for (int i = tid; i < words; i += PV_THREADS) bits[i] = 0u;
  if (tid < 2) total[tid] = 0;
  __syncthreads();

  // ---- pass 1: the occupancy bitmap of j's sample in j's model frame
  for (int p = bj + tid; p < ej; p += PV_THREADS) {
    const int ix = clamped_cell((double)a.points[(size_t)p * 3 + 0], x0[0], h, top);
    const int iy = clamped_cell((double)a.points[(size_t)p * 3 + 1], x0[1], h, top);
    const int iz = clamped_cell((double)a.points[(size_t)p * 3 + 2], x0[2], h, top);
    const int cell = (iz * G + iy) * G + ix;  // in [0, G^3): clamped
    atomicOr(&bits[cell >> 5], 1u << (cell & 31));
  }
  __syncthreads();

  // ---- pass 2: i's sample at i's pose, seen from j's model frame
  int n_in = 0, n_cells = 0;
  for (int p = bi + tid; p < ei; p += PV_THREADS) {
    const double X[3] = {(double)a.points[(size_t)p * 3 + 0], (double)a.points[(size_t)p * 3 + 1], (double)a.points[(size_t)p * 3 + 2]};
    double Xc[3], q[3];
    to_camera(Pi, X, Xc);
    const double d[3] = {Xc[0] - Pj.t[0], Xc[1] - Pj.t[1], Xc[2] - Pj.t[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double y = (Pj.R[0 * 3 + k] * d[0] + Pj.R[1 * 3 + k] * d[1]) + Pj.R[2 * 3 + k] * d[2];  // R_j^T d
      q[k] = floor((y - x0[k]) / h);
    }
    // decided in fp64: a double out of the range or a NaN is never converted
    if (!(q[0] >= 0.0 && q[0] < dG && q[1] >= 0.0 && q[1] < dG && q[2] >= 0.0 && q[2] < dG)) continue;
    const int cell = ((int)q[2] * G + (int)q[1]) * G + (int)q[0];
    n_in += (int)((bits[cell >> 5] >> (cell & 31)) & 1u);
  }
  for (int i = tid; i < words; i += PV_THREADS) n_cells += __popc(bits[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    n_in += __shfl_xor(n_in, o, 64);
    n_cells += __shfl_xor(n_cells, o, 64);
  }
  if ((tid & 63) == 0) {
    atomicAdd(&total[0], n_in);
    atomicAdd(&total[1], n_cells);
  }
  __syncthreads();
  if (tid == 0) {
    a.counts[(size_t)pair * 2 + 0] = total[0];
    a.counts[(size_t)pair * 2 + 1] = total[1];
    a.overlap[pair] = (double)total[0] / (double)(ei - bi);
    a.status[pair] = 0;
  }
}

__global__ __launch_bounds__(PN_MAX_GROUP) void pose_nms_greedy_kernel(PoseNmsArgs a) {
  __shared__ unsigned conflict[PN_MAX_GROUP * PN_ROW_WORDS];  // bit (c & 31) of word r * 8 + (c >> 5): ranks r and c conflict
  __shared__ unsigned alive[PN_ROW_WORDS];                    // bit r: rank r has not been suppressed

  const int group = blockIdx.x, tid = threadIdx.x;
  // (the host validates the tables; the clamps keep a bad one that reaches the kernel all the same inside the arrays)
  const OffsetRange poses = offset_range(a.group_off, group, a.n_poses), prs = offset_range(a.pair_off, group, a.n_pairs);
  const int begin = poses.begin, n = min(poses.n, PN_MAX_GROUP);
  const int pb = prs.begin, pe = prs.begin + prs.n;

  // ---- phase A: the conflict matrix
  for (int i = tid; i < n * PN_ROW_WORDS; i += PN_MAX_GROUP) conflict[i] = 0u;
  if (tid < PN_ROW_WORDS) {
    const int left = n - tid * 32;  // ranks of this word
    alive[tid] = left >= 32 ? 0xffffffffu : (left > 0 ? (1u << left) - 1u : 0u);
  }
  __syncthreads();
  for (int p = pb + tid; p < pe; p += PN_MAX_GROUP) {
    if (a.status[p] != 0 || !(a.overlap[p] >= a.thresh)) continue;
    const int r = a.pairs[(size_t)p * 2 + 0] - begin, c = a.pairs[(size_t)p * 2 + 1] - begin;
    if (r < 0 || r >= n || c < 0 || c >= n || r == c) continue;
    atomicOr(&conflict[r * PN_ROW_WORDS + (c >> 5)], 1u << (c & 31));
    atomicOr(&conflict[c * PN_ROW_WORDS + (r >> 5)], 1u << (r & 31));
  }

  // ---- phase B: rank by rank; every thread reaches every barrier (n is block-uniform)
  bool mine = tid < n;  // this thread's rank is alive
  int by = -1;
  for (int r = 0; r < n; ++r) {
    __syncthreads();  // phase A's bits, and the alive bits cleared for ranks below r
    if (!((alive[r >> 5] >> (r & 31)) & 1u)) continue;  // block-uniform
    if (mine && tid > r && ((conflict[r * PN_ROW_WORDS + (tid >> 5)] >> (tid & 31)) & 1u)) {
      mine = false;
      by = begin + r;
      atomicAnd(&alive[tid >> 5], ~(1u << (tid & 31)));  // read as bit `tid` only from round tid on, after a barrier
    }
  }
  if (tid < n) {
    a.keep[begin + tid] = mine ? 1 : 0;
    a.suppressed_by[begin + tid] = by;
  }
}

}  // namespace

int launch_pose_overlap(const PoseOverlapArgs& a, int num_pairs, hipStream_t st) {
  FP_REQUIRE(a.grid >= PN_MIN_GRID && a.grid <= PN_MAX_GRID, "pose_overlap: grid must be in [%d, %d] (got %d)", PN_MIN_GRID, PN_MAX_GRID, a.grid);
  FP_REQUIRE(a.m_total >= 0 && a.m_total <= (1 << 30), "pose_overlap: %d sampled points (at most 2^30: the point loop counts in int)", a.m_total);
  FP_REQUIRE(a.n_objects >= 0 && a.n_poses >= 0 && num_pairs >= 0, "pose_overlap: negative count");
  if (num_pairs == 0) return FP_OK;
  hipLaunchKernelGGL(pose_overlap_kernel, dim3(num_pairs), dim3(PV_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("pose_overlap");
  return FP_OK;
}

int launch_pose_nms_greedy(const PoseNmsArgs& a, int num_groups, hipStream_t st) {
  FP_REQUIRE(num_groups >= 0 && a.n_poses >= 0 && a.n_pairs >= 0, "pose_nms_greedy: negative count");
  FP_REQUIRE(a.thresh == a.thresh, "pose_nms_greedy: the threshold is NaN");
  if (num_groups == 0) return FP_OK;
  hipLaunchKernelGGL(pose_nms_greedy_kernel, dim3(num_groups), dim3(PN_MAX_GROUP), 0, st, a);
  FP_CHECK_LAUNCH("pose_nms_greedy");
  return FP_OK;
}
