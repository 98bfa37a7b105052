// The RANSAC skeleton shared by the two coarse-pose solvers (pnp.hip: P3P on pixels; kabsch.hip: 3D-3D on
// depth-lifted points, section 16): the pose record, the keyed sampler, the sequential best-model rule, the output records and the
// fixed-order block reduction.  One 256-thread workgroup per (detection, template slot) pair in both.  What differs between the solvers
// (the minimal solver, the residual, the refinement of the winner, the LDS layout and the barriers) stays in its own file; each keeps its
// own __global__ function and calls these pieces.
// The functions are defined here, at global scope, without `static`: that is safe only because FP_DEVICE is
// __device__ __forceinline__ (every use is inlined, no symbol is emitted twice).  Keep them FP_DEVICE.
// Every floating-point statement stands as one source expression: the library is built with -ffp-contract=on, so splitting or merging
// one changes which multiplies fuse with which adds, and with that the output bits.
#pragma once
#include "common.hpp"
#include "rot.hpp"

constexpr int RANSAC_THREADS = 256;  // the block reduction below adds the partials of four waves

struct Pose {
  double R[9];
  double t[3];
};

FP_DEVICE unsigned long long mix64(unsigned long long z) {  // splitmix64 finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

FP_DEVICE bool normalize3(double* a) {
  const double n = sqrt(dot3(a, a));
  if (!(n > 1e-300)) return false;
  a[0] /= n; a[1] /= n; a[2] /= n;
  return true;
}

// orthonormal frame of a triangle: e1 along Q1-Q0, e3 normal, e2 = e3 x e1 (columns of F)
FP_DEVICE bool tri_frame(const double* q0, const double* q1, const double* q2, double* F) {
  double e1[3] = {q1[0] - q0[0], q1[1] - q0[1], q1[2] - q0[2]};
  double d2[3] = {q2[0] - q0[0], q2[1] - q0[1], q2[2] - q0[2]};
  double e3[3], e2[3];
  if (!normalize3(e1)) return false;
  cross3(e1, d2, e3);
  if (!normalize3(e3)) return false;
  cross3(e3, e1, e2);
  for (int r = 0; r < 3; ++r) { F[r * 3 + 0] = e1[r]; F[r * 3 + 1] = e2[r]; F[r * 3 + 2] = e3[r]; }
  return true;
}

// ---- the sampler: a counter-based hash of (seed, pair key, hypothesis)
// The base of a pair.  Its key is the caller's (a pair then draws the same hypotheses wherever it sits in a launch) or the pair's index in
// this launch.
FP_DEVICE unsigned long long ransac_pair_base(unsigned long long seed, const unsigned long long* pair_keys, int pair) {
  const unsigned long long key = pair_keys ? pair_keys[pair] : (unsigned long long)pair;
  return mix64(seed ^ (key * 0xD6E8FEB86659FD93ull));
}
FP_DEVICE unsigned long long ransac_hypothesis_key(unsigned long long base, int h) { return base + (unsigned long long)h * 0x9E3779B97F4A7C15ull; }

// NIDX distinct indices below N from the mix64 chain that starts at `key`.  A repeated index, or one that `accept` turns down, is drawn
// again; the draw gives up when attempt LAST_ATTEMPT of an index fails too (attempts count from 0).
template <int NIDX, int LAST_ATTEMPT, class Accept>
FP_DEVICE bool ransac_draw(unsigned long long key, int N, int* id, Accept accept) {
  unsigned long long s = key;
  for (int j = 0; j < NIDX; ++j) {
#pragma nounroll  // a redraw is rare and each draw waits for the one before it: copies of the 64-bit modulo only lengthen the kernel
    for (int attempt = 0;; ++attempt) {
      s = mix64(s);
      const int c = (int)(s % (unsigned long long)N);
      bool bad = !accept(c);
      for (int i = 0; i < j; ++i) bad |= id[i] == c;
      if (!bad) { id[j] = c; break; }
      if (attempt >= LAST_ATTEMPT) return false;
    }
  }
  return true;
}

// RANSACUpdateNumIters of OpenCV's point-set registrator
FP_DEVICE int update_num_iters(double p, double ep, int model_points, int max_iters) {
  p = fmin(fmax(p, 0.0), 1.0);
  ep = fmin(fmax(ep, 0.0), 1.0);
  double num = fmax(1.0 - p, 2.2250738585072014e-308);
  double denom = 1.0 - pow(1.0 - ep, (double)model_points);
  if (denom < 2.2250738585072014e-308) return 0;
  num = log(num);
  denom = log(denom);
  return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

// The sequential best-model rule with the adaptive iteration budget, replayed over the counts of all hypotheses (one thread): a model
// must beat model_points - 1 inliers, the first of the highest count within the budget wins.  Returns its index, or -1.
FP_DEVICE int ransac_replay(const int* cnt, int iters, double conf, int model_points, int population, int* best_count) {
  int best = -1, best_c = model_points - 1, niters = iters;
  for (int h = 0; h < niters; ++h) {
    if (cnt[h] > best_c) {
      best_c = cnt[h];
      best = h;
      niters = update_num_iters(conf, (double)(population - best_c) / population, model_points, niters);
    }
  }
  *best_count = best_c;
  return best;
}

// ---- the output records of a pair (A: PnpArgs or KabschArgs)
// no pose: the status code, identity, zeros and an empty mask row (the whole block calls it)
template <class A>
FP_DEVICE void ransac_write_failure(const A& a, int pair, int tid, int code) {
  if (tid == 0) {
    a.success[pair] = code;
    a.n_inliers[pair] = 0;
    for (int i = 0; i < 9; ++i) a.R[(size_t)pair * 9 + i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int i = 0; i < 3; ++i) a.t[(size_t)pair * 3 + i] = 0.0;
    if (a.ransac_pose) for (int i = 0; i < 12; ++i) a.ransac_pose[(size_t)pair * 12 + i] = 0.0;
  }
  for (int i = tid; i < a.k_max; i += RANSAC_THREADS) a.inlier_mask[(size_t)pair * a.k_max + i] = 0;
}
// the winning hypothesis: its inliers among the first N correspondences (`inlier(p)`) into LDS and the mask row, itself into ransac_pose
// (the whole block calls it)
template <class A, class Inlier>
FP_DEVICE void ransac_write_winner(const A& a, int pair, int tid, int N, const Pose& cur, unsigned char* inl, Inlier inlier) {
  for (int p = tid; p < a.k_max; p += RANSAC_THREADS) {
    const unsigned char m = p < N && inlier(p);
    if (p < N) inl[p] = m;
    a.inlier_mask[(size_t)pair * a.k_max + p] = m;
  }
  if (tid == 0 && a.ransac_pose) {
    for (int i = 0; i < 9; ++i) a.ransac_pose[(size_t)pair * 12 + i] = cur.R[i];
    for (int i = 0; i < 3; ++i) a.ransac_pose[(size_t)pair * 12 + 9 + i] = cur.t[i];
  }
}
// the final pose (one thread)
template <class A>
FP_DEVICE void ransac_write_pose(const A& a, int pair, int count, const Pose& cur) {
  a.success[pair] = 1;
  a.n_inliers[pair] = count;
  for (int i = 0; i < 9; ++i) a.R[(size_t)pair * 9 + i] = cur.R[i];
  for (int i = 0; i < 3; ++i) a.t[(size_t)pair * 3 + i] = cur.t[i];
}

// ---- block reduction in a fixed order: the per-thread partial sums v[first .. NV) -> one partial per wave in acc (butterfly within a
// wave), then a barrier; block_total adds the waves 0..3 in order.  The caller places the barrier that ends the reads of acc.
template <int NV, int W>
FP_DEVICE void block_partials(const double* v, double (*acc)[W], int tid, int first = 0) {
  static_assert(NV <= W, "acc is too narrow");
  for (int i = first; i < NV; ++i) {
    double s = v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) acc[tid >> 6][i] = s;
  }
  __syncthreads();
}
template <int W>
FP_DEVICE double block_total(double (*acc)[W], int i) { return acc[0][i] + acc[1][i] + acc[2][i] + acc[3][i]; }
// ... and for a caller that wants all NV totals in out[]: one thread writes them, a barrier publishes them
template <int NV, int W>
FP_DEVICE void block_sums(const double* v, double (*acc)[W], double* out, int tid) {
  block_partials<NV>(v, acc, tid);
  if (tid == 0)
    for (int i = 0; i < NV; ++i) out[i] = block_total(acc, i);
  __syncthreads();
}
