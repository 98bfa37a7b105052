// Parts shared by the kernels that work on groups of rows behind offset tables: the two AP scorers (detection_ap.hip, coco_eval.hip), the
// detection masks, the pose NMS, VSD and the GT visibility.
//   offset_range, group_dims   a table's entry i as a range that lies inside its array whatever the table holds;
//   last_at_or_before          the owner of a position: the last entry of an ascending table that starts at or before it;
//   block_scan_inclusive       the inclusive prefix sum over the 256 threads of a workgroup;
//   greedy_match               the greedy matching of one group's estimates, in rank order, by one wave.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

// ------------------------------------------------------------------ offset tables
// Entries [begin, begin + n) of an array of `total`, as off[i] and off[i + 1] name them (the host validates the tables; the clamps keep a
// bad one that reaches the kernel all the same inside the array).
struct OffsetRange { int begin, n; };
FP_DEVICE OffsetRange offset_range(const int* off, int i, int total) {
  OffsetRange r;
  r.begin = clampi(off[i], 0, total);
  r.n = max(min(off[i + 1], total) - r.begin, 0);
  return r;
}

// A group as the kernels use it (clamped like an offset_range): rows [e0, e0 + E) of a, [g0, g0 + G) of b, output rows p0 + e G + j, all
// of them below n_pairs.
struct GroupDims { int e0, E, g0, G, p0; };
FP_DEVICE GroupDims group_dims(const GroupTables& t, int g, int max_G) {
  GroupDims d;
  d.e0 = clampi(t.est_off[g], 0, t.n_a);
  d.E = max(min(t.est_off[g + 1], t.n_a) - d.e0, 0);
  d.g0 = clampi(t.gt_off[g], 0, t.n_b);
  d.G = clampi(min(t.gt_off[g + 1], t.n_b) - d.g0, 0, max_G);
  d.p0 = clampi(t.pair_off[g], 0, t.n_pairs);
  if (d.G > 0) d.E = (int)min((long long)d.E, (long long)(t.n_pairs - d.p0) / d.G);
  return d;
}

// The last i in [0, n) with first(i) <= x, for an ascending first: the entry that owns x (entries that own nothing share a start with the
// next one, and the last of them wins).  0 when no entry starts at or before x, or n <= 0.
template <class X, class First>
FP_DEVICE int last_at_or_before(int n, X x, First first) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first(mid) <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// ------------------------------------------------------------------ the block scan
// The inclusive prefix sum of v over the 256 threads of a workgroup (int or long long: the order of the additions does not matter), and
// the sum of all 256 in `total`.  Every thread of the workgroup calls it.  slots: 4 entries of LDS; the barrier inside orders their
// writes before their reads, and the CALLER owes a __syncthreads() between this call's return and the next write of slots (the next
// call included), because a wave may still be reading them.
constexpr int BS_THREADS = 256, BS_WAVES = BS_THREADS / 64;
template <class T>
FP_DEVICE T block_scan_inclusive(T v, T* slots, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const T up = __shfl_up(v, s, 64);
    if (lane >= s) v += up;
  }
  if (lane == 63) slots[wave] = v;
  __syncthreads();
  total = 0;
#pragma unroll
  for (int w = 0; w < BS_WAVES; ++w) {
    const T t = slots[w];
    if (w < wave) v += t;
    total += t;
  }
  return v;
}

// ------------------------------------------------------------------ the greedy matcher
// One wave matches the estimates of one group, in rank order, for one column of the output.  Lane l owns the group's GT instances l, l + 64,
// l + 128, l + 192 (a group has at most GM_MAX_GT = 256) and keeps their matched bits in a register.  For every estimate each lane picks
// the best of its free candidates, a butterfly takes the best over the wave, the winner's owner sets its bit and writes the estimate's two
// outputs; lane 0 writes for an estimate without a match.  No LDS and no barrier.
//
// Both kernels launch it in one geometry: GM_WAVES waves per workgroup, wave w of the launch owning (group, column) number w; match_wave()
// gives that number, and a wave past the last one leaves at once (wave-uniform).
//
// A Policy states what differs between the scorers:
//   bool second_class(int gt_row)   the instance is of the second class (an invalid or an ignored GT): a match with it writes flag 2, any
//                                   other match flag 1;
//   double value(size_t row)        row p0 + e G + gi of the group's values;
//   bool candidate(double v)        the estimate may take an instance of this value.  Never true for a NaN, so the order below is total;
//   MatchKey none()                 the key that every candidate comes before; its index must be one that no instance has (it is how an
//                                   estimate without a match is told from a matched one);
//   bool before(MatchKey a, b)      a strict total order over (class, value, index): a is the better match.
constexpr int GM_THREADS = 256, GM_WAVES = GM_THREADS / 64;
constexpr int GM_MAX_GT = DA_MAX_GROUP_GT, GM_GT_PER_LANE = GM_MAX_GT / 64;  // 4

struct MatchKey {
  int cls;   // 1: an instance of the second class
  double v;
  int g;     // the group-local instance
};

FP_DEVICE long long match_wave() { return (long long)blockIdx.x * GM_WAVES + (threadIdx.x >> 6); }
static inline long long match_blocks(long long waves) { return (waves + GM_WAVES - 1) / GM_WAVES; }  // workgroups of GM_THREADS

template <class Policy>
FP_DEVICE void greedy_match(const Policy& p, const GroupDims& d, int lane, signed char* flag, int* matched, size_t out0, int out_stride) {
  unsigned taken = 0u;   // bit j: this lane's instance lane + 64 j is matched
  unsigned second = 0u;  // bit j: ... is of the second class
#pragma unroll
  for (int j = 0; j < GM_GT_PER_LANE; ++j) {
    const int gi = lane + 64 * j;
    if (gi < d.G && p.second_class(d.g0 + gi)) second |= 1u << j;
  }

  for (int e = 0; e < d.E; ++e) {
    const size_t row = (size_t)d.p0 + (size_t)e * d.G;
    MatchKey best = p.none();
#pragma unroll
    for (int j = 0; j < GM_GT_PER_LANE; ++j) {
      const int gi = lane + 64 * j;
      if (gi < d.G && !((taken >> j) & 1u)) {
        const MatchKey k{(int)((second >> j) & 1u), p.value(row + gi), gi};
        if (p.candidate(k.v) && p.before(k, best)) best = k;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const MatchKey k{__shfl_xor(best.cls, o, 64), __shfl_xor(best.v, o, 64), __shfl_xor(best.g, o, 64)};
      if (p.before(k, best)) best = k;
    }
    const size_t out = out0 + (size_t)e * out_stride;
    if (best.g == p.none().g) {
      if (lane == 0) { flag[out] = 0; matched[out] = -1; }
    } else if ((best.g & 63) == lane) {
      const int j = best.g >> 6;
      taken |= 1u << j;  // used up whatever its class
      flag[out] = ((second >> j) & 1u) ? 2 : 1;
      matched[out] = best.g;
    }
  }
}
