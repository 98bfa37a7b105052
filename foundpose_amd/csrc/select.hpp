// Key selection on 64-bit (value, index) keys: the two encodings, sorted per-lane lists and the minima over them.
// Device-only, no state (retrieve.hip: template retrieval; match.hip: k-NN merge, cyclic selection; f32_tile.hip: per-tile k-selection).
// A key is (32 order bits << 32) | 32-bit index, and the unsigned order of keys is the order of the selection:
// SMALLER KEY = BETTER, equal values -> the lower index wins, ~0ull = empty (never beats a real key).  The index makes
// the keys of one row distinct, so a key found by a minimum over lanes has exactly one holder.
//   distance form  pack_dist_idx: a non-negative float orders like its bit pattern -> smallest distance first.
//   score form     score_key: the float's bits folded to ascending unsigned order, then complemented -> largest score first
//                  (largest = false keeps the ascending form).  A NaN ranks by its bits: +NaN before +inf, -NaN after -inf;
//                  score_key_nan_first sends a NaN of either sign to the front, as torch.topk does.
#pragma once
#include "common.hpp"

FP_DEVICE unsigned long long pack_dist_idx(float d2, unsigned idx) { return ((unsigned long long)__float_as_uint(d2) << 32) | idx; }
FP_DEVICE unsigned long long score_key(float v, unsigned idx, bool largest = true) {
  unsigned b = __float_as_uint(v);
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);  // ascending float order as unsigned
  return ((unsigned long long)(largest ? ~b : b) << 32) | idx;
}
FP_DEVICE unsigned long long score_key_nan_first(float v, unsigned idx) { return score_key(v != v ? __uint_as_float(0x7fc00000u) : v, idx); }
// ... and back (score form, largest first): the score's own bits
FP_DEVICE float key_score(unsigned long long key) {
  const unsigned kb = ~(unsigned)(key >> 32);
  return __uint_as_float((kb & 0x80000000u) ? (kb ^ 0x80000000u) : ~kb);
}
FP_DEVICE int key_index(unsigned long long key) { return (int)(key & 0xffffffffu); }  // either form

// best[0..N) ascending (best first), empty slots last.  One compare per slot: the smaller key stays, the larger moves on.
template <int N>
FP_DEVICE void sorted_insert(unsigned long long (&best)[N], unsigned long long key) {
#pragma unroll
  for (int s = 0; s < N; ++s) {
    const unsigned long long lo = key < best[s] ? key : best[s];
    key = key < best[s] ? best[s] : key;
    best[s] = lo;
  }
}
template <int N>
FP_DEVICE void pop_front(unsigned long long (&best)[N]) {
#pragma unroll
  for (int t = 0; t + 1 < N; ++t) best[t] = best[t + 1];
  best[N - 1] = ~0ull;
}

// minimum over the 16 lanes of an aligned group (beside wave_min_u64 of common.hpp)
FP_DEVICE unsigned long long min16_u64(unsigned long long v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 16);
    v = t < v ? t : v;
  }
  return v;
}
// ... and over a block of WAVES waves through wmin[WAVES] in LDS (block-uniform; the caller puts a barrier before wmin is written again)
template <int WAVES>
FP_DEVICE unsigned long long block_min_u64(unsigned long long v, unsigned long long* wmin, int lane, int wave) {
  v = wave_min_u64(v);
  if (lane == 0) wmin[wave] = v;
  __syncthreads();
  v = wmin[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) v = wmin[w] < v ? wmin[w] : v;
  return v;
}

// The tail of a one-wave-per-row merge (score form): `rounds` (n_top, or n_top + 1 for the tie test) rounds of wave-wide arg-best
// over the lanes' sorted lists; the holder of a round's winner writes entry s < n_top of the row and pops it, a round with no key
// left writes (-1, -inf).  Returns 1 (wave-uniform) when the scores taken are not strictly decreasing: an equal pair, +-0, or a NaN.
template <int N>
FP_DEVICE int emit_best_rounds(unsigned long long (&best)[N], int rounds, int n_top, int row, int lane,
                               float* __restrict__ out_val, int* __restrict__ out_idx) {
  float prev = 0.f;
  int tie = 0;
  for (int s = 0; s < rounds; ++s) {
    const unsigned long long b = wave_min_u64(best[0]);
    if (b == ~0ull) {
      if (lane == 0 && s < n_top) { out_idx[(size_t)row * n_top + s] = -1; out_val[(size_t)row * n_top + s] = -INFINITY; }
      continue;
    }
    const float val = key_score(b);
    if (val != val || (s > 0 && !(prev > val))) tie = 1;  // wave-uniform
    prev = val;
    if (best[0] == b) {
      if (s < n_top) {
        out_idx[(size_t)row * n_top + s] = key_index(b);
        out_val[(size_t)row * n_top + s] = val;
      }
      pop_front(best);
    }
  }
  return tie;
}
