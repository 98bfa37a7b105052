// COCO average precision of a detections file (foundpose_amd/eval_coco.py): what BOP's 2D detection and 2D segmentation
// tasks measure.  The rules restate the published behaviour of pycocotools' COCOeval (evaluateImg without iscrowd instances); the package is
// not installed, so nothing is pinned against its code.  fp_detection_masks decodes the run lengths and fp_detection_ap accumulates precision
// and recall; this file holds what lies between them.
//
// mask_pack_kernel: one 256-thread workgroup per mask.  Byte masks become rows of 64-bit words, bit x % 64 of word (y, x / 64) = pixel (x, y).
//   Where the mask's base is 16-byte aligned and W is a multiple of 16 a lane reads 16 bytes (a multiply gathers the four non-zero flags of
//   a dword), four neighbouring lanes OR their quarters together with two shuffles and the first of them stores the word: the wave reads 1 KiB
//   of consecutive bytes per instruction.  Otherwise a thread assembles its word from bytes.  The area is the popcount of the words written.
//
// group_tiles_kernel: one workgroup.  The exclusive scan (group_parts.hpp's block scan, in chunks of 256 groups) of the groups' tile counts, ceil(E_g / 4) ceil(G_g / 4), and ceil(E_g / 4) for a
//   group of one instance: the tile table of the next kernel, made on the device because the group tables live there.
//
// group_mask_iou_kernel: the hot one.  A workgroup owns a tile of 4 a-rows x 4 b-rows of one group (4 x 1 where the group has one instance)
//   and walks the L words of its rows once: per word 8 loads feed 16 AND + popcount for the intersections and 8 popcounts for the areas, all
//   in registers.  A wave butterfly and 4 x 24 LDS slots finish the 24 sums; 16 threads write the tile's pairs.  Per pair this reads L / 2
//   words instead of 2 L (1.25 L in a 4 x 1 tile).  The grid is the tile count's host-side upper bound; a workgroup finds its (group,
//   a-tile, b-tile) by a binary search in the tile table (last_at_or_before) and strides on, so no tile is lost when the bound is short.  Rows past the
//   group's edge repeat its last row and are not written.
//
// group_box_iou_kernel: one thread per pair; the thread finds its group by a binary search in pair_off.  fp64, one rounded operation each.
//
// coco_match_kernel: one wave per (group, threshold), four waves per 256-thread workgroup.  The wave runs the shared greedy matcher of
//   group_parts.hpp (no barrier, no LDS) under COCO's policy: an estimate may take a free GT whose overlap reaches min(threshold, 1 - 1e-10),
//   the largest (non-ignored, overlap, GT index) wins, and a match with an ignored GT writes flag 2.
//
// All counting is integer arithmetic; an overlap is one division.  Every result depends on its own group's or mask's data only: it is the
// same bits alone, in any batch and at any position.  FMA contraction is off in the box kernel; there are no atomics.
#include "common.hpp"
#include "group_parts.hpp"

namespace {

constexpr int CE_WAVES = CE_THREADS / 64;
static_assert(CE_THREADS == BS_THREADS, "group_tiles_kernel scans with block_scan_inclusive");
constexpr int CE_SUMS = CE_TILE_A * CE_TILE_B + CE_TILE_A + CE_TILE_B;  // intersections, areas of a, areas of b

// ------------------------------------------------------------------ bytes -> bits
// bit k = byte k of v is non-zero: the carry of 0x7f + (low seven bits) or the top bit itself marks the byte, the multiply gathers the marks
FP_DEVICE unsigned nonzero_bytes(unsigned v) {
  const unsigned t = (v | ((v & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
  return (((t >> 7) * 0x01020408u) >> 24) & 0xfu;
}

__global__ __launch_bounds__(CE_THREADS) void mask_pack_kernel(MaskPackArgs a) {
  __shared__ int part[CE_WAVES];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = a.H * a.W, nw = a.H * a.Wq;  // n <= 2^30: checked by the launcher
  const unsigned char* __restrict__ m = a.masks + (size_t)p * n;
  unsigned long long* __restrict__ out = a.words + (size_t)p * nw;
  int cnt = 0;
  if ((reinterpret_cast<size_t>(m) & 15) == 0 && (a.W & 15) == 0) {  // block-uniform: every 16-pixel quarter of a word is an aligned uint4
    const int quarter = tid & 3;
    for (int w0 = 0; w0 < nw; w0 += CE_THREADS / 4) {  // the same trip count for every lane: the shuffles need all of them
      const int w = w0 + (tid >> 2);
      unsigned long long bits = 0ull;
      if (w < nw) {
        const int y = w / a.Wq, x = (w - y * a.Wq) * 64 + quarter * 16;
        if (x < a.W) {
          const uint4 v = *reinterpret_cast<const uint4*>(m + (size_t)y * a.W + x);
          const unsigned q16 = nonzero_bytes(v.x) | (nonzero_bytes(v.y) << 4) | (nonzero_bytes(v.z) << 8) | (nonzero_bytes(v.w) << 12);
          bits = (unsigned long long)q16 << (16 * quarter);
        }
      }
      bits |= __shfl_xor(bits, 1, 64);
      bits |= __shfl_xor(bits, 2, 64);
      if (w < nw && quarter == 0) {
        out[w] = bits;
        cnt += __popcll(bits);
      }
    }
  } else {
    for (int w = tid; w < nw; w += CE_THREADS) {
      const int y = w / a.Wq, x0 = (w - y * a.Wq) * 64;
      const int nb = min(64, a.W - x0);
      const unsigned char* r = m + (size_t)y * a.W + x0;
      unsigned long long bits = 0ull;
      for (int i = 0; i < nb; ++i) bits |= (unsigned long long)(r[i] != 0) << i;
      out[w] = bits;
      cnt += __popcll(bits);
    }
  }
  cnt = wave_sum(cnt);
  if ((tid & 63) == 0) part[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < CE_WAVES; ++w) cnt += part[w];
    a.area[p] = cnt;
  }
}

// ------------------------------------------------------------------ the tile table
// Tile columns of a group of G rows of b: a group with ONE instance (the common case of a BOP frame) takes 4 x 1 tiles -- a 4 x 4 tile would
// load and count its single b-row four times --, every other group 4 x 4 tiles.
FP_DEVICE int tile_cols(int G) { return G == 1 ? 1 : (G + CE_TILE_B - 1) / CE_TILE_B; }

__global__ __launch_bounds__(CE_THREADS) void group_tiles_kernel(GroupMaskIouArgs a) {
  __shared__ long long slots[BS_WAVES];
  const int tid = threadIdx.x;
  long long carry = 0;
  if (tid == 0) a.tile_off[0] = 0;
  for (int base = 0; base < a.t.n_groups; base += CE_THREADS) {
    const int g = base + tid;
    long long tiles = 0, chunk;
    if (g < a.t.n_groups) {
      const GroupDims d = group_dims(a.t, g, INT32_MAX);
      tiles = (long long)((d.E + CE_TILE_A - 1) / CE_TILE_A) * tile_cols(d.G);
    }
    const long long incl = block_scan_inclusive(tiles, slots, chunk);
    if (g < a.t.n_groups) a.tile_off[g + 1] = (int)min(carry + incl, (long long)INT32_MAX);  // (the launcher bounds the sum of a sound table)
    carry += chunk;
    __syncthreads();  // slots are written again in the next round
  }
}

// ------------------------------------------------------------------ intersections and unions of packed masks
// One tile: TA rows of a x TB rows of b of the group d, from tile row ta and tile column tb.  Block-uniform; ends behind a barrier.
template <int TA, int TB>
FP_DEVICE void mask_iou_tile(const GroupMaskIouArgs& a, const GroupDims& d, int ta, int tb, int (*red)[CE_SUMS]) {
  constexpr int NS = TA * TB + TA + TB;  // intersections, areas of a, areas of b
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, L = a.L;
  const unsigned long long* pa[TA];
  const unsigned long long* pb[TB];
#pragma unroll
  for (int i = 0; i < TA; ++i) pa[i] = a.words_a + (size_t)(d.e0 + min(ta * TA + i, d.E - 1)) * L;
#pragma unroll
  for (int j = 0; j < TB; ++j) pb[j] = a.words_b + (size_t)(d.g0 + min(tb * TB + j, d.G - 1)) * L;

  int sum[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) sum[s] = 0;
#pragma unroll 2
  for (int w = tid; w < L; w += CE_THREADS) {
    unsigned long long va[TA], vb[TB];
#pragma unroll
    for (int i = 0; i < TA; ++i) va[i] = pa[i][w];
#pragma unroll
    for (int j = 0; j < TB; ++j) vb[j] = pb[j][w];
#pragma unroll
    for (int i = 0; i < TA; ++i) {
      sum[TA * TB + i] += __popcll(va[i]);
#pragma unroll
      for (int j = 0; j < TB; ++j) sum[i * TB + j] += __popcll(va[i] & vb[j]);
    }
#pragma unroll
    for (int j = 0; j < TB; ++j) sum[TA * TB + TA + j] += __popcll(vb[j]);
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) sum[s] = wave_sum(sum[s]);
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < NS; ++s) red[wave][s] = sum[s];
  }
  __syncthreads();
  if (tid < TA * TB) {
    const int i = tid / TB, j = tid - i * TB;
    const int e = ta * TA + i, gi = tb * TB + j;
    if (e < d.E && gi < d.G) {
      int inter = 0, area_a = 0, area_b = 0;
#pragma unroll
      for (int v = 0; v < CE_WAVES; ++v) {
        inter += red[v][tid];
        area_a += red[v][TA * TB + i];
        area_b += red[v][TA * TB + TA + j];
      }
      const int uni = area_a + (area_b - inter);  // each term and the sum are at most 64 L <= 2^30
      const size_t row = (size_t)d.p0 + (size_t)e * d.G + gi;
      a.counts[row * 2 + 0] = inter;
      a.counts[row * 2 + 1] = uni;
      a.overlap[row] = uni > 0 ? (double)inter / (double)uni : 0.0;
      a.status[row] = uni > 0 ? 0 : 2;
    }
  }
  __syncthreads();  // red is written again for the next tile
}

__global__ __launch_bounds__(CE_THREADS) void group_mask_iou_kernel(GroupMaskIouArgs a) {
  __shared__ int red[CE_WAVES][CE_SUMS];
  const int NG = a.t.n_groups;
  const int total = a.tile_off[NG];
  for (int tile = blockIdx.x; tile < total; tile += gridDim.x) {  // block-uniform throughout
    const int lo = last_at_or_before(NG, tile, [&](int g) { return a.tile_off[g]; });  // the group that owns the tile
    const GroupDims d = group_dims(a.t, lo, INT32_MAX);
    if (d.E <= 0 || d.G <= 0) continue;
    const int nb = tile_cols(d.G);
    const int local = tile - a.tile_off[lo];
    const int ta = local / nb, tb = local - ta * nb;
    if (ta * CE_TILE_A >= d.E) continue;
    if (d.G == 1) mask_iou_tile<CE_TILE_A, 1>(a, d, ta, tb, red);
    else mask_iou_tile<CE_TILE_A, CE_TILE_B>(a, d, ta, tb, red);
  }
}

// ------------------------------------------------------------------ overlaps of (x, y, w, h) boxes
__global__ __launch_bounds__(CE_THREADS) void group_box_iou_kernel(GroupBoxIouArgs a) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * CE_THREADS + threadIdx.x;
  if (q >= a.t.n_pairs) return;
  const int lo = last_at_or_before(a.t.n_groups, q, [&](int g) { return a.t.pair_off[g]; });
  double ov = 0.0;
  int st = 2;  // a row that no group owns is answered like a union of 0
  const GroupDims d = group_dims(a.t, lo, INT32_MAX);
  const long long rel = (long long)q - d.p0;
  if (d.G > 0 && rel >= 0 && rel < (long long)d.E * d.G) {
    const int e = (int)(rel / d.G), gi = (int)(rel - (long long)e * d.G);
    const double* A = a.boxes_a + (size_t)(d.e0 + e) * 4;
    const double* B = a.boxes_b + (size_t)(d.g0 + gi) * 4;
    const double xa = A[0], ya = A[1], wa = A[2], ha = A[3], xb = B[0], yb = B[1], wb = B[2], hb = B[3];
    const double iw = fmin(xa + wa, xb + wb) - fmax(xa, xb);
    const double ih = fmin(ya + ha, yb + hb) - fmax(ya, yb);
    const double inter = (iw > 0.0 && ih > 0.0) ? iw * ih : 0.0;
    const double uni = (wa * ha + wb * hb) - inter;
    if (uni > 0.0) {  // false for a NaN too
      ov = inter / uni;
      st = 0;
    }
  }
  a.overlap[q] = ov;
  a.status[q] = st;
}

// ------------------------------------------------------------------ COCO's matching
// COCO's matching rule for greedy_match: one IoU threshold.
struct CocoPolicy {
  const double* overlap;  // [P]
  const int* gt_ignore;
  double bound;           // min(threshold, 1 - 1e-10)
  FP_DEVICE bool second_class(int gt_row) const { return gt_ignore[gt_row] != 0; }  // an ignored GT: it ranks below every regular one
  FP_DEVICE double value(size_t row) const { return overlap[row]; }
  FP_DEVICE bool candidate(double v) const { return v >= bound; }                   // false for a NaN
  FP_DEVICE MatchKey none() const { return {2, 0.0, -1}; }
  FP_DEVICE bool before(const MatchKey& a, const MatchKey& b) const {
    return a.cls < b.cls || (a.cls == b.cls && (a.v > b.v || (a.v == b.v && a.g > b.g)));
  }
};

__global__ __launch_bounds__(GM_THREADS) void coco_match_kernel(CocoMatchArgs a) {
  const long long w = match_wave();
  if (w >= (long long)a.t.n_groups * a.T) return;  // wave-uniform
  const int g = (int)(w / a.T), k = (int)(w % a.T);
  const GroupDims d = group_dims(a.t, g, GM_MAX_GT);
  const CocoPolicy p{a.overlap, a.gt_ignore, fmin(a.ths[k], 1.0 - 1e-10)};
  greedy_match(p, d, threadIdx.x & 63, a.flag, a.matched_gt, (size_t)d.e0 * a.T + k, a.T);
}

}  // namespace

int launch_mask_pack(const MaskPackArgs& a, int num_masks, hipStream_t st) {
  FP_REQUIRE(num_masks >= 0 && a.H >= 1 && a.W >= 1 && (long long)a.H * a.W <= (1ll << 30),
             "mask_pack: %d masks of %d x %d (H, W >= 1, H W at most 2^30: the pixel index is an int)", num_masks, a.W, a.H);
  if (num_masks == 0) return FP_OK;
  hipLaunchKernelGGL(mask_pack_kernel, dim3(num_masks), dim3(CE_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("mask_pack");
  return FP_OK;
}

int launch_group_mask_iou(const GroupMaskIouArgs& a, hipStream_t st) {
  const GroupTables& t = a.t;
  FP_REQUIRE(t.n_groups >= 0 && t.n_a >= 0 && t.n_b >= 0 && t.n_pairs >= 0, "group_mask_iou: negative count");
  FP_REQUIRE(a.L >= 1 && a.L <= (1 << 24), "group_mask_iou: rows of %d words (1 .. 2^24: the counts are int32)", a.L);
  if (t.n_groups == 0 || t.n_pairs == 0) return FP_OK;
  // ceil(E / 4) ceil(G / 4) <= E G / 16 + (E + G) / 4 + 1 per group with a pair
  const long long bound = (long long)t.n_pairs / (CE_TILE_A * CE_TILE_B) + t.n_a / CE_TILE_A + t.n_b / CE_TILE_B + (long long)t.n_groups + 3;
  FP_REQUIRE(bound <= 0x7fffffffLL, "group_mask_iou: %d pairs in %d groups are too many for one launch", t.n_pairs, t.n_groups);
  hipLaunchKernelGGL(group_tiles_kernel, dim3(1), dim3(CE_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("group_mask_iou (tiles)");
  hipLaunchKernelGGL(group_mask_iou_kernel, dim3((unsigned)bound), dim3(CE_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("group_mask_iou");
  return FP_OK;
}

int launch_group_box_iou(const GroupBoxIouArgs& a, hipStream_t st) {
  const GroupTables& t = a.t;
  FP_REQUIRE(t.n_groups >= 0 && t.n_a >= 0 && t.n_b >= 0 && t.n_pairs >= 0, "group_box_iou: negative count");
  if (t.n_groups == 0 || t.n_pairs == 0) return FP_OK;
  hipLaunchKernelGGL(group_box_iou_kernel, dim3(cdiv(t.n_pairs, CE_THREADS)), dim3(CE_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("group_box_iou");
  return FP_OK;
}

int launch_coco_match(const CocoMatchArgs& a, hipStream_t st) {
  const GroupTables& t = a.t;
  FP_REQUIRE(a.T >= 1 && a.T <= DA_MAX_THS, "coco_match: T must be in [1, %d] (got %d)", DA_MAX_THS, a.T);
  FP_REQUIRE(t.n_groups >= 0 && t.n_a >= 0 && t.n_b >= 0 && t.n_pairs >= 0, "coco_match: negative count");
  if (t.n_groups == 0) return FP_OK;
  const long long blocks = match_blocks((long long)t.n_groups * a.T);
  FP_REQUIRE(blocks <= 0x7fffffffLL, "coco_match: %d groups are too many for one launch", t.n_groups);
  hipLaunchKernelGGL(coco_match_kernel, dim3((unsigned)blocks), dim3(GM_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("coco_match");
  return FP_OK;
}
