// Labelling of class-agnostic mask proposals (foundpose_amd/detect_util.py): the device half of a CNOS-style detector.
// This stage is the project's own restatement of CNOS's published behaviour; the reference tree has no counterpart.
//
// mask_boxes_kernel: one 256-thread workgroup per proposal.  The mask is read once, 16 bytes per lane where its base is 16-byte aligned
//   (bytes otherwise and for the tail); a lane keeps min / max of x and y and a count of its set pixels, the wave butterfly and four LDS
//   slots finish them.  Integers only: box (x1, y1, x2, y2) with x2, y2 exclusive, (0, 0, 0, 0) and area 0 for an empty mask.
//
// proposal_crops_kernel: one 256-thread workgroup per (proposal, band of output rows).  With (w, h) the box size and L = max(w, h):
//   w' = max(1, (2 w S + L) / (2 L)), h' alike (integers: w S / L rounded half up), ox = (S - w') / 2, oy = (S - h') / 2.  Inside the
//   h' x w' window the value is the separable antialiased-bilinear resample (torch interpolate, bilinear, antialias, align_corners = False)
//   of image * (mask != 0) restricted to the box.  Per axis n_in -> n_out, in fp64: scale = n_in / n_out, sup = max(scale, 1), centre
//   c = scale (i + 0.5), taps lo = max(0, (int)(c - sup + 0.5)) .. hi = min(n_in, (int)(c + sup + 0.5)) exclusive, raw weight
//   r_j = max(0, 1 - |(j - c + 0.5) / sup|), n = ((r_lo + r_lo+1) + ...) j ascending, weight w_j = (float)(r_j * (1 / n)).
//   horizontal  the source rows the band needs, a chunk of rows at a time: thread (row, x) forms u[c] = fma(w_j, v_j[c], u[c]) from zero, j ascending
//               in fp32, for the three channels of one output column into LDS; consecutive lanes take consecutive x of one HWC row.  A masked
//               pixel contributes w_j * 0: it keeps its weight.
//   vertical    thread (output row, x) adds fma(w_j, u_j[c], acc[c]) for the source rows of the chunk, j ascending; its accumulators live in
//               LDS and are owned by that thread for the whole band, so the order is j ascending whatever the chunking.
//   store       every element of out[p, :, band rows, :] is written: the window from the accumulators, exact zeros elsewhere.
//   Nothing outside the box is read; an empty box, a box that leaves the image or an image_index outside its table gives status 2 and an
//   all-zero crop, and nothing is read.  No intermediate in HBM.
//
// proposal_prep_kernel / proposal_aggregate_kernel: fp_proposal_scores lists the P descriptors once per object and hands them to
//   fp_cosine_topk's own launch (tie order 0), so a similarity IS that chain's bits; the aggregate takes m = min(k, T_o) of the k best,
//   adds them left to right in fp32, divides once by (float)m and picks the best object (ties to the lower object, a NaN never wins).
//
// proposal_rank_kernel: one workgroup for one image.  Every proposal gets a decision; the candidates are laid out per object in rank order
//   (score descending, equal scores in input order), at most `max_group` of an object, together with the pairs of each group -- the tables
//   box_iou_kernel and fp_pose_nms_greedy take, made without a read-back.  Integer counting and float comparisons only.
//
// box_iou_kernel: one thread per pair; intersection and union in int64, one fp64 division.
//
// patch_cover_kernel / proposal_appearance_kernel / proposal_appearance_finish_kernel: the appearance score; their
//   comments stand with them below.
//
// Every result depends on its own row's data only: it is the same bits alone, in any batch and at any position.
#include "common.hpp"
#include "f32_stage.hpp"
#include "kernels.hpp"

namespace {

constexpr int PC_THREADS = 256;

// ------------------------------------------------------------------ tight boxes and areas
FP_DEVICE void box_take(int idx, int W, int& x1, int& y1, int& x2, int& y2, int& cnt) {
  const int y = idx / W, x = idx - y * W;
  x1 = min(x1, x); x2 = max(x2, x);
  y1 = min(y1, y); y2 = max(y2, y);
  ++cnt;
}

__global__ __launch_bounds__(PC_THREADS) void mask_boxes_kernel(MaskBoxArgs a) {
  __shared__ int part[PC_THREADS / 64][5];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = a.H * a.W;  // <= 2^30: checked by the launcher
  const unsigned char* __restrict__ m = a.masks + (size_t)p * n;
  int x1 = INT32_MAX, y1 = INT32_MAX, x2 = -1, y2 = -1, cnt = 0;
  const int nvec = ((reinterpret_cast<size_t>(m) & 15) == 0) ? n >> 4 : 0;  // block-uniform
  const uint4* __restrict__ mv = reinterpret_cast<const uint4*>(m);
  for (int v = tid; v < nvec; v += PC_THREADS) {
    const uint4 q = mv[v];
    if ((q.x | q.y | q.z | q.w) == 0u) continue;
    const unsigned wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (wd[k] == 0u) continue;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if ((wd[k] >> (8 * b)) & 0xffu) box_take(v * 16 + k * 4 + b, a.W, x1, y1, x2, y2, cnt);
    }
  }
  for (int i = nvec * 16 + tid; i < n; i += PC_THREADS)
    if (m[i]) box_take(i, a.W, x1, y1, x2, y2, cnt);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x1 = min(x1, __shfl_xor(x1, o, 64));
    y1 = min(y1, __shfl_xor(y1, o, 64));
    x2 = max(x2, __shfl_xor(x2, o, 64));
    y2 = max(y2, __shfl_xor(y2, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((tid & 63) == 0) {
    int* s = part[tid >> 6];
    s[0] = x1; s[1] = y1; s[2] = x2; s[3] = y2; s[4] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PC_THREADS / 64; ++w) {
      x1 = min(x1, part[w][0]); y1 = min(y1, part[w][1]);
      x2 = max(x2, part[w][2]); y2 = max(y2, part[w][3]);
      cnt += part[w][4];
    }
    int* o = a.box + (size_t)p * 4;
    if (cnt == 0) { o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0; }
    else { o[0] = x1; o[1] = y1; o[2] = x2 + 1; o[3] = y2 + 1; }
    a.area[p] = cnt;
  }
}

// ------------------------------------------------------------------ masked, aspect-preserving, antialiased crops
// One axis of the resample, n_in -> n_out (all fp64; see the header comment).
struct AxisMap { double scale, sup; };
FP_DEVICE AxisMap axis_map(int n_in, int n_out) {
  AxisMap m;
  m.scale = (double)n_in / (double)n_out;
  m.sup = fmax(m.scale, 1.0);
  return m;
}
FP_DEVICE double axis_centre(const AxisMap& m, int i) { return m.scale * ((double)i + 0.5); }
FP_DEVICE void axis_taps(const AxisMap& m, double c, int n_in, int& lo, int& hi) {
  lo = max(0, (int)(c - m.sup + 0.5));
  hi = min(n_in, (int)(c + m.sup + 0.5));
}
FP_DEVICE double axis_raw(const AxisMap& m, double c, int j) {
#pragma clang fp contract(off)
  return fmax(0.0, 1.0 - fabs(((double)j - c + 0.5) / m.sup));
}
// 1 / (the sum of the raw weights, j ascending)
FP_DEVICE double axis_inv_norm(const AxisMap& m, double c, int lo, int hi) {
  double n = 0.0;
  for (int j = lo; j < hi; ++j) n += axis_raw(m, c, j);
  return 1.0 / n;
}

struct AxisEntry { double inv_norm; int lo, hi; };  // of one output index

__global__ __launch_bounds__(PC_THREADS) void proposal_crops_kernel(ProposalCropArgs a) {
  extern __shared__ __attribute__((aligned(16))) char pc_smem[];
  const int p = blockIdx.y, band = blockIdx.x, tid = threadIdx.x;
  const int S = a.S;
  AxisEntry* __restrict__ xtab = reinterpret_cast<AxisEntry*>(pc_smem);       // [S] (w' used)
  AxisEntry* __restrict__ ytab = xtab + S;                                     // [band_rows]
  float* __restrict__ acc = reinterpret_cast<float*>(ytab + a.band_rows);      // [band_rows][S][3] (w' columns used)
  float* __restrict__ hbuf = acc + (size_t)a.band_rows * S * 3;                // [chunk_rows][S][3]

  const int row0 = band * a.band_rows, row1 = min(S, row0 + a.band_rows);  // output rows of this workgroup
  const size_t plane = (size_t)S * S;
  float* __restrict__ out = a.out + (size_t)p * 3 * plane;

  // ---- the proposal's geometry (block-uniform)
  const int bx1 = a.boxes[(size_t)p * 4 + 0], by1 = a.boxes[(size_t)p * 4 + 1], bx2 = a.boxes[(size_t)p * 4 + 2], by2 = a.boxes[(size_t)p * 4 + 3];
  const int img = a.image_index ? a.image_index[p] : p;
  const bool ok = img >= 0 && img < a.n_img && bx1 >= 0 && by1 >= 0 && bx2 <= a.W && by2 <= a.H && bx2 > bx1 && by2 > by1;
  if (band == 0 && tid == 0) a.status[p] = ok ? 0 : 2;
  const int w = ok ? bx2 - bx1 : 1, h = ok ? by2 - by1 : 1, L = max(w, h);
  const int wo = max(1, (int)((2ll * w * S + L) / (2ll * L))), ho = max(1, (int)((2ll * h * S + L) / (2ll * L)));  // <= S
  const int ox = (S - wo) / 2, oy = (S - ho) / 2;
  const int i0 = max(row0 - oy, 0), i1 = min(row1 - oy, ho);  // window rows of this band: [i0, i1)
  if (!ok || i0 >= i1) {  // block-uniform: nothing of the window here
    for (int e = tid; e < 3 * (row1 - row0) * S; e += PC_THREADS) {
      const int c = e / ((row1 - row0) * S), r = e - c * (row1 - row0) * S;
      out[c * plane + (size_t)row0 * S + r] = 0.f;
    }
    return;
  }
  const AxisMap mx = axis_map(w, wo), my = axis_map(h, ho);
  for (int x = tid; x < wo; x += PC_THREADS) {
    const double c = axis_centre(mx, x);
    AxisEntry e;
    axis_taps(mx, c, w, e.lo, e.hi);
    e.inv_norm = axis_inv_norm(mx, c, e.lo, e.hi);
    xtab[x] = e;
  }
  for (int i = i0 + tid; i < i1; i += PC_THREADS) {
    const double c = axis_centre(my, i);
    AxisEntry e;
    axis_taps(my, c, h, e.lo, e.hi);
    e.inv_norm = axis_inv_norm(my, c, e.lo, e.hi);
    ytab[i - i0] = e;
  }
  const int n_items = (i1 - i0) * wo;  // (window row, x) of this band; item e belongs to thread e % 256 throughout
  for (int e = tid; e < n_items * 3; e += PC_THREADS) acc[e] = 0.f;
  __syncthreads();
  const int src0 = ytab[0].lo, src1 = ytab[i1 - i0 - 1].hi;  // lo and hi do not decrease with i: the band's source rows [src0, src1)

  const float* __restrict__ image = a.images + (size_t)img * a.H * a.W * 3;
  const unsigned char* __restrict__ mask = a.masks + (size_t)p * a.H * a.W;
  for (int r0 = src0; r0 < src1; r0 += a.chunk_rows) {  // block-uniform trip count
    const int nr = min(a.chunk_rows, src1 - r0);
    // ---- horizontal pass of source rows [r0, r0 + nr) of the box
    for (int e = tid; e < nr * wo; e += PC_THREADS) {
      const int r = e / wo, x = e - r * wo;
      const AxisEntry t = xtab[x];
      const double c = axis_centre(mx, x);
      const size_t rowpix = (size_t)(by1 + r0 + r) * a.W + bx1;
      const float* __restrict__ px = image + rowpix * 3;
      const unsigned char* __restrict__ pm = mask + rowpix;
      float u0 = 0.f, u1 = 0.f, u2 = 0.f;
      for (int j = t.lo; j < t.hi; ++j) {
        const float wj = (float)(axis_raw(mx, c, j) * t.inv_norm);
        const bool on = pm[j] != 0;
        u0 = fmaf(wj, on ? px[3 * j + 0] : 0.f, u0);
        u1 = fmaf(wj, on ? px[3 * j + 1] : 0.f, u1);
        u2 = fmaf(wj, on ? px[3 * j + 2] : 0.f, u2);
      }
      hbuf[e * 3 + 0] = u0; hbuf[e * 3 + 1] = u1; hbuf[e * 3 + 2] = u2;
    }
    __syncthreads();
    // ---- vertical pass: what these rows add to the band
    for (int e = tid; e < n_items; e += PC_THREADS) {
      const int i = e / wo, x = e - i * wo;
      const AxisEntry t = ytab[i];
      const int jb = max(t.lo, r0), je = min(t.hi, r0 + nr);
      if (jb >= je) continue;
      const double c = axis_centre(my, i0 + i);
      float v0 = acc[e * 3 + 0], v1 = acc[e * 3 + 1], v2 = acc[e * 3 + 2];
      for (int j = jb; j < je; ++j) {
        const float wj = (float)(axis_raw(my, c, j) * t.inv_norm);
        const float* u = hbuf + ((j - r0) * wo + x) * 3;
        v0 = fmaf(wj, u[0], v0);
        v1 = fmaf(wj, u[1], v1);
        v2 = fmaf(wj, u[2], v2);
      }
      acc[e * 3 + 0] = v0; acc[e * 3 + 1] = v1; acc[e * 3 + 2] = v2;
    }
    __syncthreads();  // hbuf has no readers left
  }

  // ---- store: consecutive lanes on consecutive x of one channel plane (acc items are read by other threads: behind the loop's last barrier)
  const int nrow = row1 - row0;
  for (int e = tid; e < 3 * nrow * S; e += PC_THREADS) {
    const int c = e / (nrow * S), r = e - c * nrow * S;
    const int y = row0 + r / S, x = r % S;
    const int i = y - oy - i0, xx = x - ox;
    float v = 0.f;
    if (i >= 0 && i < i1 - i0 && xx >= 0 && xx < wo) v = acc[(i * wo + xx) * 3 + c];
    out[c * plane + (size_t)y * S + x] = v;
  }
}

// ------------------------------------------------------------------ per-object scores and the label
// The P descriptors listed once per object: rep [O, P, D]; seg_off [O + 1] = o P; tpl_off [O + 1] = obj_off clamped into [0, N] and made
// non-decreasing, an object clamped to max_templates rows; det_nt [O P] = the object's template count.
__global__ __launch_bounds__(PC_THREADS) void proposal_prep_kernel(ProposalScoreArgs a) {
  const long long per = (long long)a.P * a.D;  // blockIdx.y: the object whose copy this workgroup writes
  for (long long e = (long long)blockIdx.x * PC_THREADS + threadIdx.x; e < per; e += (long long)gridDim.x * PC_THREADS)
    a.rep[(long long)blockIdx.y * per + e] = a.desc_n[e];
  if (blockIdx.y != 0) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // O is small: one thread walks it, so that the offsets never decrease
    int prev = min(max(a.obj_off[0], 0), a.N);
    a.tpl_off[0] = prev;
    for (int o = 0; o < a.O; ++o) {
      const int e = min(min(max(a.obj_off[o + 1], prev), a.N), prev + a.max_templates);
      a.tpl_off[o + 1] = e;
      prev = e;
    }
  }
  for (int o = blockIdx.x * PC_THREADS + threadIdx.x; o <= a.O; o += gridDim.x * PC_THREADS) a.seg_off[o] = o * a.P;
}

__global__ __launch_bounds__(PC_THREADS) void proposal_count_kernel(ProposalScoreArgs a) {
  const int e = blockIdx.x * PC_THREADS + threadIdx.x;
  if (e >= a.O * a.P) return;
  const int o = e / a.P;
  a.det_nt[e] = a.tpl_off[o + 1] - a.tpl_off[o];
}

__global__ __launch_bounds__(PC_THREADS) void proposal_aggregate_kernel(ProposalScoreArgs a) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * PC_THREADS + threadIdx.x;
  if (p >= a.P) return;
  int best_obj = -1, best_tpl = -1;
  float best = -INFINITY;
  for (int o = 0; o < a.O; ++o) {
    const int m = min(a.k, a.tpl_off[o + 1] - a.tpl_off[o]);
    const size_t row = ((size_t)o * a.P + p) * a.k;
    float s = -INFINITY;
    if (m > 0) {
      s = a.top_val[row];
      for (int j = 1; j < m; ++j) s = s + a.top_val[row + j];
      s = s / (float)m;
    }
    a.scores[(size_t)p * a.O + o] = s;
    if (s > best) {  // false for a NaN, for -inf and at equality: ties stay with the lower object
      best = s;
      best_obj = o;
      best_tpl = a.top_idx[row];
    }
  }
  a.best_obj[p] = best_obj;
  a.best_score[p] = best;
  a.best_template[p] = best_tpl;
}

// ------------------------------------------------------------------ decisions, rank layout and the pairs of every group
FP_DEVICE int rank_decision(const ProposalRankArgs& a, int p) {
  if (a.area[p] < a.min_area) return PR_SMALL;
  if (a.crop_status[p] != 0) return PR_EMPTY;
  const int o = a.best_obj[p];
  if (o < 0 || o >= a.O) return PR_NO_OBJECT;
  if (!(a.best_score[p] >= a.min_score)) return PR_LOW_SCORE;  // a NaN ends here
  return PR_CANDIDATE;
}

__global__ __launch_bounds__(PC_THREADS) void proposal_rank_kernel(ProposalRankArgs a) {
  __shared__ int rank[PR_MAX_PROPOSALS];  // -1: no candidate
  const int tid = threadIdx.x;
  // ---- the decision and, for a candidate, its rank in its object: the candidates of the object that come before it
  for (int p = tid; p < a.P; p += PC_THREADS) {
    int d = rank_decision(a, p), r = -1;
    if (d == PR_CANDIDATE) {
      const int o = a.best_obj[p];
      const float s = a.best_score[p];
      r = 0;
      for (int q = 0; q < a.P; ++q) {
        if (q == p || a.best_obj[q] != o || rank_decision(a, q) != PR_CANDIDATE) continue;
        const float t = a.best_score[q];
        r += (t > s || (t == s && q < p)) ? 1 : 0;
      }
      if (r >= a.max_group) { d = PR_GROUP_LIMIT; r = -1; }
    }
    a.decision[p] = d;
    rank[p] = r;
    a.order[p] = -1;
    a.boxes_ranked[(size_t)p * 4 + 0] = 0; a.boxes_ranked[(size_t)p * 4 + 1] = 0;
    a.boxes_ranked[(size_t)p * 4 + 2] = 0; a.boxes_ranked[(size_t)p * 4 + 3] = 0;
  }
  __syncthreads();
  // ---- the size of every group (the ranks below max_group), then both offset tables by one thread (O is small)
  for (int o = tid; o < a.O; o += PC_THREADS) {
    int n = 0;
    for (int q = 0; q < a.P; ++q) n += (rank[q] >= 0 && a.best_obj[q] == o) ? 1 : 0;
    a.group_off[o + 1] = n;
  }
  __syncthreads();
  if (tid == 0) {
    int g = 0, pr = 0;
    a.group_off[0] = 0;
    a.pair_off[0] = 0;
    for (int o = 0; o < a.O; ++o) {
      const int n = a.group_off[o + 1];
      g += n;
      pr += n * (n - 1) / 2;  // at most P * (max_group - 1) / 2 <= max_pairs: checked by the launcher
      a.group_off[o + 1] = g;
      a.pair_off[o + 1] = pr;
    }
  }
  __syncthreads();
  // ---- the layout, its boxes and the pairs (a, b), a < b, of every group: the candidate of rank a writes its own
  for (int p = tid; p < a.P; p += PC_THREADS) {
    const int r = rank[p];
    if (r < 0) continue;
    const int o = a.best_obj[p], g0 = a.group_off[o], n = a.group_off[o + 1] - g0;
    a.order[g0 + r] = p;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.boxes_ranked[(size_t)(g0 + r) * 4 + k] = a.boxes[(size_t)p * 4 + k];
    int* pw = a.pairs + 2 * ((size_t)a.pair_off[o] + (size_t)r * (2 * n - r - 1) / 2);
    for (int b = r + 1; b < n; ++b) {
      *pw++ = g0 + r;
      *pw++ = g0 + b;
    }
  }
  for (int q = a.pair_off[a.O] + tid; q < a.max_pairs; q += PC_THREADS) {  // the unused tail names no box: status 2 downstream
    a.pairs[(size_t)q * 2 + 0] = -1;
    a.pairs[(size_t)q * 2 + 1] = -1;
  }
}

// ------------------------------------------------------------------ box overlaps
__global__ __launch_bounds__(PC_THREADS) void box_iou_kernel(BoxIouArgs a) {
  const int q = blockIdx.x * PC_THREADS + threadIdx.x;
  if (q >= a.n_pairs) return;
  const int i = a.pairs[(size_t)q * 2 + 0], j = a.pairs[(size_t)q * 2 + 1];
  double ov = 0.0;
  int st = 2;
  if (i >= 0 && i < a.n_boxes && j >= 0 && j < a.n_boxes) {
    const int* A = a.boxes + (size_t)i * 4;
    const int* B = a.boxes + (size_t)j * 4;
    const long long ax1 = A[0], ay1 = A[1], ax2 = A[2], ay2 = A[3], bx1 = B[0], by1 = B[1], bx2 = B[2], by2 = B[3];
    const long long area_a = max(ax2 - ax1, 0ll) * max(ay2 - ay1, 0ll), area_b = max(bx2 - bx1, 0ll) * max(by2 - by1, 0ll);
    const long long iw = max(min(ax2, bx2) - max(ax1, bx1), 0ll), ih = max(min(ay2, by2) - max(ay1, by1), 0ll);
    const long long inter = (area_a > 0 && area_b > 0) ? iw * ih : 0ll;  // a box of no area meets nothing
    const long long uni = area_a + area_b - inter;
    if (uni > 0) {
      ov = (double)inter / (double)uni;
      st = 0;
    }
  }
  a.overlap[q] = ov;
  a.status[q] = st;
}

// ------------------------------------------------------------------ which ViT patches of a cut-out belong to the object
// One thread per patch cell.  The geometry is proposal_crops_kernel's; a crop pixel of the window reads the mask byte under its centre.
__global__ __launch_bounds__(PC_THREADS) void patch_cover_kernel(PatchCoverArgs a) {
  const int p = blockIdx.y, g = a.S / a.ps, cell = blockIdx.x * PC_THREADS + threadIdx.x;
  if (cell >= g * g) return;
  const int bx1 = a.boxes[(size_t)p * 4 + 0], by1 = a.boxes[(size_t)p * 4 + 1], bx2 = a.boxes[(size_t)p * 4 + 2], by2 = a.boxes[(size_t)p * 4 + 3];
  const int img = a.image_index ? a.image_index[p] : p;
  const bool ok = img >= 0 && img < a.n_img && bx1 >= 0 && by1 >= 0 && bx2 <= a.W && by2 <= a.H && bx2 > bx1 && by2 > by1;
  int n = 0;
  if (ok) {
    const int S = a.S, w = bx2 - bx1, h = by2 - by1, L = max(w, h);
    const int wo = max(1, (int)((2ll * w * S + L) / (2ll * L))), ho = max(1, (int)((2ll * h * S + L) / (2ll * L)));  // <= S
    const int ox = (S - wo) / 2, oy = (S - ho) / 2;
    const int cy = cell / g, cx = cell - cy * g;
    const int X0 = max(cx * a.ps, ox), X1 = min(cx * a.ps + a.ps, ox + wo), Y0 = max(cy * a.ps, oy), Y1 = min(cy * a.ps + a.ps, oy + ho);
    const unsigned char* __restrict__ mask = a.masks + (size_t)p * a.H * a.W;
    for (int Y = Y0; Y < Y1; ++Y) {
      const int sy = by1 + (int)(((2ll * (Y - oy) + 1) * h) / (2ll * ho));  // < by2: 2 (Y - oy) + 1 < 2 h'
      const unsigned char* __restrict__ mrow = mask + (size_t)sy * a.W;
      for (int X = X0; X < X1; ++X) {
        const int sx = bx1 + (int)(((2ll * (X - ox) + 1) * w) / (2ll * wo));  // < bx2
        n += mrow[sx] != 0 ? 1 : 0;
      }
    }
  }
  a.cover[(size_t)p * g * g + cell] = n;
}

// ------------------------------------------------------------------ the appearance score
// proposal_appearance_kernel: one 256-thread workgroup per (proposal, 128 query patches).  It walks the patches of the proposal's best
//   template in 128-column tiles with f32_tile.hip's staging (f32_stage.hpp: 128 x 32 of each operand through registers into a k-major
//   LDS image, [k][row], stride 129 dwords; two stages) and its instruction, v_mfma_f32_32x32x2_f32 with k ascending: one accumulator per
//   (query patch, template patch), so a similarity is the chain acc = fmaf(q[k], t[k], acc).  Wave w owns query rows 32 w .. 32 w + 31 and
//   the tile's four 32-column blocks.  Behind the last k step of a column tile every lane folds its 16 rows x 4 columns into a running
//   (value, column) pair per row over the VALID columns -- columns arrive ascending in a lane, so the strict ">" keeps the lower one -- and
//   behind the last tile a butterfly over the 32 lanes of a row merges the pairs (greater value, then lower column).  Rows past Np and
//   columns past Np are zero-filled from clamped addresses inside the proposal's / the template's own rows: a ragged tile never touches a
//   neighbour.  proposal_appearance_finish_kernel: one thread per proposal adds the valid rows' values in ascending order.
constexpr int PA_BM = f32_stage::BM, PA_BN = f32_stage::BN, PA_BK = f32_stage::BK, PA_LDS = f32_stage::LDS_STRIDE, PA_STAGE = f32_stage::STAGE_FLOATS;

// The bank row of proposal p's best template, or -1 (status 2); obj_off is clamped into [0, N] and made non-decreasing on the way.
FP_DEVICE int appearance_row(const ProposalAppearanceArgs& a, int p) {
  const int o = a.best_obj[p], t = a.best_template[p];
  if (o < 0 || o >= a.O || t < 0) return -1;
  int prev = min(max(a.obj_off[0], 0), a.N);
  for (int i = 0; i < o; ++i) prev = min(max(a.obj_off[i + 1], prev), a.N);
  const int end = min(max(a.obj_off[o + 1], prev), a.N);
  return t < end - prev ? prev + t : -1;  // prev + t < end <= N
}

__global__ __launch_bounds__(256) void proposal_appearance_kernel(ProposalAppearanceArgs a) {
  extern __shared__ __attribute__((aligned(16))) float pa_smem[];
  float* As = pa_smem;                 // [2][PA_BK][129]
  float* Bs = pa_smem + 2 * PA_STAGE;  // [2][PA_BK][129]
  const int p = blockIdx.y, m0 = blockIdx.x * PA_BM, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Np = a.Np, D = a.D;
  const int live_m = Np - m0 < PA_BM ? Np - m0 : PA_BM;  // >= 1: the grid has cdiv(Np, 128) tiles
  const int row = appearance_row(a, p);                  // block-uniform
  float* __restrict__ out_sim = a.best_sim + (size_t)p * Np + m0;
  int* __restrict__ out_patch = a.best_patch + (size_t)p * Np + m0;
  const int* __restrict__ qc = a.q_cover + (size_t)p * Np + m0;
  const int* __restrict__ bc = a.bank_cover + (size_t)(row < 0 ? 0 : row) * Np;

  // nothing to score here: no template row, a template of no valid patch, or no valid query patch in this tile
  int tv = 0, qv = 0;
  if (row >= 0) {
    for (int i = tid; i < Np; i += 256) tv |= bc[i] >= a.min_cover ? 1 : 0;
    if (tid < live_m) qv = qc[tid] >= a.min_cover ? 1 : 0;
  }
  const int any_t = __syncthreads_or(tv), any_q = __syncthreads_or(qv);
  if (row < 0 || !any_t || !any_q) {
    for (int i = tid; i < live_m; i += 256) {
      out_sim[i] = 0.f;
      out_patch[i] = -1;
    }
    return;
  }

  const float* __restrict__ Ab = a.q + (size_t)p * Np * D;
  const float* __restrict__ Bb = a.bank + (size_t)row * Np * D;
  const int nk = (D + PA_BK - 1) / PA_BK, steps = ((Np + PA_BN - 1) / PA_BN) * nk;
  const int kh = lane >> 5, l31 = lane & 31, rb = wave * 32;
  const bool wlive = rb < live_m;  // wave-uniform: a wave of no live row only stages

  float bv[16];
  int bi[16];
  f32x16 acc[4];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    bv[r] = -INFINITY;
    bi[r] = -1;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  f32_stage::Frag fa, fb;
  f32_stage::load_tile(fa, Ab, D, m0, Np, 0, D, tid);
  f32_stage::load_tile(fb, Bb, D, 0, Np, 0, D, tid);
  f32_stage::store_tile(fa, As, tid);
  f32_stage::store_tile(fb, Bs, tid);
  __syncthreads();

  for (int s = 0; s < steps; ++s) {  // (column tile, k step), k fastest
    const int cur = s & 1, t = s / nk, kt = s - t * nk, n0 = t * PA_BN;
    if (s + 1 < steps) {
      const int t1 = (s + 1) / nk, k1 = (s + 1) - t1 * nk;
      f32_stage::load_tile(fa, Ab, D, m0, Np, k1 * PA_BK, D, tid);
      f32_stage::load_tile(fb, Bb, D, t1 * PA_BN, Np, k1 * PA_BK, D, tid);
    }
    const int ncb = Np - n0 >= PA_BN ? 4 : (Np - n0 + 31) / 32;  // 32-column blocks of this tile with a live column (block-uniform)
    if (wlive) {
      const float* as0 = As + cur * PA_STAGE + rb + l31 + kh * PA_LDS;
      const float* bs0 = Bs + cur * PA_STAGE + l31 + kh * PA_LDS;
#pragma unroll
      for (int kk = 0; kk < PA_BK / 2; ++kk) {
        const int krow = kk * 2 * PA_LDS;
        const float a0 = as0[krow];
        const float b0 = bs0[krow], b1 = bs0[krow + 32], b2 = bs0[krow + 64], b3 = bs0[krow + 96];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0], 0, 0, 0);
        if (ncb > 1) acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[1], 0, 0, 0);
        if (ncb > 2) acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b2, acc[2], 0, 0, 0);
        if (ncb > 3) acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b3, acc[3], 0, 0, 0);
      }
      if (kt == nk - 1) {
        // acc[c][r] is sim(i, j) with i = m0 + rb + (r & 3) + 8 (r >> 2) + 4 kh, j = n0 + 32 c + l31
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = n0 + c * 32 + l31;
          const bool valid = j < Np && bc[j < Np ? j : Np - 1] >= a.min_cover;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float v = acc[c][r];
            const bool take = valid && v > bv[r];  // false for a NaN and at equality
            bv[r] = take ? v : bv[r];
            bi[r] = take ? j : bi[r];
            acc[c][r] = 0.f;
          }
        }
      }
    }
    if (s + 1 < steps) {
      f32_stage::store_tile(fa, As + (cur ^ 1) * PA_STAGE, tid);
      f32_stage::store_tile(fb, Bs + (cur ^ 1) * PA_STAGE, tid);
    }
    __syncthreads();
  }
  if (!wlive) return;

  // a row's 32 lanes hold its candidates: the greater value wins, the lower column among equal values (-1, as unsigned, never does)
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float ov = __shfl_xor(bv[r], o, 64);
      const int oi = __shfl_xor(bi[r], o, 64);
      const bool take = ov > bv[r] || (ov == bv[r] && (unsigned)oi < (unsigned)bi[r]);
      bv[r] = take ? ov : bv[r];
      bi[r] = take ? oi : bi[r];
    }
  }
  if (l31 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = rb + (r & 3) + 8 * (r >> 2) + 4 * kh;
      if (i >= live_m) continue;
      const bool valid = qc[i] >= a.min_cover;
      out_sim[i] = valid ? bv[r] : 0.f;
      out_patch[i] = valid ? bi[r] : -1;
    }
  }
}

__global__ __launch_bounds__(PC_THREADS) void proposal_appearance_finish_kernel(ProposalAppearanceArgs a) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * PC_THREADS + threadIdx.x;
  if (p >= a.P) return;
  const int row = appearance_row(a, p);
  int nv = 0, st = 2;
  float app = 0.f;
  if (row >= 0) {
    const int* __restrict__ qc = a.q_cover + (size_t)p * a.Np;
    const int* __restrict__ bc = a.bank_cover + (size_t)row * a.Np;
    bool tv = false;
    for (int j = 0; j < a.Np; ++j) nv += qc[j] >= a.min_cover ? 1 : 0;
    for (int i = 0; i < a.Np; ++i) tv = tv || bc[i] >= a.min_cover;
    st = nv == 0 ? 1 : (tv ? 0 : 3);
    if (st == 0) {
      const float* __restrict__ bs = a.best_sim + (size_t)p * a.Np;
      float s = 0.f;
      bool first = true;
      for (int j = 0; j < a.Np; ++j) {
        if (qc[j] < a.min_cover) continue;
        s = first ? bs[j] : s + bs[j];
        first = false;
      }
      app = s / (float)nv;
    }
  }
  a.appearance[p] = app;
  a.n_valid[p] = nv;
  a.status[p] = st;
  a.score[p] = (a.best_score[p] + app) * 0.5f;
}

}  // namespace

int launch_proposal_patch_cover(const PatchCoverArgs& a, int num_prop, hipStream_t st) {
  FP_REQUIRE(num_prop >= 0 && num_prop <= 65535, "proposal_patch_cover: %d proposals (0 .. 65535 per call)", num_prop);
  FP_REQUIRE(a.S >= 1 && a.S <= PC_MAX_SIZE, "proposal_patch_cover: crop size %d outside [1, %d]", a.S, PC_MAX_SIZE);
  FP_REQUIRE(a.ps >= 1 && a.S % a.ps == 0, "proposal_patch_cover: the crop size %d is no multiple of the patch size %d", a.S, a.ps);
  FP_REQUIRE(a.n_img >= 1 && a.H >= 1 && a.W >= 1 && (long long)a.H * a.W <= (1ll << 30),
             "proposal_patch_cover: %d images of %d x %d (H, W >= 1, H W at most 2^30)", a.n_img, a.W, a.H);
  if (num_prop == 0) return FP_OK;
  const int g = a.S / a.ps;
  hipLaunchKernelGGL(patch_cover_kernel, dim3(cdiv(g * g, PC_THREADS), num_prop), dim3(PC_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("proposal_patch_cover");
  return FP_OK;
}

int launch_proposal_appearance(const ProposalAppearanceArgs& a, hipStream_t st) {
  FP_REQUIRE(a.P >= 0 && a.P <= 65535, "proposal_appearance: %d proposals (0 .. 65535 per call)", a.P);
  FP_REQUIRE(a.D >= 4 && a.D % 4 == 0 && a.D <= PA_MAX_DIM, "proposal_appearance: %d words (a multiple of 4, at most %d)", a.D, PA_MAX_DIM);
  FP_REQUIRE(a.Np >= 1 && a.Np <= PA_MAX_PATCHES, "proposal_appearance: %d patches outside [1, %d]", a.Np, PA_MAX_PATCHES);
  FP_REQUIRE(a.N >= 0 && a.O >= 1 && a.min_cover >= 1, "proposal_appearance: %d bank rows, %d objects, min_cover %d (N >= 0, O >= 1, min_cover >= 1)",
             a.N, a.O, a.min_cover);
  if (a.P == 0) return FP_OK;
  const size_t lds = 4 * PA_STAGE * sizeof(float);  // two double-buffered operand stages
  static FpDeviceOnce attr;
  fp_allow_dynamic_lds(attr, &proposal_appearance_kernel, (int)lds);
  hipLaunchKernelGGL(proposal_appearance_kernel, dim3(cdiv(a.Np, PA_BM), a.P), dim3(256), lds, st, a);
  FP_CHECK_LAUNCH("proposal_appearance (tiles)");
  hipLaunchKernelGGL(proposal_appearance_finish_kernel, dim3(cdiv(a.P, PC_THREADS)), dim3(PC_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("proposal_appearance (finish)");
  return FP_OK;
}

int launch_mask_boxes(const MaskBoxArgs& a, int num_prop, hipStream_t st) {
  FP_REQUIRE(num_prop >= 0 && a.H >= 1 && a.W >= 1 && (long long)a.H * a.W <= (1ll << 30),
             "mask_boxes: %d masks of %d x %d (H, W >= 1, H W at most 2^30: the pixel index is an int)", num_prop, a.W, a.H);
  if (num_prop == 0) return FP_OK;
  hipLaunchKernelGGL(mask_boxes_kernel, dim3(num_prop), dim3(PC_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("mask_boxes");
  return FP_OK;
}

// LDS of a crop workgroup: the axis tables, the band's accumulators and one chunk of horizontally resampled rows, below 64 KiB
// (S <= 1024: 16 S + 16 band + 12 S (band + chunk) bytes with band + chunk = 3840 / S rows, at least 3)
int launch_proposal_crops(ProposalCropArgs a, int num_prop, hipStream_t st) {
  FP_REQUIRE(num_prop >= 0 && num_prop <= 65535, "proposal_crops: %d proposals (0 .. 65535 per call)", num_prop);
  FP_REQUIRE(a.S >= 1 && a.S <= PC_MAX_SIZE, "proposal_crops: crop size %d outside [1, %d]", a.S, PC_MAX_SIZE);
  FP_REQUIRE(a.n_img >= 1 && a.H >= 1 && a.W >= 1 && (long long)a.H * a.W <= (1ll << 30),
             "proposal_crops: %d images of %d x %d (H, W >= 1, H W at most 2^30)", a.n_img, a.W, a.H);
  if (num_prop == 0) return FP_OK;
  const int rows = 3840 / a.S;  // >= 3
  a.band_rows = rows / 3 < 1 ? 1 : (rows / 3 > 8 ? 8 : rows / 3);
  a.band_rows = a.band_rows > a.S ? a.S : a.band_rows;
  a.chunk_rows = rows - a.band_rows > 16 ? 16 : rows - a.band_rows;
  const size_t lds = 16 * (size_t)a.S + 16 * (size_t)a.band_rows + 12 * (size_t)a.S * (a.band_rows + a.chunk_rows);
  hipLaunchKernelGGL(proposal_crops_kernel, dim3(cdiv(a.S, a.band_rows), num_prop), dim3(PC_THREADS), lds, st, a);
  FP_CHECK_LAUNCH("proposal_crops");
  return FP_OK;
}

int launch_proposal_prep(const ProposalScoreArgs& a, hipStream_t st) {
  const long long want = ((long long)a.P * a.D + PC_THREADS - 1) / PC_THREADS;
  const int blocks = want > 1024 ? 1024 : (int)want;
  hipLaunchKernelGGL(proposal_prep_kernel, dim3(blocks, a.O), dim3(PC_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("proposal_scores (list)");
  hipLaunchKernelGGL(proposal_count_kernel, dim3(cdiv(a.O * a.P, PC_THREADS)), dim3(PC_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("proposal_scores (counts)");
  return FP_OK;
}

int launch_proposal_aggregate(const ProposalScoreArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(proposal_aggregate_kernel, dim3(cdiv(a.P, PC_THREADS)), dim3(PC_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("proposal_scores (aggregate)");
  return FP_OK;
}

int launch_proposal_rank(const ProposalRankArgs& a, hipStream_t st) {
  FP_REQUIRE(a.P >= 0 && a.P <= PR_MAX_PROPOSALS, "proposal_rank: %d proposals (at most %d of one image)", a.P, PR_MAX_PROPOSALS);
  FP_REQUIRE(a.O >= 1 && a.O <= PR_MAX_OBJECTS, "proposal_rank: %d objects outside [1, %d]", a.O, PR_MAX_OBJECTS);
  FP_REQUIRE(a.max_group >= 1 && a.max_group <= PN_MAX_GROUP, "proposal_rank: max_group %d outside [1, %d]", a.max_group, PN_MAX_GROUP);
  FP_REQUIRE(a.min_score == a.min_score, "proposal_rank: the score threshold is NaN");
  FP_REQUIRE((long long)a.max_pairs >= (long long)a.P * (a.max_group - 1) / 2, "proposal_rank: room for %d pairs, %lld may be written", a.max_pairs,
             (long long)a.P * (a.max_group - 1) / 2);
  hipLaunchKernelGGL(proposal_rank_kernel, dim3(1), dim3(PC_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("proposal_rank");
  return FP_OK;
}

int launch_box_iou(const BoxIouArgs& a, hipStream_t st) {
  FP_REQUIRE(a.n_boxes >= 0 && a.n_pairs >= 0, "box_iou: negative count");
  if (a.n_pairs == 0) return FP_OK;
  hipLaunchKernelGGL(box_iou_kernel, dim3(cdiv(a.n_pairs, PC_THREADS)), dim3(PC_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("box_iou");
  return FP_OK;
}
