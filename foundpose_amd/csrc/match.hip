// Descriptor-matching kernels that are not GEMM-shaped (HBM/latency-bound integer + fp32 work):
// row norms, tf-idf histogram, cyclic best-buddy selection, bilinear sampling, the merge of the fused k-NN's per-tile
// candidates, key unpacking and the packing of the result records.  (Template retrieval lives in retrieve.hip.)
//
// Reference behaviour restated (paths in the reference project):
//   knn_merge ........ faiss heap result order (utils/knn_util.py:83): smallest distance first, ties -> lowest index
//   tfidf_build ...... utils/template_util.py:31-71 (weights, L2-normalise per query, tf = w/Q,
//                      scatter_add_ in flattened order) + the query side of cosine_similarity (:167)
//   cyclic_select .... utils/corresp_util.py:49-70,135-155
//   sample_bilinear .. utils/feature_util.py:100-131 (grid_sample bilinear, zeros, align_corners=False)
#include "common.hpp"
#include "kernels.hpp"
#include "select.hpp"
#include "stl_order.hpp"
#include "stl_wave.hpp"

namespace {

// ------------------------------------------------------------------ |x|^2 per row, k-ascending fmaf chain
__global__ void sqnorm_rows_kernel(const float* __restrict__ x, long long n, int d, int ld, float* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4* r = reinterpret_cast<const float4*>(x + i * ld);
  float acc = 0.f;
  for (int k = 0; k < d / 4; ++k) {
    float4 v = r[k];
    acc = fmaf(v.x, v.x, acc);
    acc = fmaf(v.y, v.y, acc);
    acc = fmaf(v.z, v.z, acc);
    acc = fmaf(v.w, v.w, acc);
  }
  out[i] = acc;
}

// x / max(sqrt(|x|^2), eps) per row (bank-side cosine normalisation; |x|^2 as above)
__global__ void normalize_rows_kernel(const float* __restrict__ x, long long n, int d, float eps, float* __restrict__ out) {
  // one wave per row; lane 0 computes the chain so the order matches the oracle
  long long row = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const float* r = x + row * d;
  float acc = 0.f;
  if (lane == 0)
    for (int k = 0; k < d; ++k) acc = fmaf(r[k], r[k], acc);
  acc = __shfl(acc, 0, 64);
  const float nrm = fmaxf(sqrtf(acc), eps);
  for (int k = lane; k < d; k += 64) out[row * d + k] = r[k] / nrm;
}

// ------------------------------------------------------------------ tf-idf descriptor per detection
// One block (256 threads) per segment (a detection's query patches, or a template's patches on the
// bank-builder side). Thread t owns the bins with (id & 255) == t and walks the (q, j) entries in
// flattened order, so every bin sees its addends in exactly the order scatter_add_ applies them.
__global__ __launch_bounds__(256) void tfidf_build_kernel(
    const int* __restrict__ word_ids, const float* __restrict__ word_d2, int knn_k, const int* __restrict__ seg_off,
    const float* __restrict__ idf, int num_words, int soft, float two_sigma_sq, int sqrt_dists,
    float* __restrict__ desc, float* __restrict__ desc_n, float eps) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* bins = reinterpret_cast<float*>(smem_raw);            // [num_words]
  int* ids = reinterpret_cast<int*>(bins + num_words);         // [chunk]
  float* vals = reinterpret_cast<float*>(ids + 4096);          // [chunk]
  __shared__ float s_nrm;

  const int seg = blockIdx.x, tid = threadIdx.x;
  const int q0 = seg_off[seg], Q = seg_off[seg + 1] - q0;
  const float fQ = (float)Q;
  const int total = Q * knn_k;
  if (!soft) {
    // Hard assignment (the shipped options): every entry of a bin adds the SAME value tf * idf[bin] (weights are all 1, so
    // tf = (1 / sqrt(k)) / Q for every entry), and a run of n equal fp32 addends sums to the same bits in any order.  So the
    // order-sensitive walk below is not needed: count the entries per bin with integer LDS atomics (exact, order-free,
    // all 256 threads busy), then each bin replays its n sequential additions -- bit-identical to scatter_add_, ~10x faster.
    int* cnt = reinterpret_cast<int*>(bins);
    for (int w = tid; w < num_words; w += 256) cnt[w] = 0;
    __syncthreads();
    for (int e = tid; e < total; e += 256) {
      const int id = word_ids[(size_t)q0 * knn_k + e];
      if (id >= 0) atomicAdd(&cnt[id], 1);
    }
    __syncthreads();
    float nrm2 = 0.f;
    for (int t = 0; t < knn_k; ++t) nrm2 = nrm2 + 1.f;  // sequential, like the general path below
    const float tf = (1.f / fmaxf(sqrtf(nrm2), 1e-12f)) / fQ;
    for (int w = tid; w < num_words; w += 256) {
      const int n = cnt[w];
      const float v = tf * idf[w];
      float acc = 0.f;
      for (int i = 0; i < n; ++i) acc += v;
      bins[w] = acc;  // same LDS word, read as int above by this thread only
    }
  } else {
  for (int w = tid; w < num_words; w += 256) bins[w] = 0.f;
  for (int base = 0; base < total; base += 4096) {
    __syncthreads();
    const int cnt = min(4096, total - base);
    // stage (id, tf*idf) for entries [base, base+cnt); entry e -> query e / k, neighbour e % k
    for (int e = tid; e < cnt; e += 256) {
      const int g = base + e;
      const int q = g / knn_k, j = g - q * knn_k;
      const int* idr = word_ids + (size_t)(q0 + q) * knn_k;
      const float* dr = word_d2 + (size_t)(q0 + q) * knn_k;
      float nrm2 = 0.f, wj = 1.f;
      for (int t = 0; t < knn_k; ++t) {
        float x = sqrt_dists ? sqrtf(dr[t]) : dr[t];
        const float w = expf(-(x * x) / two_sigma_sq);
        nrm2 = nrm2 + w * w;  // sequential, like a 3-element fp32 sum
        if (t == j) wj = w;
      }
      const float wn = wj / fmaxf(sqrtf(nrm2), 1e-12f);
      const float tf = wn / fQ;
      const int id = idr[j];  // -1: the k-NN had fewer than knn_k words to offer (padding, like faiss) -> no bin
      ids[e] = id;
      vals[e] = id >= 0 ? tf * idf[id] : 0.f;
    }
    __syncthreads();
    for (int e = 0; e < cnt; ++e) {
      const int id = ids[e];
      if (id >= 0 && (id & 255) == tid) bins[id] += vals[e];
    }
  }
  }
  __syncthreads();
  if (tid == 0) {  // |desc|^2 as ONE k-ascending fmaf chain (the canonical order); bins fetched 16 at a time so only the
    float acc = 0.f;  // fma latency, not an LDS round trip per element, is serial
    int w = 0;
    for (; w + 16 <= num_words; w += 16) {
      float4 b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) b[u] = *reinterpret_cast<const float4*>(bins + w + 4 * u);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc = fmaf(b[u].x, b[u].x, acc); acc = fmaf(b[u].y, b[u].y, acc);
        acc = fmaf(b[u].z, b[u].z, acc); acc = fmaf(b[u].w, b[u].w, acc);
      }
    }
    for (; w < num_words; ++w) acc = fmaf(bins[w], bins[w], acc);
    s_nrm = fmaxf(sqrtf(acc), eps);
  }
  __syncthreads();
  const float nrm = s_nrm;
  for (int w = tid; w < num_words; w += 256) {
    const float v = bins[w];
    desc[(size_t)seg * num_words + w] = v;
    if (desc_n) desc_n[(size_t)seg * num_words + w] = v / nrm;
  }
}

// ------------------------------------------------------------------ cyclic best buddies: select + gather
// |u1 - u2|_2 exactly as separate fp32 mul/add + correctly rounded sqrt (no fma contraction), so the
// heavily tied cycle distances compare bit-for-bit with the CPU.
FP_DEVICE float point_dist(float x1, float y1, float x2, float y2) {
#pragma clang fp contract(off)
  const float dx = x1 - x2, dy = y1 - y2;
  const float xx = dx * dx, yy = dy * dy;
  return sqrtf(xx + yy);
}

__global__ __launch_bounds__(256) void cyclic_select_kernel(CyclicArgs a) {
  __shared__ unsigned long long keys[2048];
  __shared__ int q2o_s[2048];
  __shared__ unsigned short lpos_s[2048], rpos_s[2048];  // strict mode: stopper ranks of the wave-parallel partition
  __shared__ stl_order::Elem tmp_s[2048];                // strict mode: target of the final stable placement
  const int pair = blockIdx.x, tid = threadIdx.x;
  const int det = pair / a.n_slots;
  const int q0 = a.q_off[det], Q = a.q_off[det + 1] - q0;
  int tpl = a.tpl_ids[pair];
  if (tpl >= 0 && a.tpl_base) tpl += a.tpl_base[det];
  const int kk = min(a.top_k, Q);
  // an empty slot (fewer templates than n_slots) or a template without features yields no correspondences
  const bool live = tpl >= 0 && a.tpl_off[tpl + 1] > a.tpl_off[tpl] && Q > 0;
  if (tid == 0) a.out_count[pair] = live ? kk : 0;
  // the kernel owns the whole padded record: entries past the count are written here (-1 ids, zeros), so the caller hands
  // over uninitialised buffers (seven fill kernels per batch otherwise)
  for (int r = (live ? kk : 0) + tid; r < a.k_max; r += 256) {
    const size_t o = (size_t)pair * a.k_max + r;
    a.out_q_ids[o] = -1;
    a.out_feat_ids[o] = -1;
    a.out_dists[o] = 0.f;
    a.out_conf[o] = 0.f;
    a.out_coord_2d[o * 2] = 0.f; a.out_coord_2d[o * 2 + 1] = 0.f;
    a.out_coord_3d[o * 3] = 0.f; a.out_coord_3d[o * 3 + 1] = 0.f; a.out_coord_3d[o * 3 + 2] = 0.f;
  }
  if (!live) return;
  const int f0 = a.tpl_off[tpl];
  // the distance tiles left one slice of nearest-neighbour keys per tile: the nearest over the whole template / crop is the
  // smallest key over the live tiles (keys order by distance, then index: the same winner an atomicMin would have kept)
  // (row_parts / col_parts == 1: one tile, one finished key per row / column)
  const int np = a.row_parts == 1 ? 1 : (a.tpl_off[tpl + 1] - f0 + 127) / 128, nq = a.col_parts == 1 ? 1 : (Q + 127) / 128;
  const unsigned long long* rb = a.row_best + (size_t)pair * a.row_parts * a.row_stride;
  const unsigned long long* cb = a.col_best + (size_t)pair * a.col_parts * a.col_stride;
  const float* pts = a.points + (size_t)q0 * 2;

  for (int i = tid; i < 2048; i += 256) {
    unsigned long long key = ~0ull;
    if (i < Q) {
      unsigned long long kr = rb[i];
      for (int t = 1; t < np; ++t) {
        const unsigned long long v = rb[(size_t)t * a.row_stride + i];
        kr = v < kr ? v : kr;
      }
      const int o = key_index(kr);                    // query -> nearest template patch
      unsigned long long kc = cb[o];
      for (int t = 1; t < nq; ++t) {
        const unsigned long long v = cb[(size_t)t * a.col_stride + o];
        kc = v < kc ? v : kc;
      }
      const int c = key_index(kc);                    // that patch -> nearest query patch
      q2o_s[i] = o;
      key = pack_dist_idx(point_dist(pts[2 * i], pts[2 * i + 1], pts[2 * c], pts[2 * c + 1]), (unsigned)i);
    }
    keys[i] = key;
  }
  __syncthreads();
  if (a.tie_mode == 1) {
    // strict mode: the reference's torch.topk(-cycle_dists, k) order, ties included -- one wave replays
    // libstdc++'s nth_element + sort (or partial_sort) on (value, index) pairs held in LDS (stl_wave.hpp)
    stl_order::Elem* el = reinterpret_cast<stl_order::Elem*>(keys);
    for (int i = tid; i < Q; i += 256) {
      const unsigned long long key = keys[i];  // each thread converts only the slots it reads itself
      el[i] = stl_order::Elem{-__uint_as_float((unsigned)(key >> 32)), i};
    }
    __syncthreads();
    if (tid < 64) stl_wave::topk_torch_largest(el, Q, kk, lpos_s, rpos_s, tmp_s, tid);
    __syncthreads();
    for (int i = tid; i < kk; i += 256) {  // back to (distance bits, query id) keys in output order
      const stl_order::Elem e = el[i];
      keys[i] = pack_dist_idx(-e.v, (unsigned)e.idx);
    }
    __syncthreads();
  } else {
  // bitonic sort of 2048 keys, ascending: (cycle distance, query index)
  for (int size = 2; size <= 2048; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < 1024; t += 256) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = ((lo & size) == 0);
        unsigned long long x = keys[lo], y = keys[hi];
        if ((x > y) == up) { keys[lo] = y; keys[hi] = x; }
      }
      __syncthreads();
    }
  }
  }
  const float dmax = __uint_as_float((unsigned)(keys[kk - 1] >> 32));
  const size_t ob = (size_t)pair * a.k_max;
  for (int r = tid; r < kk; r += 256) {
    const unsigned long long key = keys[r];
    const int qi = key_index(key);
    const float d = __uint_as_float((unsigned)(key >> 32));
    const int feat = f0 + q2o_s[qi];
    a.out_q_ids[ob + r] = qi;
    a.out_feat_ids[ob + r] = feat - a.feat_base[det];
    a.out_dists[ob + r] = d;
    a.out_conf[ob + r] = 1.0f - d / dmax;
    a.out_coord_2d[(ob + r) * 2 + 0] = pts[2 * qi];
    a.out_coord_2d[(ob + r) * 2 + 1] = pts[2 * qi + 1];
    const float* v = a.vertices + (size_t)feat * 3;
    a.out_coord_3d[(ob + r) * 3 + 0] = v[0];
    a.out_coord_3d[(ob + r) * 3 + 1] = v[1];
    a.out_coord_3d[(ob + r) * 3 + 2] = v[2];
  }
}

// ------------------------------------------------------------------ bilinear sampling of a feature map
// One wave per point. fmap addressed through element strides so both the token-major [Np, D] image the
// extractor produces (a CHW *view*, like the reference's) and a contiguous CHW tensor work.
__global__ void sample_bilinear_kernel(SampleArgs a) {
  const int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (p >= a.num_points) return;
  const int lane = threadIdx.x & 63;
  const int img = a.point_img ? a.point_img[p] : 0;
  const float px = a.points[2 * p], py = a.points[2 * p + 1];
  // uv = (2/size) * p - 1   (fp32, no fma: feature_util.py:119)
  // Rounding sequence of torch's CPU grid_sampler (vectorised kernel, fma-contracted), verified
  // bit-for-bit against torch on the fixtures:  uv = (2/size)*p - 1 (separate mul, sub);
  // ix = fma(u + 1, W/2, -0.5);  w = ix - floor(ix), e = 1 - w;  out = fma chain over nw, ne, sw, se.
  float ix, iy;
  {
#pragma clang fp contract(off)
    const float sx = 2.0f / (float)a.img_w, sy = 2.0f / (float)a.img_h;
    const float ux = sx * px, uy = sy * py;
    const float u1 = (ux - 1.0f) + 1.0f, v1 = (uy - 1.0f) + 1.0f;
    ix = fmaf(u1, (float)a.W / 2.f, -0.5f);
    iy = fmaf(v1, (float)a.H / 2.f, -0.5f);
  }
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
  float w_nw, w_ne, w_sw, w_se;
  {
#pragma clang fp contract(off)
    const float w = ix - fx, e = 1.f - w, n = iy - fy, s_ = 1.f - n;
    w_nw = s_ * e; w_ne = s_ * w; w_sw = n * e; w_se = n * w;
  }
  const bool vx0 = x0 >= 0 && x0 < a.W, vx1 = x1 >= 0 && x1 < a.W, vy0 = y0 >= 0 && y0 < a.H, vy1 = y1 >= 0 && y1 < a.H;
  const float* base = a.fmap + (size_t)img * a.stride_img;
  for (int c = lane; c < a.C; c += 64) {
    const float* bc = base + (size_t)c * a.stride_c;
    const float v_nw = (vx0 && vy0) ? bc[(size_t)y0 * a.stride_h + (size_t)x0 * a.stride_w] : 0.f;
    const float v_ne = (vx1 && vy0) ? bc[(size_t)y0 * a.stride_h + (size_t)x1 * a.stride_w] : 0.f;
    const float v_sw = (vx0 && vy1) ? bc[(size_t)y1 * a.stride_h + (size_t)x0 * a.stride_w] : 0.f;
    const float v_se = (vx1 && vy1) ? bc[(size_t)y1 * a.stride_h + (size_t)x1 * a.stride_w] : 0.f;
    float acc;
    {
#pragma clang fp contract(off)
      acc = v_nw * w_nw;
    }
    acc = fmaf(v_ne, w_ne, acc);
    acc = fmaf(v_sw, w_sw, acc);
    acc = fmaf(v_se, w_se, acc);
    a.out[(size_t)p * a.C + c] = acc;
  }
}

// Finishes the fused k-NN: per row the k best of its ncand = n_tiles * k candidate keys (canonical: smallest (d2, index)).
// 16 lanes per row: per-lane sorted lists over a strided share, then k rounds of 16-lane arg-min + pop.
__global__ __launch_bounds__(256) void knn_merge_kernel(const unsigned long long* __restrict__ cand, int rows, int ncand, int k,
                                                        float* __restrict__ out_d2, int* __restrict__ out_idx) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
  const bool live = row < rows;
  constexpr int KMAX = 8;
  unsigned long long best[KMAX];
#pragma unroll
  for (int s = 0; s < KMAX; ++s) best[s] = ~0ull;
  if (live)
    for (int c = l; c < ncand; c += 16)
      sorted_insert(best, cand[(size_t)row * ncand + c]);
  for (int s = 0; s < k; ++s) {
    const unsigned long long m = min16_u64(best[0]);
    if (m != ~0ull && best[0] == m) pop_front(best);
    if (live && l == 0) {
      out_idx[(size_t)row * k + s] = m == ~0ull ? -1 : key_index(m);
      out_d2[(size_t)row * k + s] = m == ~0ull ? INFINITY : __uint_as_float((unsigned)(m >> 32));
    }
  }
}

__global__ void unpack_best_kernel(const unsigned long long* __restrict__ best, long long n, float* __restrict__ d2, int* __restrict__ idx) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long b = best[i];
  if (d2) d2[i] = __uint_as_float((unsigned)(b >> 32));
  idx[i] = key_index(b);
}

__global__ void sqrt_inplace_kernel(float* x, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] = sqrtf(x[i]);
}

// The fixed-size record of a detection for the final gather (engine.pack_result): n x (template id, score, count) then n x K x
// (query id, feature id, distance, confidence, x, y, X, Y, Z), every field one 32-bit word; integers keep their bit patterns.
__global__ __launch_bounds__(256) void pack_records_kernel(const int* __restrict__ tpl_ids, const float* __restrict__ scores, const int* __restrict__ counts,
                                                           const int* __restrict__ q_ids, const int* __restrict__ feat_ids, const float* __restrict__ dists,
                                                           const float* __restrict__ conf, const float* __restrict__ c2d, const float* __restrict__ c3d,
                                                           int n, int K, unsigned* __restrict__ out) {
  const int pair = blockIdx.x;  // (detection, slot)
  unsigned* rec = out + (size_t)pair * (3 + (size_t)K * 9);
  if (threadIdx.x == 0) {
    rec[0] = (unsigned)tpl_ids[pair];
    rec[1] = __float_as_uint(scores[pair]);
    rec[2] = (unsigned)counts[pair];
  }
  for (int k = threadIdx.x; k < K; k += 256) {
    const size_t o = (size_t)pair * K + k;
    unsigned* r = rec + 3 + (size_t)k * 9;
    r[0] = (unsigned)q_ids[o];
    r[1] = (unsigned)feat_ids[o];
    r[2] = __float_as_uint(dists[o]);
    r[3] = __float_as_uint(conf[o]);
    r[4] = __float_as_uint(c2d[o * 2]);
    r[5] = __float_as_uint(c2d[o * 2 + 1]);
    r[6] = __float_as_uint(c3d[o * 3]);
    r[7] = __float_as_uint(c3d[o * 3 + 1]);
    r[8] = __float_as_uint(c3d[o * 3 + 2]);
  }
}
}  // namespace

int launch_pack_records(const int* tpl_ids, const float* scores, const int* counts, const int* q_ids, const int* feat_ids, const float* dists, const float* conf,
                        const float* c2d, const float* c3d, int num_det, int n, int K, float* out, hipStream_t st) {
  if (num_det * n == 0) return FP_OK;
  hipLaunchKernelGGL(pack_records_kernel, dim3(num_det * n), dim3(256), 0, st, tpl_ids, scores, counts, q_ids, feat_ids, dists, conf, c2d, c3d, n, K,
                     reinterpret_cast<unsigned*>(out));
  FP_CHECK_LAUNCH("pack_records");
  return FP_OK;
}

int launch_sqnorm_rows(const float* x, long long n, int d, int ld, float* out, hipStream_t st) {
  FP_REQUIRE(d % 4 == 0 && ld % 4 == 0, "sqnorm_rows: d and ld must be multiples of 4");
  if (n == 0) return FP_OK;
  hipLaunchKernelGGL(sqnorm_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n, d, ld, out);
  FP_CHECK_LAUNCH("sqnorm_rows");
  return FP_OK;
}

int launch_normalize_rows(const float* x, long long n, int d, float eps, float* out, hipStream_t st) {
  if (n == 0) return FP_OK;
  hipLaunchKernelGGL(normalize_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, x, n, d, eps, out);
  FP_CHECK_LAUNCH("normalize_rows");
  return FP_OK;
}

int launch_tfidf_build(const int* word_ids, const float* word_d2, int knn_k, const int* seg_off, int num_segs,
                       const float* idf, int num_words, int soft, float sigma_sq, int sqrt_dists,
                       float* desc, float* desc_n, float eps, hipStream_t st) {
  FP_REQUIRE(num_words > 0 && num_words <= 16384, "tfidf_build: num_words out of range");
  FP_REQUIRE(knn_k >= 1 && knn_k <= 16, "tfidf_build: knn_k out of range");
  if (num_segs == 0) return FP_OK;
  size_t lds = (size_t)num_words * 4 + 4096 * 8;
  static FpDeviceOnce attr;
  fp_allow_dynamic_lds(attr, &tfidf_build_kernel, 16384 * 4 + 4096 * 8);
  hipLaunchKernelGGL(tfidf_build_kernel, dim3(num_segs), dim3(256), lds, st, word_ids, word_d2, knn_k, seg_off, idf,
                     num_words, soft, 2.0f * sigma_sq, sqrt_dists, desc, desc_n, eps);
  FP_CHECK_LAUNCH("tfidf_build");
  return FP_OK;
}

int launch_cyclic_select(const CyclicArgs& a, int num_pairs, hipStream_t st) {
  FP_REQUIRE(a.q_max <= 2048, "cyclic_select: more than 2048 query points per detection (got %d)", a.q_max);
  FP_REQUIRE(a.top_k >= 1 && a.k_max >= a.top_k, "cyclic_select: bad top_k / k_max");
  if (num_pairs == 0) return FP_OK;
  hipLaunchKernelGGL(cyclic_select_kernel, dim3(num_pairs), dim3(256), 0, st, a);
  FP_CHECK_LAUNCH("cyclic_select");
  return FP_OK;
}

int launch_sample_bilinear(const SampleArgs& a, hipStream_t st) {
  if (a.num_points == 0) return FP_OK;
  hipLaunchKernelGGL(sample_bilinear_kernel, dim3(cdiv(a.num_points, 4)), dim3(256), 0, st, a);
  FP_CHECK_LAUNCH("sample_bilinear");
  return FP_OK;
}

int launch_sqrt_inplace(float* x, long long n, hipStream_t st) {
  if (n == 0) return FP_OK;
  hipLaunchKernelGGL(sqrt_inplace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n);
  FP_CHECK_LAUNCH("sqrt_inplace");
  return FP_OK;
}

int launch_knn_merge(const unsigned long long* cand, int rows, int ncand, int k, float* out_d2, int* out_idx, hipStream_t st) {
  FP_REQUIRE(k >= 1 && k <= 8, "knn_merge: k must be in [1, 8]");
  if (rows == 0) return FP_OK;
  hipLaunchKernelGGL(knn_merge_kernel, dim3(cdiv(rows, 16)), dim3(256), 0, st, cand, rows, ncand, k, out_d2, out_idx);
  FP_CHECK_LAUNCH("knn_merge");
  return FP_OK;
}

int launch_unpack_best(const unsigned long long* best, long long n, float* d2, int* idx, hipStream_t st) {
  if (n == 0) return FP_OK;
  hipLaunchKernelGGL(unpack_best_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, best, n, d2, idx);
  FP_CHECK_LAUNCH("unpack_best");
  return FP_OK;
}
