// The BOP 6D detection task's score (eval_bop24): greedy matching of every estimate group and the precision-recall
// accumulation per object, for all MSSD / MSPD thresholds at once.  The reference has no evaluation of this kind; the rules restate the
// published behaviour of bop_toolkit's detection scores.
//
// detection_match_kernel: one wave per (estimate group, column); a column is one threshold of one error type.  The wave runs the shared
//   greedy matcher of group_parts.hpp (four waves per workgroup, no barrier, no LDS) under the task's policy: an estimate may take a free
//   GT whose error is strictly below the threshold, the smallest (error, GT index) wins, and an invalid GT is taken like a valid one (the
//   estimate is then ignored, flag 2).
//
// detection_ap_kernel: one 256-thread workgroup per (object, column).  Pass 1 counts the object's true positives, false positives and
//   ignored estimates.  Thread i then finds, for recall threshold i, the smallest true-positive count m_i whose recall reaches it (a binary
//   search with the division the rule states).  Pass 2 walks the estimates in chunks of 256 from the LAST chunk to the first: an inclusive
//   scan gives every position its running counts and so its precision, a suffix maximum (carried across chunks) its envelope value, and
//   thread i picks the envelope at the position of true positive number m_i.  m_i = 0 takes the envelope of the first kept estimate, which
//   is the maximum over all.  Counts are integers, a precision and a recall are one division each, a maximum does not round: no result
//   depends on the order in which threads arrive.  FMA contraction is off; there are no float atomics.
#include "common.hpp"
#include "group_parts.hpp"

namespace {

constexpr int DA_WAVE = 64;
constexpr int DA_WAVES = DA_THREADS / DA_WAVE;
static_assert(DA_THREADS == BS_THREADS, "detection_ap_kernel scans with block_scan_inclusive");

// The 6D detection task's matching rule for greedy_match: one error type at one threshold.
struct DetectionPolicy {
  const double* err;    // [P, 2], from the column's error type on
  const int* gt_valid;
  double th;
  FP_DEVICE bool second_class(int gt_row) const { return !(gt_valid[gt_row] > 0); }  // an invalid GT: it is matched like a valid one
  FP_DEVICE double value(size_t row) const { return err[row * 2]; }
  FP_DEVICE bool candidate(double v) const { return v < th; }                        // false for a NaN; a candidate is never +inf
  FP_DEVICE MatchKey none() const { return {0, __builtin_huge_val(), 0x7fffffff}; }
  FP_DEVICE bool before(const MatchKey& a, const MatchKey& b) const { return a.v < b.v || (a.v == b.v && a.g < b.g); }  // the class does not rank
};

__global__ __launch_bounds__(GM_THREADS) void detection_match_kernel(DetMatchArgs a) {
  const int C = 2 * a.T;
  const long long w = match_wave();
  if (w >= (long long)a.t.n_groups * C) return;  // wave-uniform
  const int g = (int)(w / C), c = (int)(w % C);
  const int type = c / a.T, k = c % a.T;
  const GroupDims d = group_dims(a.t, g, GM_MAX_GT);
  const int tab = clampi(a.group_tab[g], 0, a.n_tab - 1);
  const DetectionPolicy p{a.err + type, a.gt_valid, a.ths[((size_t)tab * 2 + type) * a.T + k]};
  greedy_match(p, d, threadIdx.x & 63, a.flag, a.matched_gt, (size_t)d.e0 * C + c, C);
}

// the flag of the object's estimate at rank position `pos`: 0 false positive, 1 true positive, anything else is left out
FP_DEVICE int flag_at(const DetApArgs& a, int begin, int pos, int C, int c) {
  const int row = clampi(a.order[begin + pos], 0, a.n_est - 1);
  return (int)a.flag[(size_t)row * C + c];
}

__global__ __launch_bounds__(DA_THREADS) void detection_ap_kernel(DetApArgs a) {
#pragma clang fp contract(off)
  __shared__ int red[DA_WAVES][3];
  __shared__ int scan_slots[BS_WAVES];         // tp in the low half, fp in the high half: a chunk holds at most 256 of each
  __shared__ double wave_max[DA_WAVES];
  __shared__ int scan_tp[DA_THREADS];          // the running true-positive count at each position of the chunk
  __shared__ double env[DA_THREADS];           // the precision envelope at each position
  __shared__ double qs[DA_MAX_REC];

  const int tid = threadIdx.x, lane = tid & (DA_WAVE - 1), wave = tid >> 6;
  const int C = 2 * a.T;
  const int o = blockIdx.x / C, c = blockIdx.x % C;
  const int begin = clampi(a.obj_off[o], 0, a.n_order);
  const int n = a.n_est > 0 ? max(min(a.obj_off[o + 1], a.n_order) - begin, 0) : 0;
  const int nv = a.n_valid[o];
  const int R = a.R;
  const size_t oc = (size_t)o * C + c;

  // ---- pass 1: the totals
  int t_tp = 0, t_fp = 0, t_ig = 0;
  for (int pos = tid; pos < n; pos += DA_THREADS) {
    const int f = flag_at(a, begin, pos, C, c);
    t_tp += f == 1;
    t_fp += f == 0;
    t_ig += f != 0 && f != 1;
  }
  t_tp = wave_sum(t_tp); t_fp = wave_sum(t_fp); t_ig = wave_sum(t_ig);
  if (lane == 0) { red[wave][0] = t_tp; red[wave][1] = t_fp; red[wave][2] = t_ig; }
  __syncthreads();
  t_tp = t_fp = t_ig = 0;
#pragma unroll
  for (int v = 0; v < DA_WAVES; ++v) { t_tp += red[v][0]; t_fp += red[v][1]; t_ig += red[v][2]; }
  if (tid < 3) a.totals[oc * 3 + tid] = tid == 0 ? t_tp : (tid == 1 ? t_fp : t_ig);

  if (nv <= 0) {  // block-uniform: an object without a valid GT has no AP
    for (int i = tid; i < R; i += DA_THREADS) a.q[oc * R + i] = 0.0;
    if (tid == 0) a.ap[oc] = -1.0;
    return;
  }

  // ---- thread i: the true-positive count at which the recall reaches threshold i (t_tp + 1: never)
  const double dnv = (double)nv;
  int m_i = 0;
  double q_i = 0.0;
  if (tid < R) {
    const double thr = a.rec_thr[tid];
    int lo = 0, hi = t_tp + 1;  // the smallest m in [0, t_tp] with m / nv >= thr, else t_tp + 1 (a NaN threshold: never)
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if ((double)mid / dnv >= thr) hi = mid; else lo = mid + 1;
    }
    m_i = lo;
  }

  // ---- pass 2: the chunks from the last to the first
  int after_tp = 0, after_fp = 0;  // the counts of the chunks behind this one
  double running = -1.0;           // the largest precision behind this chunk (a precision is >= 0)
  for (int b = ((n - 1) / DA_THREADS) * DA_THREADS; n > 0 && b >= 0; b -= DA_THREADS) {
    const int pos = b + tid;
    const int f = pos < n ? flag_at(a, begin, pos, C, c) : 2;
    int chunk;  // (scan_slots are next written a barrier later: the two below)
    const int incl = block_scan_inclusive((f == 1 ? 1 : 0) | (f == 0 ? 1 << 16 : 0), scan_slots, chunk);
    const int before_tp = t_tp - after_tp - (chunk & 0xffff), before_fp = t_fp - after_fp - (chunk >> 16);
    const int tp_k = before_tp + (incl & 0xffff), fp_k = before_fp + (incl >> 16);
    double p = (f == 0 || f == 1) ? (double)tp_k / (double)(tp_k + fp_k) : -1.0;
#pragma unroll
    for (int s = 1; s < DA_WAVE; s <<= 1) {
      const double down = __shfl_down(p, s, DA_WAVE);
      if (lane + s < DA_WAVE) p = fmax(p, down);
    }
    if (lane == 0) wave_max[wave] = p;
    __syncthreads();
    double chunk_max = running;
#pragma unroll
    for (int v = 0; v < DA_WAVES; ++v) {
      if (v > wave) p = fmax(p, wave_max[v]);
      chunk_max = fmax(chunk_max, wave_max[v]);
    }
    p = fmax(p, running);
    scan_tp[tid] = tp_k;
    env[tid] = p;
    __syncthreads();
    if (tid < R && m_i >= 1 && m_i > before_tp && m_i <= before_tp + (chunk & 0xffff)) {
      int lo = 0, hi = DA_THREADS - 1;  // the first position whose count reaches m_i: true positive number m_i itself
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (scan_tp[mid] >= m_i) hi = mid; else lo = mid + 1;
      }
      q_i = env[lo];
    }
    running = chunk_max;
    after_tp += chunk & 0xffff;
    after_fp += chunk >> 16;
    __syncthreads();  // the tables are written again in the next round
  }
  if (tid < R) {
    if (m_i == 0 && t_tp + t_fp > 0) q_i = running;  // the first kept estimate: its envelope is the maximum over all
    a.q[oc * R + tid] = q_i;
    qs[tid] = q_i;
  }
  __syncthreads();
  if (tid == 0) {
    double sum = qs[0];
    for (int i = 1; i < R; ++i) sum = sum + qs[i];
    a.ap[oc] = sum / (double)R;
  }
}

}  // namespace

int launch_detection_match(const DetMatchArgs& a, hipStream_t st) {
  FP_REQUIRE(a.T >= 1 && a.T <= DA_MAX_THS, "detection_match: T must be in [1, %d] (got %d)", DA_MAX_THS, a.T);
  const GroupTables& t = a.t;
  FP_REQUIRE(t.n_groups >= 0 && t.n_a >= 0 && t.n_b >= 0 && t.n_pairs >= 0, "detection_match: negative count");
  if (t.n_groups == 0) return FP_OK;
  FP_REQUIRE(a.n_tab >= 1, "detection_match: no threshold row");
  const long long blocks = match_blocks((long long)t.n_groups * 2 * a.T);
  FP_REQUIRE(blocks <= 0x7fffffffLL, "detection_match: %d groups are too many for one launch", t.n_groups);
  hipLaunchKernelGGL(detection_match_kernel, dim3((unsigned)blocks), dim3(GM_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("detection_match");
  return FP_OK;
}

int launch_detection_ap(const DetApArgs& a, int num_objects, hipStream_t st) {
  FP_REQUIRE(a.T >= 1 && a.T <= DA_MAX_THS, "detection_ap: T must be in [1, %d] (got %d)", DA_MAX_THS, a.T);
  FP_REQUIRE(a.R >= 1 && a.R <= DA_MAX_REC, "detection_ap: R must be in [1, %d] (got %d)", DA_MAX_REC, a.R);
  FP_REQUIRE(num_objects >= 0 && a.n_order >= 0 && a.n_est >= 0, "detection_ap: negative count");
  if (num_objects == 0) return FP_OK;
  const long long blocks = (long long)num_objects * 2 * a.T;
  FP_REQUIRE(blocks <= 0x7fffffffLL, "detection_ap: %d objects are too many for one launch", num_objects);
  hipLaunchKernelGGL(detection_ap_kernel, dim3((unsigned)blocks), dim3(DA_THREADS), 0, st, a);
  FP_CHECK_LAUNCH("detection_ap");
  return FP_OK;
}
