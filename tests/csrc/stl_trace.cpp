// Test harness (host only) for the torch.topk tie-order replay:
//
//  * McIlroy's adversary ("A Killer Adversary for Quicksort", 1999) run against the REAL libstdc++ algorithms behind
//    torch.topk's CPU kernel -- std::nth_element + std::sort of the first k-1, or std::sort alone.  The comparator decides
//    the values lazily: an item is "gas" (undecided, larger than every decided item) until a comparison forces one of two
//    gas items to "freeze" at the next rank.  The ranks it leaves make the median-of-3 quicksort degenerate, so the
//    depth limit runs out and the heap fallbacks are entered.
//  * an instrumented walk of foundpose_amd/csrc/stl_order.hpp: the loops of nth_element_ / sort_ / topk_torch_largest
//    restated around the header's own pieces (unguarded_partition_pivot_, heap_select_, partial_sort_, insertion_sort_),
//    counting which branch a (values, k) case takes.  The partition sizes are classed the way stl_wave.hpp splits them
//    (scanned part of at most 64 elements: the register-only partition; more: the stopper tables in LDS).
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../foundpose_amd/csrc/stl_order.hpp"

namespace {

struct Adversary {
  std::vector<int64_t> val;  // by item; gas until frozen
  int64_t gas, nsolid = 0, candidate = 0;
  explicit Adversary(int64_t n) : val(n, n - 1), gas(n - 1) {}
  void freeze(int64_t x) { val[x] = nsolid++; }
  // comp(x, y): "x sorts before y"
  bool less(int x, int y) {
    if (val[x] == gas && val[y] == gas) freeze(x == candidate ? x : y);
    if (val[x] == gas) candidate = x;
    else if (val[y] == gas) candidate = y;
    return val[x] < val[y];
  }
};

enum { C_PARTIAL_SORT, C_PART_SMALL, C_PART_LARGE, C_SELECT_FALLBACK, C_SORT_FALLBACK, C_TWO_PASS, C_COUNT };

using stl_order::Elem;

int partition_counted(Elem* a, int first, int last, int64_t* c) {
  ++c[(last - first - 1 <= 64) ? C_PART_SMALL : C_PART_LARGE];
  return stl_order::unguarded_partition_pivot_(a, first, last);
}

void nth_element_walk(Elem* a, int first, int nth, int last, int64_t* c) {
  if (first == last || nth == last) return;
  int depth = stl_order::lg2(last - first) * 2;
  while (last - first > 3) {
    if (depth == 0) {
      ++c[C_SELECT_FALLBACK];
      stl_order::heap_select_(a + first, nth + 1 - first, last - first);
      stl_order::swap_(a[first], a[nth]);
      return;
    }
    --depth;
    const int cut = partition_counted(a, first, last, c);
    if (cut <= nth) first = cut;
    else last = cut;
  }
  stl_order::insertion_sort_(a, first, last);
}

void sort_walk(Elem* a, int first, int last, int64_t* c) {
  if (last - first < 2) return;
  struct Frame {
    int first, last, depth;
  };
  std::vector<Frame> stack;
  stack.push_back(Frame{first, last, stl_order::lg2(last - first) * 2});
  while (!stack.empty()) {
    Frame f = stack.back();
    stack.pop_back();
    while (f.last - f.first > 16) {
      if (f.depth == 0) {
        ++c[C_SORT_FALLBACK];
        stl_order::partial_sort_(a + f.first, f.last - f.first, f.last - f.first);
        break;
      }
      --f.depth;
      const int cut = partition_counted(a, f.first, f.last, c);
      stack.push_back(Frame{cut, f.last, f.depth});
      f.last = cut;
    }
  }
  if (last - first > 512) ++c[C_TWO_PASS];  // stl_wave::sort: the placement no longer fits 8 x 64 registers
  if (last - first > 16) {
    stl_order::insertion_sort_(a, first, first + 16);
    for (int i = first + 16; i != last; ++i) stl_order::unguarded_linear_insert_(a, i);
  } else {
    stl_order::insertion_sort_(a, first, last);
  }
}

}  // namespace

// Ranks the adversary leaves when std::nth_element(first, first + k - 1, last) + std::sort(first, first + k - 1) run on n
// items (k == 0: std::sort of all n alone).  An item still gas at the end keeps the rank n - 1.
extern "C" void stl_trace_adversary(int64_t n, int64_t k, int64_t* ranks) {
  Adversary adv(n);
  std::vector<int> items(n);
  for (int64_t i = 0; i < n; ++i) items[i] = (int)i;
  auto comp = [&adv](int x, int y) { return adv.less(x, y); };
  if (k > 0) {
    std::nth_element(items.begin(), items.begin() + (k - 1), items.end(), comp);
    std::sort(items.begin(), items.begin() + (k - 1), comp);
  } else {
    std::sort(items.begin(), items.end(), comp);
  }
  for (int64_t i = 0; i < n; ++i) ranks[i] = adv.val[i];
}

// topk_torch_largest of stl_order.hpp with branch counters.  counters: [partial_sort branch, partitions with a scanned part
// of <= 64, of > 64, select fallbacks, sort fallbacks, two-pass placements].
extern "C" void stl_trace_topk(const float* values, int64_t n, int64_t k, int64_t* out_idx, int64_t* counters) {
  std::vector<Elem> a(n);
  for (int64_t j = 0; j < n; ++j) a[j] = {values[j], (int)j};
  for (int i = 0; i < C_COUNT; ++i) counters[i] = 0;
  if (k > 0 && n > 0) {
    if (k * 64 <= n) {
      ++counters[C_PARTIAL_SORT];
      stl_order::partial_sort_(a.data(), (int)k, (int)n);
    } else {
      nth_element_walk(a.data(), 0, (int)k - 1, (int)n, counters);
      sort_walk(a.data(), 0, (int)k - 1, counters);
    }
  }
  for (int64_t j = 0; j < k; ++j) out_idx[j] = a[j].idx;
}
