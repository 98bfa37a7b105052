// The byte-per-pixel form of the mask overlap of csrc/coco_eval.hip, for tools/bench_coco.py's comparison: one
// 256-thread workgroup per (detection, instance) pair reads the two H x W byte masks, 16 B per lane, and counts intersection and union.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/mask_iou_bytes.hip -o tools/ubench/mask_iou_bytes
//   tools/ubench/mask_iou_bytes [groups 512] [E 12] [G 1] [H 480] [W 640] [iters 10]      -> one JSON line
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__device__ __forceinline__ unsigned marks(unsigned v) { return (v | ((v & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u; }  // bit 7 of every non-zero byte

__global__ __launch_bounds__(256) void fill(unsigned char* m, size_t n_total, int H, int W, unsigned seed) {  // one rectangle per mask
  const size_t per = (size_t)H * W;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_total; i += (size_t)gridDim.x * 256) {
    const unsigned k = (unsigned)(i / per) * 2654435761u + seed;
    const int p = (int)(i % per), y = p / W, x = p % W;
    const int x0 = (k >> 4) % (W / 2), y0 = (k >> 14) % (H / 2);
    m[i] = (x >= x0 && x < x0 + W / 3 && y >= y0 && y < y0 + H / 3) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void iou_bytes(const uint4* a, const uint4* b, int E, int G, int nvec, int2* out) {
  __shared__ int red[4][2];
  const int pair = blockIdx.x, g = pair / (E * G), r = pair - g * (E * G), e = r / G, j = r - e * G;
  const uint4* pa = a + (size_t)(g * E + e) * nvec;
  const uint4* pb = b + (size_t)(g * G + j) * nvec;
  int inter = 0, uni = 0;
  for (int v = threadIdx.x; v < nvec; v += 256) {
    const uint4 x = pa[v], y = pb[v];
    const unsigned xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned mx = marks(xs[k]), my = marks(ys[k]);
      inter += __popc(mx & my);
      uni += __popc(mx | my);
    }
  }
  for (int o = 32; o > 0; o >>= 1) { inter += __shfl_xor(inter, o, 64); uni += __shfl_xor(uni, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = inter; red[threadIdx.x >> 6][1] = uni; }
  __syncthreads();
  if (threadIdx.x == 0) out[pair] = make_int2(red[0][0] + red[1][0] + red[2][0] + red[3][0], red[0][1] + red[1][1] + red[2][1] + red[3][1]);
}

int main(int argc, char** argv) {
  const int groups = argc > 1 ? atoi(argv[1]) : 512, E = argc > 2 ? atoi(argv[2]) : 12, G = argc > 3 ? atoi(argv[3]) : 1;
  const int H = argc > 4 ? atoi(argv[4]) : 480, W = argc > 5 ? atoi(argv[5]) : 640, iters = argc > 6 ? atoi(argv[6]) : 10;
  const long long n = (long long)H * W;
  if (groups < 1 || E < 1 || G < 1 || H < 2 || W < 2 || iters < 1 || n % 16 || n > (1ll << 30) || (long long)groups * E * G > (1ll << 30)) {
    fprintf(stderr, "bad shape (H W must be a multiple of 16)\n");
    return 1;
  }
  const size_t na = (size_t)groups * E * n, nb = (size_t)groups * G * n, pairs = (size_t)groups * E * G;
  unsigned char *a, *b;
  int2* out;
  CHECK(hipMalloc(&a, na));
  CHECK(hipMalloc(&b, nb));
  CHECK(hipMalloc(&out, pairs * sizeof(int2)));
  fill<<<2048, 256>>>(a, na, H, W, 1u);
  fill<<<2048, 256>>>(b, nb, H, W, 7u);
  CHECK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<float> ms;
  for (int it = 0; it < iters + 1; ++it) {
    CHECK(hipEventRecord(e0));
    iou_bytes<<<(unsigned)pairs, 256>>>((const uint4*)a, (const uint4*)b, E, G, (int)(n / 16), out);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float t;
    CHECK(hipEventElapsedTime(&t, e0, e1));
    if (it) ms.push_back(t);  // the first launch loads the code object
  }
  std::vector<int2> h(pairs);
  CHECK(hipMemcpy(h.data(), out, pairs * sizeof(int2), hipMemcpyDeviceToHost));
  long long si = 0, su = 0;
  for (const int2& v : h) { si += v.x; su += v.y; }
  std::sort(ms.begin(), ms.end());
  const double med = ms[ms.size() / 2] * 1e-3, bytes = 2.0 * (double)pairs * (double)n;
  printf("{\"form\": \"bytes, one pair per workgroup\", \"groups\": %d, \"E\": %d, \"G\": %d, \"H\": %d, \"W\": %d, \"pairs\": %zu, \"median_s\": %.6e, "
         "\"min_s\": %.6e, \"max_s\": %.6e, \"bytes_read\": %.0f, \"bytes_per_s\": %.4e, \"sum_inter\": %lld, \"sum_union\": %lld}\n",
         groups, E, G, H, W, pairs, med, ms.front() * 1e-3, ms.back() * 1e-3, bytes, bytes / med, si, su);
  hipFree(a); hipFree(b); hipFree(out);
  return 0;
}
