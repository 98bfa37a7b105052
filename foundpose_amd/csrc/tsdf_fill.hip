// Volumetric diffusion over a TSDF volume's grid: the smoother of reconstruct.py's hole filling (fill_volume; DESIGN.md section 34,
// tests/tsdf_fill_ref.py restates it).
//
// val is [channels, nz, ny, nx] fp32, x fastest, state [nz, ny, nx] uint8: 0 UNKNOWN, 1 FIXED, 2 FREE.  One launch is one Jacobi
// iteration from (val, state) into (val_out, state_out); the host swaps the pairs between launches.  A FIXED voxel is copied.  Any
// other voxel visits centre, -x, +x, -y, +y, -z, +z, those that lie inside the volume and are not UNKNOWN: n of them, their values
// added in that order in fp32 to an accumulator that starts at +0, one accumulator per channel.  n = 0: UNKNOWN, value +0; else FREE,
// value acc / n.  The value of an UNKNOWN voxel is loaded with its row but never enters an operation: it is selected away, so a NaN
// stored there does not spread.  Every output depends on the previous iteration's seven voxels alone, so the bits do not depend on how
// the volume is cut into threads.
//
// tsdf_diffuse_kernel<C, V>   one thread per V consecutive voxels by linear index, a wave 64 V consecutive voxels: whole x-rows when
//                             nx % (64 V) == 0, else it runs on into the next row, the loads and stores contiguous either way.
//                             V = 4 when nx % 4 == 0: a thread's four voxels then lie in one row and every row starts on 16 bytes, so
//                             the centre, +-y and +-z values are one 16-byte load per channel and the states one 4-byte load; only
//                             the two x neighbours beyond the four are single loads.  V = 1 otherwise.  The traffic the algorithm needs
//                             is 4 C + 1 bytes in and out per voxel and iteration; the six neighbour reads come from lines a
//                             neighbouring lane, row or plane has just fetched.
#include "common.hpp"
#include "kernels.hpp"
#include "../../include/foundpose_amd.h"

#pragma clang fp contract(off)

namespace {

constexpr int FILL_THREADS = 256;
constexpr uint8_t ST_UNKNOWN = 0, ST_FIXED = 1, ST_FREE = 2;

template <int V> struct Row;   // V consecutive entries of a plane
template <> struct Row<1> {
  static FP_DEVICE void vals(const float* p, float* out) { out[0] = p[0]; }
  static FP_DEVICE void states(const uint8_t* p, uint8_t* out) { out[0] = p[0]; }
  static FP_DEVICE void put(float* p, const float* in) { p[0] = in[0]; }
  static FP_DEVICE void put(uint8_t* p, const uint8_t* in) { p[0] = in[0]; }
};
template <> struct Row<4> {    // p is 16-byte (values) or 4-byte (states) aligned: the launcher picks V = 4 only then
  static FP_DEVICE void vals(const float* p, float* out) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    out[0] = q.x, out[1] = q.y, out[2] = q.z, out[3] = q.w;
  }
  static FP_DEVICE void states(const uint8_t* p, uint8_t* out) {
    const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
    out[0] = (uint8_t)(q & 255u), out[1] = (uint8_t)((q >> 8) & 255u), out[2] = (uint8_t)((q >> 16) & 255u), out[3] = (uint8_t)(q >> 24);
  }
  static FP_DEVICE void put(float* p, const float* in) { *reinterpret_cast<float4*>(p) = make_float4(in[0], in[1], in[2], in[3]); }
  static FP_DEVICE void put(uint8_t* p, const uint8_t* in) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)in[0] | ((uint32_t)in[1] << 8) | ((uint32_t)in[2] << 16) | ((uint32_t)in[3] << 24);
  }
};

template <int C, int V>
__global__ __launch_bounds__(FILL_THREADS) void tsdf_diffuse_kernel(TsdfDiffuseArgs a) {
  const long long row = a.nx, plane = (long long)a.nx * a.ny, n = plane * a.nz;   // n <= 2^27
  const long long v = ((long long)blockIdx.x * FILL_THREADS + threadIdx.x) * V;
  if (v >= n) return;                                               // V = 4: n % 4 == 0, so v + 3 < n as well
  const int i = (int)(v % row), j = (int)((v / row) % a.ny), k = (int)(v / plane);
  // which of the six neighbour rows lie inside the volume (V = 4: i % 4 == 0 and nx % 4 == 0, so i + 3 < nx)
  const bool in_xm = i > 0, in_xp = i + V < a.nx, in_ym = j > 0, in_yp = j + 1 < a.ny, in_zm = k > 0, in_zp = k + 1 < a.nz;
  uint8_t sc[V], sym[V], syp[V], szm[V], szp[V];
  Row<V>::states(a.state + v, sc);
#pragma unroll
  for (int e = 0; e < V; ++e) sym[e] = syp[e] = szm[e] = szp[e] = ST_UNKNOWN;   // outside the volume: takes no part, like UNKNOWN
  if (in_ym) Row<V>::states(a.state + v - row, sym);
  if (in_yp) Row<V>::states(a.state + v + row, syp);
  if (in_zm) Row<V>::states(a.state + v - plane, szm);
  if (in_zp) Row<V>::states(a.state + v + plane, szp);
  const uint8_t sxm = in_xm ? a.state[v - 1] : ST_UNKNOWN, sxp = in_xp ? a.state[v + V] : ST_UNKNOWN;
  bool take[7][V];
  int cnt[V];
  uint8_t so[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    take[0][e] = sc[e] != ST_UNKNOWN;
    take[1][e] = (e > 0 ? sc[(e + V - 1) % V] : sxm) != ST_UNKNOWN;
    take[2][e] = (e + 1 < V ? sc[(e + 1) % V] : sxp) != ST_UNKNOWN;
    take[3][e] = sym[e] != ST_UNKNOWN, take[4][e] = syp[e] != ST_UNKNOWN;
    take[5][e] = szm[e] != ST_UNKNOWN, take[6][e] = szp[e] != ST_UNKNOWN;
    cnt[e] = 0;
#pragma unroll
    for (int d = 0; d < 7; ++d) cnt[e] += (int)take[d][e];
    so[e] = sc[e] == ST_FIXED ? ST_FIXED : (cnt[e] > 0 ? ST_FREE : ST_UNKNOWN);
  }
  Row<V>::put(a.state_out + v, so);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float* p = a.val + (long long)c * n + v;
    float vc[V], vym[V], vyp[V], vzm[V], vzp[V], out[V];
    Row<V>::vals(p, vc);
#pragma unroll
    for (int e = 0; e < V; ++e) vym[e] = vyp[e] = vzm[e] = vzp[e] = 0.f;       // never taken where the row was not loaded
    if (in_ym) Row<V>::vals(p - row, vym);
    if (in_yp) Row<V>::vals(p + row, vyp);
    if (in_zm) Row<V>::vals(p - plane, vzm);
    if (in_zp) Row<V>::vals(p + plane, vzp);
    const float vxm = in_xm ? p[-1] : 0.f, vxp = in_xp ? p[V] : 0.f;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float nb[7] = {vc[e], e > 0 ? vc[(e + V - 1) % V] : vxm, e + 1 < V ? vc[(e + 1) % V] : vxp, vym[e], vyp[e], vzm[e], vzp[e]};
      float acc = 0.f;
#pragma unroll
      for (int d = 0; d < 7; ++d) acc = take[d][e] ? __fadd_rn(acc, nb[d]) : acc;   // a select: what is not taken is never an operand
      out[e] = sc[e] == ST_FIXED ? vc[e] : (cnt[e] > 0 ? __fdiv_rn(acc, (float)cnt[e]) : 0.f);
    }
    Row<V>::put(a.val_out + (long long)c * n + v, out);
  }
}

template <int C>
void launch(const TsdfDiffuseArgs& a, hipStream_t st) {
  const long long n = (long long)a.nx * a.ny * a.nz;
  const auto aligned = [](const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; };
  if (a.nx % 4 == 0 && aligned(a.val, 16) && aligned(a.val_out, 16) && aligned(a.state, 4) && aligned(a.state_out, 4)) {
    const long long threads = n / 4;
    hipLaunchKernelGGL((tsdf_diffuse_kernel<C, 4>), dim3((unsigned)((threads + FILL_THREADS - 1) / FILL_THREADS)), dim3(FILL_THREADS), 0, st, a);
  } else {
    hipLaunchKernelGGL((tsdf_diffuse_kernel<C, 1>), dim3((unsigned)((n + FILL_THREADS - 1) / FILL_THREADS)), dim3(FILL_THREADS), 0, st, a);
  }
}

}  // namespace

int launch_tsdf_diffuse(const TsdfDiffuseArgs& a, hipStream_t st) {
  if (a.channels == 1) launch<1>(a, st);
  else launch<3>(a, st);
  FP_CHECK_LAUNCH("tsdf_diffuse");
  return FP_OK;
}
