// Operand staging of the exact-fp32 MFMA tiles (f32_tile.hip, and the appearance score in proposals.hip): 128 rows x 32 k of one operand
// go global -> registers -> a k-major LDS image ([k][row], stride 129 dwords), so that the transpose happens on the write and the
// fragment reads of v_mfma_f32_32x32x2_f32 are conflict-free ds_read_b32.
#pragma once
#include "common.hpp"

namespace f32_stage {

constexpr int BM = 128, BN = 128, BK = 32, LDS_STRIDE = 129;
constexpr int STAGE_FLOATS = BK * LDS_STRIDE;  // per operand per stage

struct Frag {
  float4 v[4];
};

// 128 rows x 32 k of one operand -> 4 float4 per thread (8 lanes cover one 128-B row).  Branch-free: a position outside the
// operand (row past the segment, k past K -- K % 4 == 0 is checked on the host) loads a clamped address and is zeroed, so
// the four loads always issue back to back and nothing waits between them.
FP_DEVICE void load_tile(Frag& f, const float* __restrict__ base, int ld, int row0, int nrows, int k0, int K, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = tid + i * 256;
    const int row = row0 + (idx >> 3), k = k0 + (idx & 7) * 4;
    const bool ok = row < nrows && k < K;
    const float4 v = *reinterpret_cast<const float4*>(base + (size_t)(row < nrows ? row : nrows - 1) * ld + (k < K ? k : K - 4));
    f.v[i] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

FP_DEVICE void store_tile(const Frag& f, float* __restrict__ lds, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int idx = tid + i * 256;
    int row = idx >> 3, c = idx & 7;
    float* p = lds + (c * 4) * LDS_STRIDE + row;
    p[0 * LDS_STRIDE] = f.v[i].x;
    p[1 * LDS_STRIDE] = f.v[i].y;
    p[2 * LDS_STRIDE] = f.v[i].z;
    p[3 * LDS_STRIDE] = f.v[i].w;
  }
}

}  // namespace f32_stage
