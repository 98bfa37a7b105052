/* Host probe of include/foundpose_amd.h for tests/test_cabi_symbols.py: what a C compiler makes of the three ViT structs, of the constants and of
 * the scratch-size macros -- everything foundpose_amd/_lib.py restates by hand.  The test checks these tables against the header's own lists of
 * names, so an entry missing here fails there. */
#include <stddef.h>
#include <stdint.h>

#include "foundpose_amd.h"

typedef struct { const char* type; const char* field; size_t offset, size; } abi_field; /* field "" : size = sizeof(type) */
#define S(t) {#t, "", 0, sizeof(t)}
#define F(t, f) {#t, #f, offsetof(t, f), sizeof(((t*)0)->f)}
#define B(f) F(fp_vit_block, f)
#define M(f) F(fp_vit_model, f)
#define W(f) F(fp_vit_workspace, f)
const abi_field abi_fields[] = {
    S(fp_vit_block), B(ln1_w), B(ln1_b), B(ln2_w), B(ln2_b), B(ls1), B(ls2), B(qkv_w), B(proj_w), B(fc1_w), B(fc2_w), B(qkv_b), B(proj_b), B(fc1_b), B(fc2_b),
    B(qkv_s), B(proj_s), B(fc1_s), B(fc2_s), B(act_scale), B(qkv_colsum), B(fc1_colsum),
    S(fp_vit_model), M(dim), M(depth), M(heads), M(hidden), M(registers), M(patch), M(ffn_swiglu), M(weight_dtype), M(patch_w), M(patch_k_pad), M(patch_b),
    M(pos_patch), M(prefix), M(norm_w), M(norm_b), M(blocks), M(ld_w_dim), M(ld_w_hidden), M(patch_stride), M(patch_acc_scale), M(ln_fold),
    S(fp_vit_workspace), W(patches), W(x), W(y), W(qkv), W(h), W(a8), W(ld_y), W(ld_h), W(ld_qkv), W(m_pad), W(m_patch_pad), W(xb), W(stats), W(sat), W(xl),
};
const int abi_num_fields = sizeof(abi_fields) / sizeof(abi_fields[0]);

typedef struct { const char* name; double value; } abi_constant; /* every value is exact in a double */
#define K(x) {#x, (double)(x)}
const abi_constant abi_constants[] = {
    K(FP_F32), K(FP_BF16), K(FP_FP8), K(FP_F16X3), K(FP_F16F8), K(FP_F16), K(FP_GEMM_SPLIT_F16F8), K(FP_GEMM_F16), K(FP_SPLIT_SCALE_ACT),
    K(FP_SPLIT_SCALE_QKV), K(FP_SPLIT_SCALE_HID), K(FP_ABI_VERSION), K(FP_POSE_ERR_TILE), K(FP_POSE_ADD_TILE), K(FP_PTS_TILE), K(FP_PTS_DIAMETER_MAX_V),
    K(FP_VSD_MAX_TAUS), K(FP_DEPTH_MAX_PLANES), K(FP_DEPTH_MAX_HYPOTHESES), K(FP_DEPTH_MAX_PROPOSALS), K(FP_DEPTH_PLANE_CHUNK), K(FP_TSDF_MAX_DIM),
    K(FP_TSDF_MAX_VOXELS), K(FP_TSDF_MAX_FRAMES), K(FP_TSDF_FRAME_DOUBLES), K(FP_TSDF_DIFFUSE_MAX_ITERS), K(FP_MESH_MAX_DIM), K(FP_MESH_MAX_ROWS),
    K(FP_REFINE_CHUNK), K(FP_REFINE_RECORD), K(FP_REFINE_STATE_BYTES), K(FP_PROPOSAL_MAX_SIZE), K(FP_PROPOSAL_MAX_K), K(FP_PROPOSAL_MAX_RANKED),
    K(FP_TEXTURE_MAX_SIDE), K(FP_VIS_MAX_MATCHES), K(FP_VIS_MAX_DILATE),
    K(FP_PROPOSAL_CANDIDATE), K(FP_PROPOSAL_SMALL), K(FP_PROPOSAL_EMPTY), K(FP_PROPOSAL_NO_OBJECT), K(FP_PROPOSAL_LOW_SCORE), K(FP_PROPOSAL_GROUP_LIMIT),
};
const int abi_num_constants = sizeof(abi_constants) / sizeof(abi_constants[0]);

/* The scratch-size macros, called the way a C caller does: with int arguments. */
#define SCRATCH_MACROS(X1, X2, X3, X5)                                                                                                          \
  X3(FP_KNN_SCRATCH_BYTES) X2(FP_COSINE_SCRATCH_FLOATS) X2(FP_COSINE_PREFILTER_SCRATCH_FLOATS) X3(FP_CYCLIC_SCRATCH_BYTES)                    \
  X3(FP_POSE_ERR_SCRATCH_BYTES) X2(FP_POSE_ADD_SCRATCH_BYTES) X1(FP_PTS_DIAMETER_SCRATCH_BYTES) X3(FP_PTS_HAUSDORFF_SCRATCH_BYTES)            \
  X1(FP_VSD_SCRATCH_BYTES) X1(FP_GT_VIS_SCRATCH_BYTES) X3(FP_DEPTH_PLANE_SCRATCH_BYTES) X2(FP_DEPTH_COMPONENTS_SCRATCH_BYTES)                 \
  X2(FP_COMPONENT_TABLE_SCRATCH_BYTES) X1(FP_TSDF_SCRATCH_BYTES) X2(FP_REFINE_SCRATCH_BYTES) X2(FP_DEPTH_REFINE_SCRATCH_BYTES)                \
  X2(FP_TSDF_TRACK_SCRATCH_BYTES) X2(FP_RGBD_REFINE_SCRATCH_BYTES) X5(FP_PROPOSAL_SCORE_SCRATCH_BYTES)

typedef struct { const char* name; int arity; } abi_scratch_macro;
#define N1(m) {#m, 1},
#define N2(m) {#m, 2},
#define N3(m) {#m, 3},
#define N5(m) {#m, 5},
const abi_scratch_macro abi_scratch_macros[] = {SCRATCH_MACROS(N1, N2, N3, N5)};
const int abi_num_scratch_macros = sizeof(abi_scratch_macros) / sizeof(abi_scratch_macros[0]);

#define E1(m) static uint64_t eval_##m(const int* a) { return m(a[0]); }
#define E2(m) static uint64_t eval_##m(const int* a) { return m(a[0], a[1]); }
#define E3(m) static uint64_t eval_##m(const int* a) { return m(a[0], a[1], a[2]); }
#define E5(m) static uint64_t eval_##m(const int* a) { return m(a[0], a[1], a[2], a[3], a[4]); }
SCRATCH_MACROS(E1, E2, E3, E5)
#define P(m) eval_##m,
static uint64_t (*const abi_scratch_eval[])(const int*) = {SCRATCH_MACROS(P, P, P, P)};

/* out[i] = macro `which` of the i-th argument tuple; args is [n, arity of the macro] */
void abi_scratch_values(int which, int64_t n, const int* args, uint64_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = abi_scratch_eval[which](args + i * abi_scratch_macros[which].arity);
}
