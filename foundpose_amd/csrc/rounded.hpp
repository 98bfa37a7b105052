// Individually rounded fp64 operations, for the kernels whose arithmetic is pinned operation for operation to a numpy chain (crop.hip,
// render.hip, pose_eval.hip, pose_add.hip, point_extremes.hip, and through bop_dist.hpp vsd.hip and gt_info.hip).  Explicit _rn
// intrinsics: no contraction into FMAs whatever the translation unit's setting.  One home, so that no copy can lose its _rn.
// Defined at global scope without `static`, like rot.hpp: safe because FP_DEVICE is __device__ __forceinline__.
#pragma once
#include "common.hpp"

FP_DEVICE double dmul(double a, double b) { return __dmul_rn(a, b); }
FP_DEVICE double dadd(double a, double b) { return __dadd_rn(a, b); }
FP_DEVICE double dsub(double a, double b) { return __dsub_rn(a, b); }
FP_DEVICE double ddiv(double a, double b) { return __ddiv_rn(a, b); }
// (a0 b0 + a1 b1) + a2 b2
FP_DEVICE double dot3(double a0, double a1, double a2, double b0, double b1, double b2) {
  return dadd(dadd(dmul(a0, b0), dmul(a1, b1)), dmul(a2, b2));
}
// r.dot(p) + t: ((r0 x + r1 y) + r2 z) + t
FP_DEVICE double affine(const double* r, double t, double x, double y, double z) {
  return dadd(dadd(dadd(dmul(r[0], x), dmul(r[1], y)), dmul(r[2], z)), t);
}
FP_DEVICE double sqdist(double dx, double dy, double dz) { return dadd(dadd(dmul(dx, dx), dmul(dy, dy)), dmul(dz, dz)); }
