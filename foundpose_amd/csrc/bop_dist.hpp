// BOP's distance image and visibility test, shared by vsd.hip and gt_info.hip: one copy, so the two cannot drift apart.
// fp64, every operation rounded on its own (rounded.hpp's _rn wrappers: no contraction whatever the translation unit's setting).
#pragma once
#include "common.hpp"
#include "rounded.hpp"

namespace {

// misc.depth_im_to_dist_im_fast: sqrt(Xs**2 + Ys**2 + depth**2) with Xs = xs * depth, Ys = ys * depth
FP_DEVICE double dist(double xs, double ys, float d) {
  const double dd = (double)d, X = dmul(xs, dd), Y = dmul(ys, dd);
  return __dsqrt_rn(dadd(dadd(dmul(X, X), dmul(Y, Y)), dmul(dd, dd)));
}
// visibility._estimate_visib_mask, bop19: (d_model.astype(f32) - d_test.astype(f32) <= delta | d_test == 0) & d_model > 0
FP_DEVICE bool visib(double dm, double dt, float delta) {
  return (__fsub_rn((float)dm, (float)dt) <= delta || dt == 0.0) && dm > 0.0;
}

}  // namespace
