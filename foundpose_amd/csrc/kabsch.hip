// Batched 3D-3D RANSAC on depth-lifted correspondences (pnp_type "kabsch_depth"): the coarse pose of a
// (detection, template slot) pair from its 2D-3D correspondences AND the frame's depth image.  This stage is the project's own; the
// reference solves its coarse poses on pixels only.
//   lift    every correspondence's pixel (solve camera) -> ray -> frame camera (rotation A, the cameras share their centre) -> nearest
//           depth pixel -> the measured point Y in the SOLVE camera, so that poses come out model -> solve camera like fp_pnp_ransac's;
//   RANSAC  3 distinct valid correspondences per hypothesis (the sampler of ransac.hpp), an edge-length congruence gate, the closed-form
//           fit R = F_Y F_X^T of the two triangle frames, t = mean(Y) - R mean(X); score = valid points within tau (mm) of their
//           measurement; all hypotheses in parallel, then the sequential best-model rule replayed over the counts (model_points 3, out
//           of the valid correspondences);
//   refit   Horn's closed form on the winner's inliers: centroids and the cross-covariance by block reductions in a fixed order, the
//           largest eigenvector of the 4x4 quaternion matrix by cyclic Jacobi on one lane.
// One 256-thread workgroup per pair; arithmetic in fp64, points stored as fp32.  The sampler, the replay, the triangle frame, the output
// records and the block reduction are ransac.hpp's, shared with pnp.hip; the lift, the gate, the fit, the residual and the refit are this
// file's, and so are the two fields PnP does not have (num_valid, the status -1).  Every sum has a fixed order and there are no atomics,
// so a pair's result depends on (seed, key, its own data) only.
#include "common.hpp"
#include "kernels.hpp"
#include "ransac.hpp"

namespace {

constexpr int KB_MAX_ITERS = 4096;
constexpr int KB_MAX_K = 4096;
constexpr int KB_JACOBI_SWEEPS = 30;
constexpr int KB_LAST_ATTEMPT = 64;  // an index is drawn at most 65 times: attempts 0..64

struct LiftCams {
  double fx, fy, cx, cy;      // solve camera
  double ffx, ffy, fcx, fcy;  // frame camera
  double A[9];                // solve camera -> frame camera
};

// One correspondence's pixel -> the measured point in the solve camera.  Every operation is a single correctly rounded fp64 operation in
// the order DESIGN.md section 16 states (no contraction into FMAs), so the tap and the stored point are the restatement's bit for bit.
FP_DEVICE bool lift_point(const LiftCams& c, double u, double v, const float* img, int H, int W, float* Y) {
#pragma clang fp contract(off)
  const double dx = (u - c.cx) / c.fx, dy = (v - c.cy) / c.fy;
  const double gx = (c.A[0] * dx + c.A[1] * dy) + c.A[2];
  const double gy = (c.A[3] * dx + c.A[4] * dy) + c.A[5];
  const double gz = (c.A[6] * dx + c.A[7] * dy) + c.A[8];
  if (!(gz > 1e-9)) return false;
  const double uf = c.ffx * gx / gz + c.fcx, vf = c.ffy * gy / gz + c.fcy;
  const double px = rint(uf), py = rint(vf);  // half to even
  if (!(px >= 0.0 && px <= (double)(W - 1) && py >= 0.0 && py <= (double)(H - 1))) return false;  // (NaN fails too) no tap outside the image
  const float D = img[(size_t)(int)py * W + (int)px];
  if (!(D > 0.f)) return false;
  const double s = (double)D / gz;
  Y[0] = (float)(s * dx);
  Y[1] = (float)(s * dy);
  Y[2] = (float)s;
  return true;
}

FP_DEVICE double dist3(const double* a, const double* b) {
  const double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
  return sqrt(dot3(d, d));
}

// squared distance of a transformed model point from its measurement (mm^2)
FP_DEVICE double resid2(const Pose& P, const float* X, const float* Y) {
  const double x = P.R[0] * X[0] + P.R[1] * X[1] + P.R[2] * X[2] + P.t[0] - Y[0];
  const double y = P.R[3] * X[0] + P.R[4] * X[1] + P.R[5] * X[2] + P.t[1] - Y[1];
  const double z = P.R[6] * X[0] + P.R[7] * X[1] + P.R[8] * X[2] + P.t[2] - Y[2];
  return x * x + y * y + z * z;
}

// hypothesis h of a pair: 3 distinct valid correspondences (an invalid or repeated index is drawn again, at most 64 redraws per index),
// the congruence gate, the triangle-frame fit
FP_DEVICE bool hypothesis(unsigned long long key, int N, const float* X3, const float* Y3, const unsigned char* valid, double tau, Pose* out) {
  int id[3];
  if (!ransac_draw<3, KB_LAST_ATTEMPT>(key, N, id, [&](int c) -> bool { return valid[c]; })) return false;
  double X[3][3], Y[3][3];
  for (int j = 0; j < 3; ++j)
    for (int r = 0; r < 3; ++r) { X[j][r] = X3[id[j] * 3 + r]; Y[j][r] = Y3[id[j] * 3 + r]; }
  // a rigid motion keeps edge lengths: three inliers of one pose (each within tau of its measurement) differ by at most 2 tau per edge
  for (int i = 0; i < 3; ++i) {
    const int j = (i + 1) % 3;
    if (!(fabs(dist3(X[i], X[j]) - dist3(Y[i], Y[j])) <= 2.0 * tau)) return false;
  }
  double Fx[9], Fy[9];
  if (!tri_frame(X[0], X[1], X[2], Fx) || !tri_frame(Y[0], Y[1], Y[2], Fy)) return false;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out->R[i * 3 + j] = Fy[i * 3 + 0] * Fx[j * 3 + 0] + Fy[i * 3 + 1] * Fx[j * 3 + 1] + Fy[i * 3 + 2] * Fx[j * 3 + 2];  // Fy Fx^T
  double mx[3], my[3];
  for (int r = 0; r < 3; ++r) { mx[r] = (X[0][r] + X[1][r] + X[2][r]) / 3.0; my[r] = (Y[0][r] + Y[1][r] + Y[2][r]) / 3.0; }
  for (int i = 0; i < 3; ++i) out->t[i] = my[i] - (out->R[i * 3 + 0] * mx[0] + out->R[i * 3 + 1] * mx[1] + out->R[i * 3 + 2] * mx[2]);
  return true;
}

// Largest eigenvector of the symmetric 4x4 M by cyclic Jacobi (row-major, destroyed): sweeps over the six off-diagonal pairs in the order
// (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), at most KB_JACOBI_SWEEPS of them; a sweep is not started once the off-diagonal sum of squares is
// <= 1e-30 of the matrix's sum of squares (off-diagonal norm <= 1e-15 of the Frobenius norm), which includes the zero matrix.
FP_DEVICE void jacobi4_largest(double* M, double* q) {
  double V[16];
  for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < KB_JACOBI_SWEEPS; ++sweep) {
    double off = 0.0, all = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        all += M[i * 4 + j] * M[i * 4 + j];
        if (i != j) off += M[i * 4 + j] * M[i * 4 + j];
      }
    if (!(off > 1e-30 * all)) break;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        const double apr = M[p * 4 + r];
        if (apr == 0.0) continue;
        const double theta = (M[r * 4 + r] - M[p * 4 + p]) / (2.0 * apr);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 4; ++k) {  // M <- M J
          const double mkp = M[k * 4 + p], mkr = M[k * 4 + r];
          M[k * 4 + p] = c * mkp - s * mkr;
          M[k * 4 + r] = s * mkp + c * mkr;
        }
        for (int k = 0; k < 4; ++k) {  // M <- J^T M
          const double mpk = M[p * 4 + k], mrk = M[r * 4 + k];
          M[p * 4 + k] = c * mpk - s * mrk;
          M[r * 4 + k] = s * mpk + c * mrk;
        }
        for (int k = 0; k < 4; ++k) {  // V <- V J
          const double vkp = V[k * 4 + p], vkr = V[k * 4 + r];
          V[k * 4 + p] = c * vkp - s * vkr;
          V[k * 4 + r] = s * vkp + c * vkr;
        }
      }
  }
  double lam = M[0];
  for (int k = 0; k < 4; ++k) q[k] = V[k * 4];
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (M[i * 5] > lam) {  // the first of equal eigenvalues
      lam = M[i * 5];
      for (int k = 0; k < 4; ++k) q[k] = V[k * 4 + i];
    }
  double n = 0.0;
  for (int k = 0; k < 4; ++k) n += q[k] * q[k];
  n = sqrt(n);
  for (int k = 0; k < 4; ++k) q[k] /= n;
}

__global__ __launch_bounds__(RANSAC_THREADS) void kabsch_ransac_kernel(KabschArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* X3 = reinterpret_cast<float*>(smem);                   // [k_max, 3] model points
  float* Y3 = X3 + (size_t)a.k_max * 3;                         // [k_max, 3] measured points, solve camera
  int* cnt = reinterpret_cast<int*>(Y3 + (size_t)a.k_max * 3);  // [iters]
  unsigned char* valid = reinterpret_cast<unsigned char*>(cnt + a.iters);  // [k_max]
  unsigned char* inl = valid + a.k_max;                         // [k_max]
  __shared__ double acc[4][12];
  __shared__ double tot[12];
  __shared__ Pose cur;
  __shared__ int s_best, s_count, s_wave[4];

  const int pair = blockIdx.x, tid = threadIdx.x;
  const int det = pair / a.n_slots;
  const int N = min(max(a.counts[pair], 0), a.k_max);
  auto fail = [&](int code, int num_valid) {
    if (tid == 0) a.num_valid[pair] = num_valid;
    ransac_write_failure(a, pair, tid, code);
  };
  const int image = a.image_index[det];
  if (image < 0 || image >= a.num_images) { fail(-1, 0); return; }  // block-uniform; reported as success = -1, the image is never read
  const double tau = a.tau[det];
  if (!(tau > 0.0)) { fail(-1, 0); return; }

  // ---- lift
  LiftCams lc;
  lc.fx = a.cam[det * 4 + 0]; lc.fy = a.cam[det * 4 + 1]; lc.cx = a.cam[det * 4 + 2]; lc.cy = a.cam[det * 4 + 3];
  lc.ffx = a.frame_cam[det * 4 + 0]; lc.ffy = a.frame_cam[det * 4 + 1]; lc.fcx = a.frame_cam[det * 4 + 2]; lc.fcy = a.frame_cam[det * 4 + 3];
  for (int i = 0; i < 9; ++i) lc.A[i] = a.A[det * 9 + i];
  const float* img = a.depth + (size_t)image * a.H * a.W;
  int nv = 0;
  for (int p = tid; p < N; p += RANSAC_THREADS) {
    const size_t g = (size_t)pair * a.k_max + p;
    float Y[3] = {0.f, 0.f, 0.f};
    const bool ok = lift_point(lc, (double)a.coord_2d[g * 2 + 0], (double)a.coord_2d[g * 2 + 1], img, a.H, a.W, Y);
    for (int r = 0; r < 3; ++r) { X3[p * 3 + r] = a.coord_3d[g * 3 + r]; Y3[p * 3 + r] = Y[r]; }
    valid[p] = ok;
    nv += ok ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o, 64);
  if ((tid & 63) == 0) s_wave[tid >> 6] = nv;
  __syncthreads();
  const int num_valid = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  if (num_valid < a.min_corresp) { fail(0, num_valid); return; }  // block-uniform
  const double thr2 = tau * tau;
  const unsigned long long base = ransac_pair_base(a.seed, a.pair_keys, pair);

  // ---- all hypotheses, scored in parallel
  for (int h = tid; h < a.iters; h += RANSAC_THREADS) {
    Pose P;
    int c = 0;
    if (hypothesis(ransac_hypothesis_key(base, h), N, X3, Y3, valid, tau, &P))
      for (int p = 0; p < N; ++p) c += (valid[p] && resid2(P, X3 + p * 3, Y3 + p * 3) <= thr2) ? 1 : 0;
    cnt[h] = c;
  }
  __syncthreads();
  // ---- the sequential best-model rule with the adaptive iteration budget, replayed over the counts
  if (tid == 0) s_best = ransac_replay(cnt, a.iters, a.conf, 3, num_valid, &s_count);  // 3 model points, out of the valid correspondences
  __syncthreads();
  if (s_best < 0) { fail(0, num_valid); return; }
  if (tid == (s_best % RANSAC_THREADS)) {  // the owner regenerates the winning hypothesis (deterministic)
    Pose P;
    hypothesis(ransac_hypothesis_key(base, s_best), N, X3, Y3, valid, tau, &P);
    cur = P;
  }
  __syncthreads();
  ransac_write_winner(a, pair, tid, N, cur, inl, [&](int p) { return valid[p] && resid2(cur, X3 + p * 3, Y3 + p * 3) <= thr2; });
  __syncthreads();

  // ---- Horn's closed-form least-squares fit on the inliers
  if (a.refit) {
    double v[9];
    for (int i = 0; i < 6; ++i) v[i] = 0.0;
    for (int p = tid; p < N; p += RANSAC_THREADS) {
      if (!inl[p]) continue;
      for (int r = 0; r < 3; ++r) { v[r] += X3[p * 3 + r]; v[3 + r] += Y3[p * 3 + r]; }
    }
    block_sums<6>(v, acc, tot, tid);
    double mx[3], my[3];
    for (int r = 0; r < 3; ++r) { mx[r] = tot[r] / s_count; my[r] = tot[3 + r] / s_count; }
    __syncthreads();  // tot is read before the next reduction rewrites it
    for (int i = 0; i < 9; ++i) v[i] = 0.0;
    for (int p = tid; p < N; p += RANSAC_THREADS) {
      if (!inl[p]) continue;
      const double x[3] = {X3[p * 3 + 0] - mx[0], X3[p * 3 + 1] - mx[1], X3[p * 3 + 2] - mx[2]};
      const double y[3] = {Y3[p * 3 + 0] - my[0], Y3[p * 3 + 1] - my[1], Y3[p * 3 + 2] - my[2]};
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i * 3 + j] += x[i] * y[j];
    }
    block_sums<9>(v, acc, tot, tid);
    if (tid == 0) {
      const double Sxx = tot[0], Sxy = tot[1], Sxz = tot[2], Syx = tot[3], Syy = tot[4], Syz = tot[5], Szx = tot[6], Szy = tot[7], Szz = tot[8];
      double M[16] = {Sxx + Syy + Szz, Syz - Szy,       Szx - Sxz,        Sxy - Syx,
                      Syz - Szy,       Sxx - Syy - Szz, Sxy + Syx,        Szx + Sxz,
                      Szx - Sxz,       Sxy + Syx,       -Sxx + Syy - Szz, Syz + Szy,
                      Sxy - Syx,       Szx + Sxz,       Syz + Szy,        -Sxx - Syy + Szz};
      double q[4];
      jacobi4_largest(M, q);
      const double w = q[0], x = q[1], y = q[2], z = q[3];
      Pose P;
      P.R[0] = w * w + x * x - y * y - z * z; P.R[1] = 2.0 * (x * y - w * z);         P.R[2] = 2.0 * (x * z + w * y);
      P.R[3] = 2.0 * (x * y + w * z);         P.R[4] = w * w - x * x + y * y - z * z; P.R[5] = 2.0 * (y * z - w * x);
      P.R[6] = 2.0 * (x * z - w * y);         P.R[7] = 2.0 * (y * z + w * x);         P.R[8] = w * w - x * x - y * y + z * z;
      for (int i = 0; i < 3; ++i) P.t[i] = my[i] - (P.R[i * 3 + 0] * mx[0] + P.R[i * 3 + 1] * mx[1] + P.R[i * 3 + 2] * mx[2]);
      cur = P;
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.num_valid[pair] = num_valid;
    ransac_write_pose(a, pair, s_count, cur);
  }
}

}  // namespace

int launch_kabsch_ransac(const KabschArgs& a, int num_pairs, hipStream_t st) {
  FP_REQUIRE(a.k_max >= 3 && a.k_max <= KB_MAX_K, "kabsch_ransac: k_max must be in [3, %d] (got %d)", KB_MAX_K, a.k_max);
  FP_REQUIRE(a.iters >= 1 && a.iters <= KB_MAX_ITERS, "kabsch_ransac: iterations must be in [1, %d] (got %d)", KB_MAX_ITERS, a.iters);
  FP_REQUIRE(a.conf > 0.0 && a.conf <= 1.0, "kabsch_ransac: bad confidence");
  FP_REQUIRE(a.n_slots >= 1 && a.min_corresp >= 3, "kabsch_ransac: bad n_slots / min_corresp");
  FP_REQUIRE(a.num_images >= 1 && a.H >= 1 && a.W >= 1, "kabsch_ransac: %d depth images of %d x %d", a.num_images, a.W, a.H);
  if (num_pairs == 0) return FP_OK;
  const size_t lds = (size_t)a.k_max * 6 * 4 + (size_t)a.iters * 4 + (size_t)a.k_max * 2;
  static FpDeviceOnce attr;
  fp_allow_dynamic_lds(attr, &kabsch_ransac_kernel, KB_MAX_K * 6 * 4 + KB_MAX_ITERS * 4 + KB_MAX_K * 2);
  hipLaunchKernelGGL(kabsch_ransac_kernel, dim3(num_pairs), dim3(RANSAC_THREADS), lds, st, a);
  FP_CHECK_LAUNCH("kabsch_ransac");
  return FP_OK;
}
