// Batched 3D-3D RANSAC on depth-lifted correspondences (pnp_type "kabsch_depth"): the coarse pose of a
// (detection, template slot) pair from its 2D-3D correspondences AND the frame's depth image.  This stage is the project's own; the
// reference solves its coarse poses on pixels only.
//   lift    every correspondence's pixel (solve camera) -> ray -> frame camera (rotation A, the cameras share their centre) -> nearest
//           depth pixel -> the measured point Y in the SOLVE camera, so that poses come out model -> solve camera like fp_pnp_ransac's;
//   RANSAC  3 distinct valid correspondences per hypothesis (the sampler of pnp.hip), an edge-length congruence gate, the closed-form
//           fit R = F_Y F_X^T of the two triangle frames, t = mean(Y) - R mean(X); score = valid points within tau (mm) of their
//           measurement; all hypotheses in parallel, then pnp.hip's sequential best-model rule replayed over the counts (model_points 3);
//   refit   Horn's closed form on the winner's inliers: centroids and the cross-covariance by block reductions in a fixed order, the
//           largest eigenvector of the 4x4 quaternion matrix by cyclic Jacobi on one lane.
// One 256-thread workgroup per pair; arithmetic in fp64, points stored as fp32.  mix64, update_num_iters, normalize3 and tri_frame are
// copies of pnp.hip's (its device code stays untouched); every sum has a fixed order and there are no atomics, so a pair's result
// depends on (seed, key, its own data) only.
#include "common.hpp"
#include "kernels.hpp"
#include "rot.hpp"

namespace {

constexpr int KB_THREADS = 256;
constexpr int KB_MAX_ITERS = 4096;
constexpr int KB_MAX_K = 4096;
constexpr int KB_JACOBI_SWEEPS = 30;

struct Pose {
  double R[9];
  double t[3];
};

FP_DEVICE unsigned long long mix64(unsigned long long z) {  // splitmix64 finaliser (pnp.hip)
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

FP_DEVICE bool normalize3(double* a) {
  const double n = sqrt(dot3(a, a));
  if (!(n > 1e-300)) return false;
  a[0] /= n; a[1] /= n; a[2] /= n;
  return true;
}

// orthonormal frame of a triangle: e1 along Q1-Q0, e3 normal, e2 = e3 x e1 (columns of F) (pnp.hip)
FP_DEVICE bool tri_frame(const double* q0, const double* q1, const double* q2, double* F) {
  double e1[3] = {q1[0] - q0[0], q1[1] - q0[1], q1[2] - q0[2]};
  double d2[3] = {q2[0] - q0[0], q2[1] - q0[1], q2[2] - q0[2]};
  double e3[3], e2[3];
  if (!normalize3(e1)) return false;
  cross3(e1, d2, e3);
  if (!normalize3(e3)) return false;
  cross3(e3, e1, e2);
  for (int r = 0; r < 3; ++r) { F[r * 3 + 0] = e1[r]; F[r * 3 + 1] = e2[r]; F[r * 3 + 2] = e3[r]; }
  return true;
}

// RANSACUpdateNumIters of OpenCV's point-set registrator (pnp.hip)
FP_DEVICE int update_num_iters(double p, double ep, int model_points, int max_iters) {
  p = fmin(fmax(p, 0.0), 1.0);
  ep = fmin(fmax(ep, 0.0), 1.0);
  double num = fmax(1.0 - p, 2.2250738585072014e-308);
  double denom = 1.0 - pow(1.0 - ep, (double)model_points);
  if (denom < 2.2250738585072014e-308) return 0;
  num = log(num);
  denom = log(denom);
  return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

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

// hypothesis h of a pair: 3 distinct valid correspondences (an invalid or repeated index is drawn again, at most 64 times per index), the
// congruence gate, the triangle-frame fit
FP_DEVICE bool hypothesis(unsigned long long key, int N, const float* X3, const float* Y3, const unsigned char* valid, double tau, Pose* out) {
  int id[3];
  unsigned long long s = key;
  for (int j = 0; j < 3; ++j) {
    for (int attempt = 0;; ++attempt) {
      s = mix64(s);
      const int c = (int)(s % (unsigned long long)N);
      bool bad = !valid[c];
      for (int i = 0; i < j; ++i) bad |= id[i] == c;
      if (!bad) { id[j] = c; break; }
      if (attempt >= 64) return false;
    }
  }
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

// NV per-thread partial sums -> their block totals in out[] (lane 0 writes; fixed order: butterfly within a wave, then waves 0..3)
template <int NV>
FP_DEVICE void block_sums(double* v, double (*acc)[12], double* out, int tid) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double s = v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((tid & 63) == 0) acc[tid >> 6][i] = s;
  }
  __syncthreads();
  if (tid == 0)
    for (int i = 0; i < NV; ++i) out[i] = acc[0][i] + acc[1][i] + acc[2][i] + acc[3][i];
  __syncthreads();
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

__global__ __launch_bounds__(KB_THREADS) void kabsch_ransac_kernel(KabschArgs a) {
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
    if (tid == 0) {
      a.success[pair] = code;
      a.n_inliers[pair] = 0;
      a.num_valid[pair] = num_valid;
      for (int i = 0; i < 9; ++i) a.R[(size_t)pair * 9 + i] = (i % 4 == 0) ? 1.0 : 0.0;
      for (int i = 0; i < 3; ++i) a.t[(size_t)pair * 3 + i] = 0.0;
      if (a.ransac_pose) for (int i = 0; i < 12; ++i) a.ransac_pose[(size_t)pair * 12 + i] = 0.0;
    }
    for (int i = tid; i < a.k_max; i += KB_THREADS) a.inlier_mask[(size_t)pair * a.k_max + i] = 0;
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
  for (int p = tid; p < N; p += KB_THREADS) {
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
  const unsigned long long key = a.pair_keys ? a.pair_keys[pair] : (unsigned long long)pair;
  const unsigned long long base = mix64(a.seed ^ (key * 0xD6E8FEB86659FD93ull));

  // ---- all hypotheses, scored in parallel
  for (int h = tid; h < a.iters; h += KB_THREADS) {
    Pose P;
    int c = 0;
    if (hypothesis(base + (unsigned long long)h * 0x9E3779B97F4A7C15ull, N, X3, Y3, valid, tau, &P))
      for (int p = 0; p < N; ++p) c += (valid[p] && resid2(P, X3 + p * 3, Y3 + p * 3) <= thr2) ? 1 : 0;
    cnt[h] = c;
  }
  __syncthreads();
  // ---- the sequential best-model rule with the adaptive iteration budget, replayed over the counts
  if (tid == 0) {
    int best = -1, best_c = 2, niters = a.iters;  // a model must beat model_points - 1 = 2 inliers
    for (int h = 0; h < niters; ++h) {
      if (cnt[h] > best_c) {
        best_c = cnt[h];
        best = h;
        niters = update_num_iters(a.conf, (double)(num_valid - best_c) / num_valid, 3, niters);
      }
    }
    s_best = best;
    s_count = best_c;
  }
  __syncthreads();
  if (s_best < 0) { fail(0, num_valid); return; }
  if (tid == (s_best % KB_THREADS)) {  // the owner regenerates the winning hypothesis (deterministic)
    Pose P;
    hypothesis(base + (unsigned long long)s_best * 0x9E3779B97F4A7C15ull, N, X3, Y3, valid, tau, &P);
    cur = P;
  }
  __syncthreads();
  for (int p = tid; p < a.k_max; p += KB_THREADS) {
    const unsigned char m = p < N && valid[p] && resid2(cur, X3 + p * 3, Y3 + p * 3) <= thr2;
    if (p < N) inl[p] = m;
    a.inlier_mask[(size_t)pair * a.k_max + p] = m;
  }
  if (tid == 0 && a.ransac_pose) {
    for (int i = 0; i < 9; ++i) a.ransac_pose[(size_t)pair * 12 + i] = cur.R[i];
    for (int i = 0; i < 3; ++i) a.ransac_pose[(size_t)pair * 12 + 9 + i] = cur.t[i];
  }
  __syncthreads();

  // ---- Horn's closed-form least-squares fit on the inliers
  if (a.refit) {
    double v[9];
    for (int i = 0; i < 6; ++i) v[i] = 0.0;
    for (int p = tid; p < N; p += KB_THREADS) {
      if (!inl[p]) continue;
      for (int r = 0; r < 3; ++r) { v[r] += X3[p * 3 + r]; v[3 + r] += Y3[p * 3 + r]; }
    }
    block_sums<6>(v, acc, tot, tid);
    double mx[3], my[3];
    for (int r = 0; r < 3; ++r) { mx[r] = tot[r] / s_count; my[r] = tot[3 + r] / s_count; }
    __syncthreads();  // tot is read before the next reduction rewrites it
    for (int i = 0; i < 9; ++i) v[i] = 0.0;
    for (int p = tid; p < N; p += KB_THREADS) {
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
    a.success[pair] = 1;
    a.n_inliers[pair] = s_count;
    a.num_valid[pair] = num_valid;
    for (int i = 0; i < 9; ++i) a.R[(size_t)pair * 9 + i] = cur.R[i];
    for (int i = 0; i < 3; ++i) a.t[(size_t)pair * 3 + i] = cur.t[i];
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
  hipLaunchKernelGGL(kabsch_ransac_kernel, dim3(num_pairs), dim3(KB_THREADS), lds, st, a);
  FP_CHECK_LAUNCH("kabsch_ransac");
  return FP_OK;
}
