"""numpy fp64 restatement of fp_kabsch_ransac's contract (include/foundpose_amd.h): the depth lift, the keyed
counter-based sampler in uint64 arithmetic, the congruence gate, the triangle-frame fit, the sequential best-model replay and Horn's
closed-form refit (largest eigenvector by numpy.linalg.eigh).  Plain loops: it is the yardstick of the tests, not a fast path.

Besides the results it returns `min_margin`: the smallest relative distance of any quantity it compared from its decision boundary
(squared residual against tau^2, edge-length difference against 2 tau, the projected depth pixel against a rounding tie -- the image
border is one --, the ray's z against 1e-9, and the adaptive budget's quotient against its rounding tie).  A fixture whose min_margin is
far above fp64 rounding noise has the same decisions in any correct fp64 implementation, whatever its summation order or FMA use.
"""

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
KEY_MUL = 0xD6E8FEB86659FD93
DBL_MIN = 2.2250738585072014e-308
MAX_REDRAWS = 64


def mix64(z: int) -> int:
    z = (z + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class Margin:
    def __init__(self):
        self.value = np.inf

    def add(self, rel):
        rel = float(np.min(rel)) if np.size(rel) else np.inf
        if rel < self.value:
            self.value = rel


def update_num_iters(p, ep, model_points, max_iters, margin=None):
    p = min(max(p, 0.0), 1.0)
    ep = min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < DBL_MIN:
        return 0
    num, denom = np.log(num), np.log(denom)
    if denom >= 0:
        return max_iters
    if margin is not None:
        margin.add(abs(-num - max_iters * (-denom)) / max(abs(num), 1e-300))
    if -num >= max_iters * (-denom):
        return max_iters
    x = num / denom
    if margin is not None:
        margin.add(abs(x - (np.floor(x) + 0.5)) / max(1.0, abs(x)))
    return int(np.rint(x))


def lift(uv, solve_cam, frame_cam, A, depth, margin=None):
    """uv [n, 2] (float32 pixels, solve camera) -> Y [n, 3] float32 (solve camera, mm), valid [n] bool.  fp64, every step one rounded
    operation in the stated order."""
    fx, fy, cx, cy = (np.float64(v) for v in solve_cam)
    ffx, ffy, fcx, fcy = (np.float64(v) for v in frame_cam)
    A = np.asarray(A, np.float64).reshape(3, 3)
    H, W = depth.shape
    n = len(uv)
    Y = np.zeros((n, 3), np.float32)
    valid = np.zeros(n, bool)
    for p in range(n):
        u, v = np.float64(uv[p, 0]), np.float64(uv[p, 1])
        dx, dy = (u - cx) / fx, (v - cy) / fy
        gx = (A[0, 0] * dx + A[0, 1] * dy) + A[0, 2]
        gy = (A[1, 0] * dx + A[1, 1] * dy) + A[1, 2]
        gz = (A[2, 0] * dx + A[2, 1] * dy) + A[2, 2]
        if margin is not None:
            margin.add(abs(gz - 1e-9) / max(abs(gz), 1e-9))
        if not gz > 1e-9:
            continue
        uf, vf = ffx * gx / gz + fcx, ffy * gy / gz + fcy
        if margin is not None:
            for x, size in ((uf, W), (vf, H)):
                if -1.0 <= x <= size:   # a tie decides the pixel (and, at -0.5 / size - 0.5, whether there is one)
                    margin.add(abs(x - (np.floor(x) + 0.5)) / max(1.0, abs(x)))
        px, py = np.rint(uf), np.rint(vf)
        if not (0.0 <= px <= W - 1 and 0.0 <= py <= H - 1):
            continue
        D = depth[int(py), int(px)]
        if not D > 0:
            continue
        s = np.float64(D) / gz
        Y[p] = (np.float32(s * dx), np.float32(s * dy), np.float32(s))
        valid[p] = True
    return Y, valid


def _normalize(a):
    n = np.sqrt(a @ a)
    return (a / n) if n > 1e-300 else None


def tri_frame(q0, q1, q2):
    e1 = _normalize(q1 - q0)
    if e1 is None:
        return None
    e3 = _normalize(np.cross(e1, q2 - q0))
    if e3 is None:
        return None
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)   # columns e1, e2, e3


def gate(X, Y, tau, margin=None):
    """The congruence gate on three correspondences X, Y [3, 3]."""
    ok = True
    for i in range(3):
        j = (i + 1) % 3
        diff = abs(np.linalg.norm(X[i] - X[j]) - np.linalg.norm(Y[i] - Y[j]))
        if margin is not None:
            margin.add(abs(diff - 2.0 * tau) / (2.0 * tau))
        ok &= bool(diff <= 2.0 * tau)
    return ok


def sample3(key: int, N: int, valid):
    ids, s = [], key
    for _ in range(3):
        attempt = 0
        while True:
            s = mix64(s)
            c = s % N
            if valid[c] and c not in ids:
                ids.append(c)
                break
            if attempt >= MAX_REDRAWS:
                return None
            attempt += 1
    return ids


def hypothesis(key, N, X, Y, valid, tau, margin=None):
    ids = sample3(key, N, valid)
    if ids is None:
        return None
    Xs, Ys = X[ids].astype(np.float64), Y[ids].astype(np.float64)
    if not gate(Xs, Ys, tau, margin):
        return None
    Fx, Fy = tri_frame(*Xs), tri_frame(*Ys)
    if Fx is None or Fy is None:
        return None
    R = Fy @ Fx.T
    t = Ys.sum(0) / 3.0 - R @ (Xs.sum(0) / 3.0)
    return R, t


def residuals2(R, t, X, Y):
    r = X.astype(np.float64) @ R.T + t - Y.astype(np.float64)
    return (r * r).sum(1)


def horn(X, Y):
    """Least-squares rigid fit Y ~ R X + t (Horn 1987, unit quaternion)."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    mx, my = X.mean(0), Y.mean(0)
    S = (X - mx).T @ (Y - my)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    Nm = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                   [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                   [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                   [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    w, x, y, z = np.linalg.eigh(Nm)[1][:, -1]
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
    return R, my - R @ mx


def kabsch_ransac_ref(coord_2d, coord_3d, counts, solve_cams, frame_cams, A, image_index, tau, depth, n_slots, iters, conf=0.99, refit=True,
                      seed=0, min_corresp=6, pair_keys=None):
    """coord_2d [P, K, 2] / coord_3d [P, K, 3] float32, counts [P]; per detection (P / n_slots): solve_cams / frame_cams [., 4], A [., 3, 3],
    image_index [.], tau [.]; depth [N, H, W] float32.  -> dict of arrays over the P pairs: success, num_valid, quality, inliers [P, K],
    best_h (-1: none), ransac_R / ransac_t (the winning hypothesis), R / t (the output pose), and min_margin (a float)."""
    coord_2d, coord_3d = np.asarray(coord_2d, np.float32), np.asarray(coord_3d, np.float32)
    P, K = coord_2d.shape[:2]
    out = {"success": np.zeros(P, bool), "num_valid": np.zeros(P, np.int64), "quality": np.zeros(P, np.int64), "inliers": np.zeros((P, K), bool),
           "best_h": np.full(P, -1, np.int64), "ransac_R": np.tile(np.eye(3), (P, 1, 1)), "ransac_t": np.zeros((P, 3)),
           "R": np.tile(np.eye(3), (P, 1, 1)), "t": np.zeros((P, 3))}
    margin = Margin()
    for pair in range(P):
        det = pair // n_slots
        N = int(min(max(int(counts[pair]), 0), K))
        th = float(tau[det])
        X = coord_3d[pair, :N]
        Y, valid = lift(coord_2d[pair, :N], solve_cams[det], frame_cams[det], A[det], depth[int(image_index[det])], margin)
        nv = int(valid.sum())
        out["num_valid"][pair] = nv
        if nv < min_corresp:
            continue
        key = pair if pair_keys is None else int(pair_keys[pair]) & M64
        base = mix64((seed & M64) ^ ((key * KEY_MUL) & M64))
        cnt = np.zeros(iters, np.int64)
        for h in range(iters):
            hyp = hypothesis((base + h * GOLDEN) & M64, N, X, Y, valid, th, margin)
            if hyp is None:
                continue
            d2 = residuals2(*hyp, X, Y)[valid]
            margin.add(np.abs(d2 - th * th) / (th * th))
            cnt[h] = int((d2 <= th * th).sum())
        best, best_c, niters, h = -1, 2, iters, 0
        while h < niters:
            if cnt[h] > best_c:
                best_c, best = int(cnt[h]), h
                niters = update_num_iters(conf, (nv - best_c) / nv, 3, niters, margin)
            h += 1
        if best < 0:
            continue
        R, t = hypothesis((base + best * GOLDEN) & M64, N, X, Y, valid, th)
        inl = valid & (residuals2(R, t, X, Y) <= th * th)
        out["success"][pair], out["quality"][pair], out["best_h"][pair] = True, best_c, best
        out["inliers"][pair, :N] = inl
        out["ransac_R"][pair], out["ransac_t"][pair] = R, t
        if refit:
            R, t = horn(X[inl], Y[inl])
        out["R"][pair], out["t"][pair] = R, t
    out["min_margin"] = margin.value
    return out


def rotation_angle(Ra, Rb):
    """Angle (rad) of Ra Rb^T, accurate near 0."""
    D = Ra @ Rb.T
    return float(np.arctan2(np.linalg.norm([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]) / 2.0, (np.trace(D) - 1.0) / 2.0))


# ---------------------------------------------------------------------------------------------------- planted scenes for the tests
def rot_xyz(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def plant_pair(rng, K, count, outlier_frac, solve_cam, frame_cam, A, depth, tau, R, t, extent=60.0, noise=0.2, holes=0, taken=None,
               keep_outside=False, write_depth=True):
    """One pair's correspondences for a planted pose (model -> solve camera), written INTO `depth` (the frame camera's image): `count`
    model points in a cube of +-extent mm; each one's pixel in the solve camera is rounded to float32 and its frame-camera depth pixel
    receives the depth that lifts to the planted point displaced along the ray by <= noise * tau (inliers) or by >= 5 tau (outliers, the
    first outlier_frac of a random order); `holes` inliers then lose their depth (0).  Points whose depth pixel is taken (`taken`: the
    set of (row, column) shared by the pairs that write into one image) are re-drawn, and so are points outside the image unless
    keep_outside: then they stay as correspondences without a measurement; write_depth=False reserves
    the pixels but leaves them 0 (a pair with no measurement at all).  -> coord_2d [K, 2], coord_3d [K, 3] float32, is_inlier [K] bool (false for holes and padding)."""
    H, W = depth.shape
    c2, c3, good = np.zeros((K, 2), np.float32), np.zeros((K, 3), np.float32), np.zeros(K, bool)
    n_out = int(round(outlier_frac * count))
    A = np.asarray(A, np.float64)
    fx, fy, cx, cy = solve_cam
    taken = set() if taken is None else taken
    p = 0
    inlier_pixels = []
    while p < min(count, K):
        X = rng.uniform(-extent, extent, 3).astype(np.float32)
        Yc = R @ X.astype(np.float64) + t
        uv = np.array([fx * Yc[0] / Yc[2] + cx, fy * Yc[1] / Yc[2] + cy]).astype(np.float32)
        d = np.array([(np.float64(uv[0]) - cx) / fx, (np.float64(uv[1]) - cy) / fy, 1.0])
        g = A @ d
        if g[2] <= 0.1:
            continue
        uf, vf = frame_cam[0] * g[0] / g[2] + frame_cam[2], frame_cam[1] * g[1] / g[2] + frame_cam[3]
        if min(abs(uf - np.floor(uf) - 0.5), abs(vf - np.floor(vf) - 0.5)) < 1e-3:
            continue
        px, py = int(np.rint(uf)), int(np.rint(vf))
        if not (0 <= px < W and 0 <= py < H):
            if keep_outside:
                c2[p], c3[p] = uv, X
                p += 1
            continue
        if (py, px) in taken:
            continue
        taken.add((py, px))
        along = np.linalg.norm(d)
        if p < n_out:
            shift = rng.choice([-1.0, 1.0]) * rng.uniform(5.5, 12.0) * tau
        else:
            shift = rng.uniform(-noise, noise) * tau
        # the lift returns s d with s = D / g.z: move the planted point by `shift` mm along its ray
        if write_depth:
            depth[py, px] = np.float32((Yc[2] + shift / along) * g[2])
        c2[p], c3[p], good[p] = uv, X, p >= n_out and write_depth
        if p >= n_out:
            inlier_pixels.append((p, py, px))
        p += 1
    for p, py, px in inlier_pixels[:holes]:
        depth[py, px] = 0.0
        good[p] = False
    return c2, c3, good


def camera_tuple(cam):
    return (float(cam.f[0]), float(cam.f[1]), float(cam.c[0]), float(cam.c[1]))


def gpu_fixture(seed=3):
    """The GPU tests' batch: 2 detections x 3 slots, K = 40, two 48 x 64 depth images that hold measurements only where a pair planted
    one.  Detection 0 solves in the frame's own camera (A = I); detection 1 in a crop camera that looks at a box near the right border
    (a rotated A), so its third pair has pixels that leave the frame image.  counts: K, 0, 5 (below min_corresp) | 57 (clamped to K), K
    with no depth under it, K.  -> dict: coord_2d / coord_3d / counts, solve / frame cameras, image_index, tau, depth, planted poses and
    inlier flags."""
    from foundpose_amd import crop_util
    rng = np.random.default_rng(seed)
    K, n = 40, 3
    Tw = np.eye(4)
    Tw[:3, :3], Tw[:3, 3] = rot_xyz(0.3, -0.2, 0.5), (120.0, -40.0, 800.0)
    frame = crop_util.PinholePlaneCameraModel(64, 48, (150.0, 152.0), (31.5, 23.5), Tw)
    crop = crop_util.construct_crop_camera(crop_util.AlignedBox2f(38.0, 12.0, 62.0, 36.0), frame, (100, 100), 0.2)
    solve, frames = [frame, crop], [frame, frame]
    rel = np.linalg.inv(frame.T_world_from_eye) @ crop.T_world_from_eye
    A = [np.eye(3), rel[:3, :3]]
    depth = np.zeros((2, 48, 64), np.float32)
    tau = [6.0, 4.5]
    counts = [K, 0, 5, 57, K, K]
    plan = [dict(outlier_frac=0.3, holes=3), None, dict(outlier_frac=0.0), dict(outlier_frac=0.5), dict(outlier_frac=0.2, write_depth=False),
            dict(outlier_frac=0.2, keep_outside=True, holes=2)]
    c2, c3 = np.zeros((6, K, 2), np.float32), np.zeros((6, K, 3), np.float32)
    good = np.zeros((6, K), bool)
    poses = []
    taken = [set(), set()]
    for pair, kw in enumerate(plan):
        det = pair // n
        R = rot_xyz(*rng.uniform(-np.pi, np.pi, 3))
        t = np.array([rng.uniform(-15, 15), rng.uniform(-10, 10), rng.uniform(560, 640)])
        if pair == 5:
            t[0] += 20.0   # towards the frame image's right border
        poses.append((R, t))
        if kw is None:
            continue
        c2[pair], c3[pair], good[pair] = plant_pair(rng, K, K, solve_cam=camera_tuple(solve[det]), frame_cam=camera_tuple(frames[det]), A=A[det],
                                                    depth=depth[det], tau=tau[det], R=R, t=t, taken=taken[det], **kw)
    return dict(coord_2d=c2, coord_3d=c3, counts=np.array(counts, np.int32), solve=solve, frames=frames, A=np.stack(A), image_index=[0, 1],
                tau=tau, depth=depth, poses=poses, good=good, n_slots=n, K=K, iters=300, seed=11)


def run_ref_on(fix, refit=True, pair_keys=None):
    return kabsch_ransac_ref(fix["coord_2d"], fix["coord_3d"], fix["counts"], [camera_tuple(c) for c in fix["solve"]],
                             [camera_tuple(c) for c in fix["frames"]], fix["A"], fix["image_index"], fix["tau"], fix["depth"], fix["n_slots"],
                             fix["iters"], 0.99, refit, fix["seed"], 6, pair_keys)
