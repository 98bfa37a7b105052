"""numpy fp64 restatement of fp_kabsch_ransac's contract (include/foundpose_amd.h): the depth lift, the keyed
counter-based sampler in uint64 arithmetic, the congruence gate, the triangle-frame fit, the sequential best-model replay and Horn's
closed-form refit (largest eigenvector by numpy.linalg.eigh).  Plain loops: it is the yardstick of the tests, not a fast path.

Besides the results it returns `min_margin`: the smallest relative distance of any quantity it compared from its decision boundary
(squared residual against tau^2, edge-length difference against 2 tau, the projected depth pixel against a rounding tie -- the image
border is one --, the ray's z against 1e-9, the adaptive budget's quotient against its rounding tie, and the two norms of either triangle
frame relative to the triangle's longest edge, an exact zero excepted: tri_frame).  A fixture whose min_margin is
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
        rel = np.asarray(rel, np.float64).reshape(-1)
        rel = rel[~np.isnan(rel)]   # a NaN operand (a point lifted from a depth of +inf) fails every comparison, in any order of evaluation
        rel = float(rel.min()) if rel.size else np.inf
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


def lift(uv, solve_cam, frame_cam, A, depth, margin=None, tie_margin=True):
    """uv [n, 2] (float32 pixels, solve camera) -> Y [n, 3] float32 (solve camera, mm), valid [n] bool.  fp64, every step one rounded
    operation in the stated order.  tie_margin=False leaves the rounding-tie margin out: only for a fixture whose projected pixels are
    exact in fp64 (A = I, one camera, power-of-two focal length), where a tie is a representable input and not a rounding accident."""
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
        if margin is not None and tie_margin:
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


def tri_frame(q0, q1, q2, margin=None):
    """The margin of the two degeneracy tests: each norm (the first edge; the triangle's height over it, |e1 x (q2 - q0)|) relative to
    the triangle's longest edge.  Only an EXACT zero is exempt: it is planted (integer coordinates on a coordinate axis, where the unit
    vector and every product of the cross product are exact whatever the order or the contraction), never a rounding accident."""
    a, b = q1 - q0, q2 - q0
    if margin is not None:
        longest = max(np.sqrt(a @ a), np.sqrt(b @ b), np.sqrt((q2 - q1) @ (q2 - q1)))
        n1 = np.sqrt(a @ a)
        if n1 != 0.0:
            margin.add(n1 / longest)
    e1 = _normalize(a)
    if e1 is None:
        return None
    c = np.cross(e1, b)
    if margin is not None:
        n3 = np.sqrt(c @ c)
        if n3 != 0.0:
            margin.add(n3 / longest)
    e3 = _normalize(c)
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


EXHAUSTED = -1   # in `draws`: the index used up its 1 + MAX_REDRAWS draws; 0: it was never reached


def sample3_draws(key: int, N: int, valid):
    """-> (the three indices or None, [draws of index 0, 1, 2]): an index takes 1 .. 1 + MAX_REDRAWS draws."""
    ids, s, draws = [], key, [0, 0, 0]
    for j in range(3):
        attempt = 0
        while True:
            s = mix64(s)
            c = s % N
            if valid[c] and c not in ids:
                ids.append(c)
                draws[j] = attempt + 1
                break
            if attempt >= MAX_REDRAWS:
                draws[j] = EXHAUSTED
                return None, draws
            attempt += 1
    return ids, draws


def sample3(key: int, N: int, valid):
    return sample3_draws(key, N, valid)[0]


def hypothesis_ex(key, N, X, Y, valid, tau, margin=None):
    """-> (pose (R, t) or None, the stage that decided: "exhausted" | "gate" | "degenerate" | "fit", draws)."""
    ids, draws = sample3_draws(key, N, valid)
    if ids is None:
        return None, "exhausted", draws
    Xs, Ys = X[ids].astype(np.float64), Y[ids].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):   # a point lifted from a depth of +inf: its edges are inf or NaN and fail the gate
        ok = gate(Xs, Ys, tau, margin)
    if not ok:
        return None, "gate", draws
    Fx, Fy = tri_frame(*Xs, margin), tri_frame(*Ys, margin)
    if Fx is None or Fy is None:
        return None, "degenerate", draws
    R = Fy @ Fx.T
    t = Ys.sum(0) / 3.0 - R @ (Xs.sum(0) / 3.0)
    return (R, t), "fit", draws


def hypothesis(key, N, X, Y, valid, tau, margin=None):
    return hypothesis_ex(key, N, X, Y, valid, tau, margin)[0]


def residuals2(R, t, X, Y):
    r = X.astype(np.float64) @ R.T + t - Y.astype(np.float64)
    return (r * r).sum(1)


def horn(X, Y, with_gap=False):
    """Least-squares rigid fit Y ~ R X + t (Horn 1987, unit quaternion)."""
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    mx, my = X.mean(0), Y.mean(0)
    S = (X - mx).T @ (Y - my)
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = S
    Nm = np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                   [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                   [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                   [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])
    lam, vec = np.linalg.eigh(Nm)
    w, x, y, z = vec[:, -1]
    R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
    if with_gap:   # the rotation is defined as far as the largest eigenvalue is separated: the gap relative to the spectrum's size
        return R, my - R @ mx, float((lam[-1] - lam[-2]) / max(np.abs(lam).max(), 1e-300))
    return R, my - R @ mx


def kabsch_ransac_ref(coord_2d, coord_3d, counts, solve_cams, frame_cams, A, image_index, tau, depth, n_slots, iters, conf=0.99, refit=True,
                      seed=0, min_corresp=6, pair_keys=None, cache=None, tie_margin=True):
    """coord_2d [P, K, 2] / coord_3d [P, K, 3] float32, counts [P]; per detection (P / n_slots): solve_cams / frame_cams [., 4], A [., 3, 3],
    image_index [.], tau [.]; depth [N, H, W] float32.  -> dict of arrays over the P pairs: success, num_valid, quality, inliers [P, K],
    best_h (-1: none), ransac_R / ransac_t (the winning hypothesis), R / t (the output pose), and min_margin (a float); per hypothesis
    cnt [P, iters], stage (what decided it: hypothesis_ex) and draws [P, iters, 3] (the draws each index took, EXHAUSTED, or 0 = not
    reached); niters_final and budget_steps (the replay's budget at its end, and how often it shrank); eig_gap (the relative gap between
    the two largest eigenvalues of Horn's matrix for the winner's inliers; NaN without a refit); base (a list: the pair's sampler
    base, hypothesis h has the key base + h * GOLDEN).
    cache: a dict the caller keeps for ONE fixture (same cameras, depth and tau): pairs with the same pixels share a lift, pairs with
    the same data and key share their counts -- a scene replicated over thousands of pairs, or replayed at another confidence, costs
    its hypotheses once.  tie_margin: lift()'s."""
    coord_2d, coord_3d = np.asarray(coord_2d, np.float32), np.asarray(coord_3d, np.float32)
    P, K = coord_2d.shape[:2]
    out = {"success": np.zeros(P, bool), "num_valid": np.zeros(P, np.int64), "quality": np.zeros(P, np.int64), "inliers": np.zeros((P, K), bool),
           "best_h": np.full(P, -1, np.int64), "ransac_R": np.tile(np.eye(3), (P, 1, 1)), "ransac_t": np.zeros((P, 3)),
           "R": np.tile(np.eye(3), (P, 1, 1)), "t": np.zeros((P, 3)), "cnt": np.zeros((P, iters), np.int64), "stage": np.full((P, iters), "", "U10"),
           "draws": np.zeros((P, iters, 3), np.int64), "niters_final": np.full(P, iters, np.int64), "budget_steps": np.zeros(P, np.int64),
           "eig_gap": np.full(P, np.nan), "base": [0] * P}
    margin = Margin()
    cache = {} if cache is None else cache
    for pair in range(P):
        det = pair // n_slots
        N = int(min(max(int(counts[pair]), 0), K))
        th = float(tau[det])
        X = coord_3d[pair, :N]
        lift_key = ("lift", det, int(image_index[det]), coord_2d[pair, :N].tobytes(), tie_margin)
        if lift_key not in cache:
            m = Margin()
            cache[lift_key] = lift(coord_2d[pair, :N], solve_cams[det], frame_cams[det], A[det], depth[int(image_index[det])], m, tie_margin) + (m.value,)
        Y, valid, m = cache[lift_key]
        margin.add(m)
        nv = int(valid.sum())
        out["num_valid"][pair] = nv
        if nv < min_corresp:
            continue
        key = pair if pair_keys is None else int(pair_keys[pair]) & M64
        base = out["base"][pair] = mix64((seed & M64) ^ ((key * KEY_MUL) & M64))
        cnt_key = ("cnt", lift_key, X.tobytes(), base, iters, th)
        if cnt_key not in cache:
            m = Margin()
            cnt, stage, draws = np.zeros(iters, np.int64), np.full(iters, "", "U10"), np.zeros((iters, 3), np.int64)
            for h in range(iters):
                hyp, stage[h], draws[h] = hypothesis_ex((base + h * GOLDEN) & M64, N, X, Y, valid, th, m)
                if hyp is None:
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    d2 = residuals2(*hyp, X, Y)[valid]
                    m.add(np.abs(d2 - th * th) / (th * th))
                    cnt[h] = int((d2 <= th * th).sum())
            cache[cnt_key] = (cnt, stage, draws, m.value)
        cnt, out["stage"][pair], out["draws"][pair], m = cache[cnt_key]
        margin.add(m)
        out["cnt"][pair] = cnt
        best, best_c, niters, h = -1, 2, iters, 0
        while h < niters:
            if cnt[h] > best_c:
                best_c, best = int(cnt[h]), h
                shrunk = update_num_iters(conf, (nv - best_c) / nv, 3, niters, margin)
                out["budget_steps"][pair] += shrunk < niters
                niters = shrunk
            h += 1
        out["niters_final"][pair] = niters
        if best < 0:
            continue
        R, t = hypothesis((base + best * GOLDEN) & M64, N, X, Y, valid, th)
        with np.errstate(invalid="ignore", over="ignore"):
            inl = valid & (residuals2(R, t, X, Y) <= th * th)
        out["success"][pair], out["quality"][pair], out["best_h"][pair] = True, best_c, best
        out["inliers"][pair, :N] = inl
        out["ransac_R"][pair], out["ransac_t"][pair] = R, t
        if refit:
            R, t, out["eig_gap"][pair] = horn(X[inl], Y[inl], with_gap=True)
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
               keep_outside=False, write_depth=True, model_points=None, shape=(1.0, 1.0, 1.0)):
    """One pair's correspondences for a planted pose (model -> solve camera), written INTO `depth` (the frame camera's image): `count`
    model points in a cube of +-extent mm; each one's pixel in the solve camera is rounded to float32 and its frame-camera depth pixel
    receives the depth that lifts to the planted point displaced along the ray by <= noise * tau (inliers) or by >= 5 tau (outliers, the
    first outlier_frac of a random order); `holes` inliers then lose their depth (0).  Points whose depth pixel is taken (`taken`: the
    set of (row, column) shared by the pairs that write into one image) are re-drawn, and so are points outside the image unless
    keep_outside: then they stay as correspondences without a measurement; write_depth=False reserves
    the pixels but leaves them 0 (a pair with no measurement at all).  model_points {index: (x, y, z)} gives those indices their model
    point (planted where it falls, or ValueError); `shape` scales the drawn cube per axis ((1, 1, 0): coplanar model points).
    -> coord_2d [K, 2], coord_3d [K, 3] float32, is_inlier [K] bool (false for holes and padding)."""
    H, W = depth.shape
    c2, c3, good = np.zeros((K, 2), np.float32), np.zeros((K, 3), np.float32), np.zeros(K, bool)
    n_out = int(round(outlier_frac * count))
    A = np.asarray(A, np.float64)
    fx, fy, cx, cy = solve_cam
    taken = set() if taken is None else taken
    p = 0
    inlier_pixels = []
    given = {} if model_points is None else model_points
    tried = None
    while p < min(count, K):
        if p in given:   # a given model point keeps its index: it is planted where it falls or not at all
            if tried == p:
                raise ValueError(f"the given model point {p} cannot be planted (a tie, a taken pixel or outside the image)")
            tried = p
            X = np.asarray(given[p], np.float32)
        else:
            X = (rng.uniform(-extent, extent, 3) * np.asarray(shape, np.float64)).astype(np.float32)
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


def run_ref_on(fix, refit=True, pair_keys=None, conf=0.99, cache=None):
    keys = None if pair_keys is None else np.asarray(pair_keys).reshape(-1)
    return kabsch_ransac_ref(fix["coord_2d"], fix["coord_3d"], fix["counts"], [camera_tuple(c) for c in fix["solve"]],
                             [camera_tuple(c) for c in fix["frames"]], fix["A"], fix["image_index"], fix["tau"], fix["depth"], fix["n_slots"],
                             fix["iters"], conf, refit, fix["seed"], 6, keys, cache, fix.get("tie_margin", True))


# ------------------------------------------------------------------------------------------------ device against restatement, per pair
BARS = dict(hyp_rad=1e-9, hyp_mm=1e-6, rad=1e-6, mm=1e-3, rot=1e-12)   # DESIGN.md sections 16 and 11


def compare(dev, ref, refit=True):
    """dev: solve_kabsch_ransac_batch's dict with ransac_pose, as numpy arrays with the pairs flattened; ref: kabsch_ransac_ref's.
    -> (mismatches [(pair, what)], figures): success, num_valid, quality and the masks must be EQUAL, a failed pair must carry the
    failure record, the winning hypothesis / output pose must be within BARS and R a rotation.  Without refit the output pose must be
    the winning hypothesis, bit for bit."""
    bad = []
    fig = dict(hyp_rad=0.0, hyp_mm=0.0, rad=0.0, mm=0.0, rot=0.0, solved=0)
    for p in range(len(ref["success"])):
        for k in ("success", "num_valid"):
            if dev[k][p] != ref[k][p]:
                bad.append((p, k))
        if dev["quality"][p] != float(ref["quality"][p]):
            bad.append((p, "quality"))
        if not np.array_equal(dev["inliers"][p], ref["inliers"][p]):
            bad.append((p, "inliers"))
        R, t, rp = dev["R"][p], dev["t"][p], dev["ransac_pose"][p]
        if not ref["success"][p]:
            if not (np.array_equal(R, np.eye(3)) and not t.any() and not rp.any() and not dev["inliers"][p].any() and dev["quality"][p] == 0):
                bad.append((p, "failure record"))
            continue
        fig["solved"] += 1
        if not (np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(rp).all()):
            bad.append((p, "not finite"))
            continue
        f = dict(hyp_rad=rotation_angle(rp[:9].reshape(3, 3), ref["ransac_R"][p]), hyp_mm=float(np.abs(rp[9:] - ref["ransac_t"][p]).max()),
                 rad=rotation_angle(R, ref["R"][p]), mm=float(np.abs(t - ref["t"][p]).max()),
                 rot=max(abs(np.linalg.det(R) - 1.0), float(np.abs(R @ R.T - np.eye(3)).max())))
        for k, v in f.items():
            fig[k] = max(fig[k], v)
            if not v < (BARS["hyp_" + k] if not refit and k in ("rad", "mm") else BARS[k]):
                bad.append((p, f"{k} {v:.3e}"))
        if not refit and not (np.array_equal(R.reshape(9), rp[:9]) and np.array_equal(t, rp[9:])):
            bad.append((p, "output is not the winning hypothesis"))
    return bad, fig


def as_device(ref):
    """A restatement's result in the layout compare() takes as the device's: what a device that agreed exactly would return."""
    rp = np.concatenate([ref["ransac_R"].reshape(-1, 9), ref["ransac_t"]], 1)
    rp[~ref["success"]] = 0.0
    return dict(ref, quality=ref["quality"].astype(np.float64), ransac_pose=rp)


def figures(fig):
    return (f"{fig['solved']} solved; winning hypothesis {fig['hyp_rad']:.3e} rad / {fig['hyp_mm']:.3e} mm, output pose {fig['rad']:.3e} rad / "
            f"{fig['mm']:.3e} mm, |det R - 1| and |R R^T - I| at most {fig['rot']:.3e}")


# ------------------------------------------------------------------------------------- fixtures of tests/test_gpu_kabsch_restatement.py
# Every seed and key below was searched on the CPU with the restatement until the fixture's conditions held (the *_conditions functions
# return the violations; tests/test_kabsch_cpu.py asserts there are none).
MIN_MARGIN = 1e-6


def _camera(W, H, f, c):
    from foundpose_amd import crop_util
    Tw = np.eye(4)
    Tw[:3, :3], Tw[:3, 3] = rot_xyz(0.3, -0.2, 0.5), (120.0, -40.0, 800.0)
    return crop_util.PinholePlaneCameraModel(W, H, f, c, Tw)


def _pose(rng, z=(560.0, 640.0)):
    return rot_xyz(*rng.uniform(-np.pi, np.pi, 3)), np.array([rng.uniform(-15, 15), rng.uniform(-10, 10), rng.uniform(*z)])


def _shuffle(rng, count, *arrays):
    """The first `count` rows of every array in one random order (plant_pair puts the outliers first)."""
    perm = rng.permutation(count)
    for a in arrays:
        a[:count] = a[:count][perm]


def _single_scene(c2, c3, good, K, count, P, cam, depth, tau, poses, iters, seed, **extra):
    """One scene replicated over P pairs of one detection (B = 1, n_slots = P; A = I)."""
    return dict(coord_2d=np.tile(c2[None], (P, 1, 1)), coord_3d=np.tile(c3[None], (P, 1, 1)), counts=np.full(P, count, np.int32), solve=[cam],
                frames=[cam], A=np.eye(3)[None], image_index=[0], tau=[tau], depth=depth, poses=poses, good=np.tile(good[None], (P, 1)), n_slots=P,
                K=K, iters=iters, seed=seed, **extra)


def _margin_violation(ref):
    return [] if ref["min_margin"] > MIN_MARGIN else [f"min_margin {ref['min_margin']:.3e} <= {MIN_MARGIN}"]


# ---- 1. hypothesis sweep
SWEEP_SEED = (4, 21)          # (scene, sampler)
SWEEP_LINE = 8                # model points 40..47 lie on the x axis at integer coordinates: their X triangles are EXACTLY degenerate


def sweep_fixture(P=4096, scene_seed=None, seed=None):
    """K = N = 48 in a 48 x 64 image, 30 % gross outliers, 4 holes; 4 096 pairs with keys 0..P-1 and ONE iteration each, refit off: every
    pair exposes hypothesis 0 of its key."""
    scene_seed, seed = SWEEP_SEED[0] if scene_seed is None else scene_seed, SWEEP_SEED[1] if seed is None else seed
    rng = np.random.default_rng(scene_seed)
    K, tau = 48, 6.0
    cam = _camera(64, 48, (150.0, 152.0), (31.5, 23.5))
    depth = np.zeros((1, 48, 64), np.float32)
    R, t = _pose(rng)
    line = {K - SWEEP_LINE + i: (-56.0 + 16.0 * i, 0.0, 0.0) for i in range(SWEEP_LINE)}
    c2, c3, good = plant_pair(rng, K, K, 0.3, camera_tuple(cam), camera_tuple(cam), np.eye(3), depth[0], tau, R, t, holes=4, model_points=line)
    return _single_scene(c2, c3, good, K, K, P, cam, depth, tau, [(R, t)], 1, seed, pair_keys=np.arange(P, dtype=np.int64))


def sweep_classes(ref):
    """The sweep's hypotheses (hypothesis 0 of every pair) by what decided them."""
    stage, cnt = ref["stage"][:, 0], ref["cnt"][:, 0]
    return dict(exhausted=int((stage == "exhausted").sum()), gate=int((stage == "gate").sum()), degenerate=int((stage == "degenerate").sum()),
                models=int((cnt > 2).sum()), fit_without_model=int(((stage == "fit") & (cnt <= 2)).sum()))


def sweep_conditions(fix, ref):
    c, v = sweep_classes(ref), _margin_violation(ref)
    if c["gate"] < 200:
        v.append(f"only {c['gate']} hypotheses rejected by the gate")
    if c["models"] < 200:
        v.append(f"only {c['models']} models")
    if c["degenerate"] < 8:
        v.append(f"only {c['degenerate']} hypotheses pass the gate and fail on the degenerate triangle")
    if not np.array_equal(ref["success"], ref["cnt"][:, 0] > 2):
        v.append("a pair's success is not its hypothesis' count > 2")
    X = fix["coord_3d"][0, fix["K"] - SWEEP_LINE:].astype(np.float64)
    if not (np.all(X[:, 1:] == 0) and np.all(X[:, 0] == np.rint(X[:, 0])) and fix["good"][0, fix["K"] - SWEEP_LINE:].all()):
        v.append("the collinear model points are not integers on the x axis, or not all inliers")
    return v


# ---- 2. sparse validity: the sampler's redraw limit
SPARSE_SEED = (4, 2)
SPARSE_VALID = 8


def sparse_fixture(P=2048, scene_seed=None, seed=None):
    """K = N = 256 of which 8 have depth under them (inliers of one pose; the rest tap zeros), 2 048 pairs with one iteration each: a draw
    is accepted with probability ~ 1/32, so indices run into the limit of 1 + 64 draws -- and some succeed on the last one."""
    scene_seed, seed = SPARSE_SEED[0] if scene_seed is None else scene_seed, SPARSE_SEED[1] if seed is None else seed
    rng = np.random.default_rng(scene_seed)
    K, tau = 256, 6.0
    cam = _camera(64, 48, (150.0, 152.0), (31.5, 23.5))
    depth = np.zeros((1, 48, 64), np.float32)
    R, t = _pose(rng)
    c2, c3, good = plant_pair(rng, K, K, 0.0, camera_tuple(cam), camera_tuple(cam), np.eye(3), depth[0], tau, R, t, holes=K - SPARSE_VALID)
    _shuffle(rng, K, c2, c3, good)
    return _single_scene(c2, c3, good, K, K, P, cam, depth, tau, [(R, t)], 1, seed, pair_keys=np.arange(P, dtype=np.int64))


def sparse_classes(ref):
    d = ref["draws"][:, 0]
    return dict(exhausted=int((d == EXHAUSTED).any(1).sum()), on_the_last_draw=int(((d == 1 + MAX_REDRAWS).any(1) & (d > 0).all(1)).sum()),
                models=int((ref["cnt"][:, 0] > 2).sum()))


def sparse_conditions(fix, ref):
    c, v = sparse_classes(ref), _margin_violation(ref)
    if not (ref["num_valid"] == SPARSE_VALID).all() or int(fix["good"][0].sum()) != SPARSE_VALID:
        v.append("not exactly 8 valid correspondences, all inliers")
    if c["exhausted"] < 20:
        v.append(f"only {c['exhausted']} hypotheses exhaust an index")
    if c["on_the_last_draw"] < 3:
        v.append(f"only {c['on_the_last_draw']} hypotheses succeed on the last allowed draw of an index")
    if c["models"] < 200:
        v.append(f"only {c['models']} models")
    return v


# ---- 3. the replay at sizes that stride
STRIDE_SEED = (1, (1 << 63) + 777)
STRIDE_KEYS = [[-(1 << 63) + 5, 7, 11], [-1, 3, (1 << 40) + 1]]    # int64: the first of either detection has the top bit set
STRIDE_COUNTS = [700, 300, 257, 64, 757, 700]
STRIDE_CONFS = (0.99, 0.5)
TIE_MM = 1.0    # "whole millimetres": a tying hypothesis moves some model point of the pair by at least this much


def stride_fixture(scene_seed=None, seed=None):
    """2 detections (A = I; a crop camera with a rotated A) x 3 slots, K = 700, two 120 x 160 depth images, 1 024 hypotheses; counts 700,
    300, 257 | 64, 757 (clamped to K), 700 with 70 % outliers; every pair's correspondences in random order."""
    from foundpose_amd import crop_util
    scene_seed, seed = STRIDE_SEED[0] if scene_seed is None else scene_seed, STRIDE_SEED[1] if seed is None else seed
    rng = np.random.default_rng(scene_seed)
    K, n = 700, 3
    frame = _camera(160, 120, (400.0, 402.0), (79.5, 59.5))
    crop = crop_util.construct_crop_camera(crop_util.AlignedBox2f(50.0, 10.0, 150.0, 110.0), frame, (200, 200), 0.2)
    solve, frames = [frame, crop], [frame, frame]
    rel = np.linalg.inv(frame.T_world_from_eye) @ crop.T_world_from_eye
    A = [np.eye(3), rel[:3, :3]]
    depth = np.zeros((2, 120, 160), np.float32)
    tau = [6.0, 4.5]
    plan = [dict(outlier_frac=0.3, holes=5), dict(outlier_frac=0.45), dict(outlier_frac=0.2, holes=3), dict(outlier_frac=0.5), dict(outlier_frac=0.6),
            dict(outlier_frac=0.7)]
    c2, c3, good = np.zeros((6, K, 2), np.float32), np.zeros((6, K, 3), np.float32), np.zeros((6, K), bool)
    poses, taken = [], [set(), set()]
    for pair, kw in enumerate(plan):
        det = pair // n
        R, t = _pose(rng)
        if det == 1:
            t[0] += 30.0    # towards the crop's box
        poses.append((R, t))
        count = min(STRIDE_COUNTS[pair], K)
        c2[pair], c3[pair], good[pair] = plant_pair(rng, K, count, solve_cam=camera_tuple(solve[det]), frame_cam=camera_tuple(frames[det]), A=A[det],
                                                    depth=depth[det], tau=tau[det], R=R, t=t, taken=taken[det], noise=0.5, **kw)
        _shuffle(rng, count, c2[pair], c3[pair], good[pair])
    return dict(coord_2d=c2, coord_3d=c3, counts=np.array(STRIDE_COUNTS, np.int32), solve=solve, frames=frames, A=np.stack(A), image_index=[0, 1],
                tau=tau, depth=depth, poses=poses, good=good, n_slots=n, K=K, iters=1024, seed=seed)


def _moved(fix, pair, ref, h):
    """How far (mm, the largest over the pair's model points) hypothesis h of the pair is from the winner."""
    det = pair // fix["n_slots"]
    N = int(min(fix["counts"][pair], fix["K"]))
    X = fix["coord_3d"][pair, :N].astype(np.float64)
    Y, valid = lift(fix["coord_2d"][pair, :N], camera_tuple(fix["solve"][det]), camera_tuple(fix["frames"][det]), fix["A"][det],
                    fix["depth"][fix["image_index"][det]])
    R, t = hypothesis((ref["base"][pair] + h * GOLDEN) & M64, N, fix["coord_3d"][pair, :N], Y, valid, fix["tau"][det])
    return float(np.linalg.norm((X @ R.T + t) - (X @ ref["ransac_R"][pair].T + ref["ransac_t"][pair]), axis=1).max())


def stride_facts(fix, refs):
    """refs: {(conf, keyed): ref}.  -> dict of the replay's witnesses over all runs: (conf, keyed, pair, ...) tuples."""
    facts = dict(beyond=[], ties=[], shrinks=[])
    for (conf, keyed), ref in refs.items():
        for p in np.nonzero(ref["success"])[0]:
            cnt, nf, b = ref["cnt"][p], int(ref["niters_final"][p]), int(ref["best_h"][p])
            if (cnt[nf:] > cnt[b]).any():
                facts["beyond"].append((conf, keyed, int(p), nf + int(np.argmax(cnt[nf:] > cnt[b]))))
            for h in np.nonzero(cnt[b + 1:nf] == cnt[b])[0][:3] + b + 1:
                d = _moved(fix, p, ref, int(h))
                if d >= TIE_MM:
                    facts["ties"].append((conf, keyed, int(p), int(h), d))
                    break
            if ref["budget_steps"][p] >= 3:
                facts["shrinks"].append((conf, keyed, int(p), int(ref["budget_steps"][p])))
    return facts


def stride_conditions(fix, refs):
    v = []
    for run, ref in refs.items():
        v += [f"{run}: {m}" for m in _margin_violation(ref)]
        if ref["success"].tolist() != [True] * 6 or (ref["num_valid"] < 60).any():
            v.append(f"{run}: not every pair is solved")
        for p in range(6):
            idx = np.nonzero(ref["inliers"][p])[0]
            waves = set(((idx % 256) // 64).tolist())
            # 64 correspondences are exactly wave 0's lanes, full: that count's witness is the empty waves 1..3 beside a full one
            if waves != ({0} if fix["counts"][p] == 64 else {0, 1, 2, 3}):
                v.append(f"{run}: pair {p}'s inliers sit in the waves {sorted(waves)}")
        if not (np.nonzero(ref["inliers"][0])[0] >= 512).any() or min(fix["counts"][0], fix["K"]) % 256 == 0:
            v.append(f"{run}: pair 0 has no inlier in a ragged third trip")
    facts = stride_facts(fix, refs)
    for k, what in (("beyond", "no better hypothesis beyond the final budget"), ("ties", "no visited later hypothesis ties the winner's count, whole mm away"),
                    ("shrinks", "no budget shrinks in three or more steps")):
        if not facts[k]:
            v.append(what)
    a, b = refs[(0.99, False)], refs[(0.5, False)]
    if np.array_equal(a["best_h"], b["best_h"]):
        v.append("the two confidences choose the same winners")
    if np.array_equal(refs[(0.99, False)]["best_h"], refs[(0.99, True)]["best_h"]) and np.allclose(refs[(0.99, False)]["ransac_t"], refs[(0.99, True)]["ransac_t"]):
        v.append("the keys do not change the winners")
    return v


def stride_refs(fix, cache=None):
    cache = {} if cache is None else cache
    return {(conf, keyed): run_ref_on(fix, True, STRIDE_KEYS if keyed else None, conf, cache) for conf in STRIDE_CONFS for keyed in (False, True)}


# ---- 4. a winner at h >= 256
LATE_SEED = (1, 2)


def late_winner_fixture(scene_seed=None, seed=None):
    """One pair, N = K = 64, 1 024 hypotheses, so many outliers that the winner comes late: lane best_h % 256 regenerates it."""
    scene_seed, seed = LATE_SEED[0] if scene_seed is None else scene_seed, LATE_SEED[1] if seed is None else seed
    rng = np.random.default_rng(scene_seed)
    K, tau = 64, 6.0
    cam = _camera(64, 48, (150.0, 152.0), (31.5, 23.5))
    depth = np.zeros((1, 48, 64), np.float32)
    R, t = _pose(rng)
    c2, c3, good = plant_pair(rng, K, K, 0.84, camera_tuple(cam), camera_tuple(cam), np.eye(3), depth[0], tau, R, t)
    _shuffle(rng, K, c2, c3, good)
    return _single_scene(c2, c3, good, K, K, 1, cam, depth, tau, [(R, t)], 1024, seed)


def late_conditions(fix, ref):
    v = _margin_violation(ref)
    b = int(ref["best_h"][0])
    if not (ref["success"][0] and b >= 256 and b % 256 != 0):
        v.append(f"best_h = {b}")
    if ref["success"][0] and (ref["quality"][0] < 6 or (ref["inliers"][0] & ~fix["good"][0]).any()):
        v.append("the winner is not the planted pose")
    return v


# ---- 5. the limits: k_max = N = 4096 with 4 096 hypotheses (120 KB of dynamic LDS)
LIMIT_SEED = (0, 5)
LIMIT_COUNTS = [4096, 4196]


def limit_fixture(scene_seed=None, seed=None):
    """Two pairs in one 240 x 320 image (f = 900), 50 % outliers, counts 4096 and 4196 (clamped): every lane holds sixteen
    correspondences and contributes to both block reductions of the refit."""
    scene_seed, seed = LIMIT_SEED[0] if scene_seed is None else scene_seed, LIMIT_SEED[1] if seed is None else seed
    rng = np.random.default_rng(scene_seed)
    K, tau = 4096, 6.0
    cam = _camera(320, 240, (900.0, 902.0), (159.5, 119.5))
    depth = np.zeros((1, 240, 320), np.float32)
    c2, c3, good = np.zeros((2, K, 2), np.float32), np.zeros((2, K, 3), np.float32), np.zeros((2, K), bool)
    poses, taken = [], set()
    for pair in range(2):
        R, t = _pose(rng)
        poses.append((R, t))
        c2[pair], c3[pair], good[pair] = plant_pair(rng, K, K, 0.5, camera_tuple(cam), camera_tuple(cam), np.eye(3), depth[0], tau, R, t, taken=taken)
    return dict(coord_2d=c2, coord_3d=c3, counts=np.array(LIMIT_COUNTS, np.int32), solve=[cam], frames=[cam], A=np.eye(3)[None], image_index=[0],
                tau=[tau], depth=depth, poses=poses, good=good, n_slots=2, K=K, iters=4096, seed=seed)


def limit_conditions(fix, ref):
    v = _margin_violation(ref)
    K = fix["K"]
    for p in range(2):
        if not (ref["success"][p] and ref["num_valid"][p] == K and ref["inliers"][p, K - 1]):
            v.append(f"pair {p}: index {K - 1} is not a valid inlier of a solved pair")
        if ref["success"][p] and len(set((np.nonzero(ref["inliers"][p])[0] % 256).tolist())) != 256:
            v.append(f"pair {p}: not every lane holds an inlier")
    return v


# ---- 6. the lift's edges, exact
EDGE_TAU = 5.0
EDGE_CAM = dict(W=64, H=48, f=(128.0, 128.0), c=(32.0, 24.0))   # power-of-two focal length, integer principal point: u_f == u in fp64


def edge_fixture(seed=4):
    """A = I, one camera, so the frame pixel of a correspondence IS its float32 pixel and a tie is representable.  Every correspondence
    below is built backwards -- pixel and depth first, the model point from them through the planted pose -- so a point is an inlier
    (to ~1e-4 mm) exactly if the lift reads the pixel that half-to-even rounding names, where `good` depth lies; the pixel a wrong
    rounding would read holds 0 or a depth 15 tau off.  -> the fixture with `expected_valid` / `expected_inlier`, hand-written here."""
    tau, W, H = EDGE_TAU, EDGE_CAM["W"], EDGE_CAM["H"]
    f, c = EDGE_CAM["f"][0], EDGE_CAM["c"]
    rng = np.random.default_rng(seed)
    R, t = rot_xyz(0.4, -0.7, 1.9), np.array([3.0, -2.0, 600.0])
    depth = np.zeros((1, H, W), np.float32)
    below = float(np.nextafter(np.float32(-0.5), np.float32(-1.0)))   # the float32 just below -0.5
    far = 15.0 * tau
    rows = []   # (u, v, the pixel (row, column) that holds the good depth or None, its depth or None = good, {other pixel: offset or None = 0}, valid, inlier)

    def point(u, v, tap, valid, inlier, other=None, tap_depth="good"):
        rows.append((u, v, tap, tap_depth, other or {}, valid, inlier))

    for i in range(12):   # ordinary inliers: quarter-pixel coordinates away from everything below
        v = 14.25 + 2.0 * (i % 6) + 0.5 * (i // 6)
        point(20.25 + 3.0 * i, v, (int(np.rint(v)), 20 + 3 * i), True, True)
    # along u (rows 2..7): ties go to the even pixel, the border at -0.5 / W - 0.5
    point(10.5, 2.25, (2, 10), True, True, {(2, 11): None})        # 10.5 -> 10; 11 holds nothing
    point(11.5, 3.25, (3, 12), True, True, {(3, 11): far})         # 11.5 -> 12; 11 holds a depth 15 tau off
    point(-0.5, 4.25, (4, 0), True, True)                          # -0.5 -> -0 -> pixel 0
    point(below, 5.25, (5, 0), False, False)                       # just below -> -1: outside, though pixel 0 holds the good depth
    point(62.5, 6.25, (6, 62), True, True, {(6, 63): None})        # 62.5 -> 62
    point(63.5, 7.25, (7, 63), False, False)                       # 63.5 -> 64: outside, though pixel 63 holds the good depth
    # along v (columns 2..7)
    point(2.25, 10.5, (10, 2), True, True, {(11, 2): None})
    point(3.25, 11.5, (12, 3), True, True, {(11, 3): far})
    point(4.25, -0.5, (0, 4), True, True)
    point(5.25, below, (0, 5), False, False)
    point(6.25, 46.5, (46, 6), True, True, {(47, 6): None})
    point(7.25, 47.5, (47, 7), False, False)
    # a NaN pixel coordinate; depths of 0, -1, NaN (no measurement) and +inf (a measurement by the contract, never an inlier)
    point(float("nan"), 30.25, (30, 9), False, False)
    point(9.25, float("nan"), (31, 9), False, False)
    point(12.25, 40.25, (40, 12), False, False, tap_depth=0.0)
    point(14.25, 40.25, (40, 14), False, False, tap_depth=-1.0)
    point(16.25, 40.25, (40, 16), False, False, tap_depth=float("nan"))
    point(18.25, 40.25, (40, 18), True, False, tap_depth=float("inf"))
    K = len(rows)
    c2, c3 = np.zeros((K, 2), np.float32), np.zeros((K, 3), np.float32)
    for i, (u, v, (py, px), tap_depth, other, valid, inlier) in enumerate(rows):
        Z = float(np.float32(560.0 + rng.uniform(0.0, 80.0)))      # exact in float32: the depth image holds it as it is
        uu, vv = (float(np.float32(x)) if np.isfinite(x) else float(px if j == 0 else py) for j, x in enumerate((u, v)))
        Yc = np.array([(uu - c[0]) / f * Z, (vv - c[1]) / f * Z, Z])
        c2[i], c3[i] = (u, v), R.T @ (Yc - t)
        assert depth[0, py, px] == 0 and all(depth[0, q[0], q[1]] == 0 for q in other), "two points of the edge fixture share a pixel"
        depth[0, py, px] = Z if tap_depth == "good" else tap_depth
        for q, off in other.items():
            depth[0, q[0], q[1]] = 0.0 if off is None else Z + off
    cam = _camera(W, H, EDGE_CAM["f"], EDGE_CAM["c"])
    fix = _single_scene(c2, c3, np.array([r[6] for r in rows]), K, K, 1, cam, depth, tau, [(R, t)], 300, 9, tie_margin=False)
    fix["expected_valid"], fix["expected_inlier"] = np.array([r[5] for r in rows]), np.array([r[6] for r in rows])
    return fix


# the hand-written expectation of the edge fixture, index by index: 12 ordinary inliers, then along u and along v (tie to 10, tie to 12,
# -0.5, just below, size - 1.5, size - 0.5), then NaN u, NaN v, depth 0, -1, NaN, +inf
EDGE_VALID = [1] * 12 + [1, 1, 1, 0, 1, 0] * 2 + [0, 0, 0, 0, 0, 1]
EDGE_INLIER = [1] * 12 + [1, 1, 1, 0, 1, 0] * 2 + [0, 0, 0, 0, 0, 0]


def edge_conditions(fix, ref):
    v = _margin_violation(ref)   # without the lift's tie margin: the ties are the point
    if fix["expected_valid"].astype(int).tolist() != EDGE_VALID or fix["expected_inlier"].astype(int).tolist() != EDGE_INLIER:
        v.append("the fixture's rows are not the hand-written list")
    if ref["num_valid"][0] != sum(EDGE_VALID) or not ref["success"][0]:
        v.append(f"num_valid {ref['num_valid'][0]}, expected {sum(EDGE_VALID)}")
    if ref["inliers"][0].astype(int).tolist() != EDGE_INLIER:
        v.append(f"the restatement's mask is {ref['inliers'][0].astype(int).tolist()}")
    c = camera_tuple(fix["solve"][0])
    if not (c == (128.0, 128.0, 32.0, 24.0) and np.array_equal(fix["A"][0], np.eye(3))):
        v.append("the camera is not exact")
    return v


# ---- 7. the refit's conditioning
COND_SEED = (5, 13)
COND_NAMES = ["six inliers", "coplanar model", "identity, noise-free", "half-turn about x", "half-turn about a skew axis", "5 m away, 300 mm wide"]


def conditioning_fixture(scene_seed=None, seed=None):
    """One detection x 6 slots, K = 40, 300 hypotheses, one 192 x 256 image at f = 600: COND_NAMES."""
    scene_seed, seed = COND_SEED[0] if scene_seed is None else scene_seed, COND_SEED[1] if seed is None else seed
    rng = np.random.default_rng(scene_seed)
    K, n, tau = 40, 6, 6.0
    cam = _camera(256, 192, (600.0, 602.0), (127.5, 95.5))
    depth = np.zeros((1, 192, 256), np.float32)
    a = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    free = [_pose(rng) for _ in range(2)]
    poses = [free[0], free[1], (np.eye(3), np.array([4.0, -3.0, 600.0])), (np.diag([1.0, -1.0, -1.0]), np.array([-5.0, 2.0, 610.0])),
             (2.0 * np.outer(a, a) - np.eye(3), np.array([6.0, 5.0, 590.0])), (rot_xyz(0.8, 0.3, -1.2), np.array([40.0, -30.0, 5000.0]))]
    plan = [dict(outlier_frac=0.0, holes=K - 6), dict(outlier_frac=0.25, shape=(1.0, 1.0, 0.0)), dict(outlier_frac=0.25, noise=0.0), dict(outlier_frac=0.25),
            dict(outlier_frac=0.25), dict(outlier_frac=0.25, extent=300.0)]
    c2, c3, good = np.zeros((n, K, 2), np.float32), np.zeros((n, K, 3), np.float32), np.zeros((n, K), bool)
    taken = set()
    for pair, kw in enumerate(plan):
        R, t = poses[pair]
        c2[pair], c3[pair], good[pair] = plant_pair(rng, K, K, solve_cam=camera_tuple(cam), frame_cam=camera_tuple(cam), A=np.eye(3), depth=depth[0],
                                                    tau=tau, R=R, t=t, taken=taken, **kw)
        _shuffle(rng, K, c2[pair], c3[pair], good[pair])
    return dict(coord_2d=c2, coord_3d=c3, counts=np.full(n, K, np.int32), solve=[cam], frames=[cam], A=np.eye(3)[None], image_index=[0], tau=[tau],
                depth=depth, poses=poses, good=good, n_slots=n, K=K, iters=300, seed=seed)


def conditioning_conditions(fix, ref):
    v = _margin_violation(ref)
    for p, name in enumerate(COND_NAMES):
        if not ref["success"][p]:
            v.append(f"{name}: not solved")
            continue
        if not ref["eig_gap"][p] > 1e-6:
            v.append(f"{name}: eig_gap {ref['eig_gap'][p]:.3e}")
        if (ref["inliers"][p] & ~fix["good"][p]).any() or ref["quality"][p] < 6:
            v.append(f"{name}: the winner is not the planted pose")
        if rotation_angle(ref["R"][p], fix["poses"][p][0]) > 0.05:
            v.append(f"{name}: the refit is {rotation_angle(ref['R'][p], fix['poses'][p][0]):.3f} rad from the planted rotation")
    if ref["num_valid"][0] != 6 or ref["quality"][0] != 6:
        v.append(f"the first pair has {ref['num_valid'][0]} valid, {ref['quality'][0]} inliers, not the minimum of six")
    if fix["coord_3d"][1, :, 2].any():
        v.append("the second pair's model is not in the plane z = 0")
    return v
