"""numpy fp64 restatement of fp_pnp_ransac / fp_pnp_ransac_keyed (csrc/pnp.hip): the keyed counter-based sampler in
uint64 arithmetic, Grunert's P3P with the kernel's guards, the fourth-point choice, the inlier counts, the sequential best-model replay with
the adaptively shortened budget, and the Levenberg-Marquardt tail (oracle.pnp.refine_lm).  Plain loops: the yardstick of the tests, not a
fast path.

Grunert's quartic is ill-conditioned at a narrow field of view, so a raw hypothesis cannot be held to fp64 rounding the way a closed-form
3D-3D fit can.  Every hypothesis is therefore computed twice:
  (a) the formula path -- the kernel's coefficients in the kernel's order, the roots by numpy.roots, the kernel's guards;
  (b) the exact path   -- each solution of (a) polished by Newton on the six-unknown problem "the three sample points re-project exactly",
                          the polished solutions chosen between by the fourth point.
delta_h, the largest pixel displacement over the pair's N points between pose (a) and pose (b), is the hypothesis's own uncertainty; the
device may differ from pose (b) by band = max(1e-6 px, 1000 * delta_h) (numpy.roots and Durand-Kerner + Newton land on different sides of
the same ill-conditioned root).  Counts come as an interval [cnt_lo, cnt_hi] (inliers at thresh - band and at thresh + band).

A hypothesis is FRAGILE -- nothing is demanded of the device there -- if a root's reality is undecided (|im| / (1 + |re|) in [1e-9, 1e-3):
fp32 rounding of the pixels turns a near-double root into a complex pair or back), if the runner-up solution's fourth-point error is within
4x the two solutions' bands of the best one's (runner_up_is_close), or if polishing does not converge (two candidates that polish into one solution included).
A fragile hypothesis has cnt_lo = 0 and cnt_hi = the best count over all of its candidate solutions, raw and polished, the near-real pairs
taken at their real part.

The replay is DECIDED when every hypothesis it visited either could not beat the best count (cnt_hi <= best_c) or beat it for certain
(cnt_lo == cnt_hi > best_c, not fragile), and the adaptive budget stayed 1e-6 away from its rounding ties.
"""

import numpy as np

from oracle import pnp as opnp
from tests.kabsch_ref import GOLDEN, KEY_MUL, Margin, mix64, rotation_angle, update_num_iters  # noqa: F401  (rotation_angle: for the tests)

M64 = (1 << 64) - 1
MAX_ATTEMPT = 64            # pnp.hip: a draw may fail while attempt <= 64
REAL_LO, REAL_HI = 1e-9, 1e-3   # a root with |im| / (1 + |re|) in [REAL_LO, REAL_HI) is neither real nor complex for certain (the kernel's own
                                # test, 1e-6, lies inside: outside the interval both agree)
RUNNER_UP = 4.0
BAND_FLOOR, BAND_FACTOR = 1e-6, 1000.0
NEWTON_ITERS, NEWTON_TOL = 25, 1e-9   # px
MERGED = 1e-6               # px: two polished candidates closer than this on all of the pair's points are one solution


# ------------------------------------------------------------------------------------------------------------------------- the sampler
def pair_base(seed: int, key: int) -> int:
    """seed: uint64; key: the pair's index in the launch or pair_keys[pair] (an int64's bits are read as uint64)."""
    return mix64((seed & M64) ^ (((key & M64) * KEY_MUL) & M64))


def hyp_key(base: int, h: int) -> int:
    return (base + h * GOLDEN) & M64


def sample4(key: int, N: int):
    """Four distinct indices below N by repeated mix64 and % N (integer arithmetic: equal to the device's, bit for bit)."""
    ids, s = [], key
    for _ in range(4):
        attempt = 0
        while True:
            s = mix64(s)
            c = s % N
            if c not in ids:
                ids.append(c)
                break
            if attempt > MAX_ATTEMPT:
                return None
            attempt += 1
    return ids


# ------------------------------------------------------------------------------------------------------------------------ the geometry
def exp_so3(w):
    th = np.sqrt(w @ w)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * K @ K


def project(R, t, X, cam):
    """-> pixels [n, 2], z [n] of R X + t (no guard: the caller looks at z)."""
    fx, fy, cx, cy = cam
    xc = X @ R.T + t
    z = xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([fx * xc[:, 0] / z + cx, fy * xc[:, 1] / z + cy], 1), z


def reproj_err(R, t, X, uv, cam):
    """-> error [n] in pixels (inf where z <= 1e-9: never an inlier), z [n]."""
    p, z = project(R, t, X, cam)
    with np.errstate(invalid="ignore"):
        e = np.sqrt(((p - uv) ** 2).sum(1))
    return np.where(z > 1e-9, e, np.inf), z


def pose_px_dist(Ra, ta, Rb, tb, X, cam):
    """The largest pixel displacement of the points X between two poses; inf if a point is in front of one camera only (or on its plane)."""
    pa, za = project(Ra, ta, X, cam)
    pb, zb = project(Rb, tb, X, cam)
    fa, fb = za > 1e-9, zb > 1e-9
    if np.any(fa != fb):
        return np.inf
    if not fa.any():
        return 0.0
    d = np.sqrt(((pa[fa] - pb[fa]) ** 2).sum(1)).max()
    return float(d) if np.isfinite(d) else np.inf


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
    return np.stack([e1, np.cross(e3, e1), e3], axis=1)


def bearings(uv, cam):
    fx, fy, cx, cy = cam
    f = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(len(uv))], 1)
    return f / np.sqrt((f * f).sum(1))[:, None]


def grunert(X, f):
    """P3P, Grunert's quartic with the kernel's coefficients and guards.  X [3, 3] model points, f [3, 3] unit bearings.
    -> list of (R, t, reality) with reality = |im| / (1 + |re|) of the root behind the solution (roots below REAL_HI only, taken at their
    real part)."""
    d12, d02, d01 = X[1] - X[2], X[0] - X[2], X[0] - X[1]
    a2, b2, c2 = d12 @ d12, d02 @ d02, d01 @ d01
    if not (a2 > 1e-18 and b2 > 1e-18 and c2 > 1e-18):
        return []
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    q, p = (a2 - c2) / b2, (a2 + c2) / b2
    A4 = (q - 1.0) * (q - 1.0) - 4.0 * c2 / b2 * ca * ca
    A3 = 4.0 * (q * (1.0 - q) * cb - (1.0 - p) * ca * cg + 2.0 * c2 / b2 * ca * ca * cb)
    A2 = 2.0 * (q * q - 1.0 + 2.0 * q * q * cb * cb + 2.0 * (b2 - c2) / b2 * ca * ca - 4.0 * p * ca * cb * cg + 2.0 * (b2 - a2) / b2 * cg * cg)
    A1 = 4.0 * (-q * (1.0 + q) * cb + 2.0 * a2 / b2 * cg * cg * cb - (1.0 - p) * ca * cg)
    A0 = (1.0 + q) * (1.0 + q) - 4.0 * a2 / b2 * cg * cg
    if not (abs(A4) > 1e-12 * (abs(A3) + abs(A2) + abs(A1) + abs(A0) + 1e-300)):
        return []
    coef = np.array([1.0, A3 / A4, A2 / A4, A1 / A4, A0 / A4])
    if not np.all(np.isfinite(coef)):
        return []
    roots = np.roots(coef)
    Fw = tri_frame(X[0], X[1], X[2])
    if Fw is None:
        return []
    sols = []
    for r in roots:
        reality = abs(r.imag) / (1.0 + abs(r.real))
        if reality >= REAL_HI:
            continue
        v = float(r.real)
        if not v > 0.0:
            continue
        den = 2.0 * (cg - v * ca)
        if not abs(den) > 1e-12:
            continue
        u = ((-1.0 + q) * v * v - 2.0 * q * cb * v + 1.0 + q) / den
        if not u > 0.0:
            continue
        s1sq = c2 / (1.0 + u * u - 2.0 * u * cg)
        if not s1sq > 0.0:
            continue
        s1 = np.sqrt(s1sq)
        P = np.stack([s1 * f[0], u * s1 * f[1], v * s1 * f[2]])
        Fc = tri_frame(P[0], P[1], P[2])
        if Fc is None:
            continue
        R = Fc @ Fw.T
        sols.append((R, P[0] - R @ X[0], reality))
    return sols


def polish(R, t, X, uv, cam):
    """Newton on (w, dt) of R' = exp([w]x) R, t' = t + dt until the three points X re-project onto uv.  -> (R, t) or None."""
    fx, fy = cam[0], cam[1]
    for _ in range(NEWTON_ITERS):
        xc = X @ R.T + t
        x, y, z = xc[:, 0], xc[:, 1], xc[:, 2]
        if not np.all(z > 1e-9) or not np.all(np.isfinite(xc)):
            return None
        iz = 1.0 / z
        r = np.concatenate([fx * x * iz + cam[2] - uv[:, 0], fy * y * iz + cam[3] - uv[:, 1]])
        if np.abs(r).max() < 1e-12:
            break
        ux, uz, vy, vz = fx * iz, -fx * x * iz * iz, fy * iz, -fy * y * iz * iz
        px, py, pz = x - t[0], y - t[1], z - t[2]
        zero = np.zeros(3)
        Ju = np.stack([uz * py, ux * pz - uz * px, -ux * py, ux, zero, uz], 1)
        Jv = np.stack([-vy * pz + vz * py, -vz * px, vy * px, zero, vy, vz], 1)
        try:
            d = np.linalg.solve(np.concatenate([Ju, Jv]), -r)
        except np.linalg.LinAlgError:
            return None
        if not np.all(np.isfinite(d)):
            return None
        R, t = exp_so3(d[:3]) @ R, t + d[3:]
    p, z = project(R, t, X, cam)
    if not (np.all(z > 1e-9) and np.abs(p - uv).max() < NEWTON_TOL):
        return None
    return R, t


def runner_up_is_close(errs, bands):
    """errs: the polished candidates' fourth-point errors (px); bands: how far the device's version of each may be from it (px).  The
    device takes the candidate with the least error, and its errors are the restated ones give or take the bands: the choice is certain when
    the runner-up's error exceeds the best one's by more than the two bands together; RUNNER_UP times that is asked."""
    o = np.argsort(errs)
    return len(o) > 1 and bool(errs[o[1]] - errs[o[0]] <= RUNNER_UP * (bands[o[0]] + bands[o[1]]))


class Hyp:
    """One hypothesis of a pair.  ids: the four drawn indices (None: the draw failed); pose: the exact path's (R, t) (None: no model);
    pose_a: the formula path's; delta: their largest pixel displacement over the pair's points; band; fragile + why; err: the exact
    pose's reprojection error of every point; cand: all candidate poses (raw and polished) of a fragile hypothesis."""
    __slots__ = ("ids", "pose", "pose_a", "delta", "band", "fragile", "why", "err", "cand", "X", "uv", "cam")

    def counts(self, thresh):
        """-> (cnt_lo, cnt_hi)."""
        if self.fragile:
            hi = 0
            for (R, t, band) in self.cand:
                e, _ = reproj_err(R, t, self.X, self.uv, self.cam)
                hi = max(hi, int((e <= thresh + band).sum()))
            return 0, hi
        if self.pose is None:
            return 0, 0
        return int((self.err <= thresh - self.band).sum()), int((self.err <= thresh + self.band).sum())

    def mask(self, thresh):
        return self.err <= thresh


def hypothesis(key, X, uv, cam):
    """Hypothesis `key` of a pair with the points X [N, 3], uv [N, 2] (fp64 arrays holding the fp32 inputs) and camera (fx, fy, cx, cy)."""
    H = Hyp()
    H.X, H.uv, H.cam = X, uv, cam
    H.pose = H.pose_a = H.err = None
    H.delta, H.band, H.fragile, H.why, H.cand = 0.0, BAND_FLOOR, False, "", []
    N = len(X)
    H.ids = sample4(key, N)
    if H.ids is None:
        return H
    i3, i4 = H.ids[:3], H.ids[3]
    sols = grunert(X[i3], bearings(uv[i3], cam))
    if not sols:
        return H
    if any(REAL_LO <= s[2] < REAL_HI for s in sols):
        H.fragile, H.why = True, "reality"
    band_of = lambda d: max(BAND_FLOOR, BAND_FACTOR * d) if np.isfinite(d) else np.inf
    e4 = lambda R, t: float(reproj_err(R, t, X[i4:i4 + 1], uv[i4:i4 + 1], cam)[0][0])
    raw = [(R, t) for (R, t, reality) in sols]
    pol = [polish(R, t, X[i3], uv[i3], cam) for (R, t) in raw]
    if not H.fragile and any(p is None for p in pol):
        H.fragile, H.why = True, "polish"
    if not H.fragile:
        for i in range(len(pol)):
            for j in range(i):
                if pose_px_dist(*pol[i], *pol[j], X, cam) < MERGED:
                    H.fragile, H.why = True, "merged"
    if not H.fragile:
        ea, eb = [e4(*p) for p in raw], [e4(*p) for p in pol]
        ia, ib = int(np.argmin(ea)), int(np.argmin(eb))
        if not np.isfinite(eb[ib]) or not np.isfinite(ea[ia]):      # the fourth point is behind every solution: no model on the device either,
            if np.isfinite(eb).any() or np.isfinite(ea).any():      # unless the two paths disagree about it
                H.fragile, H.why = True, "behind"
            else:
                return H
        elif ia != ib or runner_up_is_close(eb, [band_of(pose_px_dist(*r, *p, X, cam)) for r, p in zip(raw, pol)]):
            H.fragile, H.why = True, "runner-up"
        else:
            H.pose_a, H.pose = raw[ia], pol[ib]
            H.delta = pose_px_dist(*H.pose_a, *H.pose, X, cam)
            if not np.isfinite(H.delta):
                H.fragile, H.why = True, "plane"
            else:
                H.band = band_of(H.delta)
                H.err, _ = reproj_err(*H.pose, X, uv, cam)
    if H.fragile:
        H.pose = H.pose_a = None
        for r, p in zip(raw, pol):
            d = pose_px_dist(*r, *p, X, cam) if p is not None else 0.0
            band = band_of(d)
            H.cand.append((*r, band))
            if p is not None:
                H.cand.append((*p, band))
    return H


# -------------------------------------------------------------------------------------------------------------------------- the replay
def replay_counts(cnt, N, conf, margin=None):
    """The sequential best-model rule over plain counts (pnp.hip's replay): -> (best, best_c, niters)."""
    best, best_c, niters, h = -1, 3, len(cnt), 0
    while h < niters:
        if cnt[h] > best_c:
            best_c, best = int(cnt[h]), h
            niters = update_num_iters(conf, (N - best_c) / N, 4, niters, margin)
        h += 1
    return best, best_c, niters


def replay(get, iters, N, conf, margin=None, history=None):
    """The same rule over count intervals, evaluated lazily: get(h) -> (cnt_lo, cnt_hi, fragile), asked only while h < niters.
    -> (best, best_c, niters, decided).  An undecided hypothesis is passed over (the result then only stands in for one).  history: a list
    that receives (h, count, budget before, budget after) of every new best model."""
    margin = Margin() if margin is None else margin
    best, best_c, niters, h, decided = -1, 3, iters, 0, True
    while h < niters:
        lo, hi, fragile = get(h)
        if hi > best_c:
            if lo == hi and not fragile:
                best_c, best, before = hi, h, niters
                niters = update_num_iters(conf, (N - best_c) / N, 4, niters, margin)
                if history is not None:
                    history.append((h, hi, before, niters))
            else:
                decided = False
        h += 1
    return best, best_c, niters, bool(decided and margin.value > 1e-6)


def pnp_ransac_ref(coord_2d, coord_3d, counts, cams, n_slots, iters, thresh, conf=0.99, seed=0, min_corresp=6, pair_keys=None, refine=True,
                   cache=None):
    """coord_2d [P, K, 2] / coord_3d [P, K, 3] float32, counts [P], cams [P / n_slots, 4].  -> dict of arrays over the P pairs: success,
    quality, inliers [P, K], best_h (-1: none), ransac_R / ransac_t (the winning hypothesis, exact path), R / t (refined), decided [P], band
    [P] (the winner's), niters [P] (the budget the replay ended with), hyps: per pair the dict h -> Hyp of the hypotheses it visited, and
    history: per pair replay's list of new best models.
    cache: a dict the hypotheses are kept in between calls on the same inputs (keyed by pair data identity, camera and sampler key)."""
    coord_2d, coord_3d = np.asarray(coord_2d, np.float32), np.asarray(coord_3d, np.float32)
    P, K = coord_2d.shape[:2]
    out = {"success": np.zeros(P, bool), "quality": np.zeros(P, np.int64), "inliers": np.zeros((P, K), bool), "best_h": np.full(P, -1, np.int64),
           "ransac_R": np.zeros((P, 3, 3)), "ransac_t": np.zeros((P, 3)), "R": np.tile(np.eye(3), (P, 1, 1)), "t": np.zeros((P, 3)),
           "decided": np.ones(P, bool), "band": np.zeros(P), "niters": np.zeros(P, np.int64), "hyps": [dict() for _ in range(P)], "history": [[] for _ in range(P)]}
    cache = {} if cache is None else cache
    for pair in range(P):
        cam = tuple(float(v) for v in np.asarray(cams, np.float64)[pair // n_slots])
        N = min(int(counts[pair]), K)
        if N < min_corresp:
            continue
        X, uv = coord_3d[pair, :N].astype(np.float64), coord_2d[pair, :N].astype(np.float64)
        key = pair if pair_keys is None else int(pair_keys[pair]) & M64
        base = pair_base(seed, key)
        hyps = out["hyps"][pair]

        def get(h):
            ck = (pair, N, cam, hyp_key(base, h))
            if ck not in cache:
                cache[ck] = hypothesis(hyp_key(base, h), X, uv, cam)
            hyps[h] = cache[ck]
            return (*hyps[h].counts(thresh), hyps[h].fragile)

        best, best_c, niters, decided = replay(get, iters, N, conf, history=out["history"][pair])
        out["decided"][pair], out["niters"][pair] = decided, niters
        if best < 0:
            continue
        W = hyps[best]
        inl = W.mask(thresh)
        out["success"][pair], out["quality"][pair], out["best_h"][pair], out["band"][pair] = True, best_c, best, W.band
        out["inliers"][pair, :N] = inl
        out["ransac_R"][pair], out["ransac_t"][pair] = W.pose
        out["R"][pair], out["t"][pair] = W.pose
        if refine:
            R, t, _ = opnp.refine_lm(*W.pose, X[inl], uv[inl], cam)
            out["R"][pair], out["t"][pair] = R, t
    return out


# ------------------------------------------------------------------------------------------------------------ comparison with a device
def visited_gap(hyps, best, X, cam):
    """The smallest pixel distance (pose_px_dist over the pair's points) from the winning hypothesis to any other visited one -- for a
    fragile one, to any of its candidates."""
    W, gap = hyps[best], np.inf
    for h, H in hyps.items():
        if h == best:
            continue
        poses = [H.pose] if H.pose is not None else [(R, t) for (R, t, _) in H.cand]
        for (R, t) in poses:
            gap = min(gap, pose_px_dist(*W.pose, R, t, X, cam))
    return gap


def compare(dev, ref, coord_2d, coord_3d, counts, cams, n_slots, identify=True, refined=True):
    """A device result (solve_pnp_ransac_batch's dict as numpy arrays, pairs flattened, with ransac_pose) against pnp_ransac_ref's on the
    same inputs.  -> (list of mismatches as strings: empty = equal, figures: dict).  Equal: success, quality, the inlier masks; the failure
    record; the winning hypothesis is the predicted one -- ransac_pose within the winner's band of it and, with identify, every other visited
    hypothesis at least 1e3 times farther from ransac_pose than the predicted one; the refined pose within 1e-6 rad / 1e-3 mm."""
    bad, fig = [], {"hyp_px": 0.0, "hyp_ratio": 0.0, "rad": 0.0, "mm": 0.0, "min_gap_ratio": np.inf}
    P, K = np.asarray(coord_2d).shape[:2]
    for p in range(P):
        rp = dev["ransac_pose"][p]
        if bool(dev["success"][p]) != bool(ref["success"][p]):
            bad.append(f"pair {p}: success {bool(dev['success'][p])}, restated {bool(ref['success'][p])}")
            continue
        if int(dev["quality"][p]) != int(ref["quality"][p]):
            bad.append(f"pair {p}: quality {int(dev['quality'][p])}, restated {int(ref['quality'][p])}")
        if not np.array_equal(dev["inliers"][p], ref["inliers"][p]):
            bad.append(f"pair {p}: inlier masks differ at {np.nonzero(dev['inliers'][p] != ref['inliers'][p])[0].tolist()}")
        if not ref["success"][p]:
            if not (np.array_equal(dev["R"][p], np.eye(3)) and not dev["t"][p].any() and not rp.any() and not dev["inliers"][p].any()
                    and int(dev["quality"][p]) == 0):
                bad.append(f"pair {p}: not the failure record")
            continue
        cam = tuple(float(v) for v in np.asarray(cams, np.float64)[p // n_slots])
        N = min(int(counts[p]), K)
        X = np.asarray(coord_3d[p, :N], np.float64)
        Rd, td = rp[:9].reshape(3, 3), rp[9:]
        best = int(ref["best_h"][p])
        dist = {h: (pose_px_dist(Rd, td, *H.pose, X, cam) if H.pose is not None
                    else min([pose_px_dist(Rd, td, R, t, X, cam) for (R, t, _) in H.cand], default=np.inf)) for h, H in ref["hyps"][p].items()}
        near = min(dist, key=dist.get)
        W = ref["hyps"][p][best]
        fig["hyp_px"] = max(fig["hyp_px"], dist[best])
        fig["hyp_ratio"] = max(fig["hyp_ratio"], dist[best] / (W.band / BAND_FACTOR))   # against max(1e-9 px, delta_h): 1000 is allowed
        if near != best or not dist[best] <= W.band:
            bad.append(f"pair {p}: ransac_pose is {dist[best]:.3e} px from the predicted hypothesis {best} (band {W.band:.3e}), nearest is {near} at {dist[near]:.3e}")
        others = min([d for h, d in dist.items() if h != best], default=np.inf)
        fig["min_gap_ratio"] = min(fig["min_gap_ratio"], others / max(dist[best], 1e-300))
        if identify and not others >= 1e3 * dist[best]:
            bad.append(f"pair {p}: another hypothesis is {others:.3e} px from ransac_pose, the predicted one {dist[best]:.3e}")
        if refined:
            rad, mm = rotation_angle(dev["R"][p], ref["R"][p]), float(np.abs(dev["t"][p] - ref["t"][p]).max())
            fig["rad"], fig["mm"] = max(fig["rad"], rad), max(fig["mm"], mm)
            if not (rad < 1e-6 and mm < 1e-3):
                bad.append(f"pair {p}: refined pose off by {rad:.3e} rad / {mm:.3e} mm")
    return bad, fig


# ---------------------------------------------------------------------------------------------------- planted scenes for the tests
CAM_A = (620.0, 615.0, 259.0, 255.5)
CAM_B = (540.0, 548.0, 300.5, 240.0)
THRESH = 3.0


def scene(rng, n, n_out, noise, cam, sigma=60.0, as_float32=True):
    """n model points (Gaussian cloud, sigma mm) 0.8 - 1.2 m in front of `cam` under a random pose; their pixels with Gaussian noise (px);
    the first n_out of a random order replaced by uniform pixels (gross outliers).  -> X [n, 3] float32, uv [n, 2] float32 (or fp64, the
    unrounded pixels), truth [n] bool."""
    R = opnp.rodrigues(rng.normal(size=3))
    t = np.array([rng.normal() * 30, rng.normal() * 30, 800 + rng.random() * 400])
    X = (rng.normal(size=(n, 3)) * sigma).astype(np.float32)
    uv, _ = opnp.project(R, t, X, cam)
    uv = uv + rng.normal(size=uv.shape) * noise
    out = rng.choice(n, n_out, replace=False)
    uv[out] = rng.random((n_out, 2)) * 518
    truth = np.ones(n, bool)
    truth[out] = False
    return X, (uv.astype(np.float32) if as_float32 else uv), truth


def _pack(scenes, K, counts=None):
    P = len(scenes)
    c2, c3 = np.zeros((P, K, 2), np.float32), np.zeros((P, K, 3), np.float32)
    for p, sc in enumerate(scenes):
        if sc is not None:
            n = min(len(sc[0]), K)
            c3[p, :n], c2[p, :n] = sc[0][:n], sc[1][:n]
    cnt = np.array([0 if sc is None else len(sc[0]) for sc in scenes] if counts is None else counts, np.int32)
    return c2, c3, cnt


SWEEP_SEED = (1, 5)


def sweep_fixture():
    """The hypothesis sweep: one scene (K = 40, 30 % gross outliers, 0.5 px noise) replicated over 2 048 pairs with the keys 0..2047 and
    one iteration each -- every pair exposes hypothesis 0 of its key."""
    X, uv, _ = scene(np.random.default_rng(SWEEP_SEED[0]), 40, 12, 0.5, CAM_A)
    P = 2048
    return dict(coord_2d=np.tile(uv, (P, 1, 1)), coord_3d=np.tile(X, (P, 1, 1)), counts=np.full(P, 40, np.int32), cams=[CAM_A], B=1, n_slots=P, K=40,
                iters=1, thresh=THRESH, conf=0.99, seed=SWEEP_SEED[1], min_corresp=6, pair_keys=np.arange(P, dtype=np.int64))


def sweep_hypotheses(fix):
    X, uv = fix["coord_3d"][0].astype(np.float64), fix["coord_2d"][0].astype(np.float64)
    return [hypothesis(hyp_key(pair_base(fix["seed"], int(k)), 0), X, uv, fix["cams"][0]) for k in fix["pair_keys"]]


FOUR_POINT_SEED = (2, 9)


def four_point_fixture(P=4096):
    """P pairs of exactly four noise-free correspondences (K = 4), one iteration each."""
    rng = np.random.default_rng(FOUR_POINT_SEED[0])
    c2, c3, cnt = _pack([scene(rng, 4, 0, 0.0, CAM_A) for _ in range(P)], 4)
    return dict(coord_2d=c2, coord_3d=c3, counts=cnt, cams=[CAM_A], B=1, n_slots=P, K=4, iters=1, thresh=THRESH, conf=0.99, seed=FOUR_POINT_SEED[1],
                min_corresp=4, pair_keys=None)


def four_point_hypotheses(fix):
    return [hypothesis(hyp_key(pair_base(fix["seed"], p), 0), fix["coord_3d"][p].astype(np.float64), fix["coord_2d"][p].astype(np.float64),
                       fix["cams"][0]) for p in range(len(fix["counts"]))]


REPLAY_SEED = (16, (1 << 63) + 12345)
REPLAY_KEYS = [[-(1 << 63) + 96, 7, 11], [-1, 3, (1 << 40) + 1]]    # int64: the first of either detection has the top bit set


def replay_fixture(scene_seed=None, seed=None):
    """2 detections x 3 slots, two different cameras, K = 40, 300 hypotheses (the loop strides, unevenly).  counts: 40 (30 % outliers,
    1.5 px noise: the count climbs in several steps), 0, 5 (below min_corresp) | 57 (clamped to 40; 30 % outliers, 0.2 px noise), 6 (0.2 px
    noise), 40 (all outliers)."""
    rng = np.random.default_rng(REPLAY_SEED[0] if scene_seed is None else scene_seed)
    K = 40
    scenes = [scene(rng, 40, 12, 1.5, CAM_A), None, scene(rng, 5, 0, 0.2, CAM_A),
              scene(rng, 57, 17, 0.2, CAM_B), scene(rng, 6, 0, 0.2, CAM_B), scene(rng, 40, 40, 0.0, CAM_B)]
    c2, c3, cnt = _pack(scenes, K)
    return dict(coord_2d=c2, coord_3d=c3, counts=cnt, cams=[CAM_A, CAM_B], B=2, n_slots=3, K=K, iters=300, thresh=THRESH,
                seed=REPLAY_SEED[1] if seed is None else seed, min_corresp=6)


LATE_SEED = (240, 1)


def late_winner_fixture(scene_seed=None, seed=None):
    """One pair, K = N = 64, 16 noise-free inliers, 1 024 hypotheses: the winner lies in a thread's second trip or later (h >= 256).  The
    budget stays at 1 024, so later all-inlier triples are visited: they tie on the count and give the winner's pose to within the fp32
    rounding of the pixels (~1e-5 px) -- the 1e3 gap of the replay fixture cannot exist here; twice the band can (fixture_conditions)."""
    rng = np.random.default_rng(LATE_SEED[0] if scene_seed is None else scene_seed)
    c2, c3, cnt = _pack([scene(rng, 64, 48, 0.0, CAM_A)], 64)
    return dict(coord_2d=c2, coord_3d=c3, counts=cnt, cams=[CAM_A], B=1, n_slots=1, K=64, iters=1024, thresh=THRESH,
                seed=LATE_SEED[1] if seed is None else seed, min_corresp=6)


LDS_SEED = (0, 3)
LDS_KEYS = [1008, 268]


def lds_fixture(scene_seed=None, seed=None):
    """The kernel's limits: k_max = N = 4096 and 4 096 hypotheses, 50 % noise-free inliers; the second pair's count is 4096 + 100 (clamped).
    Run with the keys LDS_KEYS: under them the winner's three sample points are the only all-inlier triple the shortened budget visits (any
    other one gives the same pose to within the fp32 rounding of the pixels, ~1e-5 px, and could not be told from the winner)."""
    rng = np.random.default_rng(LDS_SEED[0] if scene_seed is None else scene_seed)
    c2, c3, _ = _pack([scene(rng, 4096, 2048, 0.0, CAM_A), scene(rng, 4096, 2048, 0.0, CAM_B)], 4096)
    return dict(coord_2d=c2, coord_3d=c3, counts=np.array([4096, 4196], np.int32), cams=[CAM_A, CAM_B], B=2, n_slots=1, K=4096, iters=4096,
                thresh=THRESH, seed=LDS_SEED[1] if seed is None else seed, min_corresp=6)


def run_ref_on(fix, conf=0.99, pair_keys=None, cams=None, refine=True, cache=None):
    keys = None if pair_keys is None else np.asarray(pair_keys, np.int64).reshape(-1)
    return pnp_ransac_ref(fix["coord_2d"], fix["coord_3d"], fix["counts"], fix["cams"] if cams is None else cams, fix["n_slots"], fix["iters"],
                          fix["thresh"], conf, fix["seed"], fix["min_corresp"], keys, refine, cache)


def budget_is_tight(fix, ref, pair, pair_keys=None):
    """The adaptive budget decided this pair's result from both sides: the winner was found in the last 40 % of the budget then in force (a
    budget cut shorter than that loses it), and a certain, strictly better model lies between the final budget and twice it (a budget that
    is not cut, or cut too late, takes that one)."""
    hist = ref["history"][pair]
    if len(hist) < 2:
        return False
    w, c, before, after = hist[-1]
    if not 0.6 * before <= w < after:
        return False
    N = min(int(fix["counts"][pair]), fix["K"])
    X, uv = fix["coord_3d"][pair, :N].astype(np.float64), fix["coord_2d"][pair, :N].astype(np.float64)
    key = pair if pair_keys is None else int(np.asarray(pair_keys, np.int64).reshape(-1)[pair])
    base = pair_base(fix["seed"], key)
    for h in range(after, min(2 * after, fix["iters"])):
        H = hypothesis(hyp_key(base, h), X, uv, fix["cams"][pair // fix["n_slots"]])
        if not H.fragile and H.counts(fix["thresh"])[0] > c:
            return True
    return False


def fixture_conditions(fix, ref, gap_factor=1e3 + 1.0):
    """What a replay fixture must satisfy before a device result is compared with it: every pair decided, and the winner of every
    successful pair at least gap_factor bands away from every other visited hypothesis (1e3 + 1: a device pose within the band of the winner
    then has every other hypothesis 1e3 times farther; 2: it then is nearer to the winner than to any other).  -> list of violations."""
    bad = []
    P, K = fix["coord_2d"].shape[:2]
    for p in range(P):
        if not ref["decided"][p]:
            bad.append(f"pair {p}: not decided")
        if ref["success"][p]:
            cam = tuple(np.asarray(ref.get("cams", fix["cams"]), np.float64)[p // fix["n_slots"]])
            N = min(int(fix["counts"][p]), K)
            gap = visited_gap(ref["hyps"][p], int(ref["best_h"][p]), fix["coord_3d"][p, :N].astype(np.float64), cam)
            if not gap >= gap_factor * ref["band"][p]:
                bad.append(f"pair {p}: gap {gap:.3e} px, band {ref['band'][p]:.3e} px")
    return bad


def compare_sweep(dev, hyps, fix):
    """The hypothesis sweep: pair k of `dev` ran hypothesis 0 of key k alone, so its outputs ARE that hypothesis.  For every non-fragile one:
    success == (cnt > 3); quality == cnt and the mask equal where cnt_lo == cnt_hi; the failure record where cnt <= 3; ransac_pose within the
    band of the exact pose.  -> (mismatches, figures)."""
    bad = []
    fig = {"fragile": 0, "fragile_solved": 0, "fragile_unsolved": 0, "open": 0, "checked": 0, "models": 0, "hyp_px": 0.0, "hyp_ratio": 0.0}
    X, cam, thresh = fix["coord_3d"][0].astype(np.float64), fix["cams"][0], fix["thresh"]
    for k, H in enumerate(hyps):
        ok, rp = bool(dev["success"][k]), dev["ransac_pose"][k]
        if H.fragile:
            fig["fragile"] += 1
            fig["fragile_solved" if ok else "fragile_unsolved"] += 1
            continue
        lo, hi = H.counts(thresh)
        if lo <= 3 < hi:      # the band straddles the fourth inlier: either answer stands
            fig["open"] += 1
            continue
        fig["checked"] += 1
        if ok != (lo > 3):
            bad.append(f"pair {k}: success {ok}, restated count [{lo}, {hi}]")
            continue
        if not ok:
            if not (np.array_equal(dev["R"][k], np.eye(3)) and not dev["t"][k].any() and not rp.any() and not dev["inliers"][k].any()
                    and int(dev["quality"][k]) == 0):
                bad.append(f"pair {k}: not the failure record")
            continue
        fig["models"] += 1
        q = int(dev["quality"][k])
        if not lo <= q <= hi:
            bad.append(f"pair {k}: quality {q}, restated [{lo}, {hi}]")
        if lo == hi and not np.array_equal(dev["inliers"][k], H.mask(thresh)):
            bad.append(f"pair {k}: inlier masks differ")
        if q != int(dev["inliers"][k].sum()):
            bad.append(f"pair {k}: quality {q} but {int(dev['inliers'][k].sum())} mask bits")
        d = pose_px_dist(rp[:9].reshape(3, 3), rp[9:], *H.pose, X, cam)
        fig["hyp_px"], fig["hyp_ratio"] = max(fig["hyp_px"], d), max(fig["hyp_ratio"], d / (H.band / BAND_FACTOR))
        if not d <= H.band:
            bad.append(f"pair {k}: ransac_pose {d:.3e} px from the exact pose, band {H.band:.3e} (delta {H.delta:.3e})")
    return bad, fig


def compare_four_point(dev, hyps, fix):
    """The four-point sweep: every non-fragile pair succeeds with quality 4, and its ransac_pose re-projects each of the four points to within
    the exact pose's own error there plus the band.  -> (mismatches, figures)."""
    bad, fig = [], {"fragile": 0, "device_failed": 0, "device_failed_not_fragile": 0, "hyp_px": 0.0, "hyp_ratio": 0.0, "worst_px": 0.0}
    cam = fix["cams"][0]
    for p, H in enumerate(hyps):
        ok = bool(dev["success"][p])
        fig["fragile"] += H.fragile
        fig["device_failed"] += not ok
        if H.fragile:
            continue
        if H.pose is None or not ok or int(dev["quality"][p]) != 4 or not dev["inliers"][p].all():
            fig["device_failed_not_fragile"] += not ok
            bad.append(f"pair {p}: success {ok}, quality {int(dev['quality'][p])} (delta {H.delta:.3e})")
            continue
        rp = dev["ransac_pose"][p]
        X, uv = fix["coord_3d"][p].astype(np.float64), fix["coord_2d"][p].astype(np.float64)
        e, _ = reproj_err(rp[:9].reshape(3, 3), rp[9:], X, uv, cam)
        d = pose_px_dist(rp[:9].reshape(3, 3), rp[9:], *H.pose, X, cam)
        fig["hyp_px"], fig["hyp_ratio"] = max(fig["hyp_px"], d), max(fig["hyp_ratio"], d / (H.band / BAND_FACTOR))
        fig["worst_px"] = max(fig["worst_px"], float(e.max()))
        if not np.all(e <= H.err + H.band):
            bad.append(f"pair {p}: re-projects to {e.max():.3e} px, the exact pose to {H.err.max():.3e}, band {H.band:.3e}")
    return bad, fig
