"""numpy fp64 restatement of the joint feature + depth refinement contract (csrc/rgbd_refine.hip computes it on
the GPU).

Per detection: the pose (R, t) is model -> FRAME camera (mm).  The feature term is section 11's (tests/featuremetric_ref.py), evaluated in
the feature (crop) camera at X_f = A X_c + a with its Jacobian carried back through A; the depth term is section 14's
(tests/depth_refine_ref.py) at X_c, with one more condition: a point whose four taps spread over more than tau is not measurable.
E = E_f + w_d E_d,  E_f = sum_V log(1 + s_i / sigma^2) / |V|,  E_d = sum min(r^2, tau^2) / tau^2 / N;
H = H_f / (|V| sigma^2) + w_d H_d / (N tau^2), g likewise.  The twist is left-multiplied on the frame-camera pose.
"""

import numpy as np

from tests import featuremetric_ref as fr
from tests import lm_ref
from tests.featuremetric_ref import rot_angle_deg, rot_exp, update  # noqa: F401


def rot_angle_rad(Ra, Rb):
    """The angle between two rotations, accurate near 0 (arccos of the trace resolves no angle below 2e-8 rad)."""
    D = np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)
    w = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.arctan2(np.linalg.norm(w), (np.trace(D) - 1.0) / 2.0))


def frame_points(R, t, X):
    return np.asarray(X, np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)


def valid_set(R, t, X, A, a, fcam, W, H, M):
    """Section 11's valid set of the feature term: X_f in front of the feature camera and inside the map."""
    return fr.valid_set(A, a, frame_points(R, t, X), fcam, W, H, M)


def feature_terms(R, t, X, f, A, a, fcam, W, H, M):
    """Section 11's per-point terms at X_f = A X_c + a, the Jacobian rows w.r.t. the frame-camera twist: with p the row of
    d(x_m, y_m)/dX_f, p' = A^T p and the row is [X_c x p' | p'] (zero along a clamped axis)."""
    Xc = frame_points(R, t, X)
    p = fr.point_terms(A, a, Xc, f, fcam, W, H, M)   # "model" points X_c under the "pose" (A, a)
    A = np.asarray(A, np.float64)
    px, py = p["ax"][:, 3:] @ A, p["ay"][:, 3:] @ A
    return dict(z=p["z"], r=p["r"], gx=p["gx"], gy=p["gy"], ax=np.concatenate([np.cross(Xc, px), px], 1), ay=np.concatenate([np.cross(Xc, py), py], 1))


def sigma2_at(R, t, X, f, A, a, fcam, W, H, M, valid):
    p = feature_terms(R, t, X[valid], f[valid], A, a, fcam, W, H, M)
    s = np.sum(p["r"] * p["r"], axis=1, dtype=np.float32).astype(np.float64)
    return max(float(s.sum()) / max(int(valid.sum()), 1), 1e-12)


def feature_system(R, t, X, f, A, a, fcam, W, H, M, valid, sigma2):
    """E_f (normalised), H_f [6, 6], g_f [6] (both not normalised) over the frozen valid set, and whether one of its points has z_f <= 1 mm."""
    p = feature_terms(R, t, X[valid], f[valid], A, a, fcam, W, H, M)
    zbad = bool((~(p["z"] > 1.0)).any())
    d = lambda u, v: np.sum(u * v, axis=1, dtype=np.float32).astype(np.float64)
    gxx, gxy, gyy = d(p["gx"], p["gx"]), d(p["gx"], p["gy"]), d(p["gy"], p["gy"])
    gxr, gyr, rr = d(p["gx"], p["r"]), d(p["gy"], p["r"]), d(p["r"], p["r"])
    q = rr / sigma2
    w = 1.0 / (1.0 + q)
    ax, ay = p["ax"], p["ay"]
    Hm = np.einsum("p,pi,pj->ij", w * gxx, ax, ax) + np.einsum("p,pi,pj->ij", w * gxy, ax, ay) \
        + np.einsum("p,pi,pj->ij", w * gxy, ay, ax) + np.einsum("p,pi,pj->ij", w * gyy, ay, ay)
    g = (w * gxr) @ ax + (w * gyr) @ ay
    return float(np.sum(np.log1p(q))) / max(int(valid.sum()), 1), Hm, g, zbad


def depth_terms(R, t, X, cam, D, tau):
    """Section 14's per-point terms with the tap-consistency test.  -> dict: measurable [P], r [P], J [P, 6] (0 where not measurable),
    spread [P] = max(taps) - min(taps) (inf where the taps are not all inside the image)."""
    fx, fy, cx, cy = cam
    Hd, Wd = D.shape
    Xc = frame_points(R, t, X)
    z = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * Xc[:, 0] / z + cx
        v = fy * Xc[:, 1] / z + cy
        x0f, y0f = np.floor(u), np.floor(v)
        ok = (z > 1.0) & (x0f >= 0) & (x0f + 1 <= Wd - 1) & (y0f >= 0) & (y0f + 1 <= Hd - 1)
    x0 = np.where(ok, x0f, 0).astype(np.int64)
    y0 = np.where(ok, y0f, 0).astype(np.int64)
    al = np.where(ok, u - x0, 0.0)
    be = np.where(ok, v - y0, 0.0)
    Dd = D.astype(np.float64)
    taps = np.stack([Dd[y0, x0], Dd[y0, x0 + 1], Dd[y0 + 1, x0], Dd[y0 + 1, x0 + 1]], 1)
    D00, D10, D01, D11 = taps.T
    spread = np.where(ok, taps.max(1) - taps.min(1), np.inf)
    with np.errstate(invalid="ignore"):
        ok = ok & (taps > 0).all(1) & (spread <= tau)
    d = (1 - be) * ((1 - al) * D00 + al * D10) + be * ((1 - al) * D01 + al * D11)
    zs = np.where(ok, z, 1.0)
    r = np.where(ok, d - zs, 0.0)
    du = (1 - be) * (D10 - D00) + be * (D11 - D01)
    dv = (1 - al) * (D01 - D00) + al * (D11 - D10)
    iz = 1.0 / zs
    q = np.stack([du * fx * iz, dv * fy * iz, -(du * fx * Xc[:, 0] + dv * fy * Xc[:, 1]) * iz * iz - 1.0], 1)
    J = np.concatenate([np.cross(Xc, q), q], 1)
    J[~ok] = 0.0
    return dict(measurable=ok, r=r, J=J, spread=spread)


def depth_system(R, t, X, cam, D, tau):
    """E_d = sum min(r^2, tau^2) / tau^2 / N over all N rows, H_d, g_d over the inliers (not normalised), the inlier mask."""
    p = depth_terms(R, t, X, cam, D, tau)
    with np.errstate(invalid="ignore"):
        inl = p["measurable"] & (np.abs(p["r"]) < tau)
    rho = np.where(inl, p["r"] ** 2, tau * tau) / (tau * tau)
    J, r = p["J"][inl], p["r"][inl]
    return float(rho.sum()) / len(X), J.T @ J, J.T @ r, inl


class Problem:
    """One detection's inputs; the valid set, sigma^2 and the depth decision are frozen at the input pose by start()."""

    def __init__(self, X, f, M, fcam, W, H, A, a, D, cam, tau, depth_weight=1.0):
        self.X, self.f, self.M, self.fcam, self.W, self.H = np.asarray(X, np.float64), np.asarray(f), M, fcam, W, H
        self.A, self.a, self.D, self.cam, self.tau, self.wd = np.asarray(A, np.float64), np.asarray(a, np.float64), D, cam, tau, depth_weight

    def start(self, R, t):
        self.valid = valid_set(R, t, self.X, self.A, self.a, self.fcam, self.W, self.H, self.M)
        self.nv = int(self.valid.sum())
        if self.nv < 6:
            return False
        self.sigma2 = sigma2_at(R, t, self.X, self.f, self.A, self.a, self.fcam, self.W, self.H, self.M, self.valid)
        self.ninl = int(depth_system(R, t, self.X, self.cam, self.D, self.tau)[3].sum())
        self.use_depth = self.wd > 0 and self.ninl >= 6
        return True

    def parts(self, R, t):
        Ef, Hf, gf, zbad = feature_system(R, t, self.X, self.f, self.A, self.a, self.fcam, self.W, self.H, self.M, self.valid, self.sigma2)
        Ed, Hd, gd, _ = depth_system(R, t, self.X, self.cam, self.D, self.tau)
        return (Ef, Hf, gf), (Ed, Hd, gd), zbad

    def system(self, R, t):
        (Ef, Hf, gf), (Ed, Hd, gd), zbad = self.parts(R, t)
        nf = self.nv * self.sigma2
        if not self.use_depth:
            return Ef, Hf / nf, gf / nf, zbad
        nd = len(self.X) * self.tau * self.tau
        return Ef + self.wd * Ed, Hf / nf + self.wd * Hd / nd, gf / nf + self.wd * gd / nd, zbad

    def z_gap(self, R, t):
        """1 - the smallest z_f over the frozen valid set: how far on the wrong side of 1 mm an inadmissible pose's deciding point lies."""
        return 1.0 - float(feature_terms(R, t, self.X[self.valid], self.f[self.valid], self.A, self.a, self.fcam, self.W, self.H, self.M)["z"].min())


def normal_equations(R, t, pr):
    """The kernel's optional [57] output at the input pose: H_f (21) | g_f (6) | E_f, H_d (21) | g_d (6) | E_d, E."""
    assert pr.start(R, t)
    (Ef, Hf, gf), (Ed, Hd, gd), _ = pr.parts(R, t)
    iu = np.triu_indices(6)
    return np.concatenate([Hf[iu], gf, [Ef], Hd[iu], gd, [Ed], [pr.system(R, t)[0]]])


def refine(R, t, pr, iters=30, has_pose=True, **lm):
    """Section 11's Levenberg-Marquardt loop on E.  -> dict R, t, cost_in, cost_out, num_points, num_depth_inliers, iters_used, status, trace (tests/lm_ref.lm_loop; **lm: its fault switches)."""
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    out = dict(R=R.copy(), t=t.copy(), cost_in=0.0, cost_out=0.0, num_points=0, num_depth_inliers=0, iters_used=0, status=2, trace=[])
    if not has_pose or len(pr.X) == 0:
        return out
    ok = pr.start(R, t)
    out["num_points"] = pr.nv
    if not ok:
        return out
    out["num_depth_inliers"] = pr.ninl
    E, Hm, g, _ = pr.system(R, t)
    out["cost_in"] = E
    out.update(lm_ref.lm_loop(pr.system, R, t, E, Hm, g, iters, fr.lm_solve, admissible=lambda zbad: not zbad, z_gap=pr.z_gap, **lm))
    return out


def to_feature_camera(R, t, A, a):
    """The pose model -> feature camera of a pose model -> frame camera."""
    A = np.asarray(A, np.float64)
    return A @ np.asarray(R, np.float64), A @ np.asarray(t, np.float64) + np.asarray(a, np.float64)


def plane_scene(seed, n=200, C=32, grid=37, z0=600.0, cam=(300.0, 310.0, 259.0, 255.0), W=518, H=518):
    """The complementarity scene: n points of a fronto-parallel plane z = z0 in front of one camera that is both the frame's and the
    feature map's (A = I, a = 0), an exact planted depth image (constant z0, W x H) and section 11's planted smooth feature field sampled at
    the points' projections.  The model frame is the camera's, turned and moved: -> (M, D, X, f, (R_gt, t_gt), cam, W, H)."""
    rng = np.random.default_rng(seed)
    M = fr.smooth_field(grid, grid, C, seed)
    uv = np.stack([rng.uniform(60, W - 60, n), rng.uniform(60, H - 60, n)], 1)
    Xc = np.stack([(uv[:, 0] - cam[2]) / cam[0] * z0, (uv[:, 1] - cam[3]) / cam[1] * z0, np.full(n, z0)], 1)
    R = rot_exp(rng.normal(size=3) * 0.3)
    t = np.array([5.0, -8.0, z0])
    X = ((Xc - t) @ R).astype(np.float32).astype(np.float64)      # R^T (Xc - t); what a bank stores is fp32
    f = fr.sample_at(M, R, t, X, cam, W, H)
    D = np.full((H, W), z0, np.float32)
    return M, D, X, f, (R, t), cam, W, H
