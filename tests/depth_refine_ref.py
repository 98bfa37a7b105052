"""numpy fp64 restatement of the depth refinement contract (csrc/depth_refine.hip computes it on the GPU).

Per detection: the template's points X [P, 3] (model mm), the frame's depth image D [H, W] fp32 (mm, 0 = no measurement), the
frame's pinhole camera (fx, fy, cx, cy) with pixel centres at integer coordinates, the input pose (R, t) and the truncation
distance tau (mm).  Everything after the fp32 taps is fp64.
"""

import numpy as np

from tests import lm_ref
from tests.featuremetric_ref import rot_angle_deg, rot_exp, update  # noqa: F401  (the same twist and update as section 11)


def point_terms(R, t, X, cam, D):
    """-> dict: Xc [P, 3], z, measurable [P] bool, r [P] (0 where not measurable), J [P, 6] (0 where not measurable)."""
    fx, fy, cx, cy = cam
    H, W = D.shape
    Xc = np.asarray(X, np.float64) @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    z = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * Xc[:, 0] / z + cx
        v = fy * Xc[:, 1] / z + cy
        x0f, y0f = np.floor(u), np.floor(v)
        ok = (z > 1.0) & (x0f >= 0) & (x0f + 1 <= W - 1) & (y0f >= 0) & (y0f + 1 <= H - 1)
    x0 = np.where(ok, x0f, 0).astype(np.int64)
    y0 = np.where(ok, y0f, 0).astype(np.int64)
    al = np.where(ok, u - x0, 0.0)
    be = np.where(ok, v - y0, 0.0)
    Dd = D.astype(np.float64)
    D00, D10, D01, D11 = Dd[y0, x0], Dd[y0, x0 + 1], Dd[y0 + 1, x0], Dd[y0 + 1, x0 + 1]   # (never the +1 tap of a point that is not ok)
    ok = ok & (D00 > 0) & (D10 > 0) & (D01 > 0) & (D11 > 0)
    d = (1 - be) * ((1 - al) * D00 + al * D10) + be * ((1 - al) * D01 + al * D11)
    zs = np.where(ok, z, 1.0)
    r = np.where(ok, d - zs, 0.0)
    du = (1 - be) * (D10 - D00) + be * (D11 - D01)
    dv = (1 - al) * (D01 - D00) + al * (D11 - D10)
    iz = 1.0 / zs
    q = np.stack([du * fx * iz, dv * fy * iz, -(du * fx * Xc[:, 0] + dv * fy * Xc[:, 1]) * iz * iz - 1.0], 1)   # dr/dXc
    J = np.concatenate([np.cross(Xc, q), q], 1)   # dr/dXc [-[Xc]x | I]
    J[~ok] = 0.0
    return dict(Xc=Xc, z=z, measurable=ok, r=r, J=J)


def residual(R, t, X, cam, D):
    """r [P] and the measurable mask."""
    p = point_terms(R, t, X, cam, D)
    return p["r"], p["measurable"]


def system(R, t, X, cam, D, tau):
    """cost = sum rho / N, H [6, 6], g [6] over the inliers, the inlier mask."""
    p = point_terms(R, t, X, cam, D)
    inl = p["measurable"] & (np.abs(p["r"]) < tau)
    rho = np.where(inl, p["r"] ** 2, tau * tau)
    J, r = p["J"][inl], p["r"][inl]
    return float(rho.sum()) / len(X), J.T @ J, J.T @ r, inl


def normal_equations(R, t, X, cam, D, tau):
    """The kernel's optional [28] output at the input pose: H upper triangle row-major (21), g (6), cost."""
    E, Hm, g, _ = system(R, t, X, cam, D, tau)
    return np.concatenate([Hm[np.triu_indices(6)], g, [E]])


def lm_solve(Hm, g, lam):
    A = Hm + lam * np.diag(np.diag(Hm))
    if not np.all(np.isfinite(A)) or not np.all(np.diag(A) > 0):
        return None
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.isfinite(L)):
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, -g))


def refine(R, t, X, cam, D, tau, iters=30, has_pose=True, **lm):
    """The Levenberg-Marquardt loop of section 11 on the depth term.  -> dict R, t, cost_in, cost_out, num_points (inliers at the
    input pose), iters_used, status, trace (tests/lm_ref.lm_loop; **lm: its fault switches)."""
    R = np.asarray(R, np.float64)
    t = np.asarray(t, np.float64)
    out = dict(R=R.copy(), t=t.copy(), cost_in=0.0, cost_out=0.0, num_points=0, iters_used=0, status=2, trace=[])
    if not has_pose or len(X) == 0:
        return out
    E, Hm, g, inl = system(R, t, X, cam, D, tau)
    out.update(cost_in=E, cost_out=E, num_points=int(inl.sum()))
    if inl.sum() < 6:
        return out
    out.update(lm_ref.lm_loop(lambda R, t: system(R, t, X, cam, D, tau), R, t, E, Hm, g, iters, lm_solve, **lm))
    return out


def analytic_depth(H, W, cam, z0=600.0, tilt=(0.15, -0.1), curv=4e-4):
    """A planted depth image [H, W] fp32 and its generator: a tilted plane plus a paraboloid in normalised image coordinates,
    z(u, v) = z0 (1 + tilt . n + curv' |n - n0|^2), which constrains all six degrees of freedom.  -> (D, fn(u, v) -> z)."""
    fx, fy, cx, cy = cam

    def fn(u, v):
        nx, ny = (np.asarray(u, np.float64) - cx) / fx, (np.asarray(v, np.float64) - cy) / fy
        return z0 * (1.0 + tilt[0] * nx + tilt[1] * ny + curv * z0 * ((nx - 0.01) ** 2 + 1.5 * (ny + 0.02) ** 2))
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return fn(uu, vv).astype(np.float32), fn


def backproject(D, cam, uv):
    """Camera-frame points on the BILINEAR surface of D at pixel coordinates uv [P, 2] (inside the image, on measured taps)."""
    fx, fy, cx, cy = cam
    u, v = uv[:, 0], uv[:, 1]
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    al, be = u - x0, v - y0
    Dd = D.astype(np.float64)
    z = (1 - be) * ((1 - al) * Dd[y0, x0] + al * Dd[y0, x0 + 1]) + be * ((1 - al) * Dd[y0 + 1, x0] + al * Dd[y0 + 1, x0 + 1])
    return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
