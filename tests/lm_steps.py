"""The fixtures of the step-by-step Levenberg-Marquardt tests (TEST HELPER; tests/test_lm_steps_cpu.py, tests/test_gpu_lm_steps.py): for each
of the five entry points of csrc/refine_terms.hpp's state machine a few small problems whose restated trajectory (tests/lm_ref.py)
rejects steps on a clear margin, and the PINNED PREFIX of such a trajectory -- the run of iterations before the first one where

  (a) the decision margin |Et - E| / E is below MARGIN (both sides sum the same terms in another order; the suite holds the fp64 sums
      to 1e-9 and the feature solvers' fp32 dot products to 1e-4 of the largest entry, hence their wider margin),
  (b) the restatement on the same points in reversed order decides differently or lands more than 1e-9 (|dR|_F) / 1e-6 mm away,
  (c) a per-point branch (|r| < tau, the tap spread, the map, image and volume bounds, z > 1, the colour bound) of the trial pose is
      closer than 1e-9 relative to flipping, or the z-bad rule refuses it with the deciding z less than 1e-3 mm below 1.

Every fixture is a dict-like Fixture: entry ("depth", "feat", "rgbd", "track", "track_rgb"), name, det (what the GPU tests' _run helpers
take), K (the number of iterations the GPU test sweeps, inside the prefix), run(iters, reverse=False, **switches) -> the restatement's
dict, gaps(R, t) -> the smallest relative distance of a per-point branch from flipping at a pose.  fixture("entry:name") builds one of
SPECS on first use.
"""

import functools

import numpy as np

from tests import depth_refine_ref as dr
from tests import featuremetric_ref as fr
from tests import rgbd_refine_ref as rg
from tests import tsdf_ref
from tests import tsdf_track_ref as tr
from tests import tsdf_track_rgb_ref as rr

MARGIN = {"depth": 1e-6, "track": 1e-6, "track_rgb": 1e-6, "feat": 1e-4, "rgbd": 1e-4}
BRANCH, SPREAD_R, SPREAD_T = 1e-9, 1e-9, 1e-6
Z_GAP = 1e-3                             # mm: how far below z = 1 the deciding point of a step the z-bad rule refuses has to lie
POSE_RAD, POSE_MM = 1e-6, 1e-3          # the project's bar on a pose against the restatement's
K_MAX = 24
DH, DW, DCAM = 80, 96, (180.0, 185.0, 47.3, 39.6)          # the depth image of tests/test_gpu_depth_refine.py
FW = FH = 518
FCAM = (600.0, 605.0, 259.0, 257.0)                         # the feature camera of tests/test_gpu_featuremetric.py
GRID, CH = 37, 64
NPTS = 70                                                   # three chunks of FP_REFINE_CHUNK = 32, the last one ragged
MC = tr.TRACK_MIN_COUNT


def _f64(X):
    return np.asarray(X, np.float32).astype(np.float64)


def _off(rng, R, t, rot_deg, trans_mm):
    ax, dt = rng.normal(size=3), rng.normal(size=3)
    return fr.rot_exp(ax / np.linalg.norm(ax) * np.radians(rot_deg)) @ R, t + dt * trans_mm / np.linalg.norm(dt)


def _rel(*parts):
    """The smallest of the given arrays of relative gaps (inf when all are empty)."""
    parts = [np.abs(np.asarray(p, np.float64)).ravel() for p in parts]
    parts = [p[np.isfinite(p)] for p in parts]
    return min([float(p.min()) for p in parts if p.size] or [np.inf])


def _image_gaps(Xc, cam, W, H):
    z = Xc[:, 2]
    u, v = cam[0] * Xc[:, 0] / z + cam[2], cam[1] * Xc[:, 1] / z + cam[3]
    return [z - 1.0, u / W, (u - (W - 1)) / W, v / H, (v - (H - 1)) / H]


def _map_gaps(Xf, fcam, gw, gh):
    z = Xf[:, 2]
    xm, ym = (fcam[0] * Xf[:, 0] / z + fcam[2]) * (gw / FW) - 0.5, (fcam[1] * Xf[:, 1] / z + fcam[3]) * (gh / FH) - 0.5
    return [z - 1.0, xm / gw, (xm - (gw - 1)) / gw, ym / gh, (ym - (gh - 1)) / gh]


class Fixture:
    def __init__(self, entry, name, det, K, **more):
        self.entry, self.name, self.det, self.K = entry, name, det, K
        self.__dict__.update(more)

    def __repr__(self):
        return f"{self.entry}:{self.name}"

    # ---- the restatement
    def run(self, iters, reverse=False, **lm):
        d, o = self.det, slice(None, None, -1) if reverse else slice(None)
        X = _f64(d["X"])[o]
        hp = d.get("has_pose", True)
        if self.entry == "depth":
            return dr.refine(d["R"], d["t"], X, DCAM, self.D, d["tau"], iters, hp, **lm)
        if self.entry == "feat":
            return fr.refine(d["R"], d["t"], X, d["f"][o], FCAM, FW, FH, self.M, iters, hp, **lm)
        if self.entry == "rgbd":
            pr = rg.Problem(X, d["f"][o], d["M"], d["fcam"], FW, FH, d["A"], d["a"], d["D"], d["cam"], d["tau"], 1.0)
            return rg.refine(d["R"], d["t"], pr, iters, hp, **lm)
        if self.entry == "track":
            return tr.track(self.vol, d["R"], d["t"], X, self.tau, MC, d["md"], iters, hp, **lm)
        return rr.track(self.vol, d["R"], d["t"], X, d["C"][o], self.tau, MC, d["md"], rr.RGB_WEIGHT, rr.RGB_MAX, iters, hp, **lm)

    # ---- condition (c)
    def gaps(self, R, t):
        d = self.det
        X = _f64(d["X"])
        with np.errstate(all="ignore"):
            if self.entry == "depth":
                p = dr.point_terms(R, t, X, DCAM, self.D)
                m = p["measurable"]
                return _rel((np.abs(p["r"][m]) - d["tau"]) / d["tau"], *_image_gaps(p["Xc"], DCAM, DW, DH))
            if self.entry == "feat":
                return _rel(*_map_gaps(X @ np.asarray(R).T + t, FCAM, GRID, GRID))
            if self.entry == "rgbd":
                Xc = rg.frame_points(R, t, X)
                p = rg.depth_terms(R, t, X, d["cam"], d["D"], d["tau"])
                m = p["measurable"]
                Hd, Wd = d["D"].shape
                return _rel((np.abs(p["r"][m]) - d["tau"]) / d["tau"], (p["spread"] - d["tau"]) / d["tau"], *_image_gaps(Xc, d["cam"], Wd, Hd),
                            *_map_gaps(Xc @ np.asarray(d["A"]).T + d["a"], d["fcam"], *d["M"].shape[1::-1]))
            if self.entry == "track":
                p = tr.point_terms(self.vol, R, t, X, self.tau, MC)
                more = []
            else:
                p = rr.point_terms(self.vol, R, t, X, d["C"], self.tau, MC, d["md"], rr.RGB_WEIGHT, rr.RGB_MAX)
                more = [(np.abs(p["e"][p["color_measurable"]]) - rr.RGB_MAX) / rr.RGB_MAX]
            n = np.array(self.vol["dims"], np.float64)
            m = p["measurable"]
            return _rel((np.abs(p["r"][m]) - d["md"]) / d["md"], p["g"] / n, (p["g"] - (n - 1.0)) / n, *more)


@functools.lru_cache(maxsize=None)
def _traces(fx, iters):
    return fx.run(iters), fx.run(iters, reverse=True)


def pinned_prefix(fx, iters=40):
    """-> (length of the pinned prefix, the restatement's dict at `iters`, the largest (|dR|_F, |dt|) between the two point orders over
    the prefix).  Shared: leave the dict unchanged."""
    a, b = _traces(fx, iters)
    spread = [0.0, 0.0]
    if fx.gaps(fx.det["R"], fx.det["t"]) < BRANCH:
        return 0, a, tuple(spread)
    n = 0
    for ra, rb in zip(a["trace"], b["trace"]):
        dR, dt = float(np.linalg.norm(ra["R"] - rb["R"])), float(np.linalg.norm(ra["t"] - rb["t"]))
        if ra["margin"] < MARGIN[fx.entry] or ra["kind"] != rb["kind"] or dR > SPREAD_R or dt > SPREAD_T:
            break
        if ra["trial"] is not None and fx.gaps(*ra["trial"]) < BRANCH:
            break
        if ra["kind"] == "zbad" and ra["z_gap"] < Z_GAP:
            break
        spread = [max(spread[0], dR), max(spread[1], dt)]
        n += 1
    return n, a, tuple(spread)


# ---------------------------------------------------------------------------------------------------------- the step-edge fixtures
def step_depth(H=DH, W=DW, cam=DCAM):
    """tests/depth_refine_ref.analytic_depth with its right half 30 mm nearer."""
    D, _ = dr.analytic_depth(H, W, cam)
    D = D.copy()
    D[:, W // 2:] -= np.float32(30.0)
    return D


def depth_fixture(seed, rot_deg, trans_mm, tau, K):
    rng = np.random.default_rng(seed)
    D = step_depth()
    uv = np.stack([rng.uniform(4, DW - 5, NPTS), rng.uniform(4, DH - 5, NPTS)], 1)
    R, t = fr.rot_exp(rng.normal(size=3) * 0.4), np.array([3.0, -4.0, 600.0])
    X = ((dr.backproject(D, DCAM, uv) - t) @ R).astype(np.float32)
    R0, t0 = _off(rng, R, t, rot_deg, trans_mm)
    return Fixture("depth", f"edge{seed}", dict(X=X, R=R0, t=t0, tau=tau), K, D=D)


def step_field(seed, step=1.0):
    """tests/featuremetric_ref.smooth_field with every channel of its right half moved by `step`: an edge in feature space, across
    which the linear model of a step fails as it does across the depth image's."""
    M = fr.smooth_field(GRID, GRID, CH, seed).copy()
    M[:, GRID // 2:] += np.float32(step)
    return M


def feat_fixture(seed, rot_deg, trans_mm, K, z=600.0, noise=0.1, step=1.0):
    """70 points in front of tests/test_gpu_featuremetric.py's camera with the features step_field has under the true pose, plus noise:
    the cost at the minimum is not a handful of fp32 rounding errors, so a relative margin means something there."""
    rng = np.random.default_rng(seed)
    M = step_field(seed, step)
    uv = rng.uniform(60, FW - 60, size=(NPTS, 2))
    zz = rng.uniform(z - 40.0, z + 40.0, NPTS)
    Xc = np.stack([(uv[:, 0] - FCAM[2]) / FCAM[0] * zz, (uv[:, 1] - FCAM[3]) / FCAM[1] * zz, zz], 1)
    R, t = fr.rot_exp(rng.normal(size=3) * 0.5), np.array([0.0, 0.0, z])
    X = ((Xc - t) @ R).astype(np.float32)
    f = (fr.sample_at(M, R, t, _f64(X), FCAM, FW, FH) + noise * rng.normal(size=(NPTS, CH))).astype(np.float32)
    R0, t0 = _off(rng, R, t, rot_deg, trans_mm)
    return Fixture("feat", f"edge{seed}" if step else f"field{seed}", dict(X=X, f=f, R=R0, t=t0), K, M=M)


def rgbd_fixture(seed, rot_deg, trans_mm, tau, K, Hd=48, Wd=64, noise=0.1):
    """tests/test_gpu_rgbd_refine.py's _scene on the step-edge depth image, one camera for both terms (A = I)."""
    rng = np.random.default_rng(seed)
    cam = (1.9 * Wd, 1.95 * Wd, 0.49 * Wd, 0.52 * Hd)
    D = step_depth(Hd, Wd, cam)
    uv = np.stack([rng.uniform(3, Wd - 4, NPTS), rng.uniform(3, Hd - 4, NPTS)], 1)
    Xc = dr.backproject(D, cam, uv)
    R, t = fr.rot_exp(rng.normal(size=3) * 0.4), np.array([3.0, -4.0, 600.0])
    X = ((Xc - t) @ R).astype(np.float32)
    A = fr.rot_exp(np.array([0.04, -0.06, 0.05]))
    c = Xc.mean(0)
    a = np.array([0.0, 0.0, c[2]]) - A @ c
    ff = 0.75 * FW * cam[0] / Wd
    fcam = (ff, 1.02 * ff, 259.0, 257.0)
    M = fr.smooth_field(GRID, GRID, CH, seed)
    f = (fr.sample_at(M, *rg.to_feature_camera(R, t, A, a), _f64(X), fcam, FW, FH) + noise * rng.normal(size=(NPTS, CH))).astype(np.float32)
    R0, t0 = _off(rng, R, t, rot_deg, trans_mm)
    return Fixture("rgbd", f"edge{seed}_tau{int(tau)}", dict(M=M, D=D, cam=cam, fcam=fcam, A=A, a=a, X=X, f=f, R=R0, t=t0, tau=tau), K)


def track_fixture(seed, rot_deg, trans_mm, md, K, colour=False):
    """70 of tests/tsdf_track_ref.sized_points against integrate_fixture's volume (fused by tests/tsdf_ref.integrate; the GPU test
    uploads these planes), from a start far enough off that steps overshoot."""
    fx = tr.track_fixture()
    rng = np.random.default_rng(seed)
    R0, t0 = _off(rng, fx["R_true"], fx["t_true"], rot_deg, trans_mm)
    det = dict(R=R0, t=t0, md=md)
    if colour:
        det["X"], det["C"] = rr.sized_points_rgb(NPTS, seed)
    else:
        det["X"] = tr.sized_points(NPTS, seed)
    return Fixture("track_rgb" if colour else "track", f"blob{seed}", det, K, vol=tr.fixture_volume(), tau=fx["fx"]["tau"])


# ---------------------------------------------------------------------------------------------------------- the z-bad fixtures
def zbad_fixture(entry, seed, lift, K, rot_deg=2.0, noise=0.1):
    """The planted minimum puts the nearest point at z = 0.5 mm on the optical axis (the others 80 .. 250 mm away); the start lies
    `lift` mm further along z and a little turned, with every point in front of z = 1 mm and inside the map: steps towards the minimum
    that are too long carry that point past z = 1 and are refused however much they lower the cost.  For "rgbd" the two cameras are one
    (A = I) and the depth image lies 5 m away: no depth inliers, the feature term decides alone."""
    rng = np.random.default_rng(seed)
    M = fr.smooth_field(GRID, GRID, CH, seed)
    uv = rng.uniform(80, FW - 80, size=(NPTS, 2))
    zz = rng.uniform(80.0, 250.0, NPTS)
    uv[0], zz[0] = (FCAM[2], FCAM[3]), 0.5
    Xc = np.stack([(uv[:, 0] - FCAM[2]) / FCAM[0] * zz, (uv[:, 1] - FCAM[3]) / FCAM[1] * zz, zz], 1)
    R, t = fr.rot_exp(rng.normal(size=3) * 0.5), np.array([0.0, 0.0, 150.0])
    X = ((Xc - t) @ R).astype(np.float32)
    f = (fr.sample_at(M, R, t, _f64(X), FCAM, FW, FH) + noise * rng.normal(size=(NPTS, CH))).astype(np.float32)
    ax = rng.normal(size=3)
    R0, t0 = fr.rot_exp(ax / np.linalg.norm(ax) * np.radians(rot_deg)) @ R, t + np.array([0.0, 0.0, lift])
    if entry == "feat":
        return Fixture("feat", f"zbad{seed}", dict(X=X, f=f, R=R0, t=t0), K, M=M)
    D = np.full((48, 64), 5000.0, np.float32)
    return Fixture("rgbd", f"zbad{seed}", dict(M=M, D=D, cam=(120.0, 125.0, 31.0, 25.0), fcam=FCAM, A=np.eye(3), a=np.zeros(3), X=X, f=f, R=R0, t=t0, tau=25.0), K)


# ---------------------------------------------------------------------------------------------------------- exact constructions
CEILING_ITERS = (0, 1, 5, 15, 16, 17, 30)


ELLIPSOID = dict(centre=(20.0, 1.0, -1.0), axes=(16.0, 12.0, 9.0))


@functools.lru_cache(maxsize=None)
def hand_volume():
    """integrate_fixture's box with planes written by hand (as tests/tsdf_ref.extract_fixture's), in steps of 1/8 that divide back exactly,
    every count 2, one colour everywhere.  Voxels 0 .. 15 along x: f depends on the model's z alone, so under an identity rotation a
    point's Jacobian has no entry for the rotation about z or the translation along x and y.  The rest: an ellipsoid of three different
    axes, which constrains all six (the mixed batch's descending problem).  Shared: leave it unchanged."""
    f = tsdf_ref.integrate_fixture()
    vol = tsdf_ref.new_volume(f["origin"], f["h"], f["dims"])
    X, Y, Z = (tsdf_ref.centres(f["origin"][a], n, f["h"]) for a, n in enumerate(f["dims"]))
    X, Y, Z = X[None, None, :], Y[None, :, None], Z[:, None, None]
    (cx, cy, cz), ax = ELLIPSOID["centre"], ELLIPSOID["axes"]
    s = np.sqrt(((X - cx) / ax[0]) ** 2 + ((Y - cy) / ax[1]) ** 2 + ((Z - cz) / ax[2]) ** 2)
    phi = np.where(np.arange(f["dims"][0])[None, None, :] < 16, Z / f["tau"] + 0.0 * X * Y, (s - 1.0) * min(ax) / f["tau"])
    phi = np.clip(np.rint(phi * 8.0) / 8.0, -1.0, 1.0)
    vol["sdf_cnt"][:] = 2
    vol["sdf_sum"][:] = (phi * 2).astype(np.float32)
    vol["rgb_cnt"][:] = 2
    vol["rgb_sum"][:] = np.float32(0.5 * 2)
    return vol


@functools.lru_cache(maxsize=None)
def ceiling_fixture(entry):
    """A problem with a positive cost whose normal matrix has an exactly zero diagonal entry at every lambda: every factorisation fails,
    lambda climbs from 1e-3 by x 10 until it passes 1e12, the pose never moves, status 1."""
    rng = np.random.default_rng(3)
    if entry == "depth":          # the constant image 602 mm over the plane z = 600: du = dv = 0, J = (-y, x, 0, 0, 0, -1)
        uv = np.stack([rng.uniform(4, DW - 5, NPTS), rng.uniform(4, DH - 5, NPTS)], 1)
        X = np.stack([(uv[:, 0] - DCAM[2]) / DCAM[0] * 600.0, (uv[:, 1] - DCAM[3]) / DCAM[1] * 600.0, np.full(NPTS, 600.0)], 1).astype(np.float32)
        return Fixture("depth", "ceiling", dict(X=X, R=np.eye(3), t=np.zeros(3), tau=25.0), 0, D=np.full((DH, DW), 602.0, np.float32))
    if entry in ("feat", "rgbd"):  # one feature vector over the whole map, other features at the points: no map gradient, H = 0
        M = np.broadcast_to(rng.normal(size=CH).astype(np.float32), (GRID, GRID, CH)).copy()
        uv, zz = rng.uniform(60, FW - 60, size=(NPTS, 2)), rng.uniform(560.0, 640.0, NPTS)
        X = np.stack([(uv[:, 0] - FCAM[2]) / FCAM[0] * zz, (uv[:, 1] - FCAM[3]) / FCAM[1] * zz, zz], 1).astype(np.float32)
        f = rng.normal(size=(NPTS, CH)).astype(np.float32)
        if entry == "feat":
            return Fixture("feat", "ceiling", dict(X=X, f=f, R=np.eye(3), t=np.zeros(3)), 0, M=M)
        D = np.full((48, 64), 5000.0, np.float32)      # no depth inlier either: the feature term stands alone
        return Fixture("rgbd", "ceiling", dict(M=M, D=D, cam=(120.0, 125.0, 31.0, 25.0), fcam=FCAM, A=np.eye(3), a=np.zeros(3), X=X, f=f, R=np.eye(3), t=np.zeros(3),
                                               tau=25.0), 0)
    vol = hand_volume()
    lo, hi = np.array(vol["origin"]) + 3 * vol["voxel_mm"], np.array(vol["origin"]) + (np.array([13, vol["dims"][1] - 3, 0])) * vol["voxel_mm"]
    X = np.stack([rng.uniform(lo[0], hi[0], NPTS), rng.uniform(lo[1], hi[1], NPTS), rng.uniform(2.0, 5.0, NPTS)], 1).astype(np.float32)
    det = dict(X=X, R=np.eye(3), t=np.zeros(3), md=tr.TRACK_MAX_DIST)
    if entry == "track_rgb":
        det["C"] = rng.uniform(0.3, 0.7, size=(NPTS, 3)).astype(np.float32)
    return Fixture(entry, "ceiling", det, 0, vol=vol, tau=tsdf_ref.integrate_fixture()["tau"])


@functools.lru_cache(maxsize=None)
def mixed_batch(entry):
    """Four problems that one call can hold and that go inactive at different launches: the ceiling problem, a problem that descends and
    rejects, one with fewer than 6 points, one without a pose.  The trackers' problems share one volume, the ceiling problem's: their
    descending problem lies on the ellipsoid of hand_volume()."""
    c = ceiling_fixture(entry)
    if entry in ("track", "track_rgb"):
        rng = np.random.default_rng(8)
        u = rng.normal(size=(NPTS, 3))
        X = (np.array(ELLIPSOID["centre"]) + u / np.linalg.norm(u, axis=1, keepdims=True) * np.array(ELLIPSOID["axes"])).astype(np.float32)
        det = dict(c.det, X=X, R=fr.rot_exp(np.array([0.05, -0.04, 0.06])), t=np.array([1.5, -2.0, 1.0]))
        d = Fixture(entry, "ellipsoid", det, 0, vol=c.vol, tau=c.tau)
    else:
        d = fixtures(entry)[0]
    few = {k: (v[:5] if k in ("X", "f", "C") else v) for k, v in d.det.items()}
    more = {k: v for k, v in d.__dict__.items() if k not in ("entry", "name", "det", "K")}
    return [c, d, Fixture(entry, "few", few, 0, **more), Fixture(entry, "nopose", dict(d.det, has_pose=False), 0, **more)]


MIXED_ITERS = (20, 5, 16)

# ---------------------------------------------------------------------------------------------------------- the committed fixtures
# "entry:name" -> (builder, arguments): (seed, start, ...) chosen by a search over seeds 0 .. 7 for trajectories that hold what
# tests/test_lm_steps_cpu.py asks for; K is min(pinned prefix, 24) as that test recomputes it.  Built on first use, not at import.
SPECS = {
    "depth:edge0": (depth_fixture, (0, 6.0, 25.0, 25.0, 24), {}),
    "depth:edge5": (depth_fixture, (5, 10.0, 40.0, 15.0, 24), {}),
    "depth:edge2": (depth_fixture, (2, 6.0, 25.0, 25.0, 24), {}),
    "feat:edge7": (feat_fixture, (7, 30.0, 120.0, 24), dict(step=6.0, noise=1.0)),
    "feat:edge0": (feat_fixture, (0, 30.0, 120.0, 18), dict(step=6.0, noise=2.0)),
    "feat:zbad1": (zbad_fixture, ("feat", 1, 6.0, 18), {}),
    "feat:zbad0": (zbad_fixture, ("feat", 0, 12.0, 21), {}),
    "feat:field0": (feat_fixture, (0, 10.0, 40.0, 4), dict(step=0.0)),
    "rgbd:edge5_tau25": (rgbd_fixture, (5, 6.0, 25.0, 25.0, 24), {}),
    "rgbd:zbad1": (zbad_fixture, ("rgbd", 1, 6.0, 18), {}),
    "rgbd:edge5_tau15": (rgbd_fixture, (5, 10.0, 40.0, 15.0, 24), {}),
    "track:blob0": (track_fixture, (0, 6.0, 6.0, 7.5, 24), {}),
    "track:blob4": (track_fixture, (4, 15.0, 12.0, 5.0, 24), {}),
    "track_rgb:blob3": (track_fixture, (3, 6.0, 6.0, 7.5, 24), dict(colour=True)),
    "track_rgb:blob4": (track_fixture, (4, 15.0, 12.0, 5.0, 24), dict(colour=True)),
}
ENTRIES = ("depth", "feat", "rgbd", "track", "track_rgb")
IDS = tuple(SPECS)
ZBAD_IDS = tuple(i for i in IDS if ":zbad" in i)


@functools.lru_cache(maxsize=None)
def fixture(fid):
    build, args, kw = SPECS[fid]
    fx = build(*args, **kw)
    assert repr(fx) == fid, (fx, fid)
    return fx


def fixtures(entry):
    return [fixture(i) for i in IDS if i.startswith(entry + ":")]
