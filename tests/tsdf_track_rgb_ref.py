"""numpy fp64 restatement of frame-to-model tracking on shape and colour (TEST HELPER; include/foundpose_amd.h fp_tsdf_track_rgb,
csrc/tsdf_track.hip, foundpose_amd/reconstruct.py with track_color_weight > 0), written from the contract on top of
tests/tsdf_track_ref.py: the trilinear sample of the volume's colour and its gradient, the joint per-point system, the same
Levenberg-Marquardt loop on it, the rule that lifts a frame's points with their colours and the chained driver; and the fixtures --
a volume with colours written by hand, the single-call fixture with its colours, and the ring of an ellipsoid of revolution whose
shape says nothing about the rotation about its axis."""

import functools

import numpy as np

from tests import lm_ref, tsdf_ref
from tests import tsdf_track_ref as tr
from tests.depth_refine_ref import lm_solve

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------- the term
def sample_rgb(vol, g, min_count):
    """The volume's colour at grid coordinates g [P, 3] -> countable bool [P] (inside, all eight rgb_cnt >= min_count), C [P, 3],
    grad C [P, 3 channels, 3 axes] per mm (0 where not countable): tsdf_track_ref.sample's formulas on rgb_sum / rgb_cnt."""
    nx, ny, nz = vol["dims"]
    n = np.array([nx, ny, nz], np.float64)
    with np.errstate(all="ignore"):
        ok = np.all(np.isfinite(g) & (g >= 0.0) & (g < n - 1.0), axis=1)
    gs = np.where(ok[:, None], g, 0.0)
    i0 = np.floor(gs).astype(np.int64)
    a = gs - i0
    cnt, f = [], []
    for q in range(8):
        idx = (i0[:, 2] + (q >> 2), i0[:, 1] + ((q >> 1) & 1), i0[:, 0] + (q & 1))
        c = vol["rgb_cnt"][idx]
        cnt.append(c)
        s = np.stack([vol["rgb_sum"][ch][idx] for ch in range(3)], 1).astype(np.float64)
        with np.errstate(all="ignore"):
            f.append(np.where(c[:, None] > 0, s / c[:, None].astype(np.float64), 0.0))
    ok = ok & np.all(np.stack(cnt) >= min_count, axis=0)
    ax, ay, az = a[:, 0:1], a[:, 1:2], a[:, 2:3]
    lerp = lambda w, lo, hi: (1.0 - w) * lo + w * hi   # noqa: E731
    C = lerp(az, lerp(ay, lerp(ax, f[0], f[1]), lerp(ax, f[2], f[3])), lerp(ay, lerp(ax, f[4], f[5]), lerp(ax, f[6], f[7])))
    h = np.float64(vol["voxel_mm"])
    gx = lerp(az, lerp(ay, f[1] - f[0], f[3] - f[2]), lerp(ay, f[5] - f[4], f[7] - f[6])) / h
    gy = lerp(az, lerp(ax, f[2] - f[0], f[3] - f[1]), lerp(ax, f[6] - f[4], f[7] - f[5])) / h
    gz = lerp(ay, lerp(ax, f[4] - f[0], f[5] - f[1]), lerp(ax, f[6] - f[2], f[7] - f[3])) / h
    grad = np.stack([gx, gy, gz], 2)
    return ok, np.where(ok[:, None], C, 0.0), np.where(ok[:, None, None], grad, 0.0)


def point_terms(vol, R, t, Xc, colors, tau, min_count, max_dist, weight, color_max):
    """-> dict: tsdf_track_ref.point_terms' g, measurable, r, J; inlier [P] (geometric); color_measurable [P]; e [P, 3] (C - c, 0
    where not colour-measurable); channel [P, 3] the channel inliers; Jc [P, 3, 6] the rows of weight * e for the left twist."""
    Xc = np.asarray(Xc, np.float64)
    p = tr.point_terms(vol, R, t, Xc, tau, min_count)
    with np.errstate(all="ignore"):
        inl = p["measurable"] & (np.abs(p["r"]) < max_dist)
    okc, C, gradC = sample_rgb(vol, p["g"], min_count)
    cm = inl & okc
    e = np.where(cm[:, None], C - np.asarray(colors, F32).astype(np.float64), 0.0)
    with np.errstate(all="ignore"):
        channel = cm[:, None] & (np.abs(e) < color_max)
    q = float(weight) * np.einsum("ij,pcj->pci", np.asarray(R, np.float64), gradC)   # weight R grad C_ch
    Jc = np.concatenate([np.cross(q, Xc[:, None, :]), -q], 2)
    return dict(p, inlier=inl, color_measurable=cm, e=e, channel=channel, Jc=Jc)


def residuals(vol, R, t, Xc, colors, tau, min_count, max_dist, weight, color_max):
    """-> r [P] mm, weight * e [P, 3] mm, geometric inlier [P], channel inlier [P, 3]."""
    p = point_terms(vol, R, t, Xc, colors, tau, min_count, max_dist, weight, color_max)
    return p["r"], float(weight) * p["e"], p["inlier"], p["channel"]


def system(vol, R, t, Xc, colors, tau, min_count, max_dist, weight, color_max):
    """The joint system: cost = sum (rho_geom + sum_ch rho_ch) / N, H [6, 6], g [6], the GEOMETRIC inlier mask."""
    p = point_terms(vol, R, t, Xc, colors, tau, min_count, max_dist, weight, color_max)
    inl, ch = p["inlier"], p["channel"]
    lam = np.float64(weight)
    rho = np.where(inl, p["r"] ** 2, np.float64(max_dist) * np.float64(max_dist))
    rho = rho + np.where(ch, (lam * p["e"]) ** 2, (lam * np.float64(color_max)) ** 2).sum(1)
    J, r = p["J"][inl], p["r"][inl]
    Jc, rc = p["Jc"][ch], lam * p["e"][ch]
    return float(rho.sum()) / len(Xc), J.T @ J + Jc.T @ Jc, J.T @ r + Jc.T @ rc, inl


def normal_equations(vol, R, t, Xc, colors, tau, min_count, max_dist, weight, color_max):
    """fp_tsdf_track_rgb's optional [28] output at the input pose: H upper triangle row-major (21), g (6), cost."""
    E, Hm, g, _ = system(vol, R, t, Xc, colors, tau, min_count, max_dist, weight, color_max)
    return np.concatenate([Hm[np.triu_indices(6)], g, [E]])


def track(vol, R, t, Xc, colors, tau, min_count, max_dist, weight, color_max, iters=20, has_pose=True, **lm):
    """tsdf_track_ref.track's loop (refine_terms.hpp's schedule) on the joint system; num_points and the stop on fewer than 6 inliers
    count geometric inliers.  -> dict R, t, cost_in, cost_out, num_points, iters_used, status, trace (tests/lm_ref.lm_loop; **lm: its fault switches)."""
    sys_at = lambda R, t: system(vol, R, t, Xc, colors, tau, min_count, max_dist, weight, color_max)   # noqa: E731
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    out = dict(R=R.copy(), t=t.copy(), cost_in=0.0, cost_out=0.0, num_points=0, iters_used=0, status=2, trace=[])
    if not has_pose or len(Xc) == 0:
        return out
    E, Hm, g, inl = sys_at(R, t)
    out.update(cost_in=E, cost_out=E, num_points=int(inl.sum()))
    if inl.sum() < 6:
        return out
    out.update(lm_ref.lm_loop(sys_at, R, t, E, Hm, g, iters, lm_solve, **lm))
    return out


# ---------------------------------------------------------------------------------------------------------- the driver
def lift_points_rgb(depth, mask, rgb, cam, max_points):
    """tsdf_track_ref.lift_points' points and the colours of the same pixels, uint8 / 255 as an fp32 division (what integration adds
    to the volume) -> ([P, 3] fp32, [P, 3] fp32)."""
    v, u = np.nonzero((np.asarray(mask) != 0) & (np.asarray(depth) > 0))
    step = max(1, -(-len(u) // int(max_points)))
    u, v = u[::step], v[::step]
    return tr.lift_points(depth, mask, cam, max_points), (np.asarray(rgb)[v, u].astype(F32) / F32(255)).astype(F32)


RGB_DEFAULTS = dict(tr.TRACK_DEFAULTS, track_color_weight=0.0, track_color_max=0.25)


def fuse_tracked(frames, given, origin, h, dims, trunc_voxels=4.0, sequence=None, **opts):
    """tsdf_track_ref.fuse_tracked with the two colour options: with track_color_weight > 0 a frame is tracked on the joint objective;
    the score at the result (share, rms, the lost-frame rule) stays geometric.  -> (volume, poses, records)."""
    o = dict(RGB_DEFAULTS, **opts)
    w, cmax = float(o["track_color_weight"]), float(o["track_color_max"])
    tau, md = float(trunc_voxels) * float(h), float(o["track_max_dist_voxels"]) * float(h)
    vol = tsdf_ref.new_volume(origin, h, dims)
    sequence = [0] * len(frames) if sequence is None else list(sequence)
    poses, records, history, lost_run, first = [], [], [], 0, {}
    for k, fr in enumerate(frames):
        if sequence[k] not in first:
            first[sequence[k]] = k
            history = []
        idx = k - first[sequence[k]]
        anchor = idx == 0 or (o["track_anchor_every"] > 0 and idx % o["track_anchor_every"] == 0 and given[k] is not None)
        rec = dict(frame=k, sequence=sequence[k])
        if anchor:
            if given[k] is None:
                raise ValueError(f"frame {k}: the first frame of a sequence has no pose")
            pose, lost_run = np.asarray(given[k], np.float64).reshape(12), 0
            rec.update(role="anchor")
        else:
            T0 = tr.predict(history, idx, o["track_motion"])
            X, col = lift_points_rgb(fr.depth, fr.mask, fr.rgb, fr.cam, o["track_max_points"])
            X = X.astype(np.float64)
            if w > 0:
                out = track(vol, T0[:3, :3], T0[:3, 3], X, col, tau, o["track_min_count"], md, w, cmax, o["track_iters"])
                rec.update(color_weight=w)
            else:
                out = tr.track(vol, T0[:3, :3], T0[:3, 3], X, tau, o["track_min_count"], md, o["track_iters"])
            n, share, rms = tr.score(vol, out["R"], out["t"], X, tau, o["track_min_count"], md)
            kept = share >= o["track_min_inlier_share"] and out["status"] != 2
            rec.update(role="tracked" if kept else "lost", start=np.concatenate([T0[:3, :3].reshape(9), T0[:3, 3]]), points=len(X), inliers_in=out["num_points"],
                       inliers_out=n, share=share, rms=rms, cost_in=out["cost_in"], cost_out=out["cost_out"], iters=out["iters_used"], status=out["status"])
            pose = np.concatenate([out["R"].reshape(9), out["t"]]) if kept else None
            if not kept:
                lost_run += 1
                if lost_run > o["track_max_lost"]:
                    raise RuntimeError(f"frame {k}: tracking lost on more than {o['track_max_lost']} consecutive frames")
            else:
                lost_run = 0
        records.append(rec)
        poses.append(pose)
        if pose is not None:
            tsdf_ref.integrate(vol, fr.depth[None], fr.mask[None], fr.rgb[None], np.array([fr.cam], np.float64), pose[None], tau)
            history.append((idx, tr.to_T(pose[:9], pose[9:])))
    return vol, poses, records


# ---------------------------------------------------------------------------------------------------------- fixtures
def hand_volume_rgb(seed=4):
    """tsdf_track_ref.hand_volume() with colours written by hand: three smooth fields in steps of 1/16, counts 1 .. 4, sums that divide
    back exactly."""
    rng = np.random.default_rng(seed)
    vol = tr.hand_volume()
    nx, ny, nz = vol["dims"]
    k, j, i = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    fields = (0.5 + 0.4 * np.sin(0.5 * i + 0.3 * j), 0.5 + 0.4 * np.cos(0.4 * j - 0.6 * k), 0.5 + 0.03 * (i - j + k))
    cnt = rng.integers(1, 5, size=(nz, ny, nx)).astype(np.int32)
    vol["rgb_cnt"][:] = cnt
    for ch, f in enumerate(fields):
        vol["rgb_sum"][ch] = (np.clip(np.rint(f * 16.0) / 16.0, 0.0, 1.0) * cnt).astype(F32)
    return vol


RGB_WEIGHT, RGB_MAX = 30.0, 0.25


@functools.lru_cache(maxsize=None)
def track_fixture_rgb():
    """tsdf_track_ref.track_fixture() with the colours of its points: those of frame 0's pixels the points were lifted from, and mid
    grey for the three points by hand; the point `channel_out` (a lifted point that is a channel inlier three times over) has its green
    moved by 0.4, beyond color_max.  -> track_fixture()'s dict + colors fp32 [P, 3] + kinds["channel_out"]."""
    fx = dict(tr.track_fixture())
    f = fx["fx"]
    _, col = lift_points_rgb(f["depth"][0], f["mask"][0], f["rgb"][0], f["cams"][0], 16384)
    col = np.concatenate([col, np.full((3, 3), 0.5, F32)]).astype(F32)
    p = point_terms(fixture_volume(), fx["R"], fx["t"], fx["X"].astype(np.float64), col, f["tau"], tr.TRACK_MIN_COUNT, tr.TRACK_MAX_DIST, RGB_WEIGHT, RGB_MAX)
    k = int(np.nonzero(p["channel"].all(1) & (np.abs(p["e"]).max(1) < 0.1))[0][0])
    col[k, 1] = F32(col[k, 1] + (0.4 if col[k, 1] < 0.5 else -0.4))
    fx["colors"], fx["kinds"] = col, dict(fx["kinds"], channel_out=k)
    return fx


def fixture_volume():
    return tr.fixture_volume()


def sized_points_rgb(n, seed=21):
    """tsdf_track_ref.sized_points(n) with colours: every point takes the colour the fixture's volume holds where the TRUE pose lays
    it, rounded to fp32 (mid grey where the volume holds none there), so that colour has something to say at the input pose."""
    fx = tr.track_fixture()
    P = tr.sized_points(n, seed)
    g = tr.grid_coords(fixture_volume(), fx["R_true"], fx["t_true"], P.astype(np.float64))
    ok, C, _ = sample_rgb(fixture_volume(), g, 1)
    return P, np.where(ok[:, None], C, 0.5).astype(F32)


def uncoloured_points(n=40):
    """n of the fixture's lifted points, jittered, that are geometric inliers at the input pose and whose cell has a corner with
    rgb_cnt < min_count: geometry alone can refine them.  -> (X fp32 [n, 3], colors fp32 [n, 3])."""
    fx = track_fixture_rgb()
    rng = np.random.default_rng(5)
    X = fx["X"][:-3].astype(np.float64)
    X = np.concatenate([X + rng.normal(size=X.shape) * s for s in (0.0, 0.5, 1.0, 1.5, 2.0)]).astype(F32)
    col = np.full(X.shape, 0.5, F32)
    p = point_terms(fixture_volume(), fx["R"], fx["t"], X.astype(np.float64), col, fx["fx"]["tau"], tr.TRACK_MIN_COUNT, tr.TRACK_MAX_DIST, RGB_WEIGHT, RGB_MAX)
    pick = np.nonzero(p["inlier"] & ~p["color_measurable"])[0][:n]
    return X[pick], col[pick]


# the ring of an ellipsoid of revolution: shape says nothing about the rotation about z
AMBIGUOUS_AXES = (40.0, 40.0, 48.0)


def albedo(X):
    """The unshaded colour at model points X [..., 3] on the ellipsoid, float in [0.1, 0.9]."""
    X = np.asarray(X, np.float64)
    u = X / np.array(AMBIGUOUS_AXES)
    ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
    return np.stack([0.5 + 0.4 * np.sin(2.0 * np.arctan2(X[..., 1], X[..., 0]) + 1.5 * uz), 0.5 + 0.4 * ux * np.cos(2.0 * uz), 0.5 + 0.4 * np.sin(3.0 * uy + 1.0)], -1)


def render_ellipsoid(pose):
    """One frame of the ellipsoid, analytically: per pixel centre (at integers, the frames' camera) the nearer root of the ray against
    the quadric -> (depth fp32 [H, W] mm, 0 off the object; mask uint8; rgb uint8 = the albedo at the hit, rounded)."""
    R, t = pose[:9].reshape(3, 3), pose[9:]
    fx, fy, cx, cy = tr.RING_CAM
    v, u = np.mgrid[0:tsdf_ref.SEQ_H, 0:tsdf_ref.SEQ_W].astype(np.float64)
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)          # camera-frame ray with z = 1: the parameter is the depth
    inv = 1.0 / np.array(AMBIGUOUS_AXES)
    o, dm = (-R.T @ t) * inv, (d @ R) * inv                                      # origin and direction in the model frame, over the semi-axes
    a, b, c = (dm * dm).sum(-1), (dm * o).sum(-1), float(o @ o) - 1.0
    disc = b * b - a * c
    hit = disc > 0
    s = (-b - np.sqrt(np.where(hit, disc, 0.0))) / a
    hit &= s > 0
    X = (-R.T @ t) + s[..., None] * (d @ R)
    rgb = np.rint(np.clip(albedo(X), 0.0, 1.0) * 255.0).astype(np.uint8)
    return np.where(hit, s, 0.0).astype(F32), hit.astype(np.uint8), np.where(hit[..., None], rgb, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ambiguous_ring():
    """tsdf_track_ref.ring_poses()' 24 frames of the ellipsoid, finished as stored frames -> ([RefFrame], [12-vector true pose])."""
    poses = tr.ring_poses()
    return [tr.finish_frame(*render_ellipsoid(p)) for p in poses], poses


@functools.lru_cache(maxsize=None)
def ambiguous_chain(weight):
    """The restatement's chain over the ambiguous ring from its first pose, "velocity" -> (volume, poses, records); shared: leave it
    unchanged."""
    frames, truth = ambiguous_ring()
    given = [truth[0]] + [None] * (len(frames) - 1)
    return fuse_tracked(frames, given, tr.RING_BOUNDS[0], tr.RING_H, tr.RING_DIMS, tr.RING_TRUNC_VOXELS, track_motion="velocity", track_color_weight=weight,
                        track_color_max=RGB_MAX)
