"""numpy fp64 restatement of frame-to-model tracking against a TSDF volume (TEST HELPER; include/foundpose_amd.h, csrc/tsdf_track.hip,
foundpose_amd/reconstruct.py with pose_source "track"), written from the contract: the trilinear sample of the
volume and its gradient, the per-point system, the Levenberg-Marquardt loop with refine_terms.hpp's schedule, the rule that lifts a
frame's masked depth pixels, the two motion models and the chained track / integrate driver.  Fusion is tests/tsdf_ref.integrate."""

import functools
import json
import os

import numpy as np

from tests import lm_ref, tsdf_ref
from tests.depth_refine_ref import lm_solve
from tests.featuremetric_ref import rot_angle_deg, rot_exp, update  # noqa: F401

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------- the term
def grid_coords(vol, R, t, Xc):
    """-> g fp64 [P, 3]: the grid coordinates of the camera-frame points under the model -> camera pose (R, t)."""
    d = np.asarray(Xc, np.float64) - np.asarray(t, np.float64)
    Xm = d @ np.asarray(R, np.float64)                     # X_m[i] = R[0][i] d0 + R[1][i] d1 + R[2][i] d2
    with np.errstate(all="ignore"):
        return (Xm - np.asarray(vol["origin"], np.float64)) / np.float64(vol["voxel_mm"]) - 0.5


def sample(vol, g, min_count):
    """The volume at grid coordinates g [P, 3] -> measurable bool [P], phi [P], grad phi [P, 3] per mm (0 where not measurable)."""
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
        c = vol["sdf_cnt"][idx]
        cnt.append(c)
        with np.errstate(all="ignore"):
            f.append(np.where(c > 0, vol["sdf_sum"][idx].astype(np.float64) / c.astype(np.float64), 0.0))
    ok = ok & np.all(np.stack(cnt) >= min_count, axis=0)
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    lerp = lambda w, lo, hi: (1.0 - w) * lo + w * hi   # noqa: E731
    phi = lerp(az, lerp(ay, lerp(ax, f[0], f[1]), lerp(ax, f[2], f[3])), lerp(ay, lerp(ax, f[4], f[5]), lerp(ax, f[6], f[7])))
    h = np.float64(vol["voxel_mm"])
    gx = lerp(az, lerp(ay, f[1] - f[0], f[3] - f[2]), lerp(ay, f[5] - f[4], f[7] - f[6])) / h
    gy = lerp(az, lerp(ax, f[2] - f[0], f[3] - f[1]), lerp(ax, f[6] - f[4], f[7] - f[5])) / h
    gz = lerp(ay, lerp(ax, f[4] - f[0], f[5] - f[1]), lerp(ax, f[6] - f[2], f[7] - f[3])) / h
    grad = np.stack([gx, gy, gz], 1)
    return ok, np.where(ok, phi, 0.0), np.where(ok[:, None], grad, 0.0)


def point_terms(vol, R, t, Xc, tau, min_count):
    """-> dict: g [P, 3], measurable [P], r [P] mm (0 where not measurable), J [P, 6] for the left twist (0 where not measurable)."""
    Xc = np.asarray(Xc, np.float64)
    g = grid_coords(vol, R, t, Xc)
    ok, phi, grad = sample(vol, g, min_count)
    q = float(tau) * grad @ np.asarray(R, np.float64).T     # tau R grad phi: the gradient in the camera frame
    J = np.concatenate([np.cross(q, Xc), -q], 1)
    return dict(g=g, measurable=ok, r=float(tau) * phi, J=J)


def residual(vol, R, t, Xc, tau, min_count):
    p = point_terms(vol, R, t, Xc, tau, min_count)
    return p["r"], p["measurable"]


def system(vol, R, t, Xc, tau, min_count, max_dist):
    """cost = sum rho / N, H [6, 6], g [6] over the inliers, the inlier mask."""
    p = point_terms(vol, R, t, Xc, tau, min_count)
    with np.errstate(all="ignore"):
        inl = p["measurable"] & (np.abs(p["r"]) < max_dist)
    rho = np.where(inl, p["r"] ** 2, np.float64(max_dist) * np.float64(max_dist))
    J, r = p["J"][inl], p["r"][inl]
    return float(rho.sum()) / len(Xc), J.T @ J, J.T @ r, inl


def normal_equations(vol, R, t, Xc, tau, min_count, max_dist):
    """The kernel's optional [28] output at the input pose: H upper triangle row-major (21), g (6), cost."""
    E, Hm, g, _ = system(vol, R, t, Xc, tau, min_count, max_dist)
    return np.concatenate([Hm[np.triu_indices(6)], g, [E]])


def track(vol, R, t, Xc, tau, min_count, max_dist, iters=20, has_pose=True, **lm):
    """The Levenberg-Marquardt loop of refine_terms.hpp on the term above: lambda from 1e-3, / 10 on accept (floor 1e-12), x 10 on reject
    or failed Cholesky (which counts as an iteration), stop at lambda > 1e12, at a relative decrease < 1e-10 or at `iters`.
    -> dict R, t, cost_in, cost_out, num_points (inliers at the input pose), iters_used, status, trace (tests/lm_ref.lm_loop; **lm: its fault switches)."""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    out = dict(R=R.copy(), t=t.copy(), cost_in=0.0, cost_out=0.0, num_points=0, iters_used=0, status=2, trace=[])
    if not has_pose or len(Xc) == 0:
        return out
    E, Hm, g, inl = system(vol, R, t, Xc, tau, min_count, max_dist)
    out.update(cost_in=E, cost_out=E, num_points=int(inl.sum()))
    if inl.sum() < 6:
        return out
    out.update(lm_ref.lm_loop(lambda R, t: system(vol, R, t, Xc, tau, min_count, max_dist), R, t, E, Hm, g, iters, lm_solve, **lm))
    return out


# ---------------------------------------------------------------------------------------------------------- the driver
def lift_points(depth, mask, cam, max_points):
    """The pixels with mask != 0 and depth > 0 in row-major order, every ceil(n / max_points)-th of them, lifted through the camera
    (pixel centres at integers) in fp64 and rounded to fp32 -> [P, 3]."""
    fx, fy, cx, cy = (np.float64(c) for c in cam)
    v, u = np.nonzero((np.asarray(mask) != 0) & (np.asarray(depth) > 0))
    step = max(1, -(-len(u) // int(max_points)))
    u, v = u[::step], v[::step]
    d = np.asarray(depth)[v, u].astype(np.float64)
    return np.stack([(u - cx) / fx * d, (v - cy) / fy * d, d], 1).astype(F32)


def to_T(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return T


def predict(history, index, motion):
    """The start pose (4 x 4) of frame `index` of a sequence from `history` = [(frame index, T)] of its kept frames: "hold" the last
    kept pose; "velocity" T1 T2^-1 T1 of the two frames before it when both were kept (R re-orthonormalised by SVD), else "hold"."""
    T1 = history[-1][1]
    if motion == "velocity" and len(history) >= 2 and history[-1][0] == index - 1 and history[-2][0] == index - 2:
        T = T1 @ np.linalg.inv(history[-2][1]) @ T1
        U, _, Vt = np.linalg.svd(T[:3, :3])
        T = T.copy()
        T[:3, :3] = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
        T[3] = (0.0, 0.0, 0.0, 1.0)
        return T
    return T1.copy()


TRACK_DEFAULTS = dict(track_anchor_every=0, track_iters=20, track_max_dist_voxels=3.0, track_min_count=1, track_max_points=16384,
                      track_motion="velocity", track_min_inlier_share=0.5, track_max_lost=3)


def score(vol, R, t, Xc, tau, min_count, max_dist):
    """-> (inliers, share, RMS r over the inliers) at a pose."""
    if len(Xc) == 0:
        return 0, 0.0, 0.0
    p = point_terms(vol, R, t, Xc, tau, min_count)
    inl = p["measurable"] & (np.abs(p["r"]) < max_dist)
    n = int(inl.sum())
    return n, n / len(Xc), float(np.sqrt(np.mean(p["r"][inl] ** 2))) if n else 0.0


def fuse_tracked(frames, given, origin, h, dims, trunc_voxels=4.0, sequence=None, **opts):
    """The chained driver: frames (depth, mask, rgb, cam attributes) go through one at a time, in order.  given[k]: a 12-vector pose or
    None; sequence[k]: the sequence a frame belongs to (None: one sequence).  -> (volume, poses [12-vector or None], records)."""
    o = dict(TRACK_DEFAULTS, **opts)
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
            T0 = predict(history, idx, o["track_motion"])
            X = lift_points(fr.depth, fr.mask, fr.cam, o["track_max_points"]).astype(np.float64)
            out = track(vol, T0[:3, :3], T0[:3, 3], X, tau, o["track_min_count"], md, o["track_iters"])
            n, share, rms = score(vol, out["R"], out["t"], X, tau, o["track_min_count"], md)
            kept = share >= o["track_min_inlier_share"] and out["status"] != 2
            rec.update(role="tracked" if kept else "lost", start=np.concatenate([T0[:3, :3].reshape(9), T0[:3, 3]]), points=len(X), inliers_in=out["num_points"], inliers_out=n, share=share, rms=rms,
                       cost_in=out["cost_in"], cost_out=out["cost_out"], iters=out["iters_used"], status=out["status"])
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
            history.append((idx, to_T(pose[:9], pose[9:])))
    return vol, poses, records


def mesh_from_volume(vol, min_count, largest_component):
    """tsdf_ref.mesh_from_frames' second half on a fused volume: extract, weld, keep the largest component, drop unused vertices."""
    _, keys, pos, col = tsdf_ref.extract(vol, min_count)
    v, c, faces = tsdf_ref.weld(keys, pos, col)
    faces = faces[largest_component(faces, len(v))]
    used = np.zeros(len(v), bool)
    used[faces.reshape(-1)] = True
    return v[used], np.clip(c[used], 0, 1), (np.cumsum(used) - 1)[faces].astype(np.int32)


def pose_error(pose, truth):
    """(rotation error in degrees, |dt| of the object origin in the camera, mm) between two 12-vector poses."""
    return rot_angle_deg(pose[:9].reshape(3, 3), truth[:9].reshape(3, 3)), float(np.linalg.norm(pose[9:] - truth[9:]))


# ---------------------------------------------------------------------------------------------------------- fixtures
class RefFrame:
    def __init__(self, depth, mask, rgb, cam):
        self.depth, self.mask, self.rgb, self.cam = depth, mask, rgb, cam


def hand_volume(dims=(14, 12, 11), h=2.0, origin=(-13.7, -12.2, -11.1), axes=(9.0, 7.0, 6.0), tau=4.0, seed=2):
    """A volume written by hand for the Jacobian check: f of an ellipsoid in steps of 1/8, counts 1 .. 4, sums that divide back
    exactly (as tsdf_ref.extract_fixture's)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    vol = tsdf_ref.new_volume(origin, h, dims)
    X, Y, Z = (tsdf_ref.centres(origin[a], n, h) for a, n in enumerate(dims))
    X, Y, Z = X[None, None, :], Y[None, :, None], Z[:, None, None]
    s = np.sqrt((X / axes[0]) ** 2 + (Y / axes[1]) ** 2 + (Z / axes[2]) ** 2)
    f = np.clip(np.rint((s - 1.0) * min(axes) / tau * 8.0) / 8.0, -1.0, 1.0)
    cnt = rng.integers(1, 5, size=f.shape).astype(np.int32)
    vol["sdf_cnt"][:] = cnt
    vol["sdf_sum"][:] = (f * cnt).astype(F32)
    return vol


TRACK_MIN_COUNT, TRACK_MAX_DIST = 2, 7.5


@functools.lru_cache(maxsize=None)
def track_fixture():
    """The single-call fixture: tsdf_ref.integrate_fixture()'s five frames (fused by the caller: tsdf_ref.integrate here, ops.tsdf_integrate on
    the GPU), the points of its frame 0 lifted through its camera, plus three points by hand -- the model's origin, deep inside the
    object where no frame measured (a corner below min_count); a point 50 mm in front of the camera, far outside the volume; a lifted
    point pulled 9 mm towards the camera, into truncated free space -- and an input pose 2 degrees / 2 mm off frame 0's.
    -> dict(fx = integrate_fixture(), X fp32 [P, 3], R, t, R_true, t_true, kinds = indices of the three points by hand)."""
    fx = tsdf_ref.integrate_fixture()
    rng = np.random.default_rng(11)
    Rt, tt = fx["poses"][0][:9].reshape(3, 3), fx["poses"][0][9:]
    ax, dt = rng.normal(size=3), rng.normal(size=3)
    R = rot_exp(ax / np.linalg.norm(ax) * np.radians(2.0)) @ Rt
    t = tt + dt * 2.0 / np.linalg.norm(dt)
    X = lift_points(fx["depth"][0], fx["mask"][0], fx["cams"][0], 16384)
    mid = X[len(X) // 2].astype(np.float64)
    extra = np.array([t, [0.0, 0.0, 50.0], mid * (1.0 - 9.0 / np.linalg.norm(mid))])
    X = np.concatenate([X, extra.astype(F32)])
    n = len(X)
    return dict(fx=fx, X=X, R=R, t=t, R_true=Rt, t_true=tt, kinds=dict(unseen=n - 3, outside=n - 2, free=n - 1))


@functools.lru_cache(maxsize=None)
def fixture_volume():
    """The fixture's volume by tsdf_ref.integrate (shared: leave it unchanged)."""
    fx = track_fixture()["fx"]
    vol = tsdf_ref.new_volume(fx["origin"], fx["h"], fx["dims"])
    return tsdf_ref.integrate(vol, fx["depth"], fx["mask"], fx["rgb"], fx["cams"], fx["poses"], fx["tau"])


def sized_points(n, seed=21):
    """n points for the chunk-fold sizes: the fixture's lifted points (not the three by hand) in a seeded order, the inliers at the
    input pose first (so that six points are six inliers), repeated with a jitter of 0.3 mm when n exceeds them."""
    fx = track_fixture()
    X = fx["X"][:-3].astype(np.float64)
    rng = np.random.default_rng(seed)
    idx = rng.permutation(len(X))
    inl = system(fixture_volume(), fx["R"], fx["t"], X, fx["fx"]["tau"], TRACK_MIN_COUNT, TRACK_MAX_DIST)[3]
    idx = np.concatenate([idx[inl[idx]], idx[~inl[idx]]])
    reps = -(-n // len(X))
    P = np.concatenate([X[idx] + (rng.normal(size=(len(X), 3)) * 0.3 if r else 0.0) for r in range(reps)])
    return P[:n].astype(F32)


RING_FRAMES, RING_STEP_DEG, RING_ELEVATION = 24, 5.0, 0.35
RING_H, RING_DIMS, RING_TRUNC_VOXELS = 2.5, (64, 52, 44), 4.0
RING_BOUNDS = ((-80.0, -65.0, -55.0), (80.0, 65.0, 55.0))
RING_CAM = (tsdf_ref.SEQ_K[0, 0], tsdf_ref.SEQ_K[1, 1], tsdf_ref.SEQ_K[0, 2], tsdf_ref.SEQ_K[1, 2])


def ring_poses(n=RING_FRAMES, step_deg=RING_STEP_DEG, start_deg=0.0):
    """[12-vector] model -> camera of a camera on a ring: 400 mm from the origin, elevation 0.35 rad, azimuth in steps."""
    out = []
    for k in range(n):
        az = np.radians(start_deg + k * step_deg)
        eye = tsdf_ref.SEQ_DISTANCE * np.array([np.cos(RING_ELEVATION) * np.cos(az), np.cos(RING_ELEVATION) * np.sin(az), np.sin(RING_ELEVATION)])
        R, t = tsdf_ref.look_at_pose(eye)
        out.append(np.concatenate([R.reshape(9), t]))
    return out


def ring_mesh():
    from foundpose_amd.synthetic import make_blob_mesh
    return make_blob_mesh(24, 24, radius=40)


def finish_frame(depth, mask, rgb=None):
    """What a stored frame holds: the background plane at 1 000 mm behind the object, depth in steps of 0.1 mm."""
    d = np.where(mask > 0, depth, F32(tsdf_ref.SEQ_BACKGROUND))
    d = np.clip(np.rint(d / tsdf_ref.SEQ_DEPTH_SCALE), 0, 65535).astype(np.uint16).astype(F32) * F32(tsdf_ref.SEQ_DEPTH_SCALE)
    rgb = np.zeros(depth.shape + (3,), np.uint8) if rgb is None else rgb
    return RefFrame(d, np.where(mask > 0, 255, 0).astype(np.uint8), rgb, RING_CAM)


@functools.lru_cache(maxsize=None)
def ring_frames_cpu(n=RING_FRAMES, step_deg=RING_STEP_DEG, start_deg=0.0):
    """The ring rendered by tests/render_ref.rasterize (depth only; the rasterizer samples at pixel centres x + 1/2, the frames' camera has
    them at integers: the principal point is shifted).  -> ([RefFrame], [12-vector true pose])."""
    from tests import render_ref
    mesh, poses, frames = ring_mesh(), ring_poses(n, step_deg, start_deg), []
    cam = np.array([RING_CAM[0], RING_CAM[1], RING_CAM[2] + 0.5, RING_CAM[3] + 0.5])
    for p in poses:
        depth, tri, _ = render_ref.rasterize(mesh.vertices, mesh.faces, tsdf_ref.render_cam(cam, p[:9].reshape(3, 3), p[9:]), tsdf_ref.SEQ_W, tsdf_ref.SEQ_H)
        frames.append(finish_frame(np.where(tri >= 0, depth, 0).astype(F32), (tri >= 0).astype(np.uint8)))
    return frames, poses


def write_ring_scene(scene_dir, color, depth, mask, poses, with_gt=None):
    """A BOP scene directory of the ring with tsdf_ref.write_scene's file conventions: color float [N, H, W, 3] in [0, 1], depth fp32 mm,
    mask uint8; scene_gt.json holds the frames of `with_gt` (None: all)."""
    from PIL import Image
    for sub in ("rgb", "depth", "mask_visib"):
        os.makedirs(os.path.join(scene_dir, sub), exist_ok=True)
    gts, cams = {}, {}
    for im, pose in enumerate(poses):
        d = np.where(mask[im] > 0, depth[im], F32(tsdf_ref.SEQ_BACKGROUND))
        Image.fromarray(np.clip(np.rint(d / tsdf_ref.SEQ_DEPTH_SCALE), 0, 65535).astype(np.uint16)).save(os.path.join(scene_dir, "depth", f"{im:06d}.png"))
        Image.fromarray(np.rint(np.clip(color[im], 0, 1) * 255.0).astype(np.uint8)).save(os.path.join(scene_dir, "rgb", f"{im:06d}.png"))
        Image.fromarray(np.where(mask[im] > 0, 255, 0).astype(np.uint8)).save(os.path.join(scene_dir, "mask_visib", f"{im:06d}_000000.png"))
        if with_gt is None or im in with_gt:
            gts[str(im)] = [{"cam_R_m2c": pose[:9].tolist(), "cam_t_m2c": pose[9:].tolist(), "obj_id": 1}]
        cams[str(im)] = {"cam_K": tsdf_ref.SEQ_K.reshape(-1).tolist(), "depth_scale": tsdf_ref.SEQ_DEPTH_SCALE}
    for name, obj in (("scene_gt.json", gts), ("scene_camera.json", cams)):
        with open(os.path.join(scene_dir, name), "w") as f:
            json.dump(obj, f)
