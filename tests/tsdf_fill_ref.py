"""numpy restatement of fp_tsdf_diffuse and of reconstruct.fill_volume (TEST HELPER; include/foundpose_amd.h, csrc/tsdf_fill.hip,
DESIGN.md section 34), written from the contract: fp32 rounding exactly where the contract rounds -- every addition of the accumulator,
the one division -- and selection, never multiplication by a mask, wherever an UNKNOWN voxel's value is passed over."""

import numpy as np

from tests import tsdf_ref

F32 = np.float32
UNKNOWN, FIXED, FREE = 0, 1, 2
ORDER = ((0, 0, 0), (0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0))   # (dz, dy, dx): centre, -x, +x, -y, +y, -z, +z
SNAP = F32(2.0 ** -10)


def diffuse_once(val, state):
    C, nz, ny, nx = val.shape
    known = np.zeros((nz + 2, ny + 2, nx + 2), bool)                          # the border: outside the volume, takes no part
    known[1:-1, 1:-1, 1:-1] = state != UNKNOWN
    pad = np.zeros((C, nz + 2, ny + 2, nx + 2), F32)
    pad[:, 1:-1, 1:-1, 1:-1] = val
    n = np.zeros((nz, ny, nx), np.int32)
    acc = np.zeros((C, nz, ny, nx), F32)                                      # +0.0f
    with np.errstate(all="ignore"):
        for dz, dy, dx in ORDER:
            sl = (slice(1 + dz, nz + 1 + dz), slice(1 + dy, ny + 1 + dy), slice(1 + dx, nx + 1 + dx))
            k = known[sl]
            n += k
            acc = np.where(k[None], (acc + pad[(slice(None),) + sl]).astype(F32), acc)
        mean = (acc / n.astype(F32)[None]).astype(F32)
    fixed = state == FIXED
    out = np.where(fixed[None], val, np.where((n > 0)[None], mean, F32(0.0))).astype(F32)
    return out, np.where(fixed, FIXED, np.where(n > 0, FREE, UNKNOWN)).astype(np.uint8)


def diffuse(val, state, iters):
    """val fp32 [C, nz, ny, nx], state uint8 [nz, ny, nx] -> (val', state') after `iters` Jacobi iterations."""
    val, state = np.array(val, F32), np.array(state, np.uint8)
    for _ in range(int(iters)):
        val, state = diffuse_once(val, state)
    return val, state


def diffuse_fixture(dims, seed=0):
    """Random states and values on dims = (nx, ny, nz): FIXED and FREE voxels scattered, and one UNKNOWN block across the whole of y and
    z that covers the upper two thirds of x, all but the last voxel (thicker than 9 voxels wherever nx >= 16; on 3 x 3 x 3 it is
    x = 1 alone), with NaN stored in every UNKNOWN voxel and further single UNKNOWN voxels scattered through the rest.
    -> val fp32 [3, nz, ny, nx], state uint8 [nz, ny, nx]; the one-channel case takes val[:1]."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    state = rng.choice(np.array([UNKNOWN, FIXED, FREE], np.uint8), size=(nz, ny, nx), p=(0.2, 0.4, 0.4))
    state[:, :, nx // 3:nx - 1] = UNKNOWN
    val = rng.uniform(-1.0, 1.0, size=(3, nz, ny, nx)).astype(F32)
    val[:, state == UNKNOWN] = np.nan
    return val, state


def outer_layer(shape):
    out = np.zeros(shape, bool)
    out[[0, -1]] = out[:, [0, -1]] = out[:, :, [0, -1]] = True
    return out


def crossing_ends(inside):
    """bool [nz, ny, nx]: the voxels at either end of an edge of the tetrahedral split (tsdf_ref.DIRECTIONS) whose ends differ in
    `inside`: the voxels a surface vertex takes its colour from."""
    nz, ny, nx = inside.shape
    near = np.zeros(inside.shape, bool)
    for dx, dy, dz in tsdf_ref.DIRECTIONS:
        lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        hi = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        cross = inside[lo] != inside[hi]
        near[lo] |= cross
        near[hi] |= cross
    return near


def fill_volume(vol, min_count, smooth_iters=4, color_iters=64, plane=None):
    """The restatement of reconstruct.fill_volume on a tsdf_ref volume -> (volume', stats without "seconds")."""
    (ox, oy, oz), h, (nx, ny, nz) = vol["origin"], vol["voxel_mm"], vol["dims"]
    assert min(nx, ny, nz) >= 3
    cnt = vol["sdf_cnt"]
    with np.errstate(all="ignore"):
        f = (vol["sdf_sum"].astype(np.float64) / cnt.astype(np.float64)).astype(F32)
    seen = cnt > 0
    src = cnt >= min_count
    g = np.where(seen, f, F32(-1.0)).astype(F32)
    fixed = src.copy()
    plane_voxels = 0
    if plane is not None:
        a, b, c, d = (np.float64(v) for v in plane)
        X = tsdf_ref.centres(ox, nx, h)[None, None, :]
        Y = tsdf_ref.centres(oy, ny, h)[None, :, None]
        Z = tsdf_ref.centres(oz, nz, h)[:, None, None]
        empty = ~src & ((((a * X + b * Y) + c * Z) + d) > 0)
        g[empty] = F32(1.0)
        fixed |= empty
        plane_voxels = int(empty.sum())
    outer = outer_layer(g.shape)
    clipped = int((outer & src & (f < 0)).sum())
    g[outer] = F32(1.0)
    fixed |= outer
    state = np.where(fixed, FIXED, FREE).astype(np.uint8)
    before = diffuse(g[None], state, max(smooth_iters - 1, 0))[0][0] if smooth_iters > 0 else g
    g = diffuse(before[None], state, 1)[0][0] if smooth_iters > 0 else g
    free = ~fixed
    last_change = float(np.abs(g - before)[free].max()) if smooth_iters > 0 and free.any() else 0.0
    snap = free & (np.abs(g) < SNAP)
    g = np.where(snap, SNAP, g).astype(F32)
    keep = src & ~outer
    out = dict(vol)
    out["sdf_sum"] = np.where(keep, vol["sdf_sum"], g).astype(F32)
    out["sdf_cnt"] = np.where(keep, cnt, 1).astype(np.int32)
    # colour
    has = vol["rgb_cnt"] > 0
    with np.errstate(all="ignore"):
        m = (vol["rgb_sum"] / vol["rgb_cnt"].astype(F32)[None]).astype(F32)
    m = np.where(has[None], m, F32(0.0)).astype(F32)
    m, cstate = diffuse(m, np.where(has, FIXED, UNKNOWN).astype(np.uint8), color_iters)
    got = cstate == FREE
    out["rgb_sum"] = np.where(got[None], m, vol["rgb_sum"]).astype(F32)
    out["rgb_cnt"] = np.where(got, 1, vol["rgb_cnt"]).astype(np.int32)
    inside = np.where(keep, f, g) < 0
    stats = {"filled_voxels": int((~src & inside).sum()), "plane_voxels": plane_voxels, "clipped_voxels": clipped,
             "snapped_voxels": int(snap.sum()), "uncoloured_voxels": int((crossing_ends(inside) & (out["rgb_cnt"] == 0)).sum()),
             "smooth_iters": int(smooth_iters), "color_iters": int(color_iters), "last_change": last_change}
    return out, stats


def mesh_of(vol, min_count):
    """extract + weld -> (vertices, colours, faces, keys of the vertices, topology)."""
    _, keys, pos, col = tsdf_ref.extract(vol, min_count)
    v, c, faces = tsdf_ref.weld(keys, pos, col)
    return v, c, faces, np.unique(keys), tsdf_ref.topology(faces)
