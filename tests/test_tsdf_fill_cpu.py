"""CPU: the numpy restatement of volumetric diffusion and of hole filling (tests/tsdf_fill_ref.py): the conditions
the GPU tests' fixtures have to meet, what filling does to the integrate fixture and to a blob seen from above only, and the options."""
import numpy as np
import pytest

from foundpose_amd import reconstruct, synthetic
from tests import render_ref, tsdf_fill_ref as fill, tsdf_ref as ref

DIFFUSE_DIMS = ((37, 29, 23), (70, 9, 1), (3, 3, 3), (40, 7, 5))   # the last: nx % 4 == 0, the kernel's 16-byte path, two workgroups of it
MAX_T = 9


@pytest.mark.parametrize("dims", DIFFUSE_DIMS)
def test_diffusion_fixture_meets_its_conditions(dims):
    val, state = fill.diffuse_fixture(dims)
    nx = dims[0]
    assert np.all(np.isnan(val[:, state == fill.UNKNOWN])) and not np.any(np.isnan(val[:, state != fill.UNKNOWN]))
    assert all(np.any(state == s) for s in (fill.UNKNOWN, fill.FIXED, fill.FREE)) or dims == (3, 3, 3)
    # the UNKNOWN block is open towards x = 0 and towards x = nx - 1: it thaws from both sides, one layer per iteration
    thick = (nx - 1) - nx // 3
    turned, s = [], state
    v = val
    for t in range(1, MAX_T + 1):
        v, s2 = fill.diffuse_once(v, s)
        assert not np.any(np.isnan(v)), t                               # a NaN stored in an UNKNOWN voxel never spreads
        assert np.array_equal(s2 == fill.FIXED, state == fill.FIXED)
        turned.append(int(((s == fill.UNKNOWN) & (s2 == fill.FREE)).sum()))
        s = s2
    print(dims, "block of", thick, "voxels; voxels that turned FREE per iteration", turned, "; UNKNOWN at the end", int((s == fill.UNKNOWN).sum()))
    if thick > 2 * MAX_T:                                               # thicker than 9 voxels from either side
        assert np.any(s == fill.UNKNOWN) and all(n > 0 for n in turned)
    else:                                                               # 3 x 3 x 3 has room for one UNKNOWN layer: it thaws at once
        assert dims == (3, 3, 3) and turned[0] > 0 and not np.any(s == fill.UNKNOWN)
    one = fill.diffuse(val[:1], state, MAX_T)
    assert np.array_equal(one[0][0], v[0]) and np.array_equal(one[1], s)   # one channel is the first of three: n is shared, acc is not


def test_one_iteration_by_hand():
    val = np.array([[[[np.nan, 2.0, -0.0, 4.0, np.nan, np.nan]]]], np.float32)   # 6 x 1 x 1
    state = np.array([[[0, 1, 2, 2, 0, 0]]], np.uint8)
    v, s = fill.diffuse_once(val, state)
    assert s.tolist() == [[[2, 1, 2, 2, 2, 0]]]
    assert v[0, 0, 0].tolist() == [2.0, 2.0, 2.0, 2.0, 4.0, 0.0]        # (2) / 1, fixed, (-0 + 2 + 4) / 3, (4 + -0) / 2, (4) / 1, nothing
    assert np.signbit(v[0, 0, 0, 5]) == False                           # noqa: E712  (+0.0f)
    # the order of the sum shows in the last bit: centre, -x, +x, -y, +y, -z, +z
    val = np.zeros((1, 3, 3, 3), np.float32)
    val[0, 1, 1, 1], val[0, 1, 1, 0], val[0, 1, 1, 2], val[0, 1, 0, 1], val[0, 1, 2, 1], val[0, 0, 1, 1], val[0, 2, 1, 1] = 1.0, 2.0 ** -24, 2.0 ** -24, -1.0, 3.0, 2.0 ** -24, 2.0 ** -24
    v, _ = fill.diffuse_once(val, np.full((3, 3, 3), 2, np.uint8))
    f = np.float32
    want = ((((((f(0) + f(1)) + f(2.0 ** -24)) + f(2.0 ** -24)) + f(-1)) + f(3)) + f(2.0 ** -24)) + f(2.0 ** -24)
    # 1 + 2^-24 is a tie and rounds to 1, twice; 3 + 2^-24 rounds to 3, twice: the ordered fp32 sum is 3, the exact one 3 + 2^-22 (an fp32 number)
    assert want == f(3) and v[0, 1, 1, 1] == f(3) / f(7) and float(val.astype(np.float64).sum()) == 3.0 + 2.0 ** -22


@pytest.fixture(scope="module")
def fused_fixture():
    fx = ref.integrate_fixture()
    vol = ref.new_volume(fx["origin"], fx["h"], fx["dims"])
    ref.integrate(vol, fx["depth"], fx["mask"], fx["rgb"], fx["cams"], fx["poses"], fx["tau"])
    return vol


def _by_hand(vol, min_count, T, plane):
    """clipped_voxels and snapped_voxels counted voxel by voxel, from the rules and not from fill_volume's arrays."""
    nx, ny, nz = vol["dims"]
    cnt, s = vol["sdf_cnt"], vol["sdf_sum"]
    g = np.empty((nz, ny, nx), np.float32)
    fixed = np.zeros((nz, ny, nx), bool)
    clipped = 0
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                c = int(cnt[k, j, i])
                val = np.float32(np.float64(s[k, j, i]) / np.float64(c)) if c > 0 else np.float32(-1.0)
                fx = c >= min_count
                if plane is not None and not fx:
                    X = [np.float64(o) + (np.float64(q) + 0.5) * np.float64(vol["voxel_mm"]) for o, q in zip(vol["origin"], (i, j, k))]
                    if ((plane[0] * X[0] + plane[1] * X[1]) + plane[2] * X[2]) + plane[3] > 0:
                        val, fx = np.float32(1.0), True
                if i in (0, nx - 1) or j in (0, ny - 1) or k in (0, nz - 1):
                    clipped += int(c >= min_count and val < 0)
                    val, fx = np.float32(1.0), True
                g[k, j, i], fixed[k, j, i] = val, fx
    gT = fill.diffuse(g[None], np.where(fixed, 1, 2).astype(np.uint8), T)[0][0]
    snapped = sum(1 for x, fx in zip(gT.reshape(-1), fixed.reshape(-1)) if not fx and abs(float(x)) < 2.0 ** -10)
    return clipped, snapped


@pytest.mark.parametrize("plane", (None, (0.0, 0.3, -1.0, -14.0)))
def test_fill_closes_the_integrate_fixture(fused_fixture, plane):
    vol = fused_fixture
    cnt = vol["sdf_cnt"]
    assert np.any(cnt == 0) and np.any(cnt == 1) and np.any(cnt >= 2)
    _, _, _, _, open_topo = fill.mesh_of(vol, 2)
    out, st = fill.fill_volume(vol, 2, 4, 64, plane)
    v, c, faces, keys, topo = fill.mesh_of(out, 1)
    print("plane", plane, "stats", st, "before", open_topo, "after", topo, "volume", ref.signed_volume(v, faces))
    assert open_topo["boundary_edges"] > 0
    assert topo["boundary_edges"] == 0 and topo["nonmanifold_edges"] == 0 and topo["inconsistent"] == 0 and ref.signed_volume(v, faces) > 0
    clipped, snapped = _by_hand(vol, 2, 4, plane)
    assert (st["clipped_voxels"], st["snapped_voxels"]) == (clipped, snapped)
    assert st["filled_voxels"] > 0 and (st["plane_voxels"] > 0) == (plane is not None) and 0 < st["last_change"] < 1
    # observed voxels off the outer layer keep their bits, so the edges between two of them keep their vertices
    keep = (cnt >= 2) & ~fill.outer_layer(cnt.shape)
    assert np.array_equal(out["sdf_sum"][keep], vol["sdf_sum"][keep]) and np.array_equal(out["sdf_cnt"][keep], cnt[keep])
    assert np.all(out["sdf_cnt"][~keep] == 1) and np.all(out["sdf_sum"][fill.outer_layer(cnt.shape)] == 1)
    had = vol["rgb_cnt"] > 0
    assert np.array_equal(out["rgb_sum"][:, had], vol["rgb_sum"][:, had]) and np.array_equal(out["rgb_cnt"][had], vol["rgb_cnt"][had])


def test_an_object_that_leaves_the_bounds_gets_flat_caps():
    vol = ref.sphere_volume(dims=(21, 46, 30), h=2.0, r=40.0)            # every voxel observed; the sphere sticks out through four faces
    nx, ny, nz = vol["dims"]
    f = vol["sdf_sum"] / np.float32(2)
    by_hand = sum(1 for k in range(nz) for j in range(ny) for i in range(nx)
                  if (i in (0, nx - 1) or j in (0, ny - 1) or k in (0, nz - 1)) and f[k, j, i] < 0)
    _, _, _, _, open_topo = fill.mesh_of(vol, 2)
    out, st = fill.fill_volume(vol, 2, 4, 0, None)
    v, _, faces, _, topo = fill.mesh_of(out, 1)
    print("clipped", st["clipped_voxels"], "boundary edges before", open_topo["boundary_edges"], "after", topo)
    assert st["clipped_voxels"] == by_hand > 100 and st["filled_voxels"] == 0 and st["snapped_voxels"] == 0 and st["last_change"] == 0.0
    assert open_topo["boundary_edges"] > 0 and topo["boundary_edges"] == 0 and topo["nonmanifold_edges"] == 0 and topo["inconsistent"] == 0
    assert ref.signed_volume(v, faces) > 0
    lo = np.array(vol["origin"]) + 0.5 * vol["voxel_mm"]
    hi = np.array(vol["origin"]) + (np.array(vol["dims"]) - 0.5) * vol["voxel_mm"]
    used = v[np.unique(faces)]
    assert np.all(used > lo) and np.all(used < hi)                       # no surface leaves the volume


def test_zero_iterations_and_a_fill_of_nothing(fused_fixture):
    out, st = fill.fill_volume(fused_fixture, 2, 0, 0, None)
    assert st["last_change"] == 0.0 and st["snapped_voxels"] == _by_hand(fused_fixture, 2, 0, None)[1] and np.array_equal(out["rgb_cnt"], fused_fixture["rgb_cnt"])
    _, _, _, _, topo = fill.mesh_of(out, 1)
    assert topo["boundary_edges"] == 0 and topo["nonmanifold_edges"] == 0


@pytest.fixture(scope="module")
def blob():
    """The six fibonacci_eyes() views with z > 0 of make_blob_mesh(24, 24, radius=40), fused by the restatement at h = 2.5, tau = 10 in
    the blob's vertex bounds padded by padded_box."""
    mesh = synthetic.make_blob_mesh(24, 24, radius=40)
    cam = np.array([ref.SEQ_K[0, 0], ref.SEQ_K[1, 1], ref.SEQ_K[0, 2], ref.SEQ_K[1, 2]])
    poses = [p for p, e in zip(ref.sequence_poses(), ref.fibonacci_eyes()) if e[2] > 0]
    assert len(poses) == 6
    depth, mask, rgb = [], [], []
    for R, t in poses:
        r = render_ref.render(mesh, ref.render_cam(cam, R, t), ref.SEQ_W, ref.SEQ_H)
        depth.append(np.where(r["mask"] > 0, r["depth"], np.float32(ref.SEQ_BACKGROUND)).astype(np.float32))
        mask.append(r["mask"].astype(np.uint8)), rgb.append(r["color"].astype(np.uint8))
    v = mesh.vertices.astype(np.float64)
    lo, hi = reconstruct.padded_box(v.min(0), v.max(0), 10.0)
    origin, dims = reconstruct.grid_for(lo, hi, 2.5)
    vol = ref.new_volume(origin, 2.5, dims)
    ref.integrate(vol, np.stack(depth), np.stack(mask), np.stack(rgb), np.tile(cam, (6, 1)), np.stack([np.concatenate([R.reshape(-1), t]) for R, t in poses]), 10.0)
    return mesh, vol


def test_the_blob_seen_from_above_is_closed_at_the_right_volume(blob):
    mesh, vol = blob
    assert vol["dims"] == (66, 55, 47)
    v0 = ref.signed_volume(mesh.vertices, mesh.faces)
    ov, _, of, _, open_topo = fill.mesh_of(vol, 2)
    assert open_topo["boundary_edges"] > 500 and ref.signed_volume(ov, of) < 0.7 * v0    # open, and a third of the volume is missing
    z_min = float(mesh.vertices[:, 2].min())
    for plane in (None, (0.0, 0.0, -1.0, z_min)):
        out, st = fill.fill_volume(vol, 2, 4, 64, plane)
        v, c, faces, _, topo = fill.mesh_of(out, 1)
        vol_mm3 = ref.signed_volume(v, faces)
        print("plane", plane, st, topo, "signed volume", vol_mm3, "of", v0, f"({100 * (vol_mm3 / v0 - 1):+.2f} %)")
        assert topo["boundary_edges"] == 0 and topo["nonmanifold_edges"] == 0 and topo["inconsistent"] == 0
        assert st["uncoloured_voxels"] == 0 and not np.any(np.all(c[np.unique(faces)] == np.float32(0.5), axis=1))
        assert (st["plane_voxels"] > 0) == (plane is not None)
        assert abs(vol_mm3 / v0 - 1) <= 0.04
    # without colour propagation the invented surface is grey in places: 64 iterations are what removes it
    _, st0 = fill.fill_volume(vol, 2, 4, 0, None)
    assert st0["uncoloured_voxels"] > 0


def test_options_and_refusals():
    o = reconstruct.load_opts(None)
    assert (o.fill, o.fill_smooth_iters, o.fill_color_iters, o.fill_plane) == ("none", 4, 64, None)
    o = reconstruct.load_opts({"fill": "carve", "fill_smooth_iters": 0, "fill_color_iters": 4096, "fill_plane": [0, 0, -1, 12.5]})
    assert o.fill == "carve" and o.fill_plane == (0, 0, -1, 12.5) and o.fill_smooth_iters == 0
    for bad in ({"fill": "poisson"}, {"fill": None}, {"fill_smooth_iters": -1}, {"fill_smooth_iters": 4097}, {"fill_smooth_iters": 1.5},
                {"fill_smooth_iters": True}, {"fill_color_iters": -1}, {"fill_color_iters": 4097}, {"fill_color_iters": "4"},
                {"fill_plane": [0, 0, 0, 1]}, {"fill_plane": [0, 0, 1]}, {"fill_plane": [0, 0, 1, float("nan")]}, {"fill_plane": [0, float("inf"), 1, 0]},
                {"fill_plane": "z"}, {"fill_plane": [0, 0, True, 1]}):
        with pytest.raises(ValueError):
            reconstruct.load_opts(bad)
    small = ref.new_volume((0, 0, 0), 1.0, (2, 5, 5))
    with pytest.raises(AssertionError):
        fill.fill_volume(small, 1)
