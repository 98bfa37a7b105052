"""CPU: the numpy restatement of TSDF fusion and marching tetrahedra (tests/tsdf_ref.py) on an analytic sphere and on the fixtures the
GPU tests compare the kernels on, whose conditions are checked here; the host logic of foundpose_amd/reconstruct.py."""
import numpy as np
import pytest

from foundpose_amd import reconstruct
from tests import tsdf_ref as ref


@pytest.fixture(scope="module")
def sphere():
    vol = ref.sphere_volume()
    counts, keys, pos, col = ref.extract(vol, 2)
    v, c, faces = ref.weld(keys, pos, col)
    return vol, counts, keys, v, faces


def test_sphere_is_a_closed_oriented_surface_within_the_interpolation_bound(sphere):
    vol, counts, keys, v, faces = sphere
    assert len(set(vol["dims"])) == 3 and counts.sum() * 3 == len(keys) and len(faces) > 5000
    topo = ref.topology(faces)
    print(topo)
    assert topo["boundary_edges"] == 0 and topo["nonmanifold_edges"] == 0 and topo["inconsistent"] == 0    # every edge on exactly two triangles
    assert topo["vertices"] - topo["edges"] + topo["faces"] == 2
    vol_mm3 = ref.signed_volume(v, faces)
    assert vol_mm3 > 0 and abs(vol_mm3 / (4.0 / 3.0 * np.pi * 40.0 ** 3) - 1.0) < 0.01
    used = np.unique(faces)
    miss = np.abs(np.linalg.norm(v[used].astype(np.float64), axis=1) - 40.0)
    bound = ref.sphere_bound()
    print("largest distance to the sphere", miss.max(), "bound", bound)
    assert abs(bound - 0.041) < 1e-3 and miss.max() <= bound


def test_case_table_is_complementary_and_complete():
    cases = ref.tet_cases()
    assert [len(cases[m]) for m in range(16)] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    for m in range(1, 15):          # the complement cuts the same edges, wound the other way
        edges = lambda mm: sorted(tuple(sorted(e)) for tri in cases[mm] for e in tri)   # noqa: E731
        assert edges(m) == edges(15 - m)


@pytest.fixture(scope="module")
def fixture():
    return ref.integrate_fixture()


def _run(fx, splits):
    vol = ref.new_volume(fx["origin"], fx["h"], fx["dims"])
    for a, b in splits:
        ref.integrate(vol, fx["depth"][a:b], fx["mask"][a:b], fx["rgb"][a:b], fx["cams"][a:b], fx["poses"][a:b], fx["tau"])
    return vol


def test_integrate_is_the_same_however_the_frames_are_split(fixture):
    one, two = _run(fixture, [(0, 5)]), _run(fixture, [(0, 2), (2, 5)])
    for name in ("sdf_sum", "sdf_cnt", "rgb_sum", "rgb_cnt"):
        assert np.array_equal(one[name], two[name]), name


def test_integrate_fixture_meets_its_conditions(fixture):
    fx = fixture
    vol0 = ref.new_volume(fx["origin"], fx["h"], fx["dims"])
    assert ref.taps_near_a_pixel_border(vol0, fx["cams"], fx["poses"]) == 0          # the seed is chosen so: no tap hangs on a last bit
    per = [_run({**fx, **{k: fx[k][f:f + 1] for k in ("depth", "mask", "rgb", "cams", "poses")}}, [(0, 1)]) for f in range(5)]
    n = int(np.prod(fx["dims"]))
    assert all(0 < int((p["sdf_cnt"] > 0).sum()) < n for p in per)                   # every frame adds to some voxels and skips others
    assert all(int(p["rgb_cnt"].sum()) > 0 for p in per[:3])
    assert (fx["depth"][1] == 0).sum() > 20 and ((fx["mask"][1] > 0) & (fx["depth"][1] == 0)).sum() > 20      # the hole, over the object
    z3 = ref.project(vol0, fx["cams"][3], fx["poses"][3])[0]
    assert (z3 <= 1.0).sum() > 100 and (z3 > 1.0).sum() > 100                        # voxels behind the close camera
    assert ((fx["mask"][2] == 0) & (fx["depth"][2] < 400)).sum() > 50                # the occluder: near, mask 0
    xs = np.nonzero(fx["mask"][4])[1]
    assert len(xs) > 20 and xs.max() == 95                                           # cut by the image border
    full = _run(fx, [(0, 5)])
    assert 0.0 < float(np.mean(full["sdf_sum"] / np.maximum(full["sdf_cnt"], 1) < 0)) < 0.5   # an inside and an outside
    assert int(full["sdf_cnt"].max()) == 5 and np.all(np.abs(full["sdf_sum"]) <= full["sdf_cnt"])


def test_extract_fixture_meets_its_conditions():
    vol = ref.extract_fixture()
    f, live = ref.corner_values(vol, ref.EXTRACT_MIN_COUNT)
    counts, keys, pos, col = ref.extract(vol, ref.EXTRACT_MIN_COUNT)
    inside = f < 0
    mixed = inside.any(0) & ~inside.all(0)
    assert (mixed & ~live).sum() > 10 and (mixed & live).sum() > 100                 # the unseen block lies across the surface
    assert np.all(counts[~live] == 0) and counts.sum() * 3 == len(keys) > 0
    assert ((f == 0.0).any(0) & mixed & live).sum() > 10                             # exact zeros on corners of cut cells
    v, c, faces = ref.weld(keys, pos, col)
    assert len(faces) < counts.sum()                                                 # ... whose zero-length edges give dropped triangles
    topo = ref.topology(faces)
    assert topo["boundary_edges"] > 0 and topo["inconsistent"] == 0                  # the surface leaves the volume
    assert np.any(np.all(col == ref.F32(0.5), axis=1))                               # an edge without colour at either end
    assert len(np.unique(keys)) < len(keys) and keys.min() >= 0 and keys.max() < 7 * int(np.prod(vol["dims"]))


def test_options_and_host_logic(tmp_path):
    o = reconstruct.load_opts({"voxel_mm": 2.5, "bounds": [[0, 0, 0], [10, 20, 30]]})
    assert o.trunc_mm == 10.0 and o.min_count == 2 and o.mask_dir == "mask_visib" and o.keep_largest and o.frame_batch == 32
    assert reconstruct.load_opts().voxel_mm == 2.0 and reconstruct.load_opts({"reconstruct_opts": {"min_count": 3}}).min_count == 3
    (tmp_path / "o.json").write_text('{"trunc_voxels": 3}')
    assert reconstruct.load_opts(str(tmp_path / "o.json")).trunc_mm == 6.0
    for bad in ({"voxel_mm": 0}, {"trunc_voxels": -1}, {"min_count": 0}, {"frame_batch": 0}, {"bounds": [[0, 0, 0], [1, 0, 1]]}, {"voxel": 1}):
        with pytest.raises((ValueError, TypeError)):
            reconstruct.load_opts(bad)
    assert reconstruct.grid_for(np.zeros(3), np.array([10.0, 20.1, 1.0]), 2.5) == ((0.0, 0.0, 0.0), (4, 9, 2))
    assert reconstruct.fits((512, 512, 512)) and not reconstruct.fits((513, 2, 2))
    big = reconstruct.ReconstructOpts(voxel_mm=0.1)
    h = reconstruct.suggest_voxel(np.full(3, -100.0), np.full(3, 100.0), big)
    lo, hi = reconstruct.padded_box(np.full(3, -100.0), np.full(3, 100.0), big.trunc_voxels * h)
    assert reconstruct.fits(reconstruct.grid_for(lo, hi, h)[1]) and 0.4 < h < 0.6
    with pytest.raises(ValueError, match="fits"):
        reconstruct.choose_volume([], big._replace(bounds=((0, 0, 0), (100, 100, 100))))
    # two tetrahedra that share no vertex, the second one open
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]])
    faces = np.concatenate([tet + 4, tet[:3]])
    keep = reconstruct.largest_component(faces, 8)
    assert keep.tolist() == [True] * 4 + [False] * 3
    assert reconstruct.mesh_topology(tet) == {"boundary_edges": 0, "nonmanifold_edges": 0, "watertight": True}
    assert reconstruct.mesh_topology(tet[:3]) == {"boundary_edges": 3, "nonmanifold_edges": 0, "watertight": False}
    assert ref.topology(tet)["boundary_edges"] == 0 and ref.topology(tet[:3])["boundary_edges"] == 3
