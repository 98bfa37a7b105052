"""CPU: gen_templates' views and cameras against the reference (tests/golden/template_views.npz), the PLY loader, the
rasterizer contract's numpy restatement on analytic cases (tests/render_ref.py) and the metadata gen_repre reads."""
import json
import os

import numpy as np
import pytest

from foundpose_amd import crop_util, gen_repre, gen_templates
from foundpose_amd.crop_util import PinholePlaneCameraModel
from foundpose_amd.renderer import FALLBACK_COLOR, Mesh, camera_params, load_ply, save_ply, vertex_normals

from . import render_ref


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "template_views.npz"))


@pytest.mark.parametrize("n,r,s", [(57, 14, 1), (9, 3, 1), (9, 3, 3)])
def test_views_match_reference(gold, n, r, s):
    opts = gen_templates.GenTemplatesOpts(version="v1", object_dataset="lmo", min_num_viewpoints=n, num_inplane_rotations=r, num_viewspheres=s)
    views = gen_templates.template_views(opts, tuple(gold["depth_range"]))
    R, t = gold[f"views_{n}_{r}_{s}_R"], gold[f"views_{n}_{r}_{s}_t"]
    assert len(views) == len(R) == n * r * s + (1 - n % 2) * r * s and ((n, r, s) != (57, 14, 1) or len(views) == 798)
    np.testing.assert_allclose(np.array([v["R"] for v in views]), R, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.array([v["t"] for v in views]), t, rtol=0, atol=1e-12 * 1500)


def test_images_per_view_repeats_views(gold):
    opts = gen_templates.GenTemplatesOpts(version="v1", object_dataset="lmo", min_num_viewpoints=9, num_inplane_rotations=3, images_per_view=2)
    views = gen_templates.template_views(opts, tuple(gold["depth_range"]))
    assert len(views) == 54 and np.array_equal(views[0]["R"], views[1]["R"]) and not np.array_equal(views[1]["R"], views[2]["R"])


@pytest.mark.parametrize("name", ["landscape", "portrait"])
def test_base_cameras_match_reference(gold, name):
    opts = gen_templates.GenTemplatesOpts(version="v1", object_dataset="lmo")
    cam, rc = gen_templates.base_cameras(gold[f"cam_{name}_K"], tuple(int(x) for x in gold[f"cam_{name}_size"]), opts)
    assert cam.width == cam.height and rc.width == rc.height == 4 * cam.width
    got = np.array([cam.width, *cam.f, *cam.c, rc.width, *rc.f, *rc.c], np.float64)
    assert np.array_equal(got, gold[f"cam_{name}"])
    if name == "landscape":
        assert cam.width == 630


def test_template_cameras_match_reference(gold):
    opts = gen_templates.GenTemplatesOpts(version="v1", object_dataset="lmo")
    K = gold["cam_landscape_K"]
    _, rc = gen_templates.base_cameras(K, (640, 480), opts)
    render = PinholePlaneCameraModel(rc.width, rc.height, rc.f, rc.c, gold["tcam_render_T"])
    for i in range(4):
        crop = gen_templates.crop_camera(gold[f"tcam_{i}_box"].tolist(), render, opts)
        # the focal length steps are float32 under the reference's pinned numpy 1.26 (crop_util); the fixture was taken under
        # numpy 2, where NEP 50 runs them in float64 -> equal to float32 precision (as tests/test_crop_cpu.py)
        np.testing.assert_allclose(np.array(crop.f, np.float64), gold[f"tcam_{i}_crop"][:2], rtol=3e-7)
        assert np.array_equal(np.array(crop.c, np.float64), gold[f"tcam_{i}_crop"][2:]) and (crop.width, crop.height) == (1680, 1680)
        np.testing.assert_allclose(crop.T_world_from_eye, gold[f"tcam_{i}_crop_T"], rtol=0, atol=1e-12)
        # step 6 on the reference's crop camera: exact
        ref_crop = PinholePlaneCameraModel(crop.width, crop.height, tuple(gold[f"tcam_{i}_crop"][:2]), tuple(gold[f"tcam_{i}_crop"][2:]),
                                           gold[f"tcam_{i}_crop_T"])
        tc = gen_templates.template_camera(ref_crop, opts)
        assert np.array_equal(np.array([tc.width, tc.height, *tc.f, *tc.c], np.float64), gold[f"tcam_{i}"])


def test_fit_check(gold):
    for box, rejected in zip(gold["fit_boxes"], gold["fit_rejected"]):
        if rejected:
            with pytest.raises(ValueError, match="does not fit the viewport"):
                gen_templates.check_fits(box.tolist(), 2520, 2520)
        else:
            gen_templates.check_fits(box.tolist(), 2520, 2520)


def test_unsupported_options_are_refused():
    opts = gen_templates.GenTemplatesOpts(version="v1", object_dataset="lmo", crop=False)
    with pytest.raises(NotImplementedError, match="trans_c2w"):
        gen_templates.render_templates(None, 1, [], None, opts)
    o = gen_templates.load_opts({"gen_templates_opts": {"version": "v1", "object_dataset": "lmo", "crop_size": [420, 420],
                                                        "light_type": "multi_directional", "texture_size": [1024, 1024]}})
    assert o.crop_size == (420, 420) and o.ssaa_factor == 4.0 and o.max_num_triangles == 20000


# ---------------------------------------------------------------- PLY
def _quad_mesh():
    v = np.array([[0, 0, 0], [10, 0, 0], [10, 10, 0], [0, 10, 0], [5, 5, 3]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4]], np.int32)
    c = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30], [1, 2, 3]], np.float32) / np.float32(255)
    return Mesh(v, f, c, vertex_normals(v, f))


@pytest.mark.parametrize("binary", [True, False])
def test_ply_round_trip(tmp_path, binary):
    m = _quad_mesh()
    p = str(tmp_path / "m.ply")
    save_ply(p, m, binary=binary)
    got = load_ply(p)
    assert np.array_equal(got.vertices, m.vertices) and np.array_equal(got.faces, m.faces)
    assert np.array_equal(got.colors, m.colors) and np.array_equal(got.normals, m.normals)


def test_ply_quads_fanned_colourless_and_double(tmp_path):
    p = str(tmp_path / "q.ply")
    with open(p, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 5\nproperty double x\nproperty double y\nproperty double z\n"
                "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
                "0 0 0\n1 0 0\n1 1 0\n0 1 0\n-1 0.5 0\n5 0 1 2 3 4\n")
    m = load_ply(p)
    assert m.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4]]
    assert np.array_equal(m.colors, np.tile(np.array(FALLBACK_COLOR, np.float32) / np.float32(255), (5, 1)))
    np.testing.assert_allclose(m.normals, np.tile([0, 0, 1], (5, 1)), atol=1e-7)


def test_textured_ply_raises(tmp_path):
    for head in ("comment TextureFile obj.png\n", ""):
        p = str(tmp_path / "t.ply")
        with open(p, "w") as f:
            f.write("ply\nformat ascii 1.0\n" + head + "element vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                    + ("property float texture_u\nproperty float texture_v\n" if not head else "")
                    + "element face 1\nproperty list uchar int vertex_indices\nend_header\n"
                    + ("0 0 0 0 0\n1 0 0 1 0\n0 1 0 0 1\n" if not head else "0 0 0\n1 0 0\n0 1 0\n") + "3 0 1 2\n")
        with pytest.raises(NotImplementedError):
            load_ply(p)


# ---------------------------------------------------------------- rasterizer contract (numpy restatement)
def _cam(W, H, f, c, T=None):
    return camera_params([PinholePlaneCameraModel(W, H, f, c, T)])[0]


def test_fronto_parallel_quad_depth_is_exact():
    v = np.array([[-40, -30, 500], [40, -30, 500], [40, 30, 500], [-40, 30, 500]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    depth, tri, _ = render_ref.rasterize(v, f, _cam(64, 48, (200.0, 200.0), (31.7, 23.2)), 64, 48)
    assert (tri >= 0).sum() == 32 * 24 and np.all(depth[tri >= 0] == np.float32(500.0))


def test_shared_diagonal_covers_each_pixel_once():
    rng = np.random.default_rng(0)
    for _ in range(20):
        a = np.sort(rng.uniform(0, 2 * np.pi, 4))                     # a convex quad: four points of an ellipse in angle order
        q = np.stack([55 * np.cos(a) + rng.uniform(-3, 3), 45 * np.sin(a) + rng.uniform(-3, 3), np.full(4, 400.0)], 1).astype(np.float32)
        cam = _cam(48, 40, (150.0, 150.0), (24.0, 20.0))
        n0 = (render_ref.rasterize(q, np.array([[0, 1, 2]], np.int32), cam, 48, 40)[1] >= 0).astype(int)
        n1 = (render_ref.rasterize(q, np.array([[0, 2, 3]], np.int32), cam, 48, 40)[1] >= 0).astype(int)
        both = render_ref.rasterize(q, np.array([[0, 1, 2], [0, 2, 3]], np.int32), cam, 48, 40)[1] >= 0
        assert (n0 + n1).max() <= 1 and np.array_equal((n0 + n1) > 0, both)


def test_pixel_centre_vertices_follow_top_left_rule():
    # a right triangle with its vertices on the pixel centres (2,2), (6,2), (2,6): the top edge (y = 2) and the left
    # edge (x = 2) are inside, the hypotenuse is not
    f, z, cx, cy = 100.0, 500.0, 8.0, 8.0
    px = lambda x, y: [(x + 0.5 - cx) * z / f, (y + 0.5 - cy) * z / f, z]   # noqa: E731
    v = np.array([px(2, 2), px(6, 2), px(2, 6)], np.float32)
    _, tri, _ = render_ref.rasterize(v, np.array([[0, 1, 2]], np.int32), _cam(16, 16, (f, f), (cx, cy)), 16, 16)
    cov = {(int(x), int(y)) for y, x in zip(*np.nonzero(tri >= 0))}
    expect = {(x, y) for y in range(2, 7) for x in range(2, 7) if (x - 2) + (y - 2) < 4}
    assert cov == expect
    _, tri2, _ = render_ref.rasterize(v, np.array([[0, 2, 1]], np.int32), _cam(16, 16, (f, f), (cx, cy)), 16, 16)   # winding does not matter
    assert np.array_equal(tri >= 0, tri2 >= 0)


def test_marker_lands_at_projection():
    """A small triangle at +X of the model lands at u = fx X / Z + cx, to the right of the principal point (OpenCV, not GL)."""
    X, Y, Z = 60.0, -25.0, 600.0
    v = np.array([[X - 2, Y - 2, Z], [X + 2, Y - 2, Z], [X, Y + 2, Z]], np.float32)
    fx, fy, cx, cy = 300.0, 310.0, 40.0, 30.0
    _, tri, _ = render_ref.rasterize(v, np.array([[0, 1, 2]], np.int32), _cam(80, 60, (fx, fy), (cx, cy)), 80, 60)
    ys, xs = np.nonzero(tri >= 0)
    assert len(xs) > 0 and abs(xs.mean() + 0.5 - (fx * X / Z + cx)) < 1.0 and abs(ys.mean() + 0.5 - (fy * Y / Z + cy)) < 1.5
    # the same marker seen by a camera placed by gen_templates' view convention (T_world_from_eye = inverse of the view)
    view = {"R": np.eye(3), "t": np.zeros((3, 1))}
    cam = gen_templates.view_camera(PinholePlaneCameraModel(80, 60, (fx, fy), (cx, cy)), view)
    _, tri2, _ = render_ref.rasterize(v, np.array([[0, 1, 2]], np.int32), camera_params([cam])[0], 80, 60)
    assert np.array_equal(tri, tri2)


def test_near_plane_raises():
    v = np.array([[0, 0, 90], [1, 0, 500], [0, 1, 500]], np.float32)
    with pytest.raises(ValueError):
        render_ref.rasterize(v, np.array([[0, 1, 2]], np.int32), _cam(8, 8, (10.0, 10.0), (4.0, 4.0)), 8, 8)


def test_metadata_is_read_back_by_gen_repre(tmp_path):
    cam = PinholePlaneCameraModel(224, 224, (np.float32(511.25), np.float32(511.25)), (np.float32(111.5), np.float32(111.5)),
                                  gen_templates.view_camera(PinholePlaneCameraModel(8, 8, (1.0, 1.0), (0.0, 0.0)),
                                                            gen_templates.sample_views(9, 600.0)[2]).T_world_from_eye)
    meta = [{"dataset": "lmo", "lid": 3, "template_id": 0, "pose": {"R": np.eye(3).tolist(), "t": np.zeros((3, 1)).tolist()},
             "boxes_amodal": [[1.0, 2.0, 200.0, 210.0]], "visibilities": [1.0], "cameras": gen_templates.camera_to_json(cam),
             "rgb_image_path": "a.png", "depth_map_path": "b.png", "binary_mask_path": "c.png"}]
    d = tmp_path / "templates" / "v1" / "lmo" / "3"
    d.mkdir(parents=True)
    (d / "metadata.json").write_text(json.dumps(meta))
    opts = gen_repre.GenRepreOpts(version="v1", templates_version="v1", object_dataset="lmo")
    back = gen_repre.load_template_metadata(str(tmp_path), opts, 3)
    c = back[0]["cameras"]
    got = crop_util.PinholePlaneCameraModel(c["ImageSizeX"], c["ImageSizeY"], (c["fx"], c["fy"]), (c["cx"], c["cy"]), np.array(c["T_WorldFromCamera"]))
    assert (got.width, got.height, got.f, got.c) == (224, 224, (511.25, 511.25), (111.5, 111.5))
    assert np.array_equal(got.T_world_from_eye, cam.T_world_from_eye)
    np.testing.assert_allclose(np.array(c["ModelViewMatrix"]) @ cam.T_world_from_eye, np.eye(4), atol=1e-12)


# ---------------------------------------------------------------- restatement self-checks: a watertight random sheet
SHEET_W, SHEET_H, SHEET_F, SHEET_C = 200, 150, 600.0, (100.3, 74.8)
SHEET_PLANES = {"fronto": (500.0, 0.0, 0.0), "tilted": (500.0, 0.5, 0.25)}


@pytest.mark.parametrize("kind", ["fronto", "tilted"])
def test_random_sheet_is_covered_exactly_once(kind):
    """A random triangulation of a rectangle spanning 7 x 5 tiles: by render_ref's edge functions (before any z-test) every
    pixel centre strictly inside the snapped outline is covered by exactly one face, none outside is covered, and one on
    the outline at most once."""
    plane = SHEET_PLANES[kind]
    v, f, ring = render_ref.random_sheet(12, 9, (-60.0, 60.0), (-45.0, 45.0), plane, seed=11)
    cam = _cam(SHEET_W, SHEET_H, (SHEET_F, SHEET_F), SHEET_C)
    count = render_ref.face_coverage(v, f, cam, SHEET_W, SHEET_H)
    X, Y, _, _ = render_ref.transform(v, np.zeros_like(v), cam)
    py, px = np.mgrid[0:SHEET_H, 0:SHEET_W]
    side = render_ref.inside_polygon(px.astype(np.int64) * 256 + 128, py.astype(np.int64) * 256 + 128, X[ring], Y[ring])
    assert (side == 1).sum() > 15000 and (side == -1).sum() > 5000
    assert np.all(count[side == 1] == 1) and np.all(count[side == -1] == 0) and count.max() == 1
    depth, tri, _ = render_ref.rasterize(v, f, cam, SHEET_W, SHEET_H)
    assert np.array_equal(tri >= 0, count == 1)


@pytest.mark.parametrize("kind", ["fronto", "tilted"])
def test_random_sheet_depth_is_the_plane(kind):
    """render_ref's depth against the exact fp64 ray-plane intersection.  Snapping moves each vertex by at most 1/512 px
    per axis while keeping its 1/z; 1/z is affine in the window, so at a covered pixel the interpolated 1/z is the true
    plane's at a point at most 1/512 px away per axis: |d(1/z)| <= (|d(1/z)/du| + |d(1/z)/dv|) / 512.  The fp32 vertex
    positions and the fp32 result add a few fp32 ulps."""
    p0, p1, p2 = SHEET_PLANES[kind]
    v, f, _ = render_ref.random_sheet(12, 9, (-60.0, 60.0), (-45.0, 45.0), (p0, p1, p2), seed=11)
    cam = _cam(SHEET_W, SHEET_H, (SHEET_F, SHEET_F), SHEET_C)
    depth, tri, _ = render_ref.rasterize(v, f, cam, SHEET_W, SHEET_H)
    ys, xs = np.nonzero(tri >= 0)
    rx, ry = (xs + 0.5 - SHEET_C[0]) / SHEET_F, (ys + 0.5 - SHEET_C[1]) / SHEET_F
    z_true = p0 / (1.0 - p1 * rx - p2 * ry)            # z = p0 + p1 x + p2 y with (x, y) = z (rx, ry)
    a, b = p1 / (SHEET_F * p0), p2 / (SHEET_F * p0)    # the gradient of 1/z = (1 - p1 rx - p2 ry) / p0 per pixel
    bound = z_true ** 2 * (abs(a) + abs(b)) / 512.0 * 1.001 + 4 * np.spacing(np.float32(z_true)).astype(np.float64)
    err = np.abs(depth[ys, xs].astype(np.float64) - z_true)
    assert np.all(err <= bound), (err.max(), bound.min())
    if kind == "fronto":
        assert np.all(depth[ys, xs] == np.float32(p0))
    else:
        assert err.max() > 1e-4   # the snap is visible: the bound is not vacuous


def test_tile_counts_restate_the_binning():
    """render_ref.tile_counts (vectorised) against a per-face loop over the boxes rasterize() uses, including faces that are
    off-screen, zero-area, or end exactly on a tile border."""
    from foundpose_amd import synthetic
    m = synthetic.make_blob_mesh(20, 24, radius=60.0, seed=5)
    v = np.concatenate([m.vertices, np.array([[31.5, 5.5, 512], [32.5, 40.5, 512], [-500, 3, 512], [90, 3, 512]], np.float32)])
    n = len(m.vertices)
    faces = np.concatenate([m.faces, np.array([[n, n + 1, n + 3], [n, n, n + 1], [n + 2, n + 2, n + 2], [n + 2, n + 3, n]], np.int32)])
    W, H = 100, 70
    blob_cam = _cam(W, H, (150.0, 150.0), (47.3, 33.1), np.array([[1, 0, 0, 5], [0, 1, 0, -3], [0, 0, 1, -380.0], [0, 0, 0, 1]]))
    # the blob seen from 380 mm, then the screen-space faces alone (f = 512 at z = 512: world x, y are pixels)
    for v, faces, cam in ((v, faces, blob_cam), (v[n:], faces[len(m.faces):] - n, _cam(W, H, (512.0, 512.0), (0.0, 0.0)))):
        X, Y, z, _ = render_ref.transform(v, np.zeros_like(v), cam)
        want = np.zeros((3, 4), np.int64)
        for face in faces:
            r = render_ref._setup(X, Y, z, face)
            if r is None:
                continue
            mnx, mxx, mny, mxy = r[-1]
            x0, x1 = max(-((128 - mnx) // 256), 0), min((mxx - 128) // 256, W - 1)
            y0, y1 = max(-((128 - mny) // 256), 0), min((mxy - 128) // 256, H - 1)
            if x0 <= x1 and y0 <= y1:
                want[y0 // 32:y1 // 32 + 1, x0 // 32:x1 // 32 + 1] += 1
        np.testing.assert_array_equal(render_ref.tile_counts(v, faces, cam, W, H), want.reshape(-1))
