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
