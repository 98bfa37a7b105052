"""GPU: the HIP template rasterizer (csrc/render.hip) against the numpy restatement of its contract (tests/render_ref.py),
its determinism, and the device template chain of gen_templates against a numpy restatement of steps 4-8."""
import numpy as np
import pytest
import torch

from foundpose_amd import crop_util, gen_templates, synthetic
from foundpose_amd.crop_util import PinholePlaneCameraModel
from foundpose_amd.renderer import HipRasterizer, Mesh, RenderType, camera_params, vertex_normals
from oracle import crop as ocrop

from . import render_ref

pytestmark = pytest.mark.gpu
W, H = 96, 80


def _look_cam(W, H, f, c, eye, seed_up=0.0):
    """Camera at `eye` (mm) looking at the origin, OpenCV frame."""
    fwd = -np.asarray(eye, np.float64) / np.linalg.norm(eye)
    up = np.array([seed_up, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    side = np.cross(fwd, up); side /= np.linalg.norm(side)
    down = np.cross(fwd, side)
    T = np.eye(4)
    T[:3, :3] = np.stack([side, down, fwd], 1)   # columns: eye x, y, z in the world
    T[:3, 3] = eye
    return PinholePlaneCameraModel(W, H, f, c, T)


def _pixel_mesh():
    """Coplanar overlaps, shared edges and vertices exactly on pixel centres: a fronto-parallel grid at z = 500 mm whose
    vertices project to pixel centres (f = 100, c = (48, 40)), every quad split along a diagonal, the whole grid repeated
    (coplanar duplicates: ties go to the lower face id), and a tilted quad crossing it."""
    f, z = 100.0, 500.0
    verts, faces, cols = [], [], []
    xs, ys = np.arange(10.5, 86, 6.0), np.arange(8.5, 72, 6.0)
    for copy in range(2):
        base = len(verts)
        for y in ys:
            for x in xs:
                verts.append([(x - 48.0) * z / f, (y - 40.0) * z / f, z])
                cols.append([copy, 0.5, 1 - copy])
        n = len(xs)
        for j in range(len(ys) - 1):
            for i in range(n - 1):
                a, b, c, d = base + j * n + i, base + j * n + i + 1, base + (j + 1) * n + i, base + (j + 1) * n + i + 1
                faces += [(a, b, d), (a, d, c)] if (i + j + copy) % 2 else [(a, b, c), (b, d, c)]
    base = len(verts)
    verts += [[-150, -120, 430], [160, -110, 560], [170, 130, 580], [-140, 125, 440]]
    cols += [[1, 1, 0]] * 4
    faces += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
    v = np.array(verts, np.float32)
    fc = np.array(faces, np.int32)
    return Mesh(v, fc, np.array(cols, np.float32), vertex_normals(v, fc)), PinholePlaneCameraModel(W, H, (f, f), (48.0, 40.0))


def _blob_cams(n, W, H, f, dist=420.0):
    rng = np.random.default_rng(3)
    cams = []
    for _ in range(n):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        cams.append(_look_cam(W, H, (f, f * 1.02), (W / 2 - 0.3, H / 2 + 0.2), d * dist, seed_up=rng.normal() * 0.3))
    return cams


def cam16(cam):
    """The 16 camera doubles the rasterizer takes."""
    return camera_params([cam])[0]


def _check_view(got, ref, b):
    np.testing.assert_array_equal(got["tri_id"][b].cpu().numpy(), ref["tri_id"])
    assert np.array_equal(got["depth"][b].cpu().numpy().view(np.int32), ref["depth"].view(np.int32))
    np.testing.assert_array_equal(got["mask"][b].cpu().numpy(), ref["mask"])
    c = np.rint(got["color"][b].cpu().numpy() * 255.0).astype(np.int32)
    diff = np.abs(c - ref["color"].astype(np.int32))
    assert diff.max() <= 1 and (diff == 0).mean() >= 0.999, (diff.max(), (diff == 0).mean())
    box = got["boxes"][b].tolist()
    if ref["box"] is None:
        assert box[0] > box[2]
    else:
        assert tuple(box) == tuple(int(x) for x in ref["box"])


def test_raster_matches_restatement_bit_for_bit():
    r = HipRasterizer()
    blob = synthetic.make_blob_mesh(36, 40, radius=60.0, seed=1)          # 2800 triangles
    assert 200 <= len(blob.faces) <= 3000
    r.add_object_model(1, mesh=blob)
    cams = _blob_cams(4, W, H, 150.0)
    got = r.render_views(1, cams, with_tri_id=True)
    for b, cam in enumerate(cams):
        ref = render_ref.render(blob, cam16(cam), W, H)
        assert ref["mask"].mean() > 20
        _check_view(got, ref, b)
    grid, gcam = _pixel_mesh()
    assert 200 <= len(grid.faces) <= 3000
    r.add_object_model(2, mesh=grid)
    got = r.render_views(2, [gcam], with_tri_id=True)
    ref = render_ref.render(grid, cam16(gcam), W, H)
    _check_view(got, ref, 0)
    tri = ref["tri_id"]
    n_half = (len(grid.faces) - 2) // 2
    assert ((tri >= 0) & (tri < n_half)).sum() > 1000 and not ((tri >= n_half) & (tri < 2 * n_half)).any()   # ties -> lower id



def test_raster_is_deterministic_and_batch_independent():
    r = HipRasterizer()
    r.add_object_model(1, mesh=synthetic.make_blob_mesh(36, 40, radius=60.0, seed=2))
    cams = _blob_cams(32, W, H, 150.0)
    a = r.render_views(1, cams, with_tri_id=True)
    b = r.render_views(1, cams, with_tri_id=True)
    for k in ("depth", "mask", "tri_id", "color", "boxes"):
        assert torch.equal(a[k], b[k]), k
    for i in (0, 17, 31):
        one = r.render_views(1, [cams[i]], with_tri_id=True)
        for k in ("depth", "mask", "tri_id", "color", "boxes"):
            assert torch.equal(one[k][0], a[k][i]), (k, i)
    single = r.render_object_model(1, cams[5], [RenderType.COLOR, RenderType.DEPTH, RenderType.MASK])
    assert single[RenderType.COLOR].dtype == np.float32 and single[RenderType.COLOR].shape == (H, W, 3)
    assert np.array_equal(single[RenderType.MASK], a["mask"][5].cpu().numpy() > 0)
    assert np.array_equal(single[RenderType.DEPTH], a["depth"][5].cpu().numpy())


def test_near_plane_raises():
    r = HipRasterizer()
    r.add_object_model(1, mesh=synthetic.make_blob_mesh(10, 12, radius=60.0))
    with pytest.raises(ValueError, match="near plane"):
        r.render_views(1, [_look_cam(W, H, (150.0, 150.0), (48.0, 40.0), np.array([0.0, -140.0, 0.0]))])


def test_template_chain_matches_restatement():
    """render -> box -> crop camera -> depth / colour / mask warp -> downsample -> uint8 / uint16, crop 112, SSAA 4."""
    opts = gen_templates.GenTemplatesOpts(version="v1", object_dataset="synth", crop_size=(112, 112), ssaa_factor=4.0)
    render_cam = PinholePlaneCameraModel(640, 640, (800.0, 800.0), (319.5, 320.5))
    mesh = synthetic.make_blob_mesh(36, 40, radius=60.0, seed=4)
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    views = gen_templates.template_views(opts._replace(min_num_viewpoints=3, num_inplane_rotations=2), (400.0, 440.0))[:3]
    got = gen_templates.render_templates(r, 1, views, render_cam, opts)
    dev = r.render_views(1, [gen_templates.view_camera(render_cam, v) for v in views])
    for i, v in enumerate(views):
        cam = gen_templates.view_camera(render_cam, v)
        ref = render_ref.render(mesh, cam16(cam), 640, 640)
        box = [int(x) for x in ref["box"]]
        gen_templates.check_fits(box, 640, 640)
        crop = gen_templates.crop_camera(box, cam, opts)
        params = crop_util.camera_pair_params(cam, crop)
        mx, my = ocrop.crop_maps(params, 448, 448, True)
        mask = ocrop.remap_nearest(ref["mask"], mx, my)
        depth = render_ref.warp_depth(ref["depth"], params, 448, 448, recompute=not np.allclose(cam.T_world_from_eye, crop.T_world_from_eye))
        color = ocrop.remap_linear(dev["color"][i].cpu().numpy(), mx, my).transpose(2, 0, 1)   # the device render's colour
        rgb, d16, m8 = render_ref.downsample(color, depth, mask, 4)
        np.testing.assert_array_equal(got["mask"][i].cpu().numpy(), m8)
        np.testing.assert_array_equal(got["depth"][i].cpu().numpy().astype(np.int64), d16.astype(np.int64))
        diff = np.abs(got["rgb"][i].cpu().numpy().astype(np.int32) - rgb.astype(np.int32))
        assert diff.max() <= 1 and (diff == 0).mean() >= 0.999
        ys, xs = np.nonzero(m8)
        assert got["boxes"][i] == [xs.min(), ys.min(), xs.max(), ys.max()]
        tc = got["cameras"][i]
        assert (tc.width, tc.height) == (112, 112) and tc.f[0] == float(crop.f[0]) * (112 / 448.0) and tc.c[1] == float(crop.c[1]) * 0.25
        assert 300 < d16[m8 > 0].min() and d16.max() < 520
