"""GPU: textured models in the HIP rasterizer (csrc/render.hip, render_raster_kernel<true>): the mip pyramid bit for bit,
geometry identical to the untextured render, colour against the numpy restatement (tests/texture_ref.py) under
magnification, minification, a grazing view, UVs outside [0, 1] and a seam, orientation, the material plumbing,
determinism and the argument checks."""
import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops, synthetic
from foundpose_amd.crop_util import PinholePlaneCameraModel
from foundpose_amd.renderer import HipRasterizer, Mesh, TextureMaterial, camera_params, vertex_normals

from . import render_ref, texture_ref

pytestmark = pytest.mark.gpu
W, H = 96, 80


def _look_cam(W, H, f, eye, up_hint=0.0):
    fwd = -np.asarray(eye, np.float64) / np.linalg.norm(eye)
    up = np.array([up_hint, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    side = np.cross(fwd, up); side /= np.linalg.norm(side)
    down = np.cross(fwd, side)
    T = np.eye(4)
    T[:3, :3] = np.stack([side, down, fwd], 1)
    T[:3, 3] = eye
    return PinholePlaneCameraModel(W, H, (f, f * 1.02), (W / 2 - 0.3, H / 2 + 0.2), T)


def _cams(n, f, dist, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        out.append(_look_cam(W, H, f, d * dist, rng.normal() * 0.3))
    return out


def _quad(size_mm, uv_lo, uv_hi, tex, z=0.0):
    """A square in the world plane z = `z`, facing +z, UVs spanning [uv_lo, uv_hi] (v = uv_hi at world -y)."""
    s = size_mm / 2
    v = np.array([[-s, -s, z], [s, -s, z], [s, s, z], [-s, s, z]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    uv = np.array([[uv_lo, uv_hi], [uv_hi, uv_hi], [uv_hi, uv_lo], [uv_lo, uv_lo]], np.float32)
    return Mesh(v, f, np.full((4, 3), 0.5, np.float32), vertex_normals(v, f), uv, tex)


def _untextured(m):
    return Mesh(m.vertices, m.faces, m.colors, m.normals)


def _check_colour(got, ref, b):
    np.testing.assert_array_equal(got["tri_id"][b].cpu().numpy(), ref["tri_id"])
    assert np.array_equal(got["depth"][b].cpu().numpy().view(np.int32), ref["depth"].view(np.int32))
    np.testing.assert_array_equal(got["mask"][b].cpu().numpy(), ref["mask"])
    cov = ref["mask"] > 0
    c = np.rint(got["color"][b].cpu().numpy() * 255.0).astype(np.int32)
    assert np.all(c[~cov] == 0)
    diff = np.abs(c[cov] - ref["color"][cov].astype(np.int32))
    assert diff.max() <= 1 and (diff.max(1) == 0).mean() >= 0.999, (diff.max(), (diff.max(1) == 0).mean())
    assert tuple(got["boxes"][b].tolist()) == tuple(int(x) for x in ref["box"])


@pytest.mark.parametrize("w, h", [(1, 1), (1, 7), (7, 1), (5, 3), (64, 64), (100, 37), (257, 129), (2048, 2048)])
def test_pyramid_is_bit_exact(w, h):
    img = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = ops.texture_mips(torch.from_numpy(img).cuda()).cpu().numpy().view(np.uint32)
    ref = texture_ref.pack(texture_ref.mip_levels(img))
    assert got.shape == ref.shape == (_lib.texture_levels(w, h)[1],)
    assert np.array_equal(got, ref)


def _geometry_equal(a, b, i, j):
    for k in ("depth", "mask", "tri_id", "boxes"):
        x, y = a[k][i].cpu().numpy(), b[k][j].cpu().numpy()
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def test_geometry_is_that_of_the_untextured_render():
    r = HipRasterizer()
    blob = synthetic.make_textured_blob_mesh(30, 34, radius=60.0, seed=2, tex_size=256)    # per-corner unmerged
    base = synthetic.make_blob_mesh(30, 34, radius=60.0, seed=2)                             # the same geometry, merged
    rng = np.random.default_rng(1)
    merged = Mesh(base.vertices, base.faces, base.colors, base.normals,
                  rng.uniform(-0.2, 1.2, (len(base.vertices), 2)).astype(np.float32), synthetic.make_texture(128, 2))
    for oid, m in ((1, blob), (2, _untextured(blob)), (3, merged), (4, _untextured(merged)), (5, _untextured(base))):
        r.add_object_model(oid, mesh=m)
    cams = _cams(6, 150.0, 420.0)
    out = {oid: r.render_views(oid, cams, with_tri_id=True) for oid in (1, 2, 3, 4, 5)}
    for b in range(len(cams)):
        assert out[1]["mask"][b].float().mean() > 20
        _geometry_equal(out[1], out[2], b, b)
        _geometry_equal(out[3], out[4], b, b)
        _geometry_equal(out[2], out[5], b, b)        # unmerging changes no pixel
        assert not torch.equal(out[1]["color"][b], out[2]["color"][b])


def _render_case(mesh, cams, material=None):
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh, material=material)
    got = r.render_views(1, cams, with_tri_id=True)
    mat = (material or TextureMaterial()).as_array()
    refs = [texture_ref.render_textured(mesh, camera_params([c])[0], W, H, mat) for c in cams]
    for b, ref in enumerate(refs):
        assert ref["mask"].sum() > 0
        _check_colour(got, ref, b)
    return np.concatenate([ref["lod"][ref["mask"] > 0] for ref in refs])


def test_colour_magnification():
    mesh = synthetic.make_textured_blob_mesh(30, 34, radius=60.0, seed=4, tex_size=32)
    lod = _render_case(mesh, _cams(4, 150.0, 380.0, seed=5))
    assert (lod < 0).mean() > 0.75


def test_colour_minification_across_levels():
    mesh = synthetic.make_textured_blob_mesh(30, 34, radius=60.0, seed=6, tex_size=1024)
    lod = _render_case(mesh, _cams(3, 150.0, 1500.0, seed=7) + _cams(2, 150.0, 450.0, seed=8))
    assert lod.min() < 4.5 and lod.max() > 8.0 and len(np.unique(np.floor(lod[lod > 0]))) >= 5


def test_colour_grazing_view_uv_outside_unit_square_and_other_material():
    tex = synthetic.make_texture(256, 3)
    quad = _quad(200.0, -1.5, 2.5, tex)
    cams = [_look_cam(W, H, 120.0, np.array([0.0, 380.0, 75.0]), 0.1),        # about 79 degrees off the normal
            _look_cam(W, H, 120.0, np.array([40.0, -30.0, 300.0]), 0.2)]
    lod = _render_case(quad, cams, TextureMaterial(0.3, 0.55, (0.9, 1.0, 0.7), False))
    assert lod.max() - lod.min() > 2.0


def test_colour_across_the_seam():
    mesh = synthetic.make_textured_blob_mesh(40, 48, radius=60.0, seed=9, tex_size=256)
    assert (mesh.uv[:, 0] >= 1.0).sum() > 0                                   # the wrapped corners
    # cameras looking at the seam (azimuth 0, the +x side)
    cams = [_look_cam(W, H, 150.0, np.array([420.0, 10.0, 30.0])), _look_cam(W, H, 150.0, np.array([380.0, -60.0, -120.0]), 0.3)]
    _render_case(mesh, cams)


def test_orientation_of_a_quadrant_texture():
    tex = np.zeros((64, 64, 3), np.uint8)
    tex[:32, :32] = (255, 0, 0)        # image top-left: uv (0, 1)
    tex[:32, 32:] = (0, 255, 0)
    tex[32:, :32] = (0, 0, 255)
    tex[32:, 32:] = (255, 255, 255)
    q = _quad(160.0, 0.0, 1.0, tex, z=0.0)
    quad = Mesh(q.vertices, q.faces, q.colors, -q.normals, q.uv, q.texture)     # facing the camera below it
    cam = PinholePlaneCameraModel(W, H, (100.0, 100.0), (48.0, 40.0),
                                  np.array([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, -500.0], [0, 0, 0, 1]]))
    r = HipRasterizer()
    mat = TextureMaterial(0.0, 1.0, (1, 1, 1), False)    # rough: no highlight to tint the quadrants
    r.add_object_model(1, mesh=quad, material=mat)
    c = r.render_views(1, [cam])["color"][0].cpu().numpy()
    # world -y is image up (camera y down), world -x image left; the quad spans pixels 32..63 x 24..55
    q = {"tl": c[26:38, 34:46], "tr": c[26:38, 50:62], "bl": c[42:54, 34:46], "br": c[42:54, 50:62]}
    means = {k: v.reshape(-1, 3).mean(0) for k, v in q.items()}
    assert np.argmax(means["tl"]) == 0 and means["tl"][1] < 0.1 and means["tl"][2] < 0.1
    assert np.argmax(means["tr"]) == 1 and means["tr"][0] < 0.1 and means["tr"][2] < 0.1
    assert np.argmax(means["bl"]) == 2 and means["bl"][0] < 0.1 and means["bl"][1] < 0.1
    assert means["br"].min() > 0.3
    ref = texture_ref.render_textured(quad, camera_params([cam])[0], W, H, mat.as_array())
    assert np.abs(np.rint(c * 255).astype(int) - ref["color"].astype(int)).max() <= 1


def test_material_plumbing_constant_texture_equals_vertex_colour():
    base = synthetic.make_blob_mesh(30, 34, radius=60.0, seed=10)
    k = np.array([200, 90, 30], np.uint8)
    col = np.tile(k.astype(np.float32) / np.float32(255), (len(base.vertices), 1))
    r = HipRasterizer()
    r.add_object_model(1, mesh=Mesh(base.vertices, base.faces, col, base.normals))
    r.add_object_model(2, mesh=Mesh(base.vertices, base.faces, base.colors, base.normals,
                                    np.zeros((len(base.vertices), 2), np.float32), k.reshape(1, 1, 3)),
                       material=TextureMaterial(0.2, 0.8, (1.0, 1.0, 1.0), False))
    cams = _cams(4, 150.0, 420.0, seed=11)
    a, b = r.render_views(1, cams), r.render_views(2, cams)
    assert torch.equal(a["mask"], b["mask"]) and a["mask"].float().mean() > 20
    d = (torch.round(a["color"] * 255) - torch.round(b["color"] * 255)).abs()
    assert float(d.max()) <= 1.0
    # mesh_color replaces the texture: the vertex-coloured path, bit for bit
    r.add_object_model(3, mesh=Mesh(base.vertices, base.faces, base.colors, base.normals,
                                    np.zeros((len(base.vertices), 2), np.float32), k.reshape(1, 1, 3)), mesh_color=(200, 90, 30))
    assert torch.equal(r.render_views(3, cams)["color"], a["color"])


def test_textured_render_is_deterministic_and_batch_independent():
    r = HipRasterizer()
    r.add_object_model(1, mesh=synthetic.make_textured_blob_mesh(30, 34, radius=60.0, seed=12, tex_size=512))
    cams = _cams(24, 150.0, 500.0, seed=13)
    a = r.render_views(1, cams, with_tri_id=True)
    b = r.render_views(1, cams, with_tri_id=True)
    for k in ("depth", "mask", "tri_id", "color", "boxes"):
        assert torch.equal(a[k], b[k]), k
    for i in (0, 9, 23):
        one = r.render_views(1, [cams[i]], with_tri_id=True)
        for k in ("depth", "mask", "tri_id", "color", "boxes"):
            assert torch.equal(one[k][0], a[k][i]), (k, i)
    sub = r.render_views(1, cams[5:12])
    assert torch.equal(sub["color"], a["color"][5:12])


def test_argument_checks_write_nothing():
    from foundpose_amd._lib import FoundPoseNativeError, call, ptr, stream, vp
    from foundpose_amd.renderer import TRI_BYTES, VERT_BYTES
    mesh = synthetic.make_textured_blob_mesh(10, 12, radius=60.0, seed=14, tex_size=16)
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    dm = r.objects[1]
    cams_h = camera_params(_cams(1, 150.0, 420.0))
    dev = "cuda"
    V, F = len(mesh.vertices), len(mesh.faces)
    tiles = ((W + 31) // 32) * ((H + 31) // 32)
    cams = torch.from_numpy(cams_h).to(dev)
    vert_ws = torch.empty(V * VERT_BYTES, dtype=torch.uint8, device=dev)
    tri_ws = torch.empty(F * TRI_BYTES, dtype=torch.uint8, device=dev)
    counts = torch.empty(tiles, dtype=torch.int32, device=dev)
    offsets = torch.empty(tiles + 1, dtype=torch.int64, device=dev)
    status = torch.empty(4, dtype=torch.int64, device=dev)
    color = torch.full((1, H, W, 3), -7.0, device=dev)
    depth = torch.full((1, H, W), -7.0, device=dev)
    mask = torch.full((1, H, W), 7, dtype=torch.uint8, device=dev)
    boxes = torch.full((1, 4), 7, dtype=torch.int32, device=dev)
    args = [ptr(dm.verts), ptr(dm.normals), ptr(dm.colors), V, ptr(dm.faces), F, ptr(cams), 1, W, H, ptr(vert_ws), ptr(tri_ws),
            ptr(counts), ptr(offsets)]
    tail = [ptr(status), ptr(color), ptr(depth), ptr(mask), ptr(None), ptr(boxes)]
    call("fp_render_setup", *args, ptr(None), *tail, stream())
    torch.cuda.synchronize()
    boxes.fill_(7)                        # the setup initialised the boxes; the raster must not touch them now
    lists = torch.empty(max(int(status[2]), 1), dtype=torch.int32, device=dev)
    good = TextureMaterial().as_array()
    nan = good.copy(); nan[1] = np.nan
    big = good.copy(); big[2] = 1.5
    bad_calls = [
        (ptr(dm.uv), ptr(dm.pyramid), 16385, 16, good),
        (ptr(dm.uv), ptr(dm.pyramid), 16, 0, good),
        (ptr(None), ptr(dm.pyramid), 16, 16, good),
        (ptr(dm.uv), ptr(None), 16, 16, good),
        (ptr(dm.uv), ptr(dm.pyramid), 16, 16, nan),
        (ptr(dm.uv), ptr(dm.pyramid), 16, 16, big),
    ]
    for uv_p, pyr_p, tw, th, mat in bad_calls:
        with pytest.raises(FoundPoseNativeError):
            call("fp_render_raster_textured", *args, ptr(lists), *tail, uv_p, pyr_p, tw, th, mat.ctypes.data_as(vp), stream())
    with pytest.raises(FoundPoseNativeError):
        call("fp_render_raster_textured", *args, ptr(lists), *tail, ptr(dm.uv), ptr(dm.pyramid), 16, 16, vp(0), stream())
    torch.cuda.synchronize()
    assert bool((color == -7.0).all()) and bool((depth == -7.0).all()) and bool((mask == 7).all()) and bool((boxes == 7).all())
    pyr = torch.full((8,), 5, dtype=torch.int32, device=dev)
    rgb = torch.zeros(2, 2, 3, dtype=torch.uint8, device=dev)
    for w, h in ((0, 2), (2, -1), (16385, 1)):
        with pytest.raises(FoundPoseNativeError):
            call("fp_texture_mips", ptr(rgb), w, h, ptr(pyr), stream())
    with pytest.raises(FoundPoseNativeError):
        call("fp_texture_mips", ptr(None), 2, 2, ptr(pyr), stream())
    torch.cuda.synchronize()
    assert bool((pyr == 5).all())
    with pytest.raises(ValueError):
        ops.texture_mips(torch.zeros(16385, 1, 3, dtype=torch.uint8, device=dev))
    # a good call after the refused ones renders normally
    call("fp_render_raster_textured", *args, ptr(lists), *tail, ptr(dm.uv), ptr(dm.pyramid), 16, 16, good.ctypes.data_as(vp), stream())
    torch.cuda.synchronize()
    assert bool((mask == 255).any())
