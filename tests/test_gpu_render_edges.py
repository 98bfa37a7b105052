"""GPU: the template render chain (csrc/render.hip, fp_warp_depth, fp_template_downsample) at the production shape and at
the edges where a binning / tiling rasterizer goes wrong, against the numpy restatement of its contract (tests/render_ref.py).
"Bit for bit" is what test_gpu_render._check_view asserts: tri_id, mask, depth bits and box equal, colour within one step."""
import numpy as np
import pytest
import torch

from foundpose_amd import crop_util, gen_templates, synthetic
from foundpose_amd._lib import FoundPoseNativeError, call, ptr, stream
from foundpose_amd.crop_util import PinholePlaneCameraModel
from foundpose_amd.renderer import TILE, TRI_BYTES, VERT_BYTES, HipRasterizer, Mesh, camera_params, vertex_normals
from oracle import crop as ocrop

from . import render_ref
from .test_gpu_render import _check_view, _look_cam, cam16

pytestmark = pytest.mark.gpu
KEYS = ("depth", "mask", "tri_id", "color", "boxes")
EMPTY_BOX = [2**31 - 1, 2**31 - 1, -2**31, -2**31]


def _setup_only(r, obj_id, cams, sentinel=-7):
    """fp_render_setup alone -> (tile_offsets int64 [B * tiles + 1], status int64 [4]); buffers start at `sentinel`."""
    dm = r.objects[obj_id]
    B, W, H = len(cams), cams[0].width, cams[0].height
    V, F = len(dm.mesh.vertices), len(dm.mesh.faces)
    tiles = -(-W // TILE) * -(-H // TILE)
    dev = r.device
    p = torch.from_numpy(camera_params(cams)).to(dev)
    vert_ws = torch.empty(B * V * VERT_BYTES, dtype=torch.uint8, device=dev)
    tri_ws = torch.empty(B * F * TRI_BYTES, dtype=torch.uint8, device=dev)
    counts = torch.full((B * tiles,), sentinel, dtype=torch.int32, device=dev)
    offsets = torch.full((B * tiles + 1,), sentinel, dtype=torch.int64, device=dev)
    status = torch.full((4,), sentinel, dtype=torch.int64, device=dev)
    try:
        call("fp_render_setup", ptr(dm.verts), ptr(dm.normals), ptr(dm.colors), V, ptr(dm.faces), F, ptr(p), B, W, H,
             ptr(vert_ws), ptr(tri_ws), ptr(counts), ptr(offsets), ptr(None), ptr(status), ptr(None), ptr(None), ptr(None),
             ptr(None), ptr(None), stream())
    finally:
        torch.cuda.synchronize()
    return offsets.cpu().numpy(), status.cpu().numpy(), counts.cpu().numpy()


def _check_binning(r, obj_id, mesh, cams):
    """The per-tile counts (restated from every face's pixel box) and their exclusive int64 scan, for the whole batch."""
    W, H = cams[0].width, cams[0].height
    want = np.concatenate([render_ref.tile_counts(mesh.vertices, mesh.faces, cam16(c), W, H) for c in cams])
    offsets, status, _ = _setup_only(r, obj_id, cams)
    np.testing.assert_array_equal(offsets[:-1], np.cumsum(want) - want)
    assert offsets[-1] == status[2] == want.sum() and status[1] == 0
    return want


def _render_check(r, obj_id, mesh, cams):
    got = r.render_views(obj_id, cams, with_tri_id=True)
    refs = []
    for b, cam in enumerate(cams):
        refs.append(render_ref.render(mesh, cam16(cam), cam.width, cam.height))
        _check_view(got, refs[-1], b)
    return got, refs


def _equal_views(a, i, b, j):
    for k in KEYS:
        assert torch.equal(a[k][i], b[k][j]), (k, i, j)


# ---------------------------------------------------------------- screen-space meshes: f = 512, c = 0, eye = world
def _screen_cam(W, H, c=(0.0, 0.0)):
    return PinholePlaneCameraModel(W, H, (512.0, 512.0), c)


def _screen_mesh(tris, seed=0):
    """Triangles given as window points (u, v[, z]) of _screen_cam: at z = 512 a point lands exactly on (u, v)."""
    pts = np.array([[p[0], p[1], p[2] if len(p) > 2 else 512.0] for t in tris for p in t], np.float64)
    v = np.stack([pts[:, 0] * pts[:, 2] / 512.0, pts[:, 1] * pts[:, 2] / 512.0, pts[:, 2]], 1).astype(np.float32)
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    col = np.random.default_rng(seed).integers(0, 256, (len(v), 3)).astype(np.float32) / np.float32(255)
    return Mesh(v, f, col, vertex_normals(v, f))


# ---------------------------------------------------------------- 1. production shape
def test_production_shape_bit_for_bit():
    """gen_templates at LM-O settings: ~20k triangles, 32 views of 2520 x 2520 (79 x 79 tiles, a partial last one) in one
    call.  All 199 712 tile offsets equal the restated scan (about 196 counts per scan thread); views 0, 17 and 31 (the last
    stretch of the offsets) are bit for bit and equal to the same views rendered alone."""
    opts = gen_templates.GenTemplatesOpts(version="t", object_dataset="lmo")
    K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])
    _, rc = gen_templates.base_cameras(K, (640, 480), opts)
    assert (rc.width, rc.height) == (2520, 2520)
    views = gen_templates.template_views(opts, (346.31, 1499.84))[:32]
    cams = [gen_templates.view_camera(rc, v) for v in views]
    mesh = synthetic.make_blob_mesh(100, 100, radius=70.0, seed=0)
    assert 19000 <= len(mesh.faces) <= 20000
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    counts = _check_binning(r, 1, mesh, cams)
    assert len(counts) == 32 * 79 * 79 and -(-len(counts) // 1024) >= 190
    got = r.render_views(1, cams, with_tri_id=True)
    for i in (0, 17, 31):
        ref = render_ref.render(mesh, cam16(cams[i]), 2520, 2520)
        assert ref["mask"].mean() > 2.0
        _check_view(got, ref, i)
        _equal_views(got, i, r.render_views(1, [cams[i]], with_tri_id=True), 0)


# ---------------------------------------------------------------- 2. odd viewports
@pytest.mark.parametrize("W,H,f", [(1, 1, 10.0), (33, 33, 60.0), (1001, 37, 150.0), (8192, 8, 2000.0)])
def test_odd_viewports(W, H, f):
    """Single pixel, one pixel into the second tile, a partial tile on both axes, FP_RENDER_MAX_SIDE with one tile row;
    each batch also holds a view cut by the right edge."""
    mesh = synthetic.make_blob_mesh(10, 12, radius=60.0, seed=6)
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    eye = np.array([130.0, -360.0, 150.0])
    cams = [_look_cam(W, H, (f, f * 1.01), (W / 2 + 0.13, H / 2 - 0.21), eye),
            _look_cam(W, H, (f, f), (W - 0.7 - 0.1 * f, H / 2 + 0.4), eye, seed_up=0.4)]
    _check_binning(r, 1, mesh, cams)
    _, refs = _render_check(r, 1, mesh, cams)
    assert all(ref["box"] is not None for ref in refs)
    if W == 1:
        assert refs[0]["mask"][0, 0] == 255


def test_viewport_beyond_max_side_raises_and_writes_nothing():
    mesh = synthetic.make_blob_mesh(10, 12, radius=60.0, seed=6)
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    for W, H in ((8193, 8), (8, 8193)):
        cam = _look_cam(W, H, (2000.0, 2000.0), (W / 2, H / 2), np.array([0.0, -400.0, 0.0]))
        with pytest.raises(FoundPoseNativeError, match="viewport"):
            r.render_views(1, [cam])
    # the refused call launched nothing: buffers filled before it keep their sentinel
    dm = r.objects[1]
    status = torch.full((4,), -7, dtype=torch.int64, device=r.device)
    counts = torch.full((257,), -7, dtype=torch.int32, device=r.device)
    offsets = torch.full((258,), -7, dtype=torch.int64, device=r.device)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=r.device)
    p = torch.from_numpy(camera_params([cam])).to(r.device)
    with pytest.raises(FoundPoseNativeError):
        call("fp_render_setup", ptr(dm.verts), ptr(dm.normals), ptr(dm.colors), len(dm.mesh.vertices), ptr(dm.faces),
             len(dm.mesh.faces), ptr(p), 1, 8193, 8, ptr(ws), ptr(ws), ptr(counts), ptr(offsets), ptr(None), ptr(status),
             ptr(None), ptr(None), ptr(None), ptr(None), ptr(None), stream())
    torch.cuda.synchronize()
    assert (status == -7).all() and (counts == -7).all() and (offsets == -7).all() and (ws == 0).all()


# ---------------------------------------------------------------- 3. binning edges
BW, BH = 200, 150   # 7 x 5 tiles, the last ones partial

BINNING_CASES = {
    # vertices far outside on every side: every tile, negative fixed point
    "covers_every_tile": ([[(-5000.3, -4000.7, 512), (9000.1, -3000.2, 600), (-2000.6, 9000.4, 700)]],
                          lambda m: (m == 255).all()),
    # boxes ending exactly on the pixel centres 31.5 / 32.5 either side of a tile border, and just short of it
    "tile_border": ([[(20.5, 5.5), (31.5, 5.5), (31.5, 20.5)], [(32.5, 5.5), (44.5, 5.5), (32.5, 20.5)],
                     [(5.5, 20.5), (20.5, 31.5), (5.5, 31.5)], [(5.5, 32.5), (20.5, 32.5), (5.5, 44.5)],
                     [(31.5, 31.5), (40.2, 31.5), (31.5, 45.1)], [(32.2, 60.1), (44.3, 62.2), (38.1, 63.8)],
                     [(52.1, 40.2), (63.8, 44.4), (60.0, 52.3)], [(70.2, 95.9), (90.7, 90.2), (95.8, 95.7)]],
                    # top-left rule on the centres: right and bottom edges out, left and top edges in
                    lambda m: m[5, 31] == 0 and m[5, 32] == 255 and m[31, 5] == 0 and m[32, 5] == 255 and m[31, 31] == 255),
    # one pixel wide, across the whole viewport, both diagonals; and one a third of a pixel wide
    "slivers": ([[(-2.0, -1.5, 530), (202.0, 151.5, 530), (203.0, 151.5, 530)], [(-2.0, -1.5, 530), (203.0, 151.5, 530), (-1.0, -1.5, 530)],
                 [(201.0, -1.7, 520), (-1.0, 151.2, 640), (0.0, 151.2, 640)], [(201.0, -1.7, 520), (0.0, 151.2, 640), (202.0, -1.7, 520)],
                 [(-3.0, 40.2, 700), (203.0, 120.3, 700), (203.0, 120.63, 700)]],
                lambda m: 200 < (m > 0).sum() < 800),
    # no pixel centre inside (also some left of / above the viewport: negative boxes are empty)
    "sub_pixel": ([[(x + 0.1, y + 0.05), (x + 0.45, y + 0.1), (x + 0.1, y + 0.48)] for x in (0, 31, 32, 63, 100, 199) for y in (0, 31, 32, 149)]
                  + [[(x + 0.55, y + 0.6), (x + 0.95, y + 0.9), (x + 0.6, y + 0.98)] for x in (5, 31, 64) for y in (7, 31, 100)]
                  + [[(-0.9, 10.0), (-0.1, 12.0), (-0.5, 30.0)], [(10.0, -0.9), (50.0, -0.1), (30.0, -0.6)],
                     [(-0.45, 40.0), (0.45, 40.2), (0.0, 40.3)]],
                  lambda m: not m.any()),
    # collinear faces (through pixel centres, diagonal) and a repeated vertex id (added below)
    "zero_area": ([[(10.5, 10.5), (50.5, 10.5), (90.5, 10.5)], [(10.0, 10.0), (20.0, 20.0), (30.0, 30.0)],
                   [(33.5, 5.5), (33.5, 60.5), (33.5, 140.5)]],
                  lambda m: not m.any()),
    # cut by the left, right, top and bottom edge
    "viewport_edges": ([[(-30.3, 50.2, 600), (20.4, 40.1, 600), (15.7, 80.9, 600)], [(190.2, 50.6), (230.1, 60.3), (185.4, 90.8)],
                        [(50.3, -20.2, 700), (80.9, 10.3, 650), (40.1, 15.2, 600)], [(120.4, 140.3), (150.2, 170.1), (110.8, 165.9)]],
                       lambda m: m[:, 0].any() and m[:, -1].any() and m[0].any() and m[-1].any()),
}


@pytest.mark.parametrize("case", sorted(BINNING_CASES))
def test_binning_edges(case):
    tris, expect = BINNING_CASES[case]
    mesh = _screen_mesh(tris, seed=len(case))
    if case == "zero_area":   # faces (a, a, b) and (a, b, b) on a real triangle's vertices
        v = np.concatenate([mesh.vertices, np.array([[60.0, 70.0, 512.0], [90.0, 71.0, 512.0]], np.float32)])
        n = len(mesh.vertices)
        f = np.concatenate([mesh.faces, np.array([[n, n, n + 1], [n, n + 1, n + 1], [n + 1, n, n]], np.int32)])
        mesh = Mesh(v, f, np.full((len(v), 3), 0.5, np.float32), vertex_normals(v, f))
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    cams = [_screen_cam(BW, BH), _screen_cam(BW, BH, (0.37, -0.29))]
    _check_binning(r, 1, mesh, cams)
    got, refs = _render_check(r, 1, mesh, cams)
    assert expect(refs[0]["mask"]), case
    if not refs[0]["mask"].any():
        assert got["boxes"][0].tolist() == EMPTY_BOX


# ---------------------------------------------------------------- 4. ties across LDS chunks
def test_ties_across_lds_chunks_take_the_lowest_id():
    """1200 copies of one quad and 300 of a second, interleaved and overlapping it at the same depth (z = 512 exactly),
    all in tile (1, 1) of a 96 x 96 viewport: 3000 records, 12 LDS chunks, written to the tile list in whatever order the
    atomics give.  Faces elsewhere take ids 0..699 so the lowest tied id sits in the middle of the face range.  Every
    covered pixel takes the lowest id of the faces covering it."""
    rng = np.random.default_rng(9)
    qa = [(36.2, 35.7), (59.8, 36.4), (60.3, 58.9), (35.6, 60.1)]
    qb = [(40.3, 41.1), (62.7, 40.2), (63.1, 62.8), (41.4, 63.3)]
    geo = [(qa[0], qa[1], qa[2]), (qa[0], qa[2], qa[3]), (qb[0], qb[1], qb[3]), (qb[1], qb[2], qb[3])]
    kinds = rng.permutation(np.repeat([0, 1, 2, 3], [1200, 1200, 300, 300]))
    fill = [((70.0 + (k % 20), 70.0 + (k // 20) % 20, 600), (71.5 + (k % 20), 70.2 + (k // 20) % 20, 600),
             (70.3 + (k % 20), 72.0 + (k // 20) % 20, 600)) for k in range(700)]
    tris = fill + [geo[k] for k in kinds]
    mesh = _screen_mesh(tris, seed=3)
    W = H = 96
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    cam, other = _screen_cam(W, H), _screen_cam(W, H, (1.3, -2.1))
    want_counts = _check_binning(r, 1, mesh, [cam])
    assert want_counts[1 * 3 + 1] == 3000
    got, refs = _render_check(r, 1, mesh, [cam])
    # analytic: the lowest id among the faces whose coverage holds the pixel
    expect = np.full((H, W), -1, np.int64)
    for g in range(4):
        lo = 700 + int(np.argmax(kinds == g))   # the first face of this geometry
        cov = render_ref.face_coverage(mesh.vertices, mesh.faces[lo:lo + 1], cam16(cam), W, H) > 0
        expect = np.where(cov & ((expect < 0) | (lo < expect)), lo, expect)
    tri = got["tri_id"][0].cpu().numpy()
    quad = expect >= 0
    assert quad.sum() > 500 and np.array_equal(tri[quad], expect[quad]) and len(np.unique(tri[quad])) >= 3
    assert np.all(got["depth"][0].cpu().numpy()[quad] == np.float32(512.0))
    assert np.array_equal(tri[quad], refs[0]["tri_id"][quad])
    again = r.render_views(1, [cam], with_tri_id=True)
    _equal_views(got, 0, again, 0)
    mixed = r.render_views(1, [other, cam, other], with_tri_id=True)
    _equal_views(got, 0, mixed, 1)


# ---------------------------------------------------------------- 5. fixed-point range and status bits
M21 = 2**21 - 1


def test_fixed_point_limit_renders_bit_for_bit():
    """Vertices at +-(2^21 - 1) px (+-(2^29 - 256) fixed point): edge functions near 2^60, rounded by the (double) cast."""
    mesh = _screen_mesh([[(-M21, 20.5), (M21, 30.25), (50.5, M21)],
                         [(-M21, -M21, 512), (M21, 10.3, 512), (60.7, M21, 512)],
                         [(M21, -M21, 512), (70.1, 90.6, 300), (-M21, 80.2, 512)]])
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    cams = [_screen_cam(128, 96), _screen_cam(128, 96, (0.6, 0.2))]
    X, _, _, _ = render_ref.transform(mesh.vertices, mesh.normals, cam16(cams[0]))
    assert np.abs(X).max() == M21 * 256
    _check_binning(r, 1, mesh, cams)
    _, refs = _render_check(r, 1, mesh, cams)
    assert refs[0]["mask"].all() and {0, 2} <= set(np.unique(refs[0]["tri_id"]).tolist())   # face 1 ties with 0, 2 is nearer


@pytest.mark.parametrize("u", [2**21 + 1, -(2**21 + 1)])
def test_beyond_fixed_point_range_raises(u):
    mesh = _screen_mesh([[(u, 20.5), (30.0, 30.25), (50.5, 60.0)]])
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    with pytest.raises(ValueError, match="fixed-point range"):
        r.render_views(1, [_screen_cam(64, 64)])


@pytest.mark.parametrize("bad", [3, 1000000, -1])
def test_face_id_outside_vertex_range_raises(bad):
    v = np.array([[-20, -20, 500], [20, -20, 500], [0, 20, 500]], np.float32)
    good = np.array([[0, 1, 2]], np.int32)
    f = np.array([[0, 1, 2], [0, bad, 2]], np.int32)
    mesh = Mesh(v, f, np.full((3, 3), 0.5, np.float32), vertex_normals(v, good))
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    with pytest.raises(ValueError, match="face index"):
        r.render_views(1, [PinholePlaneCameraModel(64, 64, (100.0, 100.0), (32.0, 32.0))])
    _, status, _ = _setup_only(r, 1, [PinholePlaneCameraModel(64, 64, (100.0, 100.0), (32.0, 32.0))])
    assert status[1] == 2


def test_off_screen_view_in_a_batch():
    """View 1 sees the mesh in front of the camera (beyond the near plane) but entirely off-screen: an empty box, a zero
    mask and depth, no triangle id; the views around it equal the same views rendered alone."""
    mesh = synthetic.make_blob_mesh(20, 24, radius=60.0, seed=7)
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    eye = np.array([0.0, -400.0, 60.0])
    cams = [_look_cam(96, 80, (150.0, 150.0), (48.0, 40.0), eye), _look_cam(96, 80, (150.0, 150.0), (-5000.0, 40.0), eye),
            _look_cam(96, 80, (150.0, 150.0), (60.0, 30.0), eye, seed_up=0.5)]
    got, refs = _render_check(r, 1, mesh, cams)
    assert refs[1]["box"] is None and got["boxes"][1].tolist() == EMPTY_BOX
    assert not got["mask"][1].any() and not got["depth"][1].any() and (got["tri_id"][1] == -1).all()
    for i in (0, 2):
        assert refs[i]["box"] is not None
        _equal_views(got, i, r.render_views(1, [cams[i]], with_tri_id=True), 0)


# ---------------------------------------------------------------- 8 (GPU half). the watertight random sheet
@pytest.mark.parametrize("kind", ["fronto", "tilted"])
def test_random_sheet_mask_is_the_outline(kind):
    from .test_templates_cpu import SHEET_C, SHEET_F, SHEET_H, SHEET_PLANES, SHEET_W
    v, f, ring = render_ref.random_sheet(12, 9, (-60.0, 60.0), (-45.0, 45.0), SHEET_PLANES[kind], seed=11)
    mesh = Mesh(v, f, np.full((len(v), 3), 0.7, np.float32), vertex_normals(v, f))
    cam = PinholePlaneCameraModel(SHEET_W, SHEET_H, (SHEET_F, SHEET_F), SHEET_C)
    X, Y, _, _ = render_ref.transform(v, np.zeros_like(v), cam16(cam))
    py, px = np.mgrid[0:SHEET_H, 0:SHEET_W]
    side = render_ref.inside_polygon(px.astype(np.int64) * 256 + 128, py.astype(np.int64) * 256 + 128, X[ring], Y[ring])
    count = render_ref.face_coverage(v, f, cam16(cam), SHEET_W, SHEET_H)
    r = HipRasterizer()
    r.add_object_model(1, mesh=mesh)
    got, _ = _render_check(r, 1, mesh, [cam])
    m = got["mask"][0].cpu().numpy() > 0
    assert np.array_equal(m, count == 1) and m[side == 1].all() and not m[side == -1].any()


# ---------------------------------------------------------------- 6. fp_warp_depth
def _rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    R = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    T = np.eye(4)
    T[:3, :3] = R
    return T


def _warp_depth(src, params, recompute, out_h, out_w, depth_check=1):
    B, Hs, Ws = src.shape
    s = torch.from_numpy(src).cuda()
    p = torch.from_numpy(params).cuda()
    rc = None if recompute is None else torch.tensor(recompute, dtype=torch.int32).cuda()
    out = torch.full((B, out_h, out_w), -5.0, dtype=torch.float32, device="cuda")
    call("fp_warp_depth", ptr(s), Hs, Ws, ptr(p), ptr(rc), B, out_h, out_w, depth_check, ptr(out), stream())
    return out.cpu().numpy()


def test_warp_depth_direct():
    """A 517 x 1001 source, 67 x 130 crops (not multiples of the 64 x 4 block), recompute mixed 0 / 1 and NULL; pixels that
    map outside the source and crop rays behind the source camera give 0, source depth 0 stays 0."""
    Hs, Ws, oh, ow = 517, 1001, 67, 130
    rng = np.random.default_rng(12)
    T0 = np.eye(4)
    T0[:3, :3] = _rot("x", 20)[:3, :3] @ _rot("z", 35)[:3, :3]
    T0[:3, 3] = [40.0, -25.0, -600.0]
    src_cam = PinholePlaneCameraModel(Ws, Hs, (700.0, 690.0), (500.3, 258.1), T0)
    crops = [PinholePlaneCameraModel(ow, oh, (300.0, 300.0), (65.0, 33.5), T0 @ _rot("y", 2.0)),          # inside the source
             PinholePlaneCameraModel(ow, oh, (150.0, 160.0), (-20.0, 70.0), T0 @ _rot("x", -4.0)),       # partly outside
             PinholePlaneCameraModel(ow, oh, (60.0, 60.0), (65.0, 33.0), T0 @ _rot("y", 100.0)),         # rays behind the source
             PinholePlaneCameraModel(ow, oh, (900.0, 880.0), (64.7, 33.2), T0 @ _rot("y", -5.0) @ _rot("z", 7.0))]
    B = len(crops)
    src = rng.uniform(300.0, 900.0, (B, Hs, Ws)).astype(np.float32)
    src[:, 200:330, 400:650] = 0.0                                           # background holes
    src[:, ::7, ::5] = 0.0
    params = np.stack([crop_util.camera_pair_params(src_cam, c) for c in crops])
    mixed = [1, 0, 1, 0]
    for rec in (mixed, None):
        got = _warp_depth(src, params, rec, oh, ow)
        for b in range(B):
            want = render_ref.warp_depth(src[b], params[b], oh, ow, recompute=True if rec is None else bool(rec[b]))
            assert np.array_equal(got[b].view(np.int32), want.view(np.int32)), (rec, b)
        if rec is mixed:
            by_flag = got
    full = got
    for b in range(B):   # the flag matters in every view: extrinsics differ
        assert (by_flag[b] != full[b]).sum() > 100 or mixed[b] == 1
    mx, my = ocrop.crop_maps(params[1], oh, ow, True)
    out1 = (np.rint(mx) < 0) | (np.rint(mx) >= Ws) | (np.rint(my) < 0) | (np.rint(my) >= Hs)
    assert out1.sum() > 100 and not full[1][out1].any() and full[1][~out1].any()
    mx, my = ocrop.crop_maps(params[2], oh, ow, True)
    mxn, myn = ocrop.crop_maps(params[2], oh, ow, False)
    behind = (mx == -1) & (my == -1)
    lands = behind & (np.rint(mxn) >= 0) & (np.rint(mxn) < Ws) & (np.rint(myn) >= 0) & (np.rint(myn) < Hs)
    assert lands.sum() > 20 and not full[2][behind].any()
    sx, sy = np.rint(ocrop.crop_maps(params[0], oh, ow, True)[0]).astype(int), np.rint(ocrop.crop_maps(params[0], oh, ow, True)[1]).astype(int)
    zero = src[0][sy, sx] == 0
    assert zero.sum() > 100 and not full[0][zero].any() and full[0][~zero].all()


# ---------------------------------------------------------------- 7. fp_template_downsample
def _downsample(color, depth, mask, f):
    B, _, Hs, Ws = color.shape
    oh, ow = Hs // f, Ws // f
    c, d, m = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (color, depth, mask))
    rgb = torch.empty(B, 3, oh, ow, dtype=torch.uint8, device="cuda")
    d16 = torch.empty(B, oh, ow, dtype=torch.uint16, device="cuda")
    m8 = torch.empty(B, oh, ow, dtype=torch.uint8, device="cuda")
    boxes = torch.empty(B, 4, dtype=torch.int32, device="cuda")
    call("fp_template_downsample", ptr(c), ptr(d), ptr(m), B, oh, ow, f, ptr(rgb), ptr(d16), ptr(m8), ptr(boxes), stream())
    return rgb.cpu().numpy(), d16.cpu().numpy().astype(np.int64), m8.cpu().numpy(), boxes.cpu().numpy()


def _block_value(f, k, below):
    """A colour y such that a block of f x f copies of y gives fl(255 fl(sum fl(1/f^2))) = k exactly (below: the fp32
    number just under k), in the kernel's summation order; None if no y within 512 ulps of k / 255 does."""
    y0 = np.float32(k / 255.0)
    cand = (y0.view(np.int32) + np.arange(-512, 513, dtype=np.int32)).view(np.float32)
    row = cand.copy()
    for _ in range(1, f):
        row = row + cand
    s = row.copy()
    for _ in range(1, f):
        s = s + row
    v = np.float32(255) * (s * (np.float32(1) / np.float32(f * f)))
    target = np.nextafter(np.float32(k), np.float32(0)) if below else np.float32(k)
    hit = np.nonzero(v == target)[0]
    return cand[hit[0]] if len(hit) else None


DEPTHS = [0.5, 1.5, 2.5, 3.5, 100.5, 101.5, 65534.5, 65535.5, 65535.0, -0.5, -3.5, -1e9, 0.0, 1e9, 412.49, 412.51]
DEPTH_U16 = [0, 2, 2, 4, 100, 102, 65534, 65535, 65535, 0, 0, 0, 0, 65535, 412, 413]


@pytest.mark.parametrize("f", [1, 2, 3, 5, 8, 16])
def test_template_downsample_direct(f):
    """Random views, views with block means exactly on an integer step and one fp32 ulp under it (truncation), the depth
    rounding / clamping edges at the top-left samples, masks covered at the output border only, and an empty view."""
    oh, ow = (67, 5) if f in (1, 3, 8) else (5, 67)
    Hs, Ws = oh * f, ow * f
    rng = np.random.default_rng(f)
    B = 4
    color = rng.uniform(0, 1, (B, 3, Hs, Ws)).astype(np.float32)
    color[0, :, ::3] = np.rint(color[0, :, ::3] * 255) / np.float32(255)      # k / 255 colours, as the render writes them
    depth = rng.uniform(-50, 70000, (B, Hs, Ws)).astype(np.float32)
    mask = (rng.uniform(size=(B, Hs, Ws)) < 0.5).astype(np.uint8) * 255
    # view 1: exact-integer and one-ulp-under block means; depth edges; mask only on the output border
    ks, want_rgb = [], np.zeros((3, oh, ow), np.int64)
    for i in range(oh * ow * 3):
        ch, y, x = i // (oh * ow), (i // ow) % oh, i % ow
        below = i % 2 == 1
        k = 1 + (7 * i) % 254
        val = _block_value(f, k, below)
        while val is None:
            k = k % 254 + 1
            val = _block_value(f, k, below)
        color[1, ch, y * f:(y + 1) * f, x * f:(x + 1) * f] = val
        want_rgb[ch, y, x] = k - 1 if below else k
        ks.append(k)
    d = depth[1, ::f, ::f]
    for i in range(d.size):
        d.flat[i] = DEPTHS[i % len(DEPTHS)]
    mask[1] = 0
    mask[1, 0, ::f] = mask[1, -f, ::f] = mask[1, ::f, 0] = mask[1, ::f, -f] = 200   # top-left samples of the border pixels
    if f > 1:
        mask[1, 1::f, 1::f] = 255     # covered sub-pixels that are not the top-left sample: not sampled
    # view 2: nothing covered at any top-left sample
    mask[2] = 0
    if f > 1:
        mask[2, f - 1::f, f - 1::f] = 255
    mask[3] = 0
    rgb, d16, m8, boxes = _downsample(color, depth, mask, f)
    for b in range(B):
        wr, wd, wm = render_ref.downsample(color[b], depth[b], mask[b], f)
        np.testing.assert_array_equal(rgb[b], wr)
        np.testing.assert_array_equal(d16[b], wd.astype(np.int64))
        np.testing.assert_array_equal(m8[b], wm)
        ys, xs = np.nonzero(wm)
        assert boxes[b].tolist() == ([xs.min(), ys.min(), xs.max(), ys.max()] if len(xs) else EMPTY_BOX), b
        mean64 = color[b].astype(np.float64).reshape(3, oh, f, ow, f).mean((2, 4))
        assert np.abs(rgb[b].astype(np.int64) - np.floor(255.0 * mean64)).max() <= 1
    np.testing.assert_array_equal(rgb[1].astype(np.int64), want_rgb)
    np.testing.assert_array_equal(d16[1].reshape(-1), np.resize(DEPTH_U16, oh * ow))
    ring = np.zeros((oh, ow), np.uint8)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = 200, 200, 200, 200
    np.testing.assert_array_equal(m8[1], ring)
    assert boxes[1].tolist() == [0, 0, ow - 1, oh - 1] and boxes[2].tolist() == EMPTY_BOX == boxes[3].tolist()


@pytest.mark.parametrize("f", [0, 17])
def test_template_downsample_factor_out_of_range_raises(f):
    z = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(FoundPoseNativeError, match="bad shape"):
        call("fp_template_downsample", ptr(z), ptr(z), ptr(z), 1, 2, 2, f, ptr(z), ptr(z), ptr(z), ptr(None), stream())
