"""CPU: textured models -- loading (per-vertex and per-corner UVs, ascii and binary, every incomplete case), the material
data, the pyramid layout, and self-checks of the numpy restatement of the textured shading (tests/texture_ref.py)."""
import json
import os

import numpy as np
import pytest

from foundpose_amd import _lib, eval_util, renderer, synthetic
from foundpose_amd.crop_util import PinholePlaneCameraModel
from foundpose_amd.renderer import Mesh, TextureMaterial, camera_params, load_ply, save_ply

from . import render_ref, texture_ref


def _textured(merged=True):
    """A small textured mesh with per-vertex UVs (merged) or the per-corner unmerged blob."""
    if not merged:
        return synthetic.make_textured_blob_mesh(8, 10, radius=30.0, seed=3, tex_size=32)
    m = synthetic.make_blob_mesh(8, 10, radius=30.0, seed=3)
    rng = np.random.default_rng(0)
    uv = rng.uniform(-0.5, 1.5, (len(m.vertices), 2)).astype(np.float32)
    return Mesh(m.vertices, m.faces, m.colors, m.normals, uv, synthetic.make_texture(32, 1))


@pytest.mark.parametrize("binary", [True, False])
def test_per_vertex_uv_round_trip(tmp_path, binary):
    m = _textured()
    p = str(tmp_path / "obj_000001.ply")
    save_ply(p, m, binary=binary)
    assert os.path.exists(tmp_path / "obj_000001.png")
    assert "comment TextureFile obj_000001.png" in open(p, "rb").read(400).decode("ascii", "replace")
    g = load_ply(p, textured=True)
    for k in ("vertices", "faces", "colors", "normals", "uv", "texture"):
        assert np.array_equal(getattr(g, k), getattr(m, k)), k
    assert g.uv.dtype == np.float32 and g.texture.dtype == np.uint8 and g.texture.shape == (32, 32, 3)
    with pytest.raises(NotImplementedError):
        load_ply(p)                                            # the default is unchanged
    geo = load_ply(p, geometry_only=True)
    assert geo.uv is None and np.array_equal(geo.vertices, m.vertices)


@pytest.mark.parametrize("binary", [True, False])
def test_per_corner_uv_is_unmerged_with_smooth_normals(tmp_path, binary):
    m = _textured()
    p = str(tmp_path / "obj_000002.ply")
    save_ply(p, m, binary=binary, per_corner_uv=True)
    assert b"texcoord" in open(p, "rb").read(600)
    g = load_ply(p, textured=True)
    F = len(m.faces)
    idx = m.faces.reshape(-1)
    assert len(g.vertices) == 3 * F and np.array_equal(g.faces, np.arange(3 * F, dtype=np.int32).reshape(F, 3))
    assert np.array_equal(g.vertices, m.vertices[idx]) and np.array_equal(g.colors, m.colors[idx])
    assert np.array_equal(g.normals, m.normals[idx])          # the PLY's (merged) normals, copied
    assert np.array_equal(g.uv, m.uv[idx])
    # without normals in the file: the merged mesh's area-weighted normals, not per-face ones
    p2 = str(tmp_path / "obj_000003.ply")
    save_ply(p2, m, binary=binary, with_normals=False, per_corner_uv=True)
    g2 = load_ply(p2, textured=True)
    assert np.array_equal(g2.normals, renderer.vertex_normals(m.vertices, m.faces)[idx])
    # an unmerged mesh round-trips unchanged
    u = _textured(merged=False)
    save_ply(p, u, binary=binary, per_corner_uv=True)
    g3 = load_ply(p, textured=True)
    for k in ("vertices", "faces", "colors", "normals", "uv", "texture"):
        assert np.array_equal(getattr(g3, k), getattr(u, k)), k


def test_s_t_aliases_and_quad_fanning(tmp_path):
    from PIL import Image
    Image.fromarray(np.zeros((2, 3, 3), np.uint8)).save(tmp_path / "t.png")
    head = ("ply\nformat ascii 1.0\ncomment TextureFile t.png\nelement vertex 4\nproperty float x\nproperty float y\n"
            "property float z\nproperty float s\nproperty float t\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n")
    (tmp_path / "a.ply").write_text(head + "0 0 0 0 0\n1 0 0 1 0\n1 1 0 1 1\n0 1 0 0 1\n4 0 1 2 3\n")
    g = load_ply(str(tmp_path / "a.ply"), textured=True)
    assert g.faces.tolist() == [[0, 1, 2], [0, 2, 3]] and g.uv.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]]
    head = head.replace("property float s\nproperty float t\n", "").replace("vertex_indices\n", "vertex_indices\nproperty list uchar float texcoord\n")
    (tmp_path / "b.ply").write_text(head + "0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3 8 0.1 0.2 0.3 0.4 0.5 0.6 0.7 0.8\n")
    g = load_ply(str(tmp_path / "b.ply"), textured=True)
    assert len(g.vertices) == 6 and g.faces.tolist() == [[0, 1, 2], [3, 4, 5]]
    np.testing.assert_array_equal(g.uv, np.array([[0.1, 0.2], [0.3, 0.4], [0.5, 0.6], [0.1, 0.2], [0.5, 0.6], [0.7, 0.8]], np.float32))
    np.testing.assert_array_equal(g.vertices[3:], np.array([[0, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32))


def test_incomplete_metadata_raises(tmp_path):
    m = _textured()
    p = str(tmp_path / "obj_000001.ply")
    save_ply(p, m, binary=False)
    text = open(p).read()
    cases = {
        "tex_no_uv": (text.replace("property float texture_u\nproperty float texture_v\n", "").replace("\n", "\n", 1), ValueError),
        "uv_no_tex": (text.replace("comment TextureFile obj_000001.png\n", ""), ValueError),
        "missing": (text.replace("TextureFile obj_000001.png", "TextureFile nowhere.png"), FileNotFoundError),
    }
    # drop the two uv columns of every vertex line for the no-uv case
    head, body = cases["tex_no_uv"][0].split("end_header\n")
    lines = body.splitlines()
    V = len(m.vertices)
    lines = [" ".join(l.split()[:6] + l.split()[8:]) for l in lines[:V]] + lines[V:]
    cases["tex_no_uv"] = (head + "end_header\n" + "\n".join(lines) + "\n", ValueError)
    for name, (t, exc) in cases.items():
        q = tmp_path / f"{name}.ply"
        q.write_text(t)
        with pytest.raises(exc):
            load_ply(str(q), textured=True)
    for bad in (np.nan, np.inf, 2.0 ** 15 + 1.0):
        uv = m.uv.copy()
        uv[5, 1] = bad
        save_ply(p, Mesh(m.vertices, m.faces, m.colors, m.normals, uv, m.texture), binary=True)
        with pytest.raises(ValueError):
            load_ply(p, textured=True)
    uv = m.uv.copy()
    uv[5, 1] = 2.0 ** 15                                      # the bound itself is allowed
    save_ply(p, Mesh(m.vertices, m.faces, m.colors, m.normals, uv, m.texture), binary=True)
    assert load_ply(p, textured=True).uv[5, 1] == 2.0 ** 15


def test_untextured_file_is_identical_under_textured(tmp_path):
    m = synthetic.make_blob_mesh(6, 7, radius=20.0, seed=2)
    for binary in (True, False):
        p = str(tmp_path / f"plain_{binary}.ply")
        save_ply(p, m, binary=binary)
        a, b = load_ply(p), load_ply(p, textured=True)
        assert b.uv is None and b.texture is None
        for k in ("vertices", "faces", "colors", "normals"):
            x, y = getattr(a, k), getattr(b, k)
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def test_alpha_is_dropped_and_texture_wins_over_colours(tmp_path):
    from PIL import Image
    m = _textured()
    p = str(tmp_path / "obj_000001.ply")
    save_ply(p, m)
    rgba = np.concatenate([m.texture, np.full(m.texture.shape[:2] + (1,), 7, np.uint8)], 2)
    Image.fromarray(rgba, "RGBA").save(tmp_path / "obj_000001.png")
    g = load_ply(p, textured=True)
    assert np.array_equal(g.texture, m.texture) and np.array_equal(g.colors, m.colors)


def test_eval_model_loads_a_textured_model_directory(tmp_path):
    m = _textured(merged=False)
    save_ply(str(tmp_path / "obj_000004.ply"), m)
    with open(tmp_path / "models_info.json", "w") as f:
        json.dump({"4": {"diameter": 80.0}}, f)
    em = eval_util.load_eval_model(str(tmp_path), 4)
    assert em.pts.shape == (len(m.vertices), 3) and em.diameter == 80.0


def test_material_defaults_and_checks():
    mat = TextureMaterial()
    a = mat.as_array()
    assert a.dtype == np.float32 and a[0] == 1.0 and abs(a[1] - 0.9036) < 1e-4 and a[2:5].tolist() == [1, 1, 1] and a[5] == 1
    assert TextureMaterial(0.2, 0.8, (1, 1, 1), False).as_array().tolist() == [np.float32(0.2), np.float32(0.8), 1, 1, 1, 0]
    for bad in (TextureMaterial(metallic=float("nan")), TextureMaterial(roughness=1.5), TextureMaterial(base_factor=(1, -0.1, 1))):
        with pytest.raises(ValueError):
            bad.as_array()


def test_pyramid_layout_and_hand_computed_levels():
    levels, total = _lib.texture_levels(5, 3)
    assert levels == [(0, 5, 3), (15, 2, 1), (17, 1, 1)] and total == 18
    levels, total = _lib.texture_levels(16384, 16384)
    assert len(levels) == 15 and levels[-1][1:] == (1, 1)
    assert _lib.texture_levels(1, 7)[0] == [(0, 1, 7), (7, 1, 3), (10, 1, 1)]
    # odd 3 x 3: level 1 is 1 x 1 from the top-left 2 x 2 block (min(2x+1, w-1) = 1)
    img = np.arange(27, dtype=np.uint8).reshape(3, 3, 3) * 9
    lv = texture_ref.mip_levels(img)
    assert [x.shape for x in lv] == [(3, 3, 3), (1, 1, 3)]
    b = img.astype(int)
    assert lv[1][0, 0].tolist() == [(b[0, 0, c] + b[0, 1, c] + b[1, 0, c] + b[1, 1, c] + 2) >> 2 for c in range(3)]
    # even 4 x 2 -> 2 x 1 -> 1 x 1
    img = np.array([[[0, 0, 0], [1, 2, 3], [10, 10, 10], [255, 255, 255]],
                    [[1, 1, 1], [2, 2, 2], [20, 20, 20], [254, 254, 254]]], np.uint8)
    lv = texture_ref.mip_levels(img)
    assert [x.shape[:2] for x in lv] == [(2, 4), (1, 2), (1, 1)]
    assert lv[1][0, 0].tolist() == [1, 1, 2] and lv[1][0, 1].tolist() == [135, 135, 135]   # (0+1+1+2+2)>>2, (10+255+20+254+2)>>2
    assert lv[2][0, 0].tolist() == [(1 + 135 + 1 + 135 + 2) >> 2, (1 + 135 + 1 + 135 + 2) >> 2, (2 + 135 + 2 + 135 + 2) >> 2]
    # 1 x N: the clamped index repeats the single column
    img = np.arange(15, dtype=np.uint8).reshape(5, 1, 3)
    lv = texture_ref.mip_levels(img)
    assert [x.shape[:2] for x in lv] == [(5, 1), (2, 1), (1, 1)]
    assert lv[1][:, 0, 0].tolist() == [(0 + 0 + 3 + 3 + 2) >> 2, (6 + 6 + 9 + 9 + 2) >> 2]
    packed = texture_ref.pack(lv)
    assert packed.dtype == np.uint32 and len(packed) == _lib.texture_levels(1, 5)[1] and np.all(packed >> 24 == 255)


def test_bilinear_at_texel_centres_and_repeat_wrap():
    rng = np.random.default_rng(4)
    lv = rng.integers(0, 256, (4, 8, 3), dtype=np.uint8)     # power-of-two sides: the centres are exact in fp32
    ys, xs = np.mgrid[0:4, 0:8]
    u = ((xs.astype(np.float32) + np.float32(0.5)) / np.float32(8)).reshape(-1)
    v = (np.float32(1) - (ys.astype(np.float32) + np.float32(0.5)) / np.float32(4)).reshape(-1)
    got = texture_ref.bilinear(lv, u, v)
    assert np.array_equal(got, lv.reshape(-1, 3).astype(np.float32) / np.float32(255))   # exact at the centres
    for du, dv in ((1.0, 0.0), (-2.0, 3.0), (7.0, -1.0)):
        assert np.array_equal(texture_ref.bilinear(lv, u + np.float32(du), v + np.float32(dv)), got)
    # half-way between the last and the first column wraps: the mean of the two
    mid = texture_ref.bilinear(lv, np.array([0.0], np.float32), np.array([1 - 0.5 / 4], np.float32))[0]
    np.testing.assert_allclose(mid, (lv[0, 0].astype(np.float32) + lv[0, 7]) / 510, atol=1e-6)


def _quad(tex_side, size_mm=64.0, z=500.0):
    v = np.array([[-size_mm / 2, -size_mm / 2, z], [size_mm / 2, -size_mm / 2, z], [size_mm / 2, size_mm / 2, z],
                  [-size_mm / 2, size_mm / 2, z]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    uv = np.array([[0, 1], [1, 1], [1, 0], [0, 0]], np.float32)   # image row 0 (v = 1) at the top (small y)
    tex = synthetic.make_texture(tex_side, 0)
    return Mesh(v, f, np.full((4, 3), 0.5, np.float32), renderer.vertex_normals(v, f), uv, tex)


@pytest.mark.parametrize("tex_side, expect", [(64, 0.0), (128, 1.0), (256, 2.0)])
def test_lod_of_one_to_one_and_minified_mappings(tex_side, expect):
    mesh = _quad(tex_side)
    cam = camera_params([PinholePlaneCameraModel(80, 80, (500.0, 500.0), (40.0, 40.0))])[0]   # 1 mm per pixel at z = 500
    ref = texture_ref.render_textured(mesh, cam, 80, 80, TextureMaterial().as_array())
    lam = ref["lod"][ref["tri_id"] >= 0]
    assert len(lam) == 64 * 64
    assert np.all(np.abs(lam - expect) < 1e-4), (lam.min(), lam.max())


def test_restatement_matches_vertex_colour_path_for_a_constant_texture():
    """A 1 x 1 texture of k with material (0.2, 0.8, 1, no decode) is the vertex-coloured shading of colour k / 255
    (within one step: alpha = 0.8^2 in fp32 and the blend of equal texels round differently from the constants)."""
    m = synthetic.make_blob_mesh(12, 14, radius=50.0, seed=5)
    cam = camera_params([PinholePlaneCameraModel(64, 64, (110.0, 110.0), (32.0, 32.0),
                                                 np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 400.0], [0, 0, 0, 1]]))])[0]
    k = np.array([200, 90, 30], np.uint8)
    col = np.tile(k.astype(np.float32) / np.float32(255), (len(m.vertices), 1))
    plain = render_ref.render(Mesh(m.vertices, m.faces, col, m.normals), cam, 64, 64)
    tm = Mesh(m.vertices, m.faces, m.colors, m.normals, np.zeros((len(m.vertices), 2), np.float32), k.reshape(1, 1, 3))
    tex = texture_ref.render_textured(tm, cam, 64, 64, TextureMaterial(0.2, 0.8, (1, 1, 1), False).as_array())
    assert plain["mask"].sum() > 0 and np.array_equal(plain["tri_id"], tex["tri_id"])
    assert np.abs(plain["color"].astype(int) - tex["color"].astype(int)).max() <= 1
