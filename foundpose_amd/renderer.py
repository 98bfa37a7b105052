"""Mesh renderer on the MI355X: the part of utils/renderer.py (PyrenderRasterizer) that scripts/gen_templates.py uses,
as the HIP rasterizer of csrc/render.hip.  No OpenGL: coverage, depth and mask follow an exact integer contract
 and the shading restates pyrender's metallic-roughness shader with the reference's light rig
(unpinned: pyrender is absent here).

  load_ply(path) -> Mesh                   BOP PLY models (ascii / binary_little_endian, vertex colours, optional normals;
                                           textured models with textured=True: uv + texture image)
  HipRasterizer.add_object_model(...)      one mesh per object id, uploaded once (a textured one with its mip pyramid)
  HipRasterizer.render_object_model(...)   the reference's single-view call: COLOR HxWx3 [0,1], DEPTH mm, MASK bool
  HipRasterizer.render_views(...)          B views of one object in one launch chain (what gen_templates uses)
"""

import enum
import os
import struct
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import TEXTURE_MAX_SIDE, call, ptr, stream, upload_async, vp
from .crop_util import PinholePlaneCameraModel

NEAR_PLANE_MM = 100.0                    # pyrender IntrinsicsCamera znear = 0.1 m (utils/renderer.py)
FALLBACK_COLOR = (102, 102, 102)         # trimesh's default colour for a mesh without colours
TILE, VERT_BYTES, TRI_BYTES = 32, 40, 144  # FP_RENDER_TILE / _VERT_BYTES / _TRI_BYTES of include/foundpose_amd.h
MAX_LIST_ENTRIES = 1 << 31
MAX_ABS_UV = 2.0 ** 15                   # |uv| bound of a textured model: u * texture side (<= 2^29) stays in the kernel's int range


class RenderType(enum.Enum):
    """utils/renderer_base.py:32."""
    COLOR = "rgb"
    DEPTH = "depth"
    NORMAL = "normal"
    MASK = "mask"


@dataclass
class Mesh:
    vertices: np.ndarray   # float32 [V, 3], mm
    faces: np.ndarray      # int32 [F, 3]
    colors: np.ndarray     # float32 [V, 3] in [0, 1] (k / 255)
    normals: np.ndarray    # float32 [V, 3]
    uv: Optional[np.ndarray] = None        # float32 [V, 2] of a textured model (v = 1 is row 0 of the texture)
    texture: Optional[np.ndarray] = None   # uint8 [H, W, 3] of a textured model; it wins over the colours when rendering


@dataclass(frozen=True)
class TextureMaterial:
    """The material of a textured model (unpinned): what we believe pyrender 0.1.45's Mesh.from_trimesh
    makes of trimesh's SimpleMaterial for a textured PLY -- a MetallicRoughnessMaterial with the glTF default metallic
    factor 1, roughness (2 / (Ns + 2))^(1/4) at Ns = 1, base colour factor 1 -- with the sampled base colour sRGB-decoded."""
    metallic: float = 1.0
    roughness: float = (2.0 / 3.0) ** 0.25
    base_factor: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    srgb_decode: bool = True

    def as_array(self) -> np.ndarray:
        """float32 [6]: metallic, roughness, base factor rgb, sRGB decode flag (fp_render_raster_textured's material)."""
        m = np.array([self.metallic, self.roughness, *self.base_factor, 1.0 if self.srgb_decode else 0.0], np.float32)
        if m.shape != (6,) or not np.all((m >= 0) & (m <= 1)):
            raise ValueError(f"material entries must lie in [0, 1]: {m}")
        return m


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def vertex_normals(vertices: np.ndarray, faces: np.ndarray) -> np.ndarray:
    """Area-weighted average of the incident face normals (trimesh's default vertex normals), unit length."""
    v = vertices.astype(np.float64)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])   # length = 2 x area
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, faces[:, k], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0).astype(np.float32)


def load_ply(path: str, geometry_only: bool = False, textured: bool = False) -> Mesh:
    """BOP model PLY: ascii or binary_little_endian; x, y, z float / double; optional nx, ny, nz; red, green, blue[, alpha]
    uchar; faces as `vertex_indices` lists, fanned into triangles.  Textured models raise NotImplementedError, unless
    `geometry_only` (depth-only uses such as VSD): then the texture is ignored and the colours are the fallback grey, or
    `textured`: then Mesh.uv / Mesh.texture hold the model's texture (an untextured file loads exactly as without the flag).
    UVs are per-vertex `texture_u` / `texture_v` (or `s` / `t`) or a per-corner face list `texcoord`; per-corner UVs are
    unmerged, every triangle corner its own vertex (position, colour and the merged mesh's normal copied; face order kept).
    The image is `comment TextureFile <name>` beside the PLY, decoded as RGB (alpha dropped).  Under `textured`, a texture
    without UVs, UVs without a texture, non-finite UVs or |uv| > 2^15 raise ValueError, a missing image FileNotFoundError."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    body = data[data.index(b"\n", end) + 1:]
    header = data[:end].decode("ascii", "replace").splitlines()
    fmt, elements, tex_name = None, [], None
    for line in header:
        tok = line.split()
        if not tok:
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "comment" and len(tok) > 1 and tok[1].lower() == "texturefile":
            if not geometry_only and not textured:
                raise NotImplementedError("textured PLY models are not supported (vertex colours only); load with textured=True")
            tex_name = line.split(None, 2)[2].strip() if len(tok) > 2 else ""
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if tok[1] == "list":
                elements[-1][2].append((tok[4], ("list", _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]])))
            else:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise NotImplementedError(f"PLY format {fmt}")
    for name, _, props in elements:
        names = {p[0] for p in props}
        if names & {"texture_u", "texture_v", "texcoord"} and not geometry_only and not textured:
            raise NotImplementedError("textured PLY models are not supported (vertex colours only); load with textured=True")
    vert, faces, corner_uv = None, None, None
    pos = 0
    tokens = body.split() if fmt == "ascii" else None
    for name, count, props in elements:
        has_list = any(isinstance(p[1], tuple) for p in props)
        if not has_list:
            dt = np.dtype([(p[0], "<" + p[1]) for p in props])
            if fmt == "ascii":
                n = len(props) * count
                flat = np.array(tokens[pos:pos + n], dtype=np.float64).reshape(count, len(props))
                pos += n
                arr = np.zeros(count, dt)
                for i, p in enumerate(props):
                    arr[p[0]] = flat[:, i]
            else:
                arr = np.frombuffer(body, dt, count, pos)
                pos += dt.itemsize * count
            if name == "vertex":
                vert = arr
            continue
        rows = []
        for _ in range(count):
            row = {}
            for pname, ptype in props:
                if isinstance(ptype, tuple):
                    is_float = np.dtype(ptype[2]).kind == "f"   # texcoord: floats; index lists: integers
                    if fmt == "ascii":
                        k = int(tokens[pos])
                        row[pname] = [float(t) if is_float else int(float(t)) for t in tokens[pos + 1:pos + 1 + k]]; pos += 1 + k
                    else:
                        cdt, idt = np.dtype("<" + ptype[1]), np.dtype("<" + ptype[2])
                        k = int(np.frombuffer(body, cdt, 1, pos)[0]); pos += cdt.itemsize
                        vals = np.frombuffer(body, idt, k, pos)
                        row[pname] = (vals.astype(np.float64) if is_float else vals.astype(np.int64)).tolist(); pos += idt.itemsize * k
                else:
                    if fmt == "ascii":
                        pos += 1
                    else:
                        pos += np.dtype(ptype).itemsize
            rows.append(row)
        if name == "face":
            key = "vertex_indices" if rows and "vertex_indices" in rows[0] else "vertex_index"
            tris = [(p[0], p[i], p[i + 1]) for r in rows for p in [r[key]] for i in range(1, len(p) - 1)]
            faces = np.array(tris, dtype=np.int64).reshape(-1, 3)
            if textured and not geometry_only and rows and "texcoord" in rows[0]:   # fanned like the indices
                if any(len(r["texcoord"]) != 2 * len(r[key]) for r in rows):
                    raise ValueError(f"{path}: a face's texcoord list does not hold two values per corner")
                corner_uv = np.array([(tc[0], tc[1], tc[2 * i], tc[2 * i + 1], tc[2 * i + 2], tc[2 * i + 3])
                                      for r in rows for p, tc in [(r[key], r["texcoord"])] for i in range(1, len(p) - 1)],
                                     np.float64).reshape(-1, 3, 2)
    if vert is None or faces is None:
        raise ValueError(f"{path}: no vertex or face element")
    v = np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float32)
    if faces.size and (faces.min() < 0 or faces.max() >= len(v)):
        raise ValueError(f"{path}: face index outside the vertex range")
    names = vert.dtype.names
    if {"red", "green", "blue"} <= set(names):
        col = np.stack([vert["red"], vert["green"], vert["blue"]], 1).astype(np.float32) / np.float32(255.0)
    else:
        col = np.tile(np.array(FALLBACK_COLOR, np.float32) / np.float32(255.0), (len(v), 1))
    if {"nx", "ny", "nz"} <= set(names):
        nrm = np.stack([vert["nx"], vert["ny"], vert["nz"]], 1).astype(np.float32)
    else:
        nrm = vertex_normals(v, faces)
    mesh = Mesh(vertices=v, faces=faces.astype(np.int32), colors=col.astype(np.float32), normals=nrm)
    if not textured or geometry_only:
        return mesh
    return _attach_texture(path, mesh, vert, tex_name, corner_uv)


def _attach_texture(path: str, mesh: Mesh, vert: np.ndarray, tex_name: Optional[str], corner_uv: Optional[np.ndarray]) -> Mesh:
    """load_ply(textured=True) after the geometry: UVs + image, checked; per-corner UVs unmerged."""
    names = set(vert.dtype.names)
    uv = None
    for un, vn in (("texture_u", "texture_v"), ("s", "t")):
        if {un, vn} <= names:
            uv = np.stack([vert[un], vert[vn]], 1).astype(np.float64)
            break
    if uv is None and corner_uv is not None:
        uv = corner_uv
    if tex_name is None and uv is None:
        return mesh                                        # untextured: exactly the plain load
    if tex_name is None:
        raise ValueError(f"{path}: UVs but no `comment TextureFile <image>`")
    if uv is None:
        raise ValueError(f"{path}: a TextureFile comment but no UVs (texture_u / texture_v, s / t or texcoord)")
    if not tex_name:
        raise ValueError(f"{path}: the TextureFile comment names no file")
    if not np.all(np.isfinite(uv)):
        raise ValueError(f"{path}: non-finite UVs")
    if np.abs(uv).max(initial=0.0) > MAX_ABS_UV:
        raise ValueError(f"{path}: UVs beyond +-2^15")
    img_path = os.path.join(os.path.dirname(os.path.abspath(path)), tex_name)
    if not os.path.isfile(img_path):
        raise FileNotFoundError(f"{path}: texture {img_path} not found")
    from PIL import Image
    with Image.open(img_path) as im:
        tex = np.array(im.convert("RGB"), np.uint8, order="C")
    if tex.ndim != 3 or not (1 <= tex.shape[0] <= TEXTURE_MAX_SIDE and 1 <= tex.shape[1] <= TEXTURE_MAX_SIDE):
        raise ValueError(f"{path}: texture of shape {tex.shape}; sides must lie in [1, {TEXTURE_MAX_SIDE}]")
    if uv.ndim == 3:                                       # per corner: every triangle corner becomes its own vertex
        idx = mesh.faces.reshape(-1)
        F = len(mesh.faces)
        return Mesh(mesh.vertices[idx], np.arange(3 * F, dtype=np.int32).reshape(F, 3), mesh.colors[idx], mesh.normals[idx],
                    uv.reshape(-1, 2).astype(np.float32), tex)
    return Mesh(mesh.vertices, mesh.faces, mesh.colors, mesh.normals, uv.astype(np.float32), tex)


def save_ply(path: str, mesh: Mesh, binary: bool = True, with_normals: bool = True, per_corner_uv: bool = False) -> None:
    """Writes a vertex-coloured triangle mesh in the layout load_ply reads (BOP models are written this way).  A textured
    mesh (uv and texture set) also gets `comment TextureFile <ply name>.png`, the image beside the PLY, and its UVs as
    per-vertex texture_u / texture_v (BOP's layout) or, with per_corner_uv, as a per-face `texcoord` list."""
    V, F = len(mesh.vertices), len(mesh.faces)
    tex = mesh.uv is not None and mesh.texture is not None
    vuv = tex and not per_corner_uv
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + (["texture_u", "texture_v"] if vuv else [])
    head = ["ply", f"format {'binary_little_endian' if binary else 'ascii'} 1.0"]
    if tex:
        png = os.path.splitext(os.path.basename(path))[0] + ".png"
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(mesh.texture, np.uint8)).save(os.path.join(os.path.dirname(os.path.abspath(path)), png))
        head.append(f"comment TextureFile {png}")
    head.append(f"element vertex {V}")
    head += [f"property float {p}" for p in props] + ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {F}", "property list uchar int vertex_indices"]
    head += ["property list uchar float texcoord"] if tex and per_corner_uv else []
    head.append("end_header")
    rgb = np.rint(np.asarray(mesh.colors, np.float64) * 255.0).astype(np.uint8)
    cols = [mesh.vertices] + ([mesh.normals] if with_normals else []) + ([mesh.uv] if vuv else [])
    corner = np.asarray(mesh.uv, np.float32)[mesh.faces].reshape(F, 6) if tex and per_corner_uv else None
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        if binary:
            dt = np.dtype([(p, "<f4") for p in props] + [("red", "u1"), ("green", "u1"), ("blue", "u1")])
            arr = np.zeros(V, dt)
            flat = np.concatenate(cols, 1)
            for i, p in enumerate(props):
                arr[p] = flat[:, i]
            arr["red"], arr["green"], arr["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
            f.write(arr.tobytes())
            fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))] + ([("m", "u1"), ("uv", "<f4", (6,))] if corner is not None else []))
            fa = np.zeros(F, fdt)
            fa["n"], fa["i"] = 3, mesh.faces
            if corner is not None:
                fa["m"], fa["uv"] = 6, corner
            f.write(fa.tobytes())
        else:
            flat = np.concatenate(cols, 1)
            for i in range(V):
                f.write((" ".join(repr(float(x)) for x in flat[i]) + " " + " ".join(str(int(c)) for c in rgb[i]) + "\n").encode())
            for i, tri in enumerate(mesh.faces):
                tc = "" if corner is None else " 6 " + " ".join(repr(float(x)) for x in corner[i])
                f.write(("3 " + " ".join(str(int(x)) for x in tri) + tc + "\n").encode())


def camera_params(cameras: Sequence[PinholePlaneCameraModel]) -> np.ndarray:
    """[B, 16] doubles per view: f, c, R (row-major rotation of T_world_from_eye), t."""
    out = np.empty((len(cameras), 16), np.float64)
    for i, cam in enumerate(cameras):
        T = cam.T_world_from_eye
        out[i, :4] = [cam.f[0], cam.f[1], cam.c[0], cam.c[1]]
        out[i, 4:13] = T[:3, :3].reshape(-1)
        out[i, 13:] = T[:3, 3]
    return out


class _DeviceMesh:
    def __init__(self, mesh: Mesh, device, material: Optional[TextureMaterial] = None):
        self.mesh = mesh
        self.verts = torch.from_numpy(np.ascontiguousarray(mesh.vertices, np.float32)).to(device)
        self.normals = torch.from_numpy(np.ascontiguousarray(mesh.normals, np.float32)).to(device)
        self.colors = torch.from_numpy(np.ascontiguousarray(mesh.colors, np.float32)).to(device)
        self.faces = torch.from_numpy(np.ascontiguousarray(mesh.faces, np.int32)).to(device)
        self.textured = mesh.uv is not None and mesh.texture is not None
        if self.textured:   # uploaded once per object: the UVs, the mip pyramid, the material
            from .ops import texture_mips
            uv = np.ascontiguousarray(mesh.uv, np.float32)
            if uv.shape != (len(mesh.vertices), 2) or not np.all(np.isfinite(uv)) or np.abs(uv).max(initial=0.0) > MAX_ABS_UV:
                raise ValueError("uv must be finite float32 [V, 2] within +-2^15")
            self.uv = torch.from_numpy(uv).to(device)
            tex = torch.from_numpy(np.array(mesh.texture, np.uint8, order="C")).to(device)   # a writable copy
            self.tex_h, self.tex_w = int(tex.shape[0]), int(tex.shape[1])
            self.pyramid = texture_mips(tex)
            self.material = (material or TextureMaterial()).as_array()


class HipRasterizer:
    """PyrenderRasterizer's interface (utils/renderer.py) over csrc/render.hip.  Black background, no back-face culling,
    the reference's spot light at the camera and ambient 0.02 (fixed in the kernel)."""

    def __init__(self, device: str = "cuda"):
        self.device = torch.device(device)
        self.objects: Dict[int, _DeviceMesh] = {}

    def add_object_model(self, obj_id: int, model_path: Optional[str] = None, mesh_color=None, mesh: Optional[Mesh] = None,
                         debug: bool = False, material: Optional[TextureMaterial] = None) -> None:
        """A PLY (loaded with textured=True: vertex-coloured files load as before) or a Mesh.  A textured model is shaded
        from its texture with `material` (default TextureMaterial()); mesh_color replaces the visual by one colour, so the
        model then renders as a vertex-coloured one."""
        m = mesh if mesh is not None else load_ply(model_path, textured=True)
        if mesh_color is not None:  # one colour for the whole mesh (renderer.py:72-76)
            c = np.asarray(mesh_color, np.float32)[:3]
            m = Mesh(m.vertices, m.faces, np.tile(c / (np.float32(255.0) if c.max() > 1 else np.float32(1.0)), (len(m.vertices), 1)).astype(np.float32), m.normals)
        if len(m.faces) == 0:
            raise ValueError("mesh has no faces")
        self.objects[obj_id] = _DeviceMesh(m, self.device, material)

    def render_views(self, obj_id: int, cameras: Sequence[PinholePlaneCameraModel], with_tri_id: bool = False,
                     with_color: bool = True) -> Dict[str, torch.Tensor]:
        """All cameras (one viewport size) in one launch chain -> device tensors: color fp32 [B,H,W,3] (k/255), depth fp32
        [B,H,W] mm, mask u8 [B,H,W] (255 / 0), boxes int32 [B,4] (min x, min y, max x, max y; INT_MAX/INT_MIN if empty),
        tri_id int32 [B,H,W] (-1 background) when asked.  Raises ValueError when a vertex is within the near plane."""
        dm = self.objects[obj_id]
        B = len(cameras)
        W, H = cameras[0].width, cameras[0].height
        if any((c.width, c.height) != (W, H) for c in cameras):
            raise ValueError("all cameras of a batch must share one viewport size")
        dev = self.device
        V, F = len(dm.mesh.vertices), len(dm.mesh.faces)
        tiles = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
        cams = upload_async(torch.from_numpy(camera_params(cameras)), dev)
        vert_ws = torch.empty(B * V * VERT_BYTES, dtype=torch.uint8, device=dev)
        tri_ws = torch.empty(B * F * TRI_BYTES, dtype=torch.uint8, device=dev)
        counts = torch.empty(B * tiles, dtype=torch.int32, device=dev)
        offsets = torch.empty(B * tiles + 1, dtype=torch.int64, device=dev)
        status = torch.empty(4, dtype=torch.int64, device=dev)
        color = torch.empty(B, H, W, 3, dtype=torch.float32, device=dev) if with_color else None
        depth = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        mask = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        tri = torch.empty(B, H, W, dtype=torch.int32, device=dev) if with_tri_id else None
        boxes = torch.empty(B, 4, dtype=torch.int32, device=dev)
        args = [ptr(dm.verts), ptr(dm.normals), ptr(dm.colors), V, ptr(dm.faces), F, ptr(cams), B, W, H, ptr(vert_ws), ptr(tri_ws),
                ptr(counts), ptr(offsets)]
        tail = [ptr(status), ptr(color), ptr(depth), ptr(mask), ptr(tri), ptr(boxes), stream()]
        call("fp_render_setup", *args, ptr(None), *tail)
        st = status.cpu().numpy()   # the one host synchronisation before the raster: near plane, range, list size
        min_z = struct.unpack("<d", struct.pack("<q", int(st[3])))[0]
        if not min_z > NEAR_PLANE_MM:
            raise ValueError(f"a mesh vertex is {min_z:.3f} mm in front of a camera, within the near plane ({NEAR_PLANE_MM} mm); "
                             "near-plane clipping is not implemented")
        if st[1] & 2:
            raise ValueError("face index outside the vertex range")
        if st[1] & 1:
            raise ValueError("a vertex projects beyond the rasterizer's fixed-point range (+-2^21 pixels)")
        total = int(st[2])
        if total >= MAX_LIST_ENTRIES:
            raise ValueError(f"{total} tile-list entries exceed the rasterizer workspace ({MAX_LIST_ENTRIES}); render fewer views per batch")
        lists = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        if dm.textured and color is not None:   # without a colour output the two kernels write the same bits
            call("fp_render_raster_textured", *args, ptr(lists), *tail[:-1], ptr(dm.uv), ptr(dm.pyramid), dm.tex_w, dm.tex_h,
                 dm.material.ctypes.data_as(vp), stream())
        else:
            call("fp_render_raster", *args, ptr(lists), *tail)
        out = {"depth": depth, "mask": mask, "boxes": boxes}
        if color is not None:
            out["color"] = color
        if tri is not None:
            out["tri_id"] = tri
        return out

    def render_object_model(self, obj_id: int, camera_model_c2w: PinholePlaneCameraModel, render_types: Sequence[RenderType],
                            return_tensors: bool = False, debug: bool = False) -> Dict[RenderType, object]:
        """utils/renderer.py's single-view call: COLOR HxWx3 float32 in [0,1] (k/255), DEPTH mm (0 background), MASK bool."""
        if RenderType.NORMAL in render_types:
            raise NotImplementedError("the NORMAL output is not implemented")
        r = self.render_views(obj_id, [camera_model_c2w], with_color=RenderType.COLOR in render_types)
        out: Dict[RenderType, object] = {}
        if RenderType.COLOR in render_types:
            out[RenderType.COLOR] = r["color"][0]
        if RenderType.DEPTH in render_types:
            out[RenderType.DEPTH] = r["depth"][0]
        if RenderType.MASK in render_types:
            out[RenderType.MASK] = r["mask"][0] > 0
        if not return_tensors:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        return out
