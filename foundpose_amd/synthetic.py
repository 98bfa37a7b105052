"""Seeded synthetic inputs (no network here: no checkpoints, no BOP data).

Shapes follow SURVEY.md section 8(d): random-init ViT weights in the upstream
DINOv2 state_dict key layout, [0,1] crops, disc masks, and a planted-positive
template bank laid out like the reference's `repre.pth`
(/root/reference/utils/repre_util.py:34-83, gen_repre.py:187-214).

Everything here is host-side torch-CPU data generation; nothing computes the
hot path.
"""

import math
from typing import Dict, Optional, Tuple

import torch

from .vit_config import VitArch


def make_vit_state_dict(arch: VitArch, seed: int = 1234, ls_gamma: float = 1.0) -> Dict[str, torch.Tensor]:
    """Random DINOv2 weights with the upstream key names (fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)

    def tn(*shape, std=0.02):
        t = torch.empty(*shape, dtype=torch.float32)
        torch.nn.init.trunc_normal_(t, std=std, a=-2 * std, b=2 * std, generator=g)
        return t

    D, R = arch.dim, arch.registers
    sd: Dict[str, torch.Tensor] = {}
    sd["cls_token"] = tn(1, 1, D)
    sd["pos_embed"] = tn(1, 1 + arch.pretrain_grid ** 2, D)
    if R:
        sd["register_tokens"] = tn(1, R, D)
    sd["mask_token"] = torch.zeros(1, D)
    sd["patch_embed.proj.weight"] = tn(D, 3, arch.patch, arch.patch)
    sd["patch_embed.proj.bias"] = tn(D)
    for i in range(arch.depth):
        p = f"blocks.{i}."
        # LayerNorm affine slightly off identity so that a missing gamma/beta shows up.
        sd[p + "norm1.weight"] = 1.0 + tn(D, std=0.05)
        sd[p + "norm1.bias"] = tn(D, std=0.05)
        sd[p + "attn.qkv.weight"] = tn(3 * D, D)
        sd[p + "attn.qkv.bias"] = tn(3 * D)
        sd[p + "attn.proj.weight"] = tn(D, D)
        sd[p + "attn.proj.bias"] = tn(D)
        sd[p + "ls1.gamma"] = ls_gamma * (1.0 + tn(D, std=0.05))
        sd[p + "norm2.weight"] = 1.0 + tn(D, std=0.05)
        sd[p + "norm2.bias"] = tn(D, std=0.05)
        if arch.ffn == "mlp":
            sd[p + "mlp.fc1.weight"] = tn(arch.hidden, D)
            sd[p + "mlp.fc1.bias"] = tn(arch.hidden)
            sd[p + "mlp.fc2.weight"] = tn(D, arch.hidden)
            sd[p + "mlp.fc2.bias"] = tn(D)
        else:
            sd[p + "mlp.w12.weight"] = tn(2 * arch.hidden, D)
            sd[p + "mlp.w12.bias"] = tn(2 * arch.hidden)
            sd[p + "mlp.w3.weight"] = tn(D, arch.hidden)
            sd[p + "mlp.w3.bias"] = tn(D)
        sd[p + "ls2.gamma"] = ls_gamma * (1.0 + tn(D, std=0.05))
    sd["norm.weight"] = 1.0 + tn(D, std=0.05)
    sd["norm.bias"] = tn(D, std=0.05)
    return sd


def make_crops(batch: int, size: int, seed: int = 0) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.rand(batch, 3, size, size, generator=g, dtype=torch.float32)


def make_dictionary_crops(batch: int, size: int, mask: torch.Tensor, dict_size: int = 682, patch: int = 14, seed: int = 0,
                          pixel_noise: float = 0.02, dict_seed: int = 4242) -> Tuple[torch.Tensor, torch.Tensor]:
    """Crops assembled from a dictionary of `dict_size` noise patch textures: the patches whose centre lies inside `mask`
    are DISTINCT textures (a random draw without replacement), the others random ones, plus a little pixel noise.
    Real object surfaces repeat local structure across views -- that repetition is what gives descriptors clusters for
    the visual words to sit on; iid noise crops have none (every patch is equidistant from every other, and the 3
    nearest of 2048 words are decided by rounding).
    -> (crops [B, 3, S, S] f32 in [0, 1], texture id of every patch [B, S/patch, S/patch] i64)."""
    g = torch.Generator().manual_seed(dict_seed)
    n = size // patch
    textures = torch.rand(dict_size, 3, patch, patch, generator=g, dtype=torch.float32)
    inside = mask[patch // 2::patch, patch // 2::patch][:n, :n].bool().reshape(-1)
    n_in = int(inside.sum())
    if n_in > dict_size:
        raise ValueError(f"{n_in} patches inside the mask need a dictionary of at least that many textures (got {dict_size})")
    g = torch.Generator().manual_seed(seed)
    crops = torch.full((batch, 3, size, size), 0.5, dtype=torch.float32)
    ids = torch.empty(batch, n * n, dtype=torch.int64)
    for b in range(batch):
        ids[b] = torch.randint(0, dict_size, (n * n,), generator=g)
        ids[b, inside] = torch.randperm(dict_size, generator=g)[:n_in]
        crops[b, :, : n * patch, : n * patch] = textures[ids[b]].reshape(n, n, 3, patch, patch).permute(2, 0, 3, 1, 4).reshape(3, n * patch, n * patch)
    crops += pixel_noise * torch.randn(crops.shape, generator=g)
    return crops.clamp_(0.0, 1.0), ids.reshape(batch, n, n)


def make_disc_mask(size: int, rel_radius: float = 0.35) -> torch.Tensor:
    """uint8 [S,S]: centred disc of radius rel_radius*S (Q ~ 0.385*Np grid points)."""
    ys, xs = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    c = (size - 1) / 2.0
    return (((xs - c) ** 2 + (ys - c) ** 2) <= (rel_radius * size) ** 2).to(torch.uint8)


def make_bank_features(
    num_templates: int,
    feat_dim: int = 256,
    min_patches: int = 300,
    max_patches: int = 450,
    seed: int = 7,
) -> Dict[str, torch.Tensor]:
    """Raw bank content: CSR-sorted features, vertices and the template id run per feature."""
    g = torch.Generator().manual_seed(seed)
    counts = torch.randint(min_patches, max_patches + 1, (num_templates,), generator=g)
    n_f = int(counts.sum())
    # PCA-like decaying spectrum, sigma_j ~ j^-0.5
    sigma = (torch.arange(1, feat_dim + 1, dtype=torch.float32)) ** -0.5
    feat_vectors = torch.randn(n_f, feat_dim, generator=g) * sigma
    vertices = torch.randn(n_f, 3, generator=g) * 50.0
    feat_to_template_ids = torch.repeat_interleave(
        torch.arange(num_templates, dtype=torch.int32), counts
    )
    return {
        "feat_vectors": feat_vectors.contiguous(),
        "vertices": vertices.contiguous(),
        "feat_to_template_ids": feat_to_template_ids,
        "feat_to_vertex_ids": torch.arange(n_f, dtype=torch.int32),
        "template_counts": counts,
    }


def pick_centroids(feat_vectors: torch.Tensor, num_words: int, seed: int = 11) -> torch.Tensor:
    """Visual words = random bank rows (stand-in for the offline k-means)."""
    g = torch.Generator().manual_seed(seed)
    n = feat_vectors.shape[0]
    if n >= num_words:
        ids = torch.randperm(n, generator=g)[:num_words]
        return feat_vectors[ids].clone().contiguous()
    extra = torch.randn(num_words - n, feat_vectors.shape[1], generator=g) * feat_vectors.std(0)
    return torch.cat([feat_vectors, extra], 0).contiguous()


def make_planted_query(
    bank: Dict[str, torch.Tensor],
    template_id: int,
    num_grid: int,
    seed: int,
    noise: float = 0.05,
    cell: float = 14.0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Query = noisy copy of one template's patch features at distinct grid cells.

    Returns (query_points [Q,2] f32 at cell centres, query_features [Q,d] f32).
    """
    g = torch.Generator().manual_seed(seed)
    ids = torch.nonzero(bank["feat_to_template_ids"] == template_id).flatten()
    q = min(len(ids), num_grid * num_grid)
    feats = bank["feat_vectors"][ids[:q]]
    feats = feats + noise * torch.randn(feats.shape, generator=g)
    cells = torch.randperm(num_grid * num_grid, generator=g)[:q].sort().values
    xs = (cells % num_grid).float() * cell + cell / 2
    ys = (cells // num_grid).float() * cell + cell / 2
    return torch.stack([xs, ys], 1).contiguous(), feats.contiguous()


def make_blob_mesh(num_lat: int = 50, num_lon: int = 50, radius: float = 60.0, seed: int = 0):
    """A closed, asymmetric, vertex-coloured triangle mesh (mm): a UV sphere with random low-frequency bumps, stretched
    along x, colours varying with position -> renderer.Mesh with about 2 * num_lat * num_lon triangles."""
    import numpy as np

    from .renderer import Mesh, vertex_normals
    rng = np.random.default_rng(seed)
    th = np.linspace(0, np.pi, num_lat + 1)[1:-1]                 # rings between the poles
    ph = np.linspace(0, 2 * np.pi, num_lon, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    d = np.concatenate([[[0.0, 0.0, 1.0]], d, [[0.0, 0.0, -1.0]]])
    bump = np.zeros(len(d))
    for _ in range(6):
        c = rng.normal(size=3)
        c /= np.linalg.norm(c)
        bump += rng.uniform(0.05, 0.2) * np.exp(-np.sum((d - c) ** 2, 1) / rng.uniform(0.1, 0.5))
    v = d * (radius * (1.0 + bump))[:, None] * np.array([1.4, 1.0, 0.8])
    v[:, 0] += 0.3 * radius * (d[:, 1] > 0.5)                      # a lopsided ridge: no rotational symmetry
    faces = []
    ring = lambda i, j: 1 + i * num_lon + (j % num_lon)            # noqa: E731
    for j in range(num_lon):
        faces.append((0, ring(0, j), ring(0, j + 1)))
        faces.append((len(d) - 1, ring(num_lat - 2, j + 1), ring(num_lat - 2, j)))
    for i in range(num_lat - 2):
        for j in range(num_lon):
            faces.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            faces.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    faces = np.array(faces, np.int32)
    u = (d + 1.0) / 2.0
    col = np.stack([u[:, 0], 0.5 + 0.5 * np.sin(6 * u[:, 1] + 3 * u[:, 2]), 1.0 - u[:, 2]], 1)
    col = np.rint(np.clip(col, 0, 1) * 255.0).astype(np.float32) / np.float32(255.0)
    v = v.astype(np.float32)
    return Mesh(vertices=v, faces=faces, colors=col.astype(np.float32), normals=vertex_normals(v, faces))


def make_texture(size: int = 256, seed: int = 0):
    """A procedural RGB texture, uint8 [size, size, 3]: colour ramps along both axes, a checker of size / 16 cells, an
    off-centre disc and an L-shaped bar (no symmetry), and bright stripes along the left and right borders (the seam)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size].astype(np.float64) / size
    cell = max(size // 16, 1)
    chk = ((np.arange(size)[:, None] // cell + np.arange(size)[None, :] // cell) % 2).astype(np.float64)
    img = np.stack([x, 0.3 + 0.5 * y, 0.25 + 0.5 * chk], -1)
    cx, cy = rng.uniform(0.55, 0.75, 2)
    img[(x - cx) ** 2 + (y - cy) ** 2 < 0.01] = (1.0, 0.9, 0.1)
    img[(x > 0.15) & (x < 0.2) & (y > 0.1) & (y < 0.45)] = (0.1, 0.1, 0.9)
    img[(x > 0.15) & (x < 0.35) & (y > 0.4) & (y < 0.45)] = (0.1, 0.1, 0.9)
    img[(x < 0.02) | (x > 0.98)] = (1.0, 0.2, 0.6)
    return np.rint(np.clip(img, 0, 1) * 255.0).astype(np.uint8)


def make_textured_blob_mesh(num_lat: int = 50, num_lon: int = 50, radius: float = 60.0, seed: int = 0, tex_size: int = 256):
    """make_blob_mesh's geometry with a spherical UV map and make_texture(tex_size): per-corner UVs, unmerged (every
    triangle corner its own vertex, the merged mesh's normals, face order kept).  u = azimuth / 2 pi, v = 1 - polar / pi;
    a triangle across the seam gets u > 1 on its wrapped corners (REPEAT makes that the same texels), a pole corner the
    mean u of the other two."""
    import numpy as np

    from .renderer import Mesh
    m = make_blob_mesh(num_lat, num_lon, radius, seed)
    d = m.vertices.astype(np.float64) / (np.array([1.4, 1.0, 0.8]) * radius)
    u = (np.arctan2(d[:, 1], d[:, 0]) % (2 * np.pi)) / (2 * np.pi)
    v = 1.0 - np.arccos(np.clip(d[:, 2] / np.linalg.norm(d, axis=1), -1, 1)) / np.pi
    cu, cv = u[m.faces], v[m.faces]                                   # [F, 3]
    lo = cu.max(1, keepdims=True) - cu > 0.5
    cu = np.where(lo, cu + 1.0, cu)                                   # the seam: wrap the low corners past 1
    pole = (m.faces == 0) | (m.faces == len(m.vertices) - 1)
    other = np.where(pole, np.nan, cu)
    cu = np.where(pole, np.nanmean(other, 1, keepdims=True), cu)
    idx = m.faces.reshape(-1)
    F = len(m.faces)
    uv = np.stack([cu.reshape(-1), cv.reshape(-1)], 1).astype(np.float32)
    return Mesh(m.vertices[idx], np.arange(3 * F, dtype=np.int32).reshape(F, 3), m.colors[idx], m.normals[idx], uv,
                make_texture(tex_size, seed))


def make_bop_eval_scene(root: str, num_images: int = 4, num_objects: int = 2, width: int = 320, height: int = 240,
                        mesh_res: int = 40, gts_per_image: int = 2, depth_scale: float = 0.1, seed: int = 0,
                        device: str = "cuda"):
    """A BOP split for evaluation, generated from a seed on the GPU: <root>/synth/{models/, test/000001/, test_targets_bop19.json}.
    Objects are make_blob_mesh(mesh_res, mesh_res) blobs (about 2 mesh_res^2 triangles); every image shows gts_per_image
    distinct objects, one instance each.  The test depth is the GT renders composited over a background plane at 1500 mm,
    with a 40 mm occluder in front of the first instance and a hole (no measurement), stored as uint16 PNG in depth_scale
    units.  -> dict: split_dir, models_dir, K, width, height, diameters, images [(im_id, [(obj_id, 4x4 m2c)])]."""
    import json
    import os

    import numpy as np
    from PIL import Image

    from .renderer import HipRasterizer, save_ply
    from .eval_bop19 import _Camera
    rng = np.random.default_rng(seed)
    ds = os.path.join(root, "synth")
    split, models = os.path.join(ds, "test"), os.path.join(ds, "models")
    sdir = os.path.join(split, "000001")
    os.makedirs(os.path.join(sdir, "depth"), exist_ok=True)
    os.makedirs(models, exist_ok=True)
    ras = HipRasterizer(device)
    diam, info = {}, {}
    for lid in range(1, num_objects + 1):
        m = make_blob_mesh(mesh_res, mesh_res, radius=float(rng.uniform(35, 55)), seed=seed * 100 + lid)
        save_ply(os.path.join(models, f"obj_{lid:06d}.ply"), m)
        diam[lid] = float(2.0 * np.linalg.norm(m.vertices.astype(np.float64), axis=1).max())
        info[str(lid)] = {"diameter": diam[lid]}
        ras.add_object_model(lid, mesh=m)
    with open(os.path.join(models, "models_info.json"), "w") as f:
        json.dump(info, f)
    K = np.array([[572.4, 0.0, width / 2 + 5.3], [0.0, 573.6, height / 2 + 2.0], [0.0, 0.0, 1.0]])
    images, cams, gts, infos, targets = [], {}, {}, {}, []
    for im in range(num_images):
        objs = rng.choice(np.arange(1, num_objects + 1), size=min(gts_per_image, num_objects), replace=False)
        inst = []
        for lid in objs:
            a = rng.normal(size=3)
            a /= np.linalg.norm(a)
            ang = rng.uniform(-np.pi, np.pi)
            Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            T = np.eye(4)
            T[:3, :3] = np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx
            z = rng.uniform(700, 1100)
            T[:3, 3] = [rng.uniform(-0.3, 0.3) * z * width / K[0, 0], rng.uniform(-0.3, 0.3) * z * height / K[1, 1], z]
            inst.append((int(lid), T))
        renders = [ras.render_views(lid, [_Camera(K, width, height, np.linalg.inv(T))], with_color=False)["depth"][0].cpu().numpy()
                   for lid, T in inst]
        depth = np.full((height, width), 1500.0, np.float32)
        for r in renders:
            depth = np.where((r > 0) & (r < depth), r, depth)
        m0 = renders[0] > 0
        if m0.any():   # an occluder 40 mm in front of a strip of the first instance
            ys, xs = np.nonzero(m0)
            y0, x0 = int(np.median(ys)), int(np.median(xs))
            depth[y0:y0 + 12, :x0] = np.where(m0[y0:y0 + 12, :x0], renders[0][y0:y0 + 12, :x0] - 40.0, depth[y0:y0 + 12, :x0])
        hy, hx = int(rng.integers(0, height - 20)), int(rng.integers(0, width - 20))
        depth[hy:hy + 20, hx:hx + 20] = 0.0
        u16 = np.clip(np.rint(depth / depth_scale), 0, 65535).astype(np.uint16)
        Image.fromarray(u16).save(os.path.join(sdir, "depth", f"{im:06d}.png"))
        stored = u16.astype(np.float32) * np.float32(depth_scale)
        cams[str(im)] = {"cam_K": K.ravel().tolist(), "depth_scale": depth_scale}
        gts[str(im)] = [{"cam_R_m2c": T[:3, :3].ravel().tolist(), "cam_t_m2c": T[:3, 3].tolist(), "obj_id": lid} for lid, T in inst]
        vis = []
        for r in renders:
            m = r > 0
            vis.append(float(np.sum(m & ((np.abs(r - stored) <= 15.0) | (stored == 0))) / max(int(m.sum()), 1)))
        infos[str(im)] = [{"visib_fract": v} for v in vis]
        targets += [{"scene_id": 1, "im_id": im, "obj_id": lid, "inst_count": 1} for lid, _ in inst]
        images.append((im, inst))
    for name, obj in (("scene_camera.json", cams), ("scene_gt.json", gts), ("scene_gt_info.json", infos)):
        with open(os.path.join(sdir, name), "w") as f:
            json.dump(obj, f)
    with open(os.path.join(ds, "test_targets_bop19.json"), "w") as f:
        json.dump(targets, f)
    return {"split_dir": split, "models_dir": models, "K": K, "width": width, "height": height, "diameters": diam, "images": images,
            "targets": targets}


def write_bop_results_csv(path: str, estimates) -> None:
    """estimates: [(scene_id, im_id, obj_id, score, 4x4 m2c, time)] -> the BOP19 csv in eval_util.prepare_bop_submission's format."""
    import numpy as np
    lines = ["scene_id,im_id,obj_id,score,R,t,time"]
    for s, im, lid, score, T, tm in estimates:
        T = np.asarray(T, np.float64)
        lines.append("{},{},{},{},{},{},{}".format(s, im, lid, score, " ".join(map(str, T[:3, :3].ravel().tolist())),
                                                   " ".join(map(str, T[:3, 3].tolist())), tm))
    with open(path, "w") as f:
        f.write("\n".join(lines))
