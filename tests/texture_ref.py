"""Numpy restatement of the textured shading of csrc/render.hip (TEST HELPER; DESIGN.md section 8, "Textured models").

Coverage, depth and the lighting rig come from tests/render_ref.py; this restates what differs for a textured winner, in the
kernel's operation order: the mip pyramid (integer, exact), the perspective-correct uv (fp32), its analytic screen
derivatives (fp64), the LOD (fp32 log2), GL LINEAR / LINEAR_MIPMAP_LINEAR with REPEAT wrap, the sRGB decode and the
metallic-roughness shading with the material as data.  log2, pow and division are the only non-exact device functions, so
the device's uint8 colour matches this on >= 99.9 % of covered pixels and within +-1 everywhere.
"""

import numpy as np

from . import render_ref

F32 = np.float32


def mip_levels(img):
    """uint8 [h, w, 3] -> the pyramid levels, uint8 [h_l, w_l, 3] each, down to 1 x 1 (fp_texture_mips)."""
    levels = [np.ascontiguousarray(img, np.uint8)]
    while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
        src = levels[-1].astype(np.int64)
        h, w = src.shape[:2]
        dh, dw = max(1, h >> 1), max(1, w >> 1)
        y, x = np.arange(dh), np.arange(dw)
        s = 0
        for j in (0, 1):
            for i in (0, 1):
                s = s + src[np.minimum(2 * y + j, h - 1)][:, np.minimum(2 * x + i, w - 1)]
        levels.append(((s + 2) >> 2).astype(np.uint8))
    return levels


def pack(levels):
    """The levels -> packed RGBA8 uint32 texels back to back (the device pyramid's layout)."""
    out = []
    for lv in levels:
        p = lv.astype(np.uint32)
        out.append((p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16) | np.uint32(0xFF000000)).reshape(-1))
    return np.concatenate(out)


def bilinear(level, u, v):
    """GL LINEAR on one level (uint8 [h, w, 3]) at fp32 u, v [N] -> fp32 [N, 3]; REPEAT wrap, row 0 is v = 1."""
    h, w = level.shape[:2]
    u, v = np.asarray(u, F32), np.asarray(v, F32)
    s = u * F32(w) - F32(0.5)
    r = (F32(1) - v) * F32(h) - F32(0.5)
    fs, fr = np.floor(s), np.floor(r)
    al, be = s - fs, r - fr
    i0 = np.clip(fs, F32(-2.0 ** 30), F32(2.0 ** 30)).astype(np.int64)
    j0 = np.clip(fr, F32(-2.0 ** 30), F32(2.0 ** 30)).astype(np.int64)
    x0, x1, y0, y1 = i0 % w, (i0 + 1) % w, j0 % h, (j0 + 1) % h
    t = lambda y, x: level[y, x].astype(F32) / F32(255)   # noqa: E731
    t00, t10, t01, t11 = t(y0, x0), t(y0, x1), t(y1, x0), t(y1, x1)
    a1, b1 = (F32(1) - al)[:, None], (F32(1) - be)[:, None]
    al, be = al[:, None], be[:, None]
    return b1 * (a1 * t00 + al * t10) + be * (a1 * t01 + al * t11)


def lod(q, qx, qy, u, v, uk, vk, tex_w, tex_h):
    """GL's isotropic level of detail from the analytic derivatives: q, qx, qy fp64 [3][N] (q_k and its screen
    derivatives), u, v fp32 [N], uk, vk fp32 [N, 3] (the corners') -> lambda fp32 [N]."""
    D, Dx, Dy = (q[0] + q[1]) + q[2], (qx[0] + qx[1]) + qx[2], (qy[0] + qy[1]) + qy[2]
    uk, vk = uk.astype(np.float64), vk.astype(np.float64)
    ud, vd = u.astype(np.float64), v.astype(np.float64)

    def d(qd, c, cd, Dd):
        return (((qd[0] * c[:, 0] + qd[1] * c[:, 1]) + qd[2] * c[:, 2]) - cd * Dd) / D
    ax, bx = d(qx, uk, ud, Dx) * float(tex_w), d(qx, vk, vd, Dx) * float(tex_h)
    ay, by = d(qy, uk, ud, Dy) * float(tex_w), d(qy, vk, vd, Dy) * float(tex_h)
    rho2 = np.maximum(ax * ax + bx * bx, ay * ay + by * by)
    with np.errstate(divide="ignore"):
        return F32(0.5) * np.log2(rho2.astype(F32))


def trilinear(levels, lam, u, v):
    """LINEAR (lambda <= 0, level 0) / LINEAR_MIPMAP_LINEAR (levels floor(lambda), +1, blended by frac) -> fp32 [N, 3]."""
    top = len(levels) - 1
    lam = np.asarray(lam, F32)
    mag = ~(lam > 0)
    at_top = ~mag & (lam >= F32(top))
    fl = np.floor(np.where(mag | at_top, F32(0), lam))
    d1 = np.where(at_top, top, np.where(mag, 0, fl.astype(np.int64)))
    f = np.where(at_top | mag, F32(0), lam - fl).astype(F32)
    out = np.zeros((len(lam), 3), F32)
    for l in np.unique(d1):
        sel = d1 == l
        c = bilinear(levels[l], u[sel], v[sel])
        blend = sel & ~mag & (d1 < top)
        if l < top and blend.any():
            b = blend[sel]
            c2 = bilinear(levels[l + 1], u[sel][b], v[sel][b])
            fb = f[sel][b][:, None]
            c[b] = (F32(1) - fb) * c[b] + fb * c2
        out[sel] = c
    return out


def srgb_decode(c):
    c = np.asarray(c, F32)
    return np.where(c <= F32(0.04045), c / F32(12.92), np.power((c + F32(0.055)) / F32(1.055), F32(2.4))).astype(F32)


def shade_textured(mesh, cam, W, H, depth, tri, recs, material, levels=None):
    """uint8 colour [H, W, 3] of a textured mesh's winners (material: float[6] = metallic, roughness, factor rgb, sRGB flag),
    plus lambda [H, W] (NaN off the object) for the tests that check the level of detail."""
    m = np.asarray(material, F32)
    levels = levels if levels is not None else mip_levels(mesh.texture)
    tex_h, tex_w = mesh.texture.shape[:2]
    _, _, _, ne = render_ref.transform(mesh.vertices, mesh.normals, cam)
    c = np.asarray(cam, np.float64)
    fx, fy, cx, cy = F32(c[0]), F32(c[1]), F32(c[2]), F32(c[3])
    out = np.zeros((H, W, 3), np.uint8)
    lam_img = np.full((H, W), np.nan, F32)
    ys, xs = np.nonzero(tri >= 0)
    if len(ys) == 0:
        return out, lam_img
    t = tri[ys, xs]
    A = np.array([recs[i][0] for i in t], np.int64)
    B = np.array([recs[i][1] for i in t], np.int64)
    C = np.array([recs[i][2] for i in t], np.int64)
    zz = np.array([recs[i][3] for i in t], np.float64)
    ar = np.array([recs[i][4] for i in t], np.float64)
    vid = np.array([recs[i][5] for i in t], np.int64)
    PX, PY = xs.astype(np.int64) * 256 + 128, ys.astype(np.int64) * 256 + 128
    q = [((A[:, k] * PX + B[:, k] * PY + C[:, k]).astype(np.float64) / ar) / zz[:, k] for k in range(3)]
    qx = [((256.0 * A[:, k].astype(np.float64)) / ar) / zz[:, k] for k in range(3)]
    qy = [((256.0 * B[:, k].astype(np.float64)) / ar) / zz[:, k] for k in range(3)]
    z = 1.0 / ((q[0] + q[1]) + q[2])
    w = [(q[k] * z).astype(F32) for k in range(3)]
    uv = np.asarray(mesh.uv, F32)
    uk, vk = uv[vid, 0], uv[vid, 1]                                   # [N, 3]
    u = (w[0] * uk[:, 0] + w[1] * uk[:, 1]) + w[2] * uk[:, 2]
    v = (w[0] * vk[:, 0] + w[1] * vk[:, 1]) + w[2] * vk[:, 2]
    lam = lod(q, qx, qy, u, v, uk, vk, tex_w, tex_h)
    lam_img[ys, xs] = lam
    col = trilinear(levels, lam, u, v)
    if m[5] != 0:
        col = srgb_decode(col)
    base = [m[2 + ch] * col[:, ch] for ch in range(3)]
    # lighting: render_ref.shade's chain with the material's metallic and alpha = roughness^2
    n = [(w[0] * ne[vid[:, 0], ch] + w[1] * ne[vid[:, 1], ch]) + w[2] * ne[vid[:, 2], ch] for ch in range(3)]
    nn = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    n = [np.where(nn > 0, ch / np.where(nn > 0, nn, F32(1)), F32(0)).astype(F32) for ch in n]
    zm = depth[ys, xs] * F32(0.001)
    pxe = (((xs.astype(F32) + F32(0.5)) - cx) / fx) * zm
    pye = (((ys.astype(F32) + F32(0.5)) - cy) / fy) * zm
    d2 = (pxe * pxe + pye * pye) + zm * zm
    dl = np.sqrt(d2)
    l = [-pxe / dl, -pye / dl, -zm / dl]
    h = [l[0] + l[0], l[1] + l[1], l[2] + l[2]]
    hn = np.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
    ndl = (n[0] * l[0] + n[1] * l[1]) + n[2] * l[2]
    nl = np.clip(ndl, F32(0.001), F32(1))
    nv = np.clip(np.abs(ndl), F32(0.001), F32(1))
    nh = np.clip(((n[0] * h[0] + n[1] * h[1]) + n[2] * h[2]) / hn, F32(0), F32(1))
    vh = np.clip(((l[0] * h[0] + l[1] * h[1]) + l[2] * h[2]) / hn, F32(0), F32(1))
    cd = zm / dl
    scale = F32(1) / (F32(0.98078528040323) - F32(0.86602540378444))
    offset = -F32(0.86602540378444) * scale
    sa = np.clip(cd * scale + offset, F32(0), F32(1))
    sa = sa * sa
    radiance = (F32(2.4) * sa) / d2
    metallic, alpha, pi, f0 = m[0], m[1] * m[1], F32(3.14159265358979), F32(0.04)
    refl = np.zeros_like(zm)
    for ch in range(3):
        refl = np.maximum(refl, F32(0.04) * (F32(1) - metallic) + base[ch] * metallic)
    F90 = np.clip(refl * F32(25), F32(0), F32(1))
    for ch in range(3):
        b = base[ch]
        diffuse_color = (b * (F32(1) - f0)) * (F32(1) - metallic)
        spec_color = f0 * (F32(1) - metallic) + b * metallic
        one_vh = np.clip(F32(1) - vh, F32(0), F32(1))
        p5 = (((one_vh * one_vh) * one_vh) * one_vh) * one_vh
        Fr = spec_color + (F90 - spec_color) * p5
        a2 = alpha * alpha
        gl = (F32(2) * nl) / (nl + np.sqrt(a2 + (F32(1) - a2) * (nl * nl)))
        gv = (F32(2) * nv) / (nv + np.sqrt(a2 + (F32(1) - a2) * (nv * nv)))
        G = gl * gv
        fd = ((nh * a2 - nh) * nh) + F32(1)
        Dd = a2 / ((pi * fd) * fd)
        diff = (F32(1) - Fr) * (diffuse_color / pi)
        spec = ((Fr * G) * Dd) / ((F32(4) * nl) * nv)
        cc = np.clip((nl * radiance) * (diff + spec) + F32(0.02) * b, F32(0), F32(1))
        out[ys, xs, ch] = np.rint(cc * F32(255)).astype(np.uint8)
    return out, lam_img


def render_textured(mesh, cam, W, H, material):
    """-> dict(depth, tri_id, mask, color u8 [H, W, 3], lod fp32 [H, W], box) of a textured mesh."""
    depth, tri, recs = render_ref.rasterize(mesh.vertices, mesh.faces, cam, W, H)
    color, lam = shade_textured(mesh, cam, W, H, depth, tri, recs, material)
    ys, xs = np.nonzero(tri >= 0)
    box = (xs.min(), ys.min(), xs.max(), ys.max()) if len(xs) else None
    return {"depth": depth, "tri_id": tri, "mask": np.where(tri >= 0, 255, 0).astype(np.uint8), "color": color, "lod": lam,
            "box": box}
