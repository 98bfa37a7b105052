"""Numpy restatement of the template renderer's contract (TEST HELPER; DESIGN.md section 8, csrc/render.hip).

Coverage, depth, mask and triangle id are restated exactly (int64 edge functions, individually rounded fp64 operations in
the kernel's order), so the device must match them bit for bit; the shading is restated in fp32 with the kernel's
operation order (uint8 colour may differ by one step where a correctly rounded fp32 operation lands on a .5 boundary).
The template chain (steps 5-8 of scripts/gen_templates.py) is restated on top: depth warp, downsample, output casts.
"""

import numpy as np

from oracle import crop as ocrop

F32 = np.float32


def _dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def transform(verts, normals, cam):
    """cam: 16 doubles (f, c, R row-major, t) -> X, Y (int64 fixed point), z fp64, eye normals fp32 [V,3]."""
    c = np.asarray(cam, np.float64)
    R = c[4:13]
    v = verts.astype(np.float64)
    dx, dy, dz = v[:, 0] - c[13], v[:, 1] - c[14], v[:, 2] - c[15]
    ex, ey, ez = _dot3(dx, dy, dz, R[0], R[3], R[6]), _dot3(dx, dy, dz, R[1], R[4], R[7]), _dot3(dx, dy, dz, R[2], R[5], R[8])
    u, w = (ex / ez) * c[0] + c[2], (ey / ez) * c[1] + c[3]
    X, Y = np.rint(u * 256.0).astype(np.int64), np.rint(w * 256.0).astype(np.int64)
    Rf = R.astype(F32)
    n = normals.astype(F32)
    ne = np.stack([_dot3(n[:, 0], n[:, 1], n[:, 2], Rf[0], Rf[3], Rf[6]), _dot3(n[:, 0], n[:, 1], n[:, 2], Rf[1], Rf[4], Rf[7]),
                   _dot3(n[:, 0], n[:, 1], n[:, 2], Rf[2], Rf[5], Rf[8])], 1)
    return X, Y, ez, ne


def _setup(X, Y, z, face):
    """-> None (dropped) or (A, B, C, z, area, vid, tl) after winding normalisation; edge k is opposite vertex k."""
    vid = [int(face[0]), int(face[1]), int(face[2])]
    x, y, zz = [int(X[i]) for i in vid], [int(Y[i]) for i in vid], [z[i] for i in vid]
    area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    if area == 0:
        return None
    if area < 0:
        for arr in (x, y, zz, vid):
            arr[1], arr[2] = arr[2], arr[1]
        area = -area
    A, B, C, tl = [], [], [], []
    for k in range(3):
        ia, ib = (k + 1) % 3, (k + 2) % 3
        ddx, ddy = x[ib] - x[ia], y[ib] - y[ia]
        A.append(-ddy)
        B.append(ddx)
        C.append(ddy * x[ia] - ddx * y[ia])
        tl.append(ddy < 0 or (ddy == 0 and ddx > 0))
    return A, B, C, zz, area, vid, tl, (min(x), max(x), min(y), max(y))


def rasterize(verts, faces, cam, W, H):
    """-> depth fp32 [H,W], tri_id int32 [H,W] (-1 background), plus the per-pixel (E0, E1, E2, record) of the winner."""
    X, Y, z, _ = transform(verts, np.zeros_like(verts), cam)
    if z.min() <= 100.0:
        raise ValueError("near plane")
    depth = np.full((H, W), np.inf, np.float32)
    tri = np.full((H, W), -1, np.int32)
    recs = {}
    for f, face in enumerate(faces):
        r = _setup(X, Y, z, face)
        if r is None:
            continue
        A, B, C, zz, area, vid, tl, (mnx, mxx, mny, mxy) = r
        x0, x1 = max(-((128 - mnx) // 256), 0), min((mxx - 128) // 256, W - 1)
        y0, y1 = max(-((128 - mny) // 256), 0), min((mxy - 128) // 256, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        recs[f] = r
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        PX, PY = px.astype(np.int64) * 256 + 128, py.astype(np.int64) * 256 + 128
        E = [A[k] * PX + B[k] * PY + C[k] for k in range(3)]
        inside = np.ones(PX.shape, bool)
        for k in range(3):
            inside &= (E[k] > 0) | ((E[k] == 0) & tl[k])
        if not inside.any():
            continue
        ar = np.float64(area)
        q = [(E[k].astype(np.float64) / ar) / zz[k] for k in range(3)]
        zf = (1.0 / ((q[0] + q[1]) + q[2])).astype(np.float32)
        cur_z, cur_t = depth[y0:y1 + 1, x0:x1 + 1], tri[y0:y1 + 1, x0:x1 + 1]
        win = inside & ((zf < cur_z) | ((zf == cur_z) & (f < cur_t)))
        cur_z[win], cur_t[win] = zf[win], f
    depth[tri < 0] = 0.0
    return depth, tri, recs


def shade(verts, normals, colors, faces, cam, W, H, depth, tri, recs):
    """uint8 colour [H,W,3] of the winners, in the kernel's fp32 operation order."""
    _, _, _, ne = transform(verts, normals, cam)
    c = np.asarray(cam, np.float64)
    fx, fy, cx, cy = F32(c[0]), F32(c[1]), F32(c[2]), F32(c[3])
    out = np.zeros((H, W, 3), np.uint8)
    ys, xs = np.nonzero(tri >= 0)
    if len(ys) == 0:
        return out
    t = tri[ys, xs]
    A = np.array([recs[i][0] for i in t], np.int64)
    B = np.array([recs[i][1] for i in t], np.int64)
    C = np.array([recs[i][2] for i in t], np.int64)
    zz = np.array([recs[i][3] for i in t], np.float64)
    ar = np.array([recs[i][4] for i in t], np.float64)
    vid = np.array([recs[i][5] for i in t], np.int64)
    PX, PY = xs.astype(np.int64) * 256 + 128, ys.astype(np.int64) * 256 + 128
    q = [((A[:, k] * PX + B[:, k] * PY + C[:, k]).astype(np.float64) / ar) / zz[:, k] for k in range(3)]
    z = 1.0 / ((q[0] + q[1]) + q[2])
    w = [(q[k] * z).astype(F32) for k in range(3)]
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
    base = [(w[0] * colors[vid[:, 0], ch] + w[1] * colors[vid[:, 1], ch]) + w[2] * colors[vid[:, 2], ch] for ch in range(3)]
    refl = np.zeros_like(zm)
    for ch in range(3):
        refl = np.maximum(refl, F32(0.04) * F32(0.8) + base[ch] * F32(0.2))
    F90 = np.clip(refl * F32(25), F32(0), F32(1))
    pi, metallic, alpha, f0 = F32(3.14159265358979), F32(0.2), F32(0.64), F32(0.04)
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
        D = a2 / ((pi * fd) * fd)
        diff = (F32(1) - Fr) * (diffuse_color / pi)
        spec = ((Fr * G) * D) / ((F32(4) * nl) * nv)
        col = np.clip((nl * radiance) * (diff + spec) + F32(0.02) * b, F32(0), F32(1))
        out[ys, xs, ch] = np.rint(col * F32(255)).astype(np.uint8)
    return out


def render(mesh, cam, W, H):
    """-> dict(depth, tri_id, mask u8 255/0, color u8 [H,W,3], box (x0, y0, x1, y1) or None)."""
    depth, tri, recs = rasterize(mesh.vertices, mesh.faces, cam, W, H)
    color = shade(mesh.vertices, mesh.normals, mesh.colors, mesh.faces, cam, W, H, depth, tri, recs)
    ys, xs = np.nonzero(tri >= 0)
    box = (xs.min(), ys.min(), xs.max(), ys.max()) if len(xs) else None
    return {"depth": depth, "tri_id": tri, "mask": np.where(tri >= 0, 255, 0).astype(np.uint8), "color": color, "box": box}


def warp_depth(src, params, out_h, out_w, recompute=True):
    """utils/misc.py:522-557 in the kernel's order (fp_warp_depth)."""
    mx, my = ocrop.crop_maps(params, out_h, out_w, True)
    sx, sy = np.rint(mx).astype(np.int64), np.rint(my).astype(np.int64)
    Hs, Ws = src.shape
    ok = (sx >= 0) & (sx < Ws) & (sy >= 0) & (sy < Hs)
    d = np.where(ok, src[np.clip(sy, 0, Hs - 1), np.clip(sx, 0, Ws - 1)], F32(0)).astype(np.float32)
    if not recompute:
        return d
    p = np.asarray(params, np.float64)
    fs, cs, Rs, ts = p[16:18], p[18:20], p[20:29], p[29:32]
    Rd, td = p[4:13], p[13:16]
    qx, qy = (sx - cs[0]) / fs[0], (sy - cs[1]) / fs[1]
    n = np.maximum(5.43e-20, np.sqrt((qx * qx + qy * qy) + 1.0))
    vx, vy, vz = qx / n, qy / n, 1.0 / n
    s = d.astype(np.float64) / vz
    ex, ey, ez = vx * s, vy * s, vz * s
    wx = _dot3(ex, ey, ez, Rs[0], Rs[1], Rs[2]) + ts[0]
    wy = _dot3(ex, ey, ez, Rs[3], Rs[4], Rs[5]) + ts[1]
    wz = _dot3(ex, ey, ez, Rs[6], Rs[7], Rs[8]) + ts[2]
    z = _dot3(wx - td[0], wy - td[1], wz - td[2], Rd[2], Rd[5], Rd[8]).astype(np.float32)
    return np.where(d > 0, z, d).astype(np.float32)


def downsample(color_chw, depth, mask, f):
    """cv2.resize INTER_AREA (block mean, rows summed then the row sums) / INTER_NEAREST, then the output casts."""
    C, Hs, Ws = color_chw.shape
    h, w = Hs // f, Ws // f
    blk = color_chw.reshape(C, h, f, w, f).astype(np.float32)
    s = None
    for r in range(f):
        row = blk[:, :, r, :, 0]
        for c in range(1, f):
            row = row + blk[:, :, r, :, c]
        s = row if s is None else s + row
    mean = s * (F32(1) / F32(f * f))
    rgb = (F32(255) * mean).astype(np.uint8)
    d = np.clip(np.rint(depth[::f, ::f]), 0, 65535).astype(np.uint16)
    return rgb, d, mask[::f, ::f].copy()


def _boxes(X, Y, faces, W, H):
    """Per-face pixel box (x0, y0, x1, y1) as render_setup_kernel clamps it, and whether the face is binned at all
    (non-zero area, box not empty); vectorised over faces."""
    x, y = X[faces], Y[faces]
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    x0 = np.maximum(-((128 - x.min(1)) // 256), 0)
    x1 = np.minimum((x.max(1) - 128) // 256, W - 1)
    y0 = np.maximum(-((128 - y.min(1)) // 256), 0)
    y1 = np.minimum((y.max(1) - 128) // 256, H - 1)
    return x0, y0, x1, y1, (area != 0) & (x0 <= x1) & (y0 <= y1)


def tile_counts(verts, faces, cam, W, H, tile=32):
    """int64 [tiles_y * tiles_x]: how many triangle records each tile list holds (render_setup_kernel, pass 0)."""
    X, Y, _, _ = transform(verts, np.zeros_like(verts), cam)
    x0, y0, x1, y1, live = _boxes(X, Y, np.asarray(faces, np.int64), W, H)
    tx, ty = -(-W // tile), -(-H // tile)
    d = np.zeros((ty + 1, tx + 1), np.int64)   # 2-D difference array over each face's tile rectangle
    tx0, ty0, tx1, ty1 = x0[live] // tile, y0[live] // tile, x1[live] // tile + 1, y1[live] // tile + 1
    np.add.at(d, (ty0, tx0), 1)
    np.add.at(d, (ty0, tx1), -1)
    np.add.at(d, (ty1, tx0), -1)
    np.add.at(d, (ty1, tx1), 1)
    return d.cumsum(0).cumsum(1)[:ty, :tx].reshape(-1)


def face_coverage(verts, faces, cam, W, H):
    """int32 [H,W]: how many faces cover each pixel centre by the edge-function test alone (no z-test)."""
    X, Y, z, _ = transform(verts, np.zeros_like(verts), cam)
    count = np.zeros((H, W), np.int32)
    for face in faces:
        r = _setup(X, Y, z, face)
        if r is None:
            continue
        A, B, C, _, _, _, tl, (mnx, mxx, mny, mxy) = r
        x0, x1 = max(-((128 - mnx) // 256), 0), min((mxx - 128) // 256, W - 1)
        y0, y1 = max(-((128 - mny) // 256), 0), min((mxy - 128) // 256, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        PX, PY = px.astype(np.int64) * 256 + 128, py.astype(np.int64) * 256 + 128
        inside = np.ones(PX.shape, bool)
        for k in range(3):
            E = A[k] * PX + B[k] * PY + C[k]
            inside &= (E > 0) | ((E == 0) & tl[k])
        count[y0:y1 + 1, x0:x1 + 1] += inside
    return count


def random_sheet(nx, ny, x_range, y_range, plane, seed):
    """A random triangulation of the world rectangle x_range x y_range on the plane z = plane[0] + plane[1] x + plane[2] y
    (mm): a (nx+1) x (ny+1) vertex grid, interior vertices jittered by up to 0.3 cells, each cell split along a random
    diagonal.  -> vertices float32 [V,3], faces int32 [F,3], the boundary vertex ids in order around the rectangle."""
    rng = np.random.default_rng(seed)
    gx, gy = np.linspace(*x_range, nx + 1), np.linspace(*y_range, ny + 1)
    X, Y = np.meshgrid(gx, gy)                                    # [ny+1, nx+1]
    hx, hy = (gx[1] - gx[0]) * 0.3, (gy[1] - gy[0]) * 0.3
    X[1:-1, 1:-1] += rng.uniform(-hx, hx, (ny - 1, nx - 1))
    Y[1:-1, 1:-1] += rng.uniform(-hy, hy, (ny - 1, nx - 1))
    x, y = X.astype(np.float32).astype(np.float64).reshape(-1), Y.astype(np.float32).astype(np.float64).reshape(-1)
    z = plane[0] + plane[1] * x + plane[2] * y
    verts = np.stack([x, y, z], 1).astype(np.float32)
    idx = lambda i, j: j * (nx + 1) + i   # noqa: E731
    faces = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i, j + 1), idx(i + 1, j + 1)
            faces += [(a, b, d), (a, d, c)] if rng.random() < 0.5 else [(a, b, c), (b, d, c)]
    ring = [idx(i, 0) for i in range(nx)] + [idx(nx, j) for j in range(ny)] + [idx(i, ny) for i in range(nx, 0, -1)] + \
        [idx(0, j) for j in range(ny, 0, -1)]
    return verts, np.array(faces, np.int32), np.array(ring, np.int64)


def inside_polygon(PX, PY, px, py):
    """Exact (integer) point-in-polygon of the points (PX, PY) against the closed polygon (px, py), all int64 fixed point.
    -> +1 strictly inside, -1 strictly outside, 0 on the outline."""
    inside = np.zeros(PX.shape, bool)
    on = np.zeros(PX.shape, bool)
    n = len(px)
    for k in range(n):
        ax, ay, bx, by = int(px[k]), int(py[k]), int(px[(k + 1) % n]), int(py[(k + 1) % n])
        cross = (bx - ax) * (PY - ay) - (by - ay) * (PX - ax)
        on |= (cross == 0) & (PX >= min(ax, bx)) & (PX <= max(ax, bx)) & (PY >= min(ay, by)) & (PY <= max(ay, by))
        up = (ay <= PY) & (by > PY)
        down = (by <= PY) & (ay > PY)
        inside ^= (up & (cross > 0)) | (down & (cross < 0))
    return np.where(on, 0, np.where(inside, 1, -1))
