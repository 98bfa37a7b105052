"""Freezes tests/golden/template_views.npz by running the REFERENCE's own view sampling and crop-camera code
(utils/misc.py sample_views, calc_crop_box, construct_crop_camera; utils/geometry.py rotation_matrix_numpy;
utils/structs.py PinholePlaneCameraModel) through oracle.ref_shim.  Build container only (needs the reference):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_templates.py

What the fixture holds (data only):
  views_<n>_<r>_<s>   scripts/gen_templates.py's view list for min_num_viewpoints n, num_inplane_rotations r, s view spheres
                      over the depth range DEPTH_RANGE: rotations [N,3,3] and translations [N,3,1]
  cam_<name>          step 1 for a dataset camera: (side, f, c) of the square template camera, then (size, f, c) of the
                      SSAA render camera
  tcam_<i>            steps 5-6 for a box in the lmo render camera: crop camera f, c, T_world_from_eye, then the template
                      camera's size, f, c.  Step 6 multiplies float32 camera numbers by a Python float: under the
                      reference's pinned numpy (1.26, NEP 50 not yet in force) that product is float64, which is what is
                      frozen here regardless of the numpy running this tool.
  fit_<i>             boxes and whether the reference's border rule rejects them.
"""

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_shim  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "template_views.npz")
DEPTH_RANGE = (346.31, 1499.84)
VIEW_CASES = [(57, 14, 1), (9, 3, 1), (9, 3, 3)]
CAMERAS = {"landscape": ([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], 640, 480),
           "portrait": ([[600.5, 0.0, 241.25], [0.0, 601.25, 318.75], [0.0, 0.0, 1.0]], 480, 640)}
BOXES = [(900, 1100, 1500, 1400), (1200, 1180, 1300, 1350), (40, 300, 2000, 2400), (1000, 900, 1017, 2012)]
PATCH, SSAA, CROP, PAD = 14, 4.0, (420, 420), 0.2


def main() -> None:
    ref = ref_shim.import_reference()
    import importlib
    structs = importlib.import_module("utils.structs")
    geometry = importlib.import_module("utils.geometry")
    out = {"depth_range": np.array(DEPTH_RANGE)}
    for n, r, s in VIEW_CASES:
        lo, hi = min(DEPTH_RANGE), max(DEPTH_RANGE)
        radii = [lo + (i + 0.5) * (hi - lo) / float(s) for i in range(s)]
        sphere = [v for rad in radii for v in ref.misc.sample_views(min_n_views=n, radius=rad, mode="fibonacci")[0]]
        views = []
        for v in sphere:
            for k in range(r):
                Ri = geometry.rotation_matrix_numpy(2 * np.pi / r * k, np.array([0, 0, 1]))[:3, :3]
                views.append((Ri.dot(v["R"]), Ri.dot(v["t"])))
        out[f"views_{n}_{r}_{s}_R"] = np.array([v[0] for v in views])
        out[f"views_{n}_{r}_{s}_t"] = np.array([v[1] for v in views])
    for name, (K, W, H) in CAMERAS.items():
        K = np.array(K)
        side = PATCH * int(max(W, H) / PATCH)
        cam = structs.PinholePlaneCameraModel(width=side, height=side, f=(K[0, 0], K[1, 1]),
                                              c=(K[0, 2] - 0.5 * (W - side), K[1, 2] - 0.5 * (H - side)))
        rc = structs.PinholePlaneCameraModel(width=int(cam.width * SSAA), height=int(cam.height * SSAA), f=(cam.f[0] * SSAA, cam.f[1] * SSAA),
                                             c=(cam.c[0] * SSAA, cam.c[1] * SSAA))
        out[f"cam_{name}_K"] = K
        out[f"cam_{name}_size"] = np.array([W, H])
        out[f"cam_{name}"] = np.array([side, *cam.f, *cam.c, rc.width, *rc.f, *rc.c], np.float64)
    K, W, H = CAMERAS["landscape"]
    side = PATCH * int(max(W, H) / PATCH)
    f = np.array(K)[[0, 1], [0, 1]] * SSAA
    c = (np.array(K)[[0, 1], [2, 2]] - 0.5 * (np.array([W, H]) - side)) * SSAA
    view = ref.misc.sample_views(min_n_views=9, radius=700.0, mode="fibonacci")[0][3]
    Rc = view["R"].T
    T = np.eye(4)
    T[:3, :3], T[:3, 3:] = Rc, -Rc.dot(view["t"])
    render = structs.PinholePlaneCameraModel(width=int(side * SSAA), height=int(side * SSAA), f=tuple(f), c=tuple(c), T_world_from_eye=T)
    out["tcam_render_T"] = T
    for i, b in enumerate(BOXES):
        box = structs.AlignedBox2f(left=b[0], top=b[1], right=b[2], bottom=b[3])
        cb = ref.misc.calc_crop_box(box=box, make_square=True)
        cc = ref.misc.construct_crop_camera(box=cb, camera_model_c2w=render, viewport_size=(int(CROP[0] * SSAA), int(CROP[1] * SSAA)),
                                            viewport_rel_pad=PAD)
        scale = CROP[0] / float(cc.width)
        out[f"tcam_{i}_box"] = np.array(b)
        out[f"tcam_{i}_crop"] = np.array([*cc.f, *cc.c], np.float64)
        out[f"tcam_{i}_crop_T"] = np.array(cc.T_world_from_eye)
        out[f"tcam_{i}"] = np.array([CROP[0], CROP[1], np.float64(cc.f[0]) * scale, np.float64(cc.f[1]) * scale,
                                     np.float64(cc.c[0]) * scale, np.float64(cc.c[1]) * scale], np.float64)
    fits = [(1, 1, 2518, 2518), (0, 5, 100, 100), (5, 0, 100, 100), (5, 5, 2519, 100), (5, 5, 100, 2519), (0, 0, 0, 0)]
    out["fit_boxes"] = np.array(fits)
    out["fit_rejected"] = np.array([b[0] == 0 or b[1] == 0 or b[2] == 2520 - 1 or b[3] == 2520 - 1 for b in fits])
    np.savez_compressed(OUT, **out)
    print(OUT, sorted(out))


if __name__ == "__main__":
    main()
