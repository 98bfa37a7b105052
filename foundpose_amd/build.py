"""Builds foundpose_amd/lib/libfoundpose_amd.so with hipcc for gfx950 (cross-compiles without a GPU).

    python -m foundpose_amd.build [--force]
"""

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
OBJDIR = os.path.join(HERE, "lib", "obj")
SO = os.path.join(LIBDIR, "libfoundpose_amd.so")
SOURCES = ["api.cpp", "f32_tile.hip", "match.hip", "retrieve.hip", "gemm_bf16.hip", "gemm_fp8.hip", "gemm_split.hip", "gemm_splitx.hip", "gemm_f16.hip", "attn.hip", "vit.hip", "crop.hip", "pnp.hip", "kabsch.hip", "verify.hip", "mask_verify.hip", "det_masks.hip", "pose_nms.hip", "detection_ap.hip", "coco_eval.hip", "proposals.hip", "render.hip", "pose_eval.hip", "pose_add.hip", "point_extremes.hip", "vsd.hip", "gt_info.hip", "tsdf.hip", "tsdf_fill.hip", "tsdf_track.hip", "multiview.hip", "mask_refine.hip", "simplify.hip", "depth_proposals.hip", "refine.hip", "depth_refine.hip", "rgbd_refine.hip", "vis.hip"]
HEADERS = ["common.hpp", "f32_stage.hpp", "kernels.hpp", "select.hpp", "stl_order.hpp", "stl_wave.hpp", "rot.hpp", "ransac.hpp", "refine_terms.hpp", "verify_grid.hpp", "gemm_kernel.hpp", "rounded.hpp", "bop_dist.hpp", "group_parts.hpp", os.path.join("..", "..", "include", "foundpose_amd.h"), os.path.join("..", "..", "include", "foundpose_amd_multiview.h"),
           os.path.join("..", "..", "include", "foundpose_amd_mask_refine.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "-Wno-unused-value",
         # MFMA results feed VALU epilogues/softmax directly: keep accumulators in the VGPR half of the unified
         # register file instead of AGPRs (saves ~100 v_accvgpr moves per attention tile)
         "-mllvm", "-amdgpu-mfma-vgpr-form"]


def _newer(a, b):
    return not os.path.exists(b) or os.path.getmtime(a) > os.path.getmtime(b)


def build(force: bool = False, verbose: bool = True) -> str:
    """Compiles the stale objects and links the library; returns its path."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJDIR, exist_ok=True)
    hdr_paths = [os.path.join(CSRC, h) for h in HEADERS]
    jobs = []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        obj = os.path.join(OBJDIR, os.path.splitext(src)[0] + ".o")
        stale = force or _newer(sp, obj) or any(_newer(h, obj) for h in hdr_paths)
        jobs.append((sp, obj, stale))

    def compile_one(job):
        sp, obj, stale = job
        if not stale:
            return
        cmd = [hipcc, *FLAGS, "-x", "hip", "-c", sp, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        list(ex.map(compile_one, jobs))
    objs = [j[1] for j in jobs]
    if force or any(_newer(o, SO) for o in objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO, *objs]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return SO


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
