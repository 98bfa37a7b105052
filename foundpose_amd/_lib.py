"""ctypes binding of libfoundpose_amd.so (the C ABI in include/foundpose_amd.h).

The header is the one declaration of the ABI: the argument types of every entry point, the list of exported symbols and ABI_VERSION are
parsed from it on import (_parse_header); entry points declared in a header of their own beside it (EXTENSION_HEADERS) are parsed the same way.  What stays written by hand here -- the three ViT structs, the FP_* constants and the scratch-size
formulas -- is compared with the header, compiled, by tests/test_cabi_symbols.py.

There is NO fallback: if the library is missing or a call fails, this raises. The product
path never computes on the CPU and never touches oracle/.
"""

import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# FOUNDPOSE_AMD_LIB: another build of the SAME library (a measurement variant from tools/build_variant.sh, for same-box A/B runs); it must
# export the same ABI version.  Never a different implementation: there is one product path.
LIB_PATH = os.environ.get("FOUNDPOSE_AMD_LIB") or os.path.join(_HERE, "lib", "libfoundpose_amd.so")

FP_F32, FP_BF16, FP_FP8, FP_F16X3, FP_F16F8, FP_F16 = 0, 1, 2, 3, 4, 5
GEMM_SPLIT_F16F8 = 1 << 20   # FP_GEMM_SPLIT_F16F8 of the header
GEMM_F16 = 1 << 21           # FP_GEMM_F16 of the header: IEEE fp16 operands / outputs in fp_gemm_bf16, fp_gemm_bf16_ln
SPLIT_SCALE_ACT, SPLIT_SCALE_QKV, SPLIT_SCALE_HID = 16.0, 16.0, 4.0  # FP_SPLIT_SCALE_* of the header


class FoundPoseNativeError(RuntimeError):
    pass


class FoundPoseSaturationError(FoundPoseNativeError):
    """The f16x3 (near-exact) mode clamped an activation to the range of its split-fp16 row (+-4094 for LayerNorm outputs / q / k / v,
    +-16376 for hidden activations; include/foundpose_amd.h): the features are then no longer the fp32 arithmetic's, and the mode whose
    purpose is index-exact matching must not return a plausible wrong neighbour silently."""


vp, i32, i64, f32, f64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_uint64


class VitBlock(C.Structure):
    _fields_ = [(n, vp) for n in (
        "ln1_w", "ln1_b", "ln2_w", "ln2_b", "ls1", "ls2",
        "qkv_w", "proj_w", "fc1_w", "fc2_w",
        "qkv_b", "proj_b", "fc1_b", "fc2_b", "qkv_s", "proj_s", "fc1_s", "fc2_s")] + [("act_scale", f32 * 4), ("qkv_colsum", vp), ("fc1_colsum", vp)]


class VitModel(C.Structure):
    _fields_ = [
        ("dim", i32), ("depth", i32), ("heads", i32), ("hidden", i32), ("registers", i32), ("patch", i32),
        ("ffn_swiglu", i32), ("weight_dtype", i32),
        ("patch_w", vp), ("patch_k_pad", i32), ("patch_b", vp), ("pos_patch", vp), ("prefix", vp),
        ("norm_w", vp), ("norm_b", vp), ("blocks", C.POINTER(VitBlock)), ("ld_w_dim", i32), ("ld_w_hidden", i32), ("patch_stride", i32), ("patch_acc_scale", f32), ("ln_fold", i32),
    ]


class VitWorkspace(C.Structure):
    _fields_ = [
        ("patches", vp), ("x", vp), ("y", vp), ("qkv", vp), ("h", vp), ("a8", vp),
        ("ld_y", i32), ("ld_h", i32), ("ld_qkv", i32), ("m_pad", i32), ("m_patch_pad", i32), ("xb", vp), ("stats", vp), ("sat", vp), ("xl", vp),
    ]


_BY_VALUE = {"int": i32, "int32_t": i32, "int64_t": i64, "float": f32, "double": f64, "uint64_t": u64, "size_t": C.c_size_t, "fp_stream_t": vp}
_BY_POINTER = {"fp_vit_model": C.POINTER(VitModel), "fp_vit_workspace": C.POINTER(VitWorkspace)}  # every other pointer: c_void_p


def _parse_header(path, versioned=True):
    """The prototypes (name -> argtypes; all return int), every declared symbol and FP_ABI_VERSION, read from the header's declarations
    `ret fp_name(args);`.  Nothing is guessed: whatever has no ctypes mapping below raises, naming the declaration.
    versioned=False: a header of further entry points beside the main one, which defines no version of its own (-> version None)."""
    try:
        text = open(path).read()
    except OSError as e:
        raise FoundPoseNativeError(f"cannot read the C ABI header {path}: {e}") from None
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    version = re.search(r"^#define\s+FP_ABI_VERSION\s+(\d+)\s*$", text, re.M)
    if version is None and versioned:
        raise FoundPoseNativeError(f"{path}: no #define FP_ABI_VERSION <integer>")
    protos, names = {}, ["fp_last_error"]
    for ret, name, params in re.findall(r"^([A-Za-z_][\w \t*]*?)\s*\b(fp_\w+)\s*\(([^()]*)\)\s*;", text, re.M):
        ret = " ".join(ret.replace("*", " * ").split())
        if name == "fp_last_error" and (ret, params.strip()) == ("const char *", "void"):
            continue
        if ret != "int":
            raise FoundPoseNativeError(f"{path}: {name} returns '{ret}'; the binding knows int (and const char* fp_last_error(void)) only")
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\*?)\s*\w+\s*", p)
            table = _BY_POINTER if m and m.group(2) else _BY_VALUE
            if m is None or (table is _BY_VALUE and m.group(1) not in table):
                raise FoundPoseNativeError(f"{path}: {name}: parameter '{' '.join(p.split())}' has no ctypes mapping")
            args.append(table.get(m.group(1), vp))
        protos[name] = args
        names.append(name)
    partial = sorted(set(re.findall(r"\b(fp_\w+)\s*\(", text)) - set(names))
    if partial:
        raise FoundPoseNativeError(f"{path}: cannot parse the declaration of {', '.join(partial)}")
    return protos, sorted(names), int(version.group(1)) if version else None


_PROTOS, _SYMBOLS, ABI_VERSION = _parse_header(os.path.join(_HERE, "..", "include", "foundpose_amd.h"))
# entry points declared in headers of their own beside the main one (same library, same ABI version, same parser): header -> prototypes
EXTENSION_HEADERS = ("foundpose_amd_multiview.h",)
_EXT_PROTOS = {h: _parse_header(os.path.join(_HERE, "..", "include", h), versioned=False)[0] for h in EXTENSION_HEADERS}
# the headers of features added since, one per feature (same library, same ABI version, same parser): a new feature appends its header
# here and nothing else changes -- lib() binds whatever the table holds, after the entry points above
FEATURE_HEADERS = ("foundpose_amd_mask_refine.h",)
_FEATURE_PROTOS = {h: _parse_header(os.path.join(_HERE, "..", "include", h), versioned=False)[0] for h in FEATURE_HEADERS}

_lib = None


def lib() -> C.CDLL:
    """Loads the HIP library (after torch, so both share one libamdhip64 runtime)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FoundPoseNativeError(
                f"{LIB_PATH} is missing: build it with `python -m foundpose_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        handle.fp_last_error.restype = C.c_char_p
        handle.fp_last_error.argtypes = []
        for name, args in [*_PROTOS.items(), *(item for table in (_EXT_PROTOS, _FEATURE_PROTOS) for protos in table.values() for item in protos.items())]:
            fn = getattr(handle, name)  # AttributeError here = header/library mismatch
            fn.argtypes = args
            fn.restype = i32
        if handle.fp_abi_version() != ABI_VERSION:
            raise FoundPoseNativeError("libfoundpose_amd.so ABI version mismatch; rebuild")
        _lib = handle
    return _lib


def cosine_scratch_floats(num_det: int, max_templates: int) -> int:
    """FP_COSINE_SCRATCH_FLOATS of include/foundpose_amd.h."""
    return 2 * num_det * max_templates + 17 * num_det + 2


def cosine_prefilter_scratch_floats(num_det: int, max_templates: int) -> int:
    """FP_COSINE_PREFILTER_SCRATCH_FLOATS of include/foundpose_amd.h."""
    return cosine_scratch_floats(num_det, max_templates) + 3 * num_det * max_templates + 32 * num_det + 16


def cyclic_scratch_bytes(pairs: int, q_max: int, p_max: int) -> int:
    """FP_CYCLIC_SCRATCH_BYTES of include/foundpose_amd.h."""
    tiles = 8 * pairs * (((p_max + 127) // 128) * q_max + ((q_max + 127) // 128) * p_max)
    cand = 8 * pairs * (q_max + p_max) + 448 * pairs * max(q_max, p_max)
    return max(tiles, cand)


def knn_scratch_bytes(m: int, n: int, k: int) -> int:
    """FP_KNN_SCRATCH_BYTES of include/foundpose_amd.h."""
    if k == 1:
        return m * 8
    if k <= 8:
        return m * max(((n + 127) // 128) * k * 8, 704)
    return m * n * 4


POSE_ERR_TILE = 64 * 8  # FP_POSE_ERR_TILE of the header


def pose_err_scratch_bytes(num_hyp: int, max_pts: int, max_syms: int) -> int:
    """FP_POSE_ERR_SCRATCH_BYTES of include/foundpose_amd.h."""
    return 32 * ((num_hyp + 7) // 8) * 8 + 24 * num_hyp * max_syms * ((max_pts + POSE_ERR_TILE - 1) // POSE_ERR_TILE)


POSE_ADD_TILE = 256  # FP_POSE_ADD_TILE of the header


def pose_add_scratch_bytes(num_pairs: int, max_pts: int) -> int:
    """FP_POSE_ADD_SCRATCH_BYTES of include/foundpose_amd.h."""
    return 32 * ((num_pairs + 7) // 8) * 8 + 16 * num_pairs * ((max_pts + POSE_ADD_TILE - 1) // POSE_ADD_TILE)


PTS_TILE = 1024  # FP_PTS_TILE of the header
PTS_DIAMETER_MAX_V = 65535 * PTS_TILE  # FP_PTS_DIAMETER_MAX_V of the header


def pts_diameter_scratch_bytes(num_pts: int) -> int:
    """FP_PTS_DIAMETER_SCRATCH_BYTES of include/foundpose_amd.h."""
    tiles = (num_pts + PTS_TILE - 1) // PTS_TILE
    return 16 * (tiles * (tiles + 1) // 2)


def pts_hausdorff_scratch_bytes(num_pts: int, query_stride: int, num_transforms: int) -> int:
    """FP_PTS_HAUSDORFF_SCRATCH_BYTES of include/foundpose_amd.h."""
    nq = (num_pts + query_stride - 1) // query_stride
    return 16 * num_transforms * ((nq + PTS_TILE - 1) // PTS_TILE)


VSD_MAX_TAUS = 16  # FP_VSD_MAX_TAUS of the header


def vsd_scratch_bytes(num_pairs: int) -> int:
    """FP_VSD_SCRATCH_BYTES of include/foundpose_amd.h."""
    return 96 * num_pairs


def gt_vis_scratch_bytes(num_inst: int) -> int:
    """FP_GT_VIS_SCRATCH_BYTES of include/foundpose_amd.h."""
    return 80 * num_inst


DEPTH_MAX_PLANES, DEPTH_MAX_HYPOTHESES, DEPTH_MAX_PROPOSALS, DEPTH_PLANE_CHUNK = 4, 4096, 1024, 4096  # FP_DEPTH_* of the header


def depth_plane_scratch_bytes(num_frames: int, pixels: int, hypotheses: int) -> int:
    """FP_DEPTH_PLANE_SCRATCH_BYTES of include/foundpose_amd.h."""
    return (256 * num_frames + 16 * ((num_frames * pixels + 15) // 16) + 8 * ((num_frames * hypotheses + 1) // 2)
            + 64 * num_frames * ((pixels + DEPTH_PLANE_CHUNK - 1) // DEPTH_PLANE_CHUNK))


def depth_components_scratch_bytes(num_frames: int, pixels: int) -> int:
    """FP_DEPTH_COMPONENTS_SCRATCH_BYTES of include/foundpose_amd.h."""
    return 64 * num_frames + 4 * num_frames * pixels


def component_table_scratch_bytes(num_frames: int, pixels: int) -> int:
    """FP_COMPONENT_TABLE_SCRATCH_BYTES of include/foundpose_amd.h."""
    return 16 * num_frames + 28 * num_frames * pixels


TSDF_MAX_DIM, TSDF_MAX_VOXELS, TSDF_MAX_FRAMES, TSDF_FRAME_DOUBLES = 512, 1 << 27, 4096, 16  # FP_TSDF_* of the header
TSDF_DIFFUSE_MAX_ITERS = 4096  # FP_TSDF_DIFFUSE_MAX_ITERS


MESH_MAX_DIM, MESH_MAX_ROWS = 1 << 20, 2**31 - 1  # FP_MESH_* of the header


def tsdf_scratch_bytes(num_frames: int) -> int:
    """FP_TSDF_SCRATCH_BYTES of include/foundpose_amd.h."""
    return 8 * TSDF_FRAME_DOUBLES * num_frames


REFINE_CHUNK, REFINE_RECORD, REFINE_STATE_BYTES = 32, 32, 512  # FP_REFINE_* of the header


def refine_scratch_bytes(num_det: int, max_points: int) -> int:
    """FP_REFINE_SCRATCH_BYTES of include/foundpose_amd.h."""
    chunks = (max_points + REFINE_CHUNK - 1) // REFINE_CHUNK
    return REFINE_STATE_BYTES * num_det + 8 * REFINE_RECORD * num_det * chunks + ((num_det * max_points + 7) // 8) * 8 + 8


def depth_refine_scratch_bytes(num_det: int, max_points: int) -> int:
    """FP_DEPTH_REFINE_SCRATCH_BYTES of include/foundpose_amd.h."""
    chunks = (max_points + REFINE_CHUNK - 1) // REFINE_CHUNK
    return REFINE_STATE_BYTES * num_det + 8 * REFINE_RECORD * num_det * chunks + 8


def tsdf_track_scratch_bytes(num_det: int, max_points: int) -> int:
    """FP_TSDF_TRACK_SCRATCH_BYTES of include/foundpose_amd.h."""
    return depth_refine_scratch_bytes(num_det, max_points)


def multiview_scratch_bytes(num_det: int, max_points: int) -> int:
    """fp_multiview_refine's scratch: FP_DEPTH_REFINE_SCRATCH_BYTES of include/foundpose_amd.h, the same layout."""
    return depth_refine_scratch_bytes(num_det, max_points)


def mask_refine_scratch_bytes(num_det: int, max_points: int, max_contour: int) -> int:
    """FP_MASK_REFINE_SCRATCH_BYTES of include/foundpose_amd_mask_refine.h."""
    chunks = (max_points + REFINE_CHUNK - 1) // REFINE_CHUNK
    bchunks = (max_contour + REFINE_CHUNK - 1) // REFINE_CHUNK
    return (REFINE_STATE_BYTES * num_det + 8 * REFINE_RECORD * num_det * (chunks + bchunks) + 8 + 16 * num_det * max_points
            + ((num_det * max_points + 1) // 2) * 8)


def rgbd_refine_scratch_bytes(num_det: int, max_points: int) -> int:
    """FP_RGBD_REFINE_SCRATCH_BYTES of include/foundpose_amd.h."""
    chunks = (max_points + REFINE_CHUNK - 1) // REFINE_CHUNK
    return REFINE_STATE_BYTES * num_det + 16 * REFINE_RECORD * num_det * chunks + ((num_det * max_points + 7) // 8) * 8 + 8


PROPOSAL_MAX_SIZE, PROPOSAL_MAX_K, PROPOSAL_MAX_RANKED = 1024, 16, 4096  # FP_PROPOSAL_MAX_* of the header
APPEARANCE_MAX_DIM, APPEARANCE_MAX_PATCHES, APPEARANCE_MAX_PROPOSALS = 4096, 8192, 65535  # fp_proposal_appearance's limits
PROPOSAL_DECISIONS = ("candidate", "small", "empty", "no_object", "low_score", "group_limit")  # FP_PROPOSAL_CANDIDATE .. _GROUP_LIMIT


def proposal_score_scratch_bytes(num_prop: int, num_obj: int, dim: int, max_templates: int, k: int) -> int:
    """FP_PROPOSAL_SCORE_SCRATCH_BYTES of include/foundpose_amd.h."""
    up16 = lambda b: (b + 15) // 16 * 16
    rows = num_obj * num_prop
    return (up16(4 * cosine_scratch_floats(rows, max_templates)) + up16(4 * rows * dim) + 2 * up16(4 * (num_obj + 1)) + up16(4 * rows)
            + 2 * up16(4 * rows * k))


TEXTURE_MAX_SIDE = 16384  # FP_TEXTURE_MAX_SIDE of the header
VIS_MAX_MATCHES, VIS_MAX_DILATE = 1024, 8  # FP_VIS_MAX_MATCHES / FP_VIS_MAX_DILATE of the header


def texture_levels(width: int, height: int):
    """The pyramid layout of fp_texture_mips (include/foundpose_amd.h): [(texel offset, w, h)] per level, and the total."""
    out, off, w, h = [], 0, int(width), int(height)
    while True:
        out.append((off, w, h))
        off += w * h
        if w == 1 and h == 1:
            return out, off
        w, h = max(1, w >> 1), max(1, h >> 1)


def exported_symbols():
    return list(_SYMBOLS)


def call(name: str, *args, invalid=None) -> None:
    """Runs an entry point; a non-zero status raises FoundPoseNativeError.  invalid: the exception type a wrapper raises instead for status 1
    (an invalid argument) when the C entry's validation is its only one; the message is then the library's text alone."""
    rc = getattr(lib(), name)(*args)
    if rc == 1 and invalid is not None:
        raise invalid(lib().fp_last_error().decode())
    if rc != 0:
        raise FoundPoseNativeError(f"{name} failed (code {rc}): {lib().fp_last_error().decode()}")


def ptr(t) -> vp:
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return vp(0)
    return vp(t.data_ptr())


def stream() -> vp:
    return vp(torch.cuda.current_stream().cuda_stream)


def require_cuda(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise FoundPoseNativeError(
                "foundpose_amd runs on the MI355X only: got a CPU tensor (move inputs to 'cuda'; no CPU fallback exists)")


def upload_async(host: torch.Tensor, device) -> torch.Tensor:
    """A small host table -> device through pinned staging, asynchronously on the current stream.  A pageable upload (torch.tensor(..., device=),
    .to(device) of a pageable tensor) blocks the host until everything queued on the stream before it has drained -- a whole batch of the backbone --
    and the launches behind it then reach an idle GPU one launch latency at a time; the caching host allocator keeps the pinned block alive
    until the copy has run."""
    host = host.contiguous()
    staged = torch.empty(host.shape, dtype=host.dtype, pin_memory=True)
    staged.copy_(host)
    return staged.to(device, non_blocking=True)
