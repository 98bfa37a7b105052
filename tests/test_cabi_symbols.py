"""CPU: the C-ABI library loads and exports every symbol include/foundpose_amd.h declares; the ctypes prototypes follow from the header, and
what _lib.py still restates by hand (the ViT structs, the FP_* constants, the scratch-size formulas) equals what a C compiler reads in the header."""

import os
import re

import pytest


def test_library_exports_exactly_the_declared_symbols():
    import torch  # noqa: F401  (loads the HIP runtime the library links against)
    from foundpose_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from foundpose_amd import build
        build.build(verbose=False)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "foundpose_amd.h")).read()
    declared = set(re.findall(r"\b(fp_[a-z0-9_]+)\s*\(", header)) - {"fp_stream_t"}
    handle = _lib.lib()
    for name in sorted(declared):
        assert hasattr(handle, name), f"{name} declared in the header but not exported"
    assert declared == set(_lib.exported_symbols()), "ctypes prototypes out of sync with the header"
    assert handle.fp_abi_version() == _lib.ABI_VERSION == 20


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_text():
    """include/foundpose_amd.h without its comments."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(ROOT, "include", "foundpose_amd.h")).read(), flags=re.S)


def test_every_declaration_has_a_prototype_of_its_length():
    """_lib._PROTOS is derived from the header: one prototype per declared function, one entry per parameter (counted here on its own: the commas
    of the declaration), and the parser's type map pinned at a few fixed declarations."""
    import ctypes as C
    from foundpose_amd import _lib
    from foundpose_amd._lib import f64, i32, i64, u64, vp
    text = _header_text()
    declared = set(re.findall(r"\b(fp_[a-z0-9_]+)\s*\(", text))
    assert len(declared) == 89 and declared == set(_lib._PROTOS) | {"fp_last_error"} and "fp_last_error" not in _lib._PROTOS
    assert _lib.exported_symbols() == sorted(declared)
    for name, args in _lib._PROTOS.items():
        params = re.search(r"\b%s\s*\(([^()]*)\)\s*;" % name, text).group(1)
        count = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(args) == count, f"{name}: {len(args)} ctypes entries for {count} parameters"
    assert _lib._PROTOS["fp_abi_version"] == [] and len(_lib._PROTOS["fp_sqnorm_rows"]) == 5 and len(_lib._PROTOS["fp_gemm_resid_tile_rows"]) == 3
    spot = {"fp_sqnorm_rows": {0: vp, 1: i64, 2: i32, 3: vp, 4: vp}, "fp_pnp_ransac": {8: f64, 9: f64, 12: u64}, "fp_proposal_scores": {10: C.c_size_t},
            "fp_sample_bilinear": {0: vp, 1: i64, 2: i64, 3: i64, 4: i64, 5: i32}, "fp_normalize_rows": {3: _lib.f32},
            "fp_vit_forward": {0: C.POINTER(_lib.VitModel), 1: C.POINTER(_lib.VitWorkspace), 2: vp, 7: vp}, "fp_gemm_resid_tile_rows": {0: i32, 1: i32, 2: i32}}
    for name, expected in spot.items():
        for i, ty in expected.items():
            got = _lib._PROTOS[name][i]
            assert got is ty, f"{name}: parameter {i} is bound as {got.__name__}, this test pins {ty.__name__}"


@pytest.mark.parametrize("old, new, culprit", [
    ("int fp_sqnorm_rows(const float* x, int64_t n,", "int fp_sqnorm_rows(const float* x, long n,", r"fp_sqnorm_rows: parameter 'long n'"),
    ("int fp_sqnorm_rows(const float* x, int64_t n,", "int fp_sqnorm_rows(const float* x, unsigned int n,", r"fp_sqnorm_rows: parameter 'unsigned int n'"),
    ("int fp_sqnorm_rows(const float* x, int64_t n,", "int fp_sqnorm_rows(const float* x, int64_t,", r"fp_sqnorm_rows: parameter 'int64_t'"),
    ("int fp_sqnorm_rows(", "void fp_sqnorm_rows(", r"fp_sqnorm_rows returns 'void'"),
    ("int fp_sqnorm_rows(", "static inline int fp_sqnorm_rows(", r"fp_sqnorm_rows returns 'static inline int'"),
    ("float* out, fp_stream_t stream);\n\n/* out = x / max", "float* out, int (*done)(void), fp_stream_t stream);\n\n/* out = x / max", r"declaration of fp_sqnorm_rows"),
    ("#define FP_ABI_VERSION 20", "#define FP_ABI_VERSION (19 + 1)", r"FP_ABI_VERSION"),
])
def test_the_header_parser_does_not_guess(tmp_path, old, new, culprit):
    """What the parser cannot map raises, naming the declaration; nothing becomes c_void_p by default."""
    from foundpose_amd import _lib
    text = open(os.path.join(ROOT, "include", "foundpose_amd.h")).read()
    assert text.count(old) == 1
    path = tmp_path / "foundpose_amd.h"
    path.write_text(text.replace(old, new))
    with pytest.raises(_lib.FoundPoseNativeError, match=culprit):
        _lib._parse_header(str(path))
    with pytest.raises(_lib.FoundPoseNativeError, match="missing.h"):
        _lib._parse_header(str(tmp_path / "missing.h"))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/csrc/abi_probe.c: the header through a C compiler."""
    import ctypes as C
    import subprocess
    so = str(tmp_path_factory.mktemp("abi") / "libabi_probe.so")
    subprocess.check_call(["gcc", "-O1", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-o", so, os.path.join(ROOT, "tests", "csrc", "abi_probe.c")])
    lib = C.CDLL(so)

    def table(name, count, fields):
        row = type(name, (C.Structure,), {"_fields_": fields})
        return list((row * C.c_int.in_dll(lib, count).value).in_dll(lib, name))
    lib.fields = table("abi_fields", "abi_num_fields", [("type", C.c_char_p), ("field", C.c_char_p), ("offset", C.c_size_t), ("size", C.c_size_t)])
    lib.constants = {r.name.decode(): r.value for r in table("abi_constants", "abi_num_constants", [("name", C.c_char_p), ("value", C.c_double)])}
    lib.macros = [(r.name.decode(), r.arity) for r in table("abi_scratch_macros", "abi_num_scratch_macros", [("name", C.c_char_p), ("arity", C.c_int)])]
    lib.abi_scratch_values.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
    lib.abi_scratch_values.restype = None
    return lib


def test_vit_struct_mirrors_have_the_compilers_layout(probe):
    """sizeof, and name, order, offset and size of every field of the three structs that cross the ABI by pointer: the header's field list (read
    from its text), the compiler's layout (the probe) and the ctypes mirrors agree."""
    import ctypes as C
    from foundpose_amd import _lib
    text = _header_text()
    for ctype, mirror, size in (("fp_vit_block", _lib.VitBlock, 176), ("fp_vit_model", _lib.VitModel, 120), ("fp_vit_workspace", _lib.VitWorkspace, 104)):
        body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % ctype, text).group(1)
        in_header = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
        rows = [r for r in probe.fields if r.type.decode() == ctype]
        assert rows[0].field == b"" and rows[0].size == C.sizeof(mirror) == size, f"sizeof({ctype}) = {rows[0].size}, ctypes mirror {C.sizeof(mirror)}"
        compiled = [(r.field.decode(), r.offset, r.size) for r in rows[1:]]
        assert [f[0] for f in compiled] == in_header, f"{ctype}: the probe's field list is not the header's"
        mirrored = [(n, getattr(mirror, n).offset, getattr(mirror, n).size) for n, _ in mirror._fields_]
        assert mirrored == compiled, f"{ctype}: (field, offset, size) differ: " + str([(m, c) for m, c in zip(mirrored, compiled) if m != c][:2])


def test_mirrored_constants_equal_the_headers(probe):
    """Every FP_* constant _lib.py restates: the value the compiler sees.  (APPEARANCE_MAX_* have no macro in the header.)"""
    from foundpose_amd import _lib
    dtypes = ("FP_F32", "FP_BF16", "FP_FP8", "FP_F16X3", "FP_F16F8", "FP_F16")
    decisions = ["FP_PROPOSAL_" + d.upper() for d in _lib.PROPOSAL_DECISIONS]
    assert [probe.constants[d] for d in decisions] == list(range(6)), "PROPOSAL_DECISIONS is not in the order of the FP_PROPOSAL_* codes"
    mirrored = {n: v for n, v in vars(_lib).items() if n.isupper() and isinstance(v, (int, float)) and not n.startswith("APPEARANCE_MAX_")}
    assert {n if n in dtypes else "FP_" + n for n in mirrored} == set(probe.constants) - set(decisions), "a constant of _lib.py is not probed, or the reverse"
    for name, value in mirrored.items():
        c_name = name if name in dtypes else "FP_" + name
        assert value == probe.constants[c_name], f"_lib.{name} = {value}, {c_name} = {probe.constants[c_name]}"


_GRID = (1, 2, 7, 8, 9, 127, 128, 129, 300, 1000, 4097)
_TILES = ("FP_POSE_ERR_TILE", "FP_POSE_ADD_TILE", "FP_PTS_TILE", "FP_DEPTH_PLANE_CHUNK", "FP_REFINE_CHUNK")


def test_scratch_formulas_equal_the_headers_macros(probe):
    """Every FP_*_SCRATCH_BYTES / _FLOATS macro against the _lib function of the same name: the full grid for up to three arguments, a fixed-seed
    sample for five, and in every argument the first three multiples of every tile the macros round at, each -1, +0, +1.  fp_knn_l2, fp_cosine_topk*
    and fp_cyclic_buddies take no scratch size: for them the Python formula alone decides how much the kernels may write."""
    import itertools
    import random
    import numpy as np
    from foundpose_amd import _lib
    in_header = set(re.findall(r"#define\s+(FP_\w+_SCRATCH_(?:BYTES|FLOATS))\(", _header_text()))
    assert in_header == {m for m, _ in probe.macros} and len(probe.macros) == 19, in_header ^ {m for m, _ in probe.macros}
    edges = sorted({k * int(probe.constants[t]) + d for t in _TILES for k in (1, 2, 3) for d in (-1, 0, 1)})
    rng = random.Random(0)
    checked = 0
    for which, (macro, arity) in enumerate(probe.macros):
        fn = getattr(_lib, macro[3:].lower())
        tuples = list(itertools.product(_GRID, repeat=arity)) if arity <= 3 else [tuple(rng.choice(_GRID) for _ in range(arity)) for _ in range(300)]
        tuples += [tuple(e if j == i else other for j in range(arity)) for i in range(arity) for e in edges for other in (2, 129)]
        args = np.ascontiguousarray(tuples, dtype=np.intc)
        out = np.empty(len(tuples), np.uint64)
        probe.abi_scratch_values(which, len(tuples), args.ctypes.data, out.ctypes.data)
        for t, c in zip(tuples, out.tolist()):
            assert fn(*t) == c, f"_lib.{fn.__name__}{t} = {fn(*t)}, {macro}{t} = {c}"
        checked += len(tuples)
    assert checked > 10000


def test_product_never_imports_oracle():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foundpose_amd")
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".hpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f"{f} imports the oracle"
                assert "liboracle" not in src


def test_cpu_tensor_is_rejected_loudly():
    import torch
    from foundpose_amd import _lib, ops
    with pytest.raises(_lib.FoundPoseNativeError):
        ops.sqnorm_rows(torch.zeros(4, 8))


def test_bank_builder_entry_points_refuse_cpu_tensors_and_bad_names():
    """Host logic that needs no GPU: loud failures instead of silent CPU work."""
    import torch
    from foundpose_amd import cluster_util, feature_util, knn_util
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster_util.kmeans(torch.zeros(64, 8), 4, verbose=False)
    with pytest.raises(NotImplementedError):
        feature_util.make_feature_extractor("resnet50")                      # feature_util.py:18-23 in the reference
    with pytest.raises(AssertionError, match="should divide patch_size"):                    # dinov2_utils.py:378-380 in the reference
        feature_util.make_feature_extractor("dinov2_version=vits14-reg_stride=5_facet=token_layer=9_norm=1")
    assert feature_util.make_feature_extractor("dinov2_version=vits14-reg_stride=7_facet=token_layer=9_norm=1", random_init_seed=0).stride == 7
    with pytest.raises(NotImplementedError):
        feature_util.make_feature_extractor("dinov2_version=vits14-reg_stride=14_facet=attn_layer=9_norm=1")
    with pytest.raises(ValueError):
        knn_util.KNN(k=1, metric="manhattan").fit(torch.zeros(4, 4))         # knn_util.py:61-63 in the reference


def test_infer_driver_refuses_options_it_would_otherwise_ignore():
    """scripts/infer.py options the batched path does not implement are refused before any GPU work: a max_num_queries that could trigger the
    reference's random subsampling (infer.py:482-485), unknown matching / pose types.  (crop=False runs: tests/test_gpu_infer_driver.py.)"""
    from foundpose_amd import infer
    base = dict(version="v", repre_version="r", object_dataset="lmo")
    for bad, exc in ((dict(max_num_queries=500), NotImplementedError),
                     (dict(match_template_type="sift"), ValueError), (dict(match_feat_matching_type="1nn"), ValueError),
                     (dict(final_pose_type="refined"), ValueError)):
        with pytest.raises(exc):
            infer.infer_object(infer.InferOpts(**base, **bad), 1, None, [], {})
    assert infer.load_opts({"infer_opts": dict(base, crop_size=[420, 420])}).max_num_queries == 1000000


def test_oracle_topn_is_clamped_to_the_template_count():
    """torch.topk raises when there are fewer templates than top_n -- and so do the drop-in establish_correspondences / tfidf_matching
    (tests/test_gpu_matching.py::test_random_sweep_vs_oracle_both_tie_orders); the oracle, like the batched match_batch / engine, returns what exists."""
    import numpy as np
    from oracle import clib, match as om
    from oracle.make_golden import build_match_inputs
    c = dict(T=2, pmin=20, pmax=20, W=16, tpl=1, noise=0.05, top_n=5, top_k=10, soft=False, bank_seed=5, q_seed=6, dup=0)
    bank, centroids, pts, feats = build_match_inputs(c)
    r = om.build_synthetic_repre({k: v.numpy() for k, v in bank.items()}, centroids.numpy())
    out = om.establish_correspondences(pts.numpy(), feats.numpy(), r, 5, 10)
    assert [o["template_id"] for o in out][0] == 1 and len(out) == 2
    with pytest.raises(ValueError):
        clib.topk_torch(np.zeros(3, np.float32), 5)


def test_graft_entry_build_runs():
    """The driver's "does it build" hook: compiles what is stale (nothing, normally), loads the library, checks the ABI."""
    import __graft_entry__ as entry
    entry.build()


def test_library_and_package_read_no_environment_variable():
    """the library keeps no global mutable state and has no hidden switches.  It does not even IMPORT getenv (the A/B
    switches of measurements are explicit arguments -- fp_vit_model.flags, the variant bits of fp_attention*), and no Python file of the
    package reads an FP_* variable either (extractor / engine constructor arguments instead)."""
    import subprocess
    import torch  # noqa: F401
    from foundpose_amd import _lib
    _lib.lib()
    syms = subprocess.run(["nm", "-D", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "getenv" not in syms and "knn_cand" not in syms
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foundpose_amd")
    reads = [(fn, m) for fn in sorted(os.listdir(pkg)) if fn.endswith(".py")
             for m in re.findall(r"environ(?:\.get)?\W+[\"'](FP_[A-Z0-9_]+)[\"']", open(os.path.join(pkg, fn)).read())]
    assert not reads, f"package files read FP_* variables: {reads}"
