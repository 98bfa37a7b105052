"""The query-feature hand-off, kernel by kernel, against tests/sampling_ref.py: what sits between the ViT's feature map and the matcher.

A  fp_sample_bilinear (sample_bilinear_kernel): every map and point of the shared table, in three memory layouts, bit for bit against the
   restatement that tests/test_sampling_cpu.py holds to torch's grid_sample; the same rows for reordered, single and per-image launches.
B  the fused final norm + sampling (ln_sample_kernel) against forward()["feature_maps"] sampled by fp_sample_bilinear, on a non-square
   batch and at the two instantiations nothing else runs plainly: <4, 8> (dim 1536) and <2, 16> (dim 640).
C  fp_pca_project (the F32_EPI_SUB_VEC / F32_EPI_STORE epilogues of the fp32 tile engine) against the k-ascending fmaf chain.
D  fp_sqnorm_rows and fp_normalize_rows against oracle.clib.sqnorm and oracle.match.l2_normalize_rows.

Every comparison is on the bits."""
import numpy as np
import pytest
import torch

from foundpose_amd import _lib, feature_util, ops, projector_util, synthetic
from foundpose_amd._lib import ptr, stream
from foundpose_amd.dinov2_utils import DinoFeatureExtractor
from foundpose_amd.vit_config import VitArch
from oracle import clib
from oracle import match as om
from tests import sampling_ref as sr

pytestmark = pytest.mark.gpu

MAPS = list(range(len(sr.SAMPLE_MAPS)))
MAP_IDS = ["x".join(str(v) for v in m) for m in sr.SAMPLE_MAPS]
SENTINEL = 0x35
_CACHE = {}


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _assert_bits(got, want, what):
    """got: a tensor; want: a tensor or an fp32 numpy array.  Same shape, same dtype, same bytes (-0 is not +0, a NaN equals only itself)."""
    got = got.detach().cpu().contiguous()
    want = (torch.from_numpy(np.ascontiguousarray(want)) if isinstance(want, np.ndarray) else want.detach().cpu()).contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} against {want.dtype} {tuple(want.shape)}"
    if got.numel() == 0:
        return
    diff = (got.view(torch.uint8) != want.view(torch.uint8)).reshape(got.shape[0], -1)
    if bool(diff.any()):
        r, c = (int(v) for v in diff.nonzero()[0])
        raise AssertionError(f"{what}: {int(diff.any(1).sum())} of {got.shape[0]} rows differ, the first is row {r} (byte {c})")


def _case(i):
    """Map i of the table, its points and the restatement's rows: computed once, shared, never written."""
    if i not in _CACHE:
        fmap = sr.sample_map(i)
        pts, img, label = sr.sample_points(i)
        size = sr.SAMPLE_MAPS[i][4:]
        want, taps = sr.sample_bilinear(fmap, pts, img, size)
        _CACHE[i] = dict(fmap=fmap, pts=pts, img=img, label=label, size=size, want=want, taps=taps)
    return _CACHE[i]


# ------------------------------------------------------------------------------------------------ A: fp_sample_bilinear
def _layout(fmap, layout):
    """The map [B, C, H, W] on the device as: "bchw" contiguous; "token" the permuted view of a token-major [B, H W, C] buffer (stride_c == 1,
    what the extractor hands over); "slice" every other image and a channel slice of a larger tensor (the base pointer is offset and stride_img
    is not C H W; the images and channels around it hold other numbers)."""
    B, C, H, W = fmap.shape
    f = _dev(fmap)
    if layout == "bchw":
        v = f
    elif layout == "token":
        v = f.permute(0, 2, 3, 1).reshape(B, H * W, C).contiguous().reshape(B, H, W, C).permute(0, 3, 1, 2)
        assert v.stride(1) == 1 and (not v.is_contiguous() or C == 1)
    else:
        big = torch.randn(2 * B, C + 7, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) + 3.0
        big[::2, 3:3 + C] = f
        v = big[::2, 3:3 + C]
        assert v.stride(0) == 2 * (C + 7) * H * W and v.data_ptr() != big.data_ptr()
    assert v.shape == f.shape and torch.equal(v, f)
    return v


@pytest.mark.parametrize("layout", ["bchw", "token", "slice"])
@pytest.mark.parametrize("i", MAPS, ids=MAP_IDS)
def test_sample_bilinear_equals_the_restatement(i, layout):
    c = _case(i)
    v = _layout(c["fmap"], layout)
    img = None if c["img"] is None else _dev(c["img"])
    got = ops.sample_bilinear(v, _dev(c["pts"]), img, c["size"])
    _assert_bits(got, c["want"], f"sample_bilinear map {sr.SAMPLE_MAPS[i]} {layout}")
    none_out = ~c["taps"].valid.any(1)                      # all four taps outside: +0.0 in every channel
    assert not bool(got.cpu().view(torch.int32)[torch.from_numpy(none_out)].any())


@pytest.mark.parametrize("i", MAPS, ids=MAP_IDS)
def test_sample_bilinear_rows_do_not_depend_on_the_launch(i):
    """The points reversed; each of the first 16 points alone; the points of one image sampled with point_img=None from that image's
    [1, C, H, W] slice (of the contiguous tensor and of the strided view): always the rows of the whole launch."""
    c = _case(i)
    B = sr.SAMPLE_MAPS[i][0]
    f = _layout(c["fmap"], "bchw")
    pts = _dev(c["pts"])
    img = None if c["img"] is None else _dev(c["img"])
    want = c["want"]
    rev = ops.sample_bilinear(f, pts.flip(0).contiguous(), None if img is None else img.flip(0).contiguous(), c["size"])
    _assert_bits(rev, want[::-1], "points reversed")
    for p in range(16):
        one = ops.sample_bilinear(f, pts[p:p + 1], None if img is None else img[p:p + 1], c["size"])
        _assert_bits(one, want[p:p + 1], f"point {p} alone")
    sliced = _layout(c["fmap"], "slice")
    for b in range(B):
        sel = np.arange(sr.NUM_POINTS) if c["img"] is None else np.nonzero(c["img"] == b)[0]
        assert sel.size > 0
        for src in (f, sliced):
            got = ops.sample_bilinear(src[b:b + 1], pts[torch.from_numpy(sel).cuda()], None, c["size"])
            _assert_bits(got, want[sel], f"image {b} alone")


@pytest.mark.parametrize("i", [0, 1], ids=[MAP_IDS[0], MAP_IDS[1]])
def test_sample_feature_map_at_points_keeps_the_callers_device(i):
    c = _case(i)
    sel = np.arange(sr.NUM_POINTS) if c["img"] is None else np.nonzero(c["img"] == 0)[0]
    fmap_chw, pts = torch.from_numpy(c["fmap"][0]), torch.from_numpy(c["pts"][sel])
    out = feature_util.sample_feature_map_at_points(fmap_chw, pts, c["size"])
    assert not out.is_cuda
    _assert_bits(out, c["want"][sel], "CPU tensors in, CPU tensor out")
    out = feature_util.sample_feature_map_at_points(fmap_chw.cuda(), pts.cuda(), c["size"])
    assert out.is_cuda
    _assert_bits(out, c["want"][sel], "device tensors")


def test_sample_bilinear_of_no_points_is_empty():
    f = _layout(_case(1)["fmap"], "bchw")
    out = ops.sample_bilinear(f, torch.empty(0, 2, device="cuda"), torch.empty(0, dtype=torch.int32, device="cuda"), _case(1)["size"])
    assert out.shape == (0, f.shape[1]) and out.dtype == torch.float32 and out.is_cuda
    out = ops.sample_bilinear(f[:1], torch.empty(0, 2, device="cuda"), None, _case(1)["size"])
    assert out.shape == (0, f.shape[1])


# ------------------------------------------------------------------------------------------------ B: the fused final norm + sampling
WIDE1536 = VitArch("wide1536-reg", dim=1536, depth=2, heads=24, ffn="mlp", hidden=512, registers=4, pretrain_grid=4, interp_antialias=True, interp_offset=0.0)
WIDE640 = VitArch("wide640-reg", dim=640, depth=2, heads=10, ffn="mlp", hidden=512, registers=4, pretrain_grid=4, interp_antialias=True, interp_offset=0.0)


def _fused_against_unfused(ex, B, img_h, img_w, seed):
    """forward_hidden + sample_patch_features == forward()["feature_maps"] sampled by ops.sample_bilinear, and the latter == the restatement
    applied to the device's own feature map: together they hold ln_sample_kernel to torch's grid_sample on this batch."""
    gh, gw = img_h // 14, img_w // 14
    imgs = torch.rand(B, 3, img_h, img_w, generator=torch.Generator().manual_seed(seed)).cuda()
    pts_np, img_np, _ = sr.make_points(B, gh, gw, img_w, img_h, 7600 + seed)
    pts, img = _dev(pts_np), _dev(img_np)
    fmap = ex(imgs)["feature_maps"]
    assert fmap.shape == (B, ex.arch.dim, gh, gw) and fmap.stride(1) == 1
    want = ops.sample_bilinear(fmap, pts, img, (img_w, img_h))
    ref, taps = sr.sample_bilinear(fmap.cpu().numpy(), pts_np, img_np, (img_w, img_h))
    k = sr.classify(taps, gh, gw)
    assert min(int(k[n].sum()) for n in ("a", "bx", "by", "cx", "cy", "all_out")) >= sr.MIN_PER_CLASS and int(k["round_trip"].sum()) >= sr.MIN_ROUND_TRIP
    _assert_bits(want, ref, "sample_bilinear of the extractor's feature map against the restatement")
    ex.forward_hidden(imgs)
    got = ex.sample_patch_features(pts, img)
    _assert_bits(got, want, "fused final norm + sampling against the sampled feature map")
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0.1


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_fused_sampling_on_a_non_square_batch(precision):
    """Three images 126 wide and 84 high (a 9 x 6 grid), vits14-reg at layer 1: ln_sample_kernel<2, 4>."""
    ex = feature_util.make_feature_extractor("dinov2_version=vits14-reg_stride=14_facet=token_layer=1_norm=1", random_init_seed=8, precision=precision).to("cuda")
    _fused_against_unfused(ex, 3, 84, 126, 1)


@pytest.mark.parametrize("arch", [WIDE1536, WIDE640], ids=["dim1536-vec4x8", "dim640-vec2x16"])
def test_fused_sampling_at_the_wide_instantiations(arch):
    """dim 1536 (a multiple of 256 beyond 1024) -> ln_sample_kernel<4, 8>; dim 640 (no multiple of 256, beyond 512) -> ln_sample_kernel<2, 16>.
    A two-block architecture of that width, fp32, two images 84 wide and 56 high (a 6 x 4 grid)."""
    sd = synthetic.make_vit_state_dict(arch, seed=1)
    name = f"dinov2_version={arch.name}_stride=14_facet=token_layer=1_norm=1"
    ex = DinoFeatureExtractor(name, state_dict=sd, arch=arch, precision="fp32").to("cuda")
    _fused_against_unfused(ex, 2, 56, 84, 2)


# ------------------------------------------------------------------------------------------------ C: fp_pca_project
PCA_IDS = [f"{'x'.join(map(str, s))}-{'mean' if m else 'nomean'}" for s, m in sr.PCA_CASES]


def _projector(comps, mean):
    return projector_util.projector_from_tensordict({"pca_projector": {
        "components": torch.from_numpy(comps), "mean": torch.from_numpy(mean), "whiten": torch.tensor(False)}})


@pytest.mark.parametrize("shape,with_mean", sr.PCA_CASES, ids=PCA_IDS)
def test_pca_project_equals_the_fmaf_chain(shape, with_mean):
    x, comps, mean = sr.pca_case(shape, with_mean)
    want = sr.pca_project(x, comps, mean)
    xd, cd = _dev(x), _dev(comps)
    if not with_mean:
        _assert_bits(ops.pca_project(xd, cd, None), want, f"pca_project {shape}, no mean")
        return
    mean_proj = ops.pca_project(_dev(mean[None]), cd, None).reshape(-1).contiguous()
    _assert_bits(mean_proj, sr.chain_matrix(mean[None], comps)[0], f"mean projection {shape}")
    _assert_bits(ops.pca_project(xd, cd, mean_proj), want, f"pca_project {shape}")
    proj = _projector(comps, mean)
    first = proj.transform(xd)
    second = proj.transform(xd)                      # the cached device state
    assert len(proj._dev) == 1
    _assert_bits(first, want, f"PCAProjector.transform {shape}")
    _assert_bits(second, want, f"PCAProjector.transform {shape}, second call")
    for r in sorted({0, shape[0] // 2, shape[0] - 1}):             # a row alone: the chain of an output does not depend on the tile it sits in
        _assert_bits(ops.pca_project(xd[r:r + 1], cd, mean_proj), want[r:r + 1], f"pca_project {shape}, row {r} alone")


def test_project_features_chains_two_projectors():
    x, c1, m1 = sr.pca_case((133, 36, 100), True)
    rng = np.random.default_rng(7)
    c2 = rng.standard_normal((24, 100)).astype(np.float32)
    m2 = (3.0 * rng.standard_normal(100)).astype(np.float32)
    want = sr.pca_project(sr.pca_project(x, c1, m1), c2, m2)
    got = projector_util.project_features(_dev(x), [_projector(c1, m1), _projector(c2, m2)])
    _assert_bits(got, want, "two projectors in a row")


def test_pca_project_of_no_rows_is_empty():
    _, comps, mean = sr.pca_case((1, 48, 16), True)
    cd = _dev(comps)
    mean_proj = ops.pca_project(_dev(mean[None]), cd, None).reshape(-1).contiguous()
    for mp in (None, mean_proj):
        out = ops.pca_project(torch.empty(0, 48, device="cuda"), cd, mp)
        assert out.shape == (0, 16) and out.dtype == torch.float32 and out.is_cuda


def test_pca_project_refuses_a_row_length_off_the_float4_grid():
    """D = 50: the tile engine stages 16-byte pieces.  Refused by name, and nothing is written."""
    rng = np.random.default_rng(3)
    x, comps = _dev(rng.standard_normal((8, 50)).astype(np.float32)), _dev(rng.standard_normal((16, 50)).astype(np.float32))
    mean_proj = torch.zeros(16, device="cuda")
    for mp in (None, mean_proj):
        with pytest.raises(_lib.FoundPoseNativeError, match="f32_tile"):
            ops.pca_project(x, comps, mp)
        out = torch.empty(8 + 2, 16, device="cuda")
        out.view(torch.uint8).fill_(SENTINEL)
        rc = _lib.lib().fp_pca_project(ptr(x), 8, 50, ptr(comps), 16, ptr(mp), ptr(out[1:]), stream())
        torch.cuda.synchronize()
        assert rc != 0 and "f32_tile" in _lib.lib().fp_last_error().decode()
        assert bool((out.view(torch.uint8) == SENTINEL).all()), "refused, yet the output was written"


# ------------------------------------------------------------------------------------------------ D: row norms
@pytest.mark.parametrize("shape", sr.SQNORM_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sqnorm_rows_equals_the_oracle(shape):
    x = sr.sqnorm_case(shape)
    want = clib.sqnorm(x)
    xd = _dev(x)
    _assert_bits(ops.sqnorm_rows(xd), want, f"sqnorm_rows {shape}")
    for r in sorted({0, shape[0] // 2, shape[0] - 1}):
        _assert_bits(ops.sqnorm_rows(xd[r:r + 1]), want[r:r + 1], f"sqnorm_rows {shape}, row {r} alone")


@pytest.mark.parametrize("shape", sr.NORMALIZE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_normalize_rows_equals_the_oracle(shape):
    x, rows = sr.normalize_case(shape)
    with np.errstate(over="ignore"):
        want = om.l2_normalize_rows(x, sr.EPS)
    xd = _dev(x)
    got = ops.normalize_rows(xd, sr.EPS)
    _assert_bits(got, want, f"normalize_rows {shape}")
    assert bool(torch.isfinite(got[:len(rows)]).all()), "a special row (zero, below eps, one element, overflowing) is not finite"
    _assert_bits(ops.normalize_rows(xd), want, f"normalize_rows {shape}, default eps")
    for r in range(shape[0]):
        _assert_bits(ops.normalize_rows(xd[r:r + 1], sr.EPS), want[r:r + 1], f"normalize_rows {shape}, row {r} alone")


def test_row_norms_refusals_and_empty_inputs():
    with pytest.raises(_lib.FoundPoseNativeError, match="sqnorm_rows"):
        ops.sqnorm_rows(torch.ones(3, 6, device="cuda"))
    out = ops.sqnorm_rows(torch.empty(0, 8, device="cuda"))
    assert out.shape == (0,) and out.dtype == torch.float32 and out.is_cuda
    out = ops.normalize_rows(torch.empty(0, 7, device="cuda"))
    assert out.shape == (0, 7) and out.dtype == torch.float32 and out.is_cuda
