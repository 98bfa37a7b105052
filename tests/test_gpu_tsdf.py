"""GPU: fp_tsdf_integrate, fp_tsdf_count_triangles and fp_tsdf_emit_triangles (csrc/tsdf.hip) against the numpy restatement
tests/tsdf_ref.py, on the fixtures whose conditions tests/test_reconstruct_cpu.py checks: shapes ragged against the 256-thread
workgroups, more than one workgroup, and every branch of the per-frame decision."""
import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops
from tests import tsdf_ref as ref

pytestmark = pytest.mark.gpu
PLANES = ("sdf_sum", "sdf_cnt", "rgb_sum", "rgb_cnt")


@pytest.fixture(scope="module")
def fixture():
    fx = ref.integrate_fixture()
    want = ref.new_volume(fx["origin"], fx["h"], fx["dims"])
    ref.integrate(want, fx["depth"], fx["mask"], fx["rgb"], fx["cams"], fx["poses"], fx["tau"])
    for a in want.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    dev = {k: torch.from_numpy(fx[k]).cuda() for k in ("depth", "mask", "rgb")}
    return fx, want, dev


def _integrate(fx, dev, splits):
    vol = ops.tsdf_new_volume(fx["origin"], fx["h"], fx["dims"])
    for a, b in splits:
        ops.tsdf_integrate(vol, dev["depth"][a:b], dev["mask"][a:b], dev["rgb"][a:b], fx["cams"][a:b], fx["poses"][a:b], fx["tau"])
    return vol


def test_integrate_equals_the_restatement(fixture):
    fx, want, dev = fixture
    assert fx["dims"] == (37, 29, 23) and fx["depth"].shape == (5, 80, 96)
    got = {k: v.cpu().numpy() for k, v in _integrate(fx, dev, [(0, 5)]).items() if k in PLANES}
    assert np.array_equal(got["sdf_cnt"], want["sdf_cnt"]) and np.array_equal(got["rgb_cnt"], want["rgb_cnt"])
    tol = 5 * 2.0 ** -23                       # one fp32 rounding of a value <= 1 per frame: s / tau may differ in its last bit
    for name in ("sdf_sum", "rgb_sum"):
        err = np.abs(got[name].astype(np.float64) - want[name].astype(np.float64)).max()
        print(name, "largest difference", err, "of", tol, "; differing entries", int((got[name] != want[name]).sum()))
        assert err <= tol
    assert want["sdf_cnt"].max() == 5 and want["rgb_cnt"].sum() > 1000


def test_integrate_is_bit_identical_however_the_frames_are_split(fixture):
    fx, _, dev = fixture
    one, two = _integrate(fx, dev, [(0, 5)]), _integrate(fx, dev, [(0, 2), (2, 5)])
    for name in PLANES:
        assert torch.equal(one[name], two[name]), name


def _to_device(vol):
    out = dict(vol)
    for k in PLANES:
        out[k] = torch.from_numpy(np.ascontiguousarray(vol[k])).cuda()
    return out


def test_count_and_emit_equal_the_restatement():
    vol = ref.extract_fixture()
    assert vol["dims"] == (33, 18, 9)
    w_counts, w_keys, w_pos, w_col = ref.extract(vol, ref.EXTRACT_MIN_COUNT)
    counts, keys, pos, col = (t.cpu().numpy() for t in ops.tsdf_extract(_to_device(vol), ref.EXTRACT_MIN_COUNT))
    assert counts.dtype == np.int32 and np.array_equal(counts, w_counts)
    assert len(keys) == len(w_keys) == 3 * int(w_counts.sum()) and set(keys.tolist()) == set(w_keys.tolist())
    # per key one position and one colour, whichever tetrahedron wrote it; then key by key against the restatement
    order, w_order = np.argsort(keys, kind="stable"), np.argsort(w_keys, kind="stable")
    assert np.array_equal(keys[order], w_keys[w_order])
    first = np.concatenate([[True], np.diff(keys[order]) != 0])
    group = np.cumsum(first) - 1
    assert np.array_equal(pos[order], pos[order][first][group]) and np.array_equal(col[order], col[order][first][group])
    ulp = np.spacing(np.float32(np.abs(w_pos).max()))
    d_pos, d_col = np.abs(pos[order].astype(np.float64) - w_pos[w_order]).max(), np.abs(col[order].astype(np.float64) - w_col[w_order]).max()
    print("positions differ by at most", d_pos, "of", 2 * ulp, "; colours by", d_col)
    assert d_pos <= 2 * ulp and d_col <= 1e-6
    assert np.array_equal(keys, w_keys)            # ... and in the contract's order: cells, tetrahedra, case table


def test_sphere_volume_is_closed_oriented_and_within_the_bound():
    vol = ref.sphere_volume()
    counts, keys, pos, col = (t.cpu().numpy() for t in ops.tsdf_extract(_to_device(vol), 2))
    v, _, faces = ref.weld(keys, pos, col)
    topo = ref.topology(faces)
    assert topo["boundary_edges"] == 0 and topo["nonmanifold_edges"] == 0 and topo["inconsistent"] == 0
    assert topo["vertices"] - topo["edges"] + topo["faces"] == 2 and ref.signed_volume(v, faces) > 0
    miss = np.abs(np.linalg.norm(v[np.unique(faces)].astype(np.float64), axis=1) - 40.0).max()
    print("largest distance to the sphere", miss, "bound", ref.sphere_bound())
    assert miss <= ref.sphere_bound()
    assert np.all(col == np.float32(0.5))          # no colour was ever added


def test_refusals_write_nothing(fixture):
    fx, _, dev = fixture
    vol = _integrate(fx, dev, [(0, 1)])
    before = {k: vol[k].clone() for k in PLANES}
    args = lambda **kw: {**dict(volume=vol, depth=dev["depth"], mask=dev["mask"], rgb=dev["rgb"], cams=fx["cams"], poses=fx["poses"],   # noqa: E731
                                trunc_mm=fx["tau"]), **kw}
    refused = (ValueError, _lib.FoundPoseNativeError)
    for bad in (args(mask=dev["mask"][:4]), args(depth=dev["depth"][:, :79]), args(depth=dev["depth"].cpu()), args(rgb=dev["rgb"][..., :2]),
                args(trunc_mm=0.0), args(trunc_mm=-1.0), args(trunc_mm=float("nan")), args(cams=fx["cams"][:4]),
                args(cams=np.where(np.arange(4) == 0, -1.0, fx["cams"])), args(poses=torch.from_numpy(fx["poses"]).cuda()),
                args(volume={**vol, "dims": (37, 29, 24)}), args(volume={**vol, "sdf_cnt": vol["sdf_cnt"].cpu()}),
                args(volume={**vol, "voxel_mm": 0.0})):
        with pytest.raises(refused):
            ops.tsdf_integrate(**bad)
    for dims in ((513, 2, 2), (2, 513, 2), (2, 2, 513), (2 ** 27 + 1, 1, 1), (0, 4, 4)):   # 512^3 = 2^27: a volume past the voxel limit is past a dimension's too
        with pytest.raises(refused):
            ops.tsdf_new_volume((0, 0, 0), 1.0, dims)
    assert ops.tsdf_new_volume((0, 0, 0), 1.0, (4, 3, 2))["rgb_sum"].shape == (3, 2, 3, 4)
    for mc in (0, -1, 1.5, True):
        with pytest.raises(refused):
            ops.tsdf_extract(vol, mc)
    with pytest.raises(refused):
        ops.tsdf_extract(ops.tsdf_new_volume((0, 0, 0), 1.0, (1, 8, 8)), 1)
    # the C entries refuse on their own, before any launch
    L, vp, box = _lib.lib(), _lib.vp, np.array([0.0, 0.0, 0.0, 1.0])
    p = lambda t: _lib.ptr(t)   # noqa: E731
    fr = np.ascontiguousarray(np.concatenate([fx["cams"], fx["poses"]], 1))
    scratch = torch.empty(_lib.tsdf_scratch_bytes(5), dtype=torch.uint8, device="cuda")
    def integrate(nx=37, ny=29, nz=23, tau=10.0, nbytes=scratch.numel(), frames=5, box=box):   # noqa: E306
        return L.fp_tsdf_integrate(p(dev["depth"]), p(dev["mask"]), p(dev["rgb"]), frames, 80, 96, fr.ctypes.data_as(vp), box.ctypes.data_as(vp), nx, ny, nz,
                                   tau, p(scratch), nbytes, p(vol["sdf_sum"]), p(vol["sdf_cnt"]), p(vol["rgb_sum"]), p(vol["rgb_cnt"]), _lib.stream())
    for kw in (dict(nx=513), dict(nz=0), dict(tau=0.0), dict(nbytes=scratch.numel() - 1), dict(frames=0), dict(frames=_lib.TSDF_MAX_FRAMES + 1),
               dict(box=np.array([0.0, 0.0, np.inf, 1.0])), dict(box=np.array([0.0, 0.0, 0.0, -1.0]))):
        assert integrate(**kw) == 1 and b"fp_tsdf_integrate" in L.fp_last_error(), kw
    counts = torch.zeros(36 * 28 * 22, dtype=torch.int32, device="cuda")
    assert L.fp_tsdf_count_triangles(p(vol["sdf_sum"]), p(vol["sdf_cnt"]), 37, 29, 23, 0, p(counts), _lib.stream()) == 1
    assert L.fp_tsdf_count_triangles(p(vol["sdf_sum"]), p(vol["sdf_cnt"]), 37, 1, 23, 1, p(counts), _lib.stream()) == 1
    assert L.fp_tsdf_emit_triangles(p(vol["sdf_sum"]), p(vol["sdf_cnt"]), p(vol["rgb_sum"]), p(vol["rgb_cnt"]), box.ctypes.data_as(vp), 37, 29, 23, 1,
                                    p(counts), -1, None, None, None, _lib.stream()) == 1
    torch.cuda.synchronize()
    assert all(torch.equal(vol[k], before[k]) for k in PLANES) and int(counts.sum()) == 0
    assert _lib.tsdf_scratch_bytes(3) == 3 * 128
