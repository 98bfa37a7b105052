"""GPU: fp_tsdf_diffuse (csrc/tsdf_fill.hip) and reconstruct.fill_volume against the numpy restatement tests/tsdf_fill_ref.py, bit for
bit, on the fixtures whose conditions tests/test_tsdf_fill_cpu.py checks: rows ragged against the waves and rows of whole 16-byte
pieces, more than one workgroup, volumes one voxel thin, NaN stored where nothing is known."""
import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops, reconstruct
from tests import tsdf_fill_ref as fill, tsdf_ref as ref

pytestmark = pytest.mark.gpu
DIMS = ((37, 29, 23), (70, 9, 1), (3, 3, 3), (40, 7, 5))           # the issue's three, and one with nx % 4 == 0: the 16-byte path
ITERS = (0, 1, 2, 3, 4, 5, 9)
PLANES = ("sdf_sum", "sdf_cnt", "rgb_sum", "rgb_cnt")
REFUSED = (ValueError, _lib.FoundPoseNativeError)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def wanted():
    """Per dims: the fixture and the restatement's (values of three channels, states) after every iteration count of ITERS."""
    out = {}
    for dims in DIMS:
        val, state = fill.diffuse_fixture(dims)
        at, v, s = {0: (val, state)}, val, state
        for t in range(1, max(ITERS) + 1):
            v, s = fill.diffuse_once(v, s)
            at[t] = (v, s)
        for v, s in at.values():
            v.setflags(write=False), s.setflags(write=False)
        out[dims] = at
    return out


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("dims", DIMS)
def test_kernel_equals_the_restatement_bit_for_bit(wanted, dims, channels):
    val0, state0 = wanted[dims][0]
    val, state = torch.from_numpy(val0[:channels].copy()).cuda(), torch.from_numpy(state0.copy()).cuda()
    for t in ITERS:
        v, s = ops.tsdf_diffuse(val, state, t)
        w_v, w_s = wanted[dims][t]
        assert tuple(v.shape) == (channels, dims[2], dims[1], dims[0]) and v.dtype == torch.float32 and s.dtype == torch.uint8
        assert np.array_equal(s.cpu().numpy(), w_s), (dims, channels, t)
        assert np.array_equal(_bits(v.cpu().numpy()), _bits(w_v[:channels])), (dims, channels, t)   # NaN payloads at T = 0 and the sign of zero too
    assert np.array_equal(_bits(val.cpu().numpy()), _bits(val0[:channels])) and np.array_equal(state.cpu().numpy(), state0)   # the arguments are left alone


@pytest.mark.parametrize("dims", DIMS)
def test_iterations_split_into_calls_give_the_same_bits(wanted, dims):
    val0, state0 = wanted[dims][0]
    for channels in (1, 3):
        val, state = torch.from_numpy(val0[:channels].copy()).cuda(), torch.from_numpy(state0.copy()).cuda()
        one = ops.tsdf_diffuse(val, state, 5)
        v, s = val, state
        for _ in range(5):
            v, s = ops.tsdf_diffuse(v, s, 1)
        two = ops.tsdf_diffuse(*ops.tsdf_diffuse(val, state, 2), 3)
        for got in ((v, s), two):
            assert torch.equal(got[1], one[1]) and torch.equal(got[0].view(torch.int32), one[0].view(torch.int32))


def test_refusals_write_nothing(wanted):
    val0, state0 = wanted[(37, 29, 23)][0]
    val, state = torch.from_numpy(val0.copy()).cuda(), torch.from_numpy(state0.copy()).cuda()
    bad_state = state.clone()
    bad_state[3, 4, 5] = 3
    for kw in (dict(val=val.cpu()), dict(state=state.cpu()), dict(val=val.double()), dict(state=state.int()), dict(val=val[:2]), dict(val=val[0]),
               dict(state=state[:-1]), dict(state=bad_state), dict(iters=-1), dict(iters=4097), dict(iters=1.5), dict(iters=True),
               dict(val=torch.zeros(1, 1, 1, 513, device="cuda"), state=torch.zeros(1, 1, 513, dtype=torch.uint8, device="cuda"))):
        with pytest.raises(REFUSED):
            ops.tsdf_diffuse(**{**dict(val=val, state=state, iters=1), **kw})
    # the C entry refuses on its own, before any launch
    L, p = _lib.lib(), _lib.ptr
    v, s = val.clone(), state.clone()
    vt, st = torch.zeros_like(v), torch.zeros_like(s)
    def run(val=v, state=s, val_tmp=vt, state_tmp=st, channels=3, nx=37, ny=29, nz=23, iters=1):   # noqa: E306
        return L.fp_tsdf_diffuse(p(val) if val is not None else None, p(state), p(val_tmp), p(state_tmp), channels, nx, ny, nz, iters, _lib.stream())
    for kw in (dict(val=None), dict(val_tmp=v), dict(state_tmp=s), dict(channels=2), dict(channels=0), dict(nx=0), dict(nx=513), dict(iters=-1),
               dict(iters=4097)):
        assert run(**kw) == 1 and b"fp_tsdf_diffuse" in L.fp_last_error(), kw
    assert run(iters=0) == 0                                          # zero iterations touch nothing, the scratch included
    torch.cuda.synchronize()
    assert torch.equal(v.view(torch.int32), val.view(torch.int32)) and torch.equal(s, state) and int(vt.abs().sum()) == 0 and int(st.sum()) == 0
    with pytest.raises(REFUSED):
        reconstruct.fill_volume(ops.tsdf_new_volume((0, 0, 0), 1.0, (2, 8, 8)), {"fill": "carve"})


@pytest.fixture(scope="module")
def fused():
    """The integrate fixture fused by ops.tsdf_integrate (DESIGN.md section 29 pins it), on the device and as numpy."""
    fx = ref.integrate_fixture()
    vol = ops.tsdf_new_volume(fx["origin"], fx["h"], fx["dims"])
    ops.tsdf_integrate(vol, *(torch.from_numpy(fx[k]).cuda() for k in ("depth", "mask", "rgb")), fx["cams"], fx["poses"], fx["tau"])
    host = {k: (v.cpu().numpy() if k in PLANES else v) for k, v in vol.items()}
    for k in PLANES:
        host[k].setflags(write=False)
    return vol, host


@pytest.mark.parametrize("plane", (None, (0.0, 0.3, -1.0, -14.0)))
def test_fill_volume_equals_the_restatement_and_closes_the_surface(fused, plane):
    vol, host = fused
    before = {k: vol[k].clone() for k in PLANES}
    opts = {"fill": "carve", "fill_plane": plane}
    out, st = reconstruct.fill_volume(vol, opts)
    want, w_st = fill.fill_volume(host, 2, 4, 64, plane)
    assert all(torch.equal(vol[k], before[k]) for k in PLANES)        # the input is left as it is
    for k in PLANES:
        got = out[k].cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(_bits(got), _bits(want[k])), k
    seconds = st.pop("seconds")
    print("plane", plane, "stats", st, "seconds", seconds)
    assert st == w_st and seconds > 0 and st["filled_voxels"] > 0 and (st["plane_voxels"] > 0) == (plane is not None)
    # closed, on the kernel's own output through the extraction kernels
    _, keys, pos, col = (t.cpu().numpy() for t in ops.tsdf_extract(out, 1))
    v, c, faces = ref.weld(keys, pos, col)
    topo = ref.topology(faces)
    assert topo["boundary_edges"] == 0 and topo["nonmanifold_edges"] == 0 and topo["inconsistent"] == 0 and ref.signed_volume(v, faces) > 0
    assert not np.any(np.all(c[np.unique(faces)] == np.float32(0.5), axis=1))
    # every vertex of the unfilled surface between two voxels off the outer layer is there still, with the same bits
    _, keys0, pos0, _ = (t.cpu().numpy() for t in ops.tsdf_extract(vol, 2))
    nx, ny, nz = host["dims"]
    lo = keys0 // 7
    ijk = np.stack([lo % nx, (lo // nx) % ny, lo // (nx * ny)], 1)
    hi = ijk + np.array(ref.DIRECTIONS)[keys0 % 7]
    inner = np.all((ijk >= 1) & (hi <= np.array([nx, ny, nz]) - 2), axis=1)
    assert inner.sum() > 1000
    at = {int(k): p.tobytes() for k, p in zip(keys, pos)}
    assert all(at.get(int(k)) == p.tobytes() for k, p in zip(keys0[inner], pos0[inner]))
