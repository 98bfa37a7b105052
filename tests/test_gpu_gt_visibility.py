"""GPU: fp_gt_visibility (csrc/gt_info.hip) against the numpy restatement tests/gt_info_ref.py on arrays made with torch, no rasterizer
involved: counts, all eight box entries and both masks byte for byte; the float32 delta boundary; ragged boxes over several workgroups;
batch order, split and repetition; every output byte defined; refused calls writing nothing."""
import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops
from tests import gt_info_ref as ref

pytestmark = pytest.mark.gpu
W, H, WR, HR = 40, 30, 120, 90
OX, OY = 40, 30
K = (60.3, 61.1, 19.7, 14.2)            # fx, fy, cx, cy: a non-integer principal point
DELTA = 15.0


def _tight(a):
    ys, xs = np.nonzero(a)
    return (0, 0, -1, -1) if xs.size == 0 else (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))


def _build():
    """Five instances over two depth images.  0: a disc across the image's left and top edges; 1: a rectangle entirely in the margin;
    2: an empty render with an empty scan box; 3: a disc and a margin piece, scanned over the full window (10 800 pixels: eleven
    workgroups, the last one ragged); 4: a sloped rectangle over an occluder strip and a hole, in a window whose image sits at another
    offset, with a 37 x 29 box (1 073 pixels: one pixel row into a second workgroup)."""
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(HR, dtype=torch.float32), torch.arange(WR, dtype=torch.float32), indexing="ij")
    test = torch.full((2, H, W), 1500.0)
    test[0, 10:14, :] = 800.0                                   # an occluder strip
    test[0, 18:26, 22:34] = 0.0                                 # a hole
    test[1] = 1000.0 + 3.0 * torch.arange(W, dtype=torch.float32)[None, :] + torch.rand(H, W, generator=g) * 40.0 - 20.0
    test[1, 5:9, 10:30] = 0.0
    test[1, 20:24, :] = 700.0
    large = torch.zeros(5, HR, WR)
    disc = (xx - (OX + 2)) ** 2 + (yy - (OY + 3)) ** 2 <= 81.0
    large[0][disc] = (900.0 + 2.0 * xx + yy)[disc]
    large[1, 5:21, 90:111] = 1200.0
    disc3 = (xx - 61.5) ** 2 + (yy - 47.0) ** 2 <= 200.0
    large[3][disc3] = (1000.0 + 3.0 * (xx - OX) + 0.5 * yy)[disc3]      # within +-delta of test[1] here and there
    large[3, 80:88, 3:30] = 950.0
    large[4, 60:89, 81:118] = (990.0 + 1.5 * (xx - 80) + 0.7 * (yy - 60))[60:89, 81:118]
    inst = np.array([(0,) + _tight(large[0].numpy()) + (OX, OY),
                     (1,) + _tight(large[1].numpy()) + (OX, OY),
                     (1, 7, 9, 6, 20, OX, OY),
                     (1, 0, 0, WR - 1, HR - 1, OX, OY),
                     (0,) + _tight(large[4].numpy()) + (80, 60)], np.int64)
    params = np.array([K + (DELTA,)] * 5, np.float64)
    params[3, 4] = 12.5
    want = [ref.gt_visibility(test[r[0]].numpy(), large[p].numpy(), np.array([[q[0], 0, q[2]], [0, q[1], q[3]], [0, 0, 1]]), q[4], r[5], r[6])
            for p, (r, q) in enumerate(zip(inst, params))]
    return dict(test=test, large=large, inst=inst, params=params, rows=np.stack([w[0] for w in want]),
                mask=np.stack([w[1] for w in want]), visib=np.stack([w[2] for w in want]))


@pytest.fixture(scope="module")
def batch():
    b = _build()     # the restatement runs once, here
    return dict(b, test=b["test"].cuda(), large=b["large"].cuda())


def _run(b, sel=(0, 1, 2, 3, 4)):
    sel = list(sel)
    out, mask, visib = ops.gt_visibility(b["test"], b["large"][torch.tensor(sel, device="cuda")], b["inst"][sel], b["params"][sel])
    return out.cpu().numpy(), mask.cpu().numpy(), visib.cpu().numpy()


def test_counts_boxes_and_masks_equal_the_restatement(batch):
    rows, mask, visib = _run(batch)
    want = batch["rows"]
    # the cases the fixture is built for are really there
    assert want[0][3] < 0 and want[0][4] < 0 and 0 < want[0][2] < want[0][0]                        # across the left and top edges
    assert want[1].tolist() == [16 * 21, 0, 0, 50, -25, 70, -10] + ref.EMPTY_BOX                    # entirely in the margin
    assert want[2].tolist() == [0, 0, 0] + ref.EMPTY_BOX + ref.EMPTY_BOX                            # nothing scanned
    assert 0 < want[3][2] < want[3][1] and want[3][0] > want[3][1]                                  # occluded in part, margin counted
    assert want[4].tolist() == [1073, 1073 - 96, 1073 - 148, 1, 0, 37, 28, 1, 0, 37, 28]           # hole: visible, not valid; strip: hidden
    assert rows.dtype == np.int32 and mask.dtype == np.uint8 and rows.shape == (5, 11) and mask.shape == (5, H, W)
    for p in range(5):
        print(p, rows[p].tolist(), want[p].tolist())
    assert np.array_equal(rows.astype(np.int64), want)
    assert np.array_equal(mask, batch["mask"]) and np.array_equal(visib, batch["visib"])
    assert set(np.unique(mask)) <= {0, 255} and (visib <= mask).all() and (visib != mask).any()


def test_delta_boundary_is_decided_in_float32():
    """At an integer principal point dist = depth exactly: 1015 mm against 1000 mm is visible at delta 15, the next float32 is not."""
    test = torch.full((1, H, W), 1000.0, device="cuda")
    large = torch.zeros(2, HR, WR)
    above = np.nextafter(np.float32(1015), np.float32(2000))
    large[0, OY + 15, OX + 20], large[1, OY + 15, OX + 20] = 1015.0, float(above)
    inst = [(0, OX + 20, OY + 15, OX + 20, OY + 15, OX, OY)] * 2
    params = [(60.0, 61.0, 20.0, 15.0, 15.0)] * 2
    rows, mask, visib = ops.gt_visibility(test, large.cuda(), inst, params)
    rows = rows.cpu().numpy()
    assert rows[0].tolist() == [1, 1, 1, 20, 15, 20, 15, 20, 15, 20, 15]
    assert rows[1].tolist() == [1, 1, 0, 20, 15, 20, 15] + ref.EMPTY_BOX
    assert mask[:, 15, 20].tolist() == [255, 255] and visib[:, 15, 20].tolist() == [255, 0] and int(visib.sum()) == 255
    Kc = np.array([[60.0, 0, 20.0], [0, 61.0, 15.0], [0, 0, 1]])
    for p in range(2):
        assert np.array_equal(ref.gt_visibility(test[0].cpu().numpy(), large[p].numpy(), Kc, 15.0, OX, OY)[0], rows[p].astype(np.int64))


def test_same_results_reversed_split_and_repeated(batch):
    a = _run(batch)
    b = _run(batch)
    rev = _run(batch, (4, 3, 2, 1, 0))
    first, second = _run(batch, (0, 1)), _run(batch, (2, 3, 4))
    singles = [_run(batch, (p,)) for p in range(5)]
    for k in range(3):
        assert np.array_equal(a[k], b[k])
        assert np.array_equal(a[k], rev[k][::-1])
        assert np.array_equal(a[k], np.concatenate([first[k], second[k]]))
        assert np.array_equal(a[k], np.concatenate([s[k] for s in singles]))


def _raw(b, out, mask, visib, scratch, inst=None, params=None, n=None, num_test=2, h=H, w=W, hr=HR, wr=WR, nbytes=None, null=None):
    inst = np.ascontiguousarray(b["inst"] if inst is None else inst, np.int32)
    params = np.ascontiguousarray(b["params"] if params is None else params, np.float64)
    ptrs = [_lib.ptr(b["test"]), _lib.ptr(b["large"]), _lib.ptr(scratch), _lib.ptr(out), _lib.ptr(mask), _lib.ptr(visib)]
    if null is not None:
        ptrs[null] = _lib.vp(0)
    return _lib.lib().fp_gt_visibility(ptrs[0], num_test, h, w, ptrs[1], hr, wr, inst.ctypes.data_as(_lib.vp), params.ctypes.data_as(_lib.vp),
                                       len(inst) if n is None else n, ptrs[2], scratch.numel() if nbytes is None else nbytes, ptrs[3], ptrs[4],
                                       ptrs[5], _lib.stream())


def _buffers():
    return (torch.full((5, 11), -7, dtype=torch.int32, device="cuda"), torch.full((5, H, W), 0xAB, dtype=torch.uint8, device="cuda"),
            torch.full((5, H, W), 0xCD, dtype=torch.uint8, device="cuda"), torch.zeros(4096, dtype=torch.uint8, device="cuda"))


def test_every_output_byte_is_defined_over_garbage(batch):
    out, mask, visib, scratch = _buffers()
    assert _raw(batch, out, mask, visib, scratch) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().astype(np.int64), batch["rows"])
    assert np.array_equal(mask.cpu().numpy(), batch["mask"]) and np.array_equal(visib.cpu().numpy(), batch["visib"])
    assert (mask[2] == 0).all() and (mask[1] == 0).all()         # nothing scanned / nothing inside the image: zero all the same


def test_invalid_arguments_raise_and_write_nothing(batch):
    out, mask, visib, scratch = _buffers()
    inst, params = batch["inst"], batch["params"]

    def edited(table, row, col, v):
        t = table.copy()
        t[row, col] = v
        return t
    bad_inst = [(0, 0, 2), (1, 0, -1),                               # test index out of range
                (0, 1, -1), (0, 2, -1), (3, 3, WR), (3, 4, HR), (1, 1, 112), (1, 2, 22),   # box outside the render / x0 > x1 + 1
                (0, 5, -1), (0, 6, -1), (0, 5, WR - W + 1), (4, 6, HR - H + 1)]            # window outside the render
    bad_par = [(0, 0, 0.0), (1, 1, -2.0), (2, 0, np.nan), (3, 4, np.nan)]
    rcs = [_raw(batch, out, mask, visib, scratch, inst=edited(inst, *e)) for e in bad_inst]
    rcs += [_raw(batch, out, mask, visib, scratch, params=edited(params, *e)) for e in bad_par]
    rcs += [_raw(batch, out, mask, visib, scratch, n=0), _raw(batch, out, mask, visib, scratch, n=-1), _raw(batch, out, mask, visib, scratch, nbytes=399),
            _raw(batch, out, mask, visib, scratch, h=0), _raw(batch, out, mask, visib, scratch, num_test=0),
            _raw(batch, out, mask, visib, scratch, hr=65536, wr=32768)]
    rcs += [_raw(batch, out, mask, visib, scratch, null=k) for k in range(6)]
    torch.cuda.synchronize()
    assert rcs == [1] * len(rcs)                                     # FP_ERR_INVALID
    assert (out == -7).all() and (mask == 0xAB).all() and (visib == 0xCD).all() and (scratch == 0).all()
    # the wrapper raises ValueError for the same calls, and for tensors that are not on the device
    for e in bad_inst:
        with pytest.raises(ValueError):
            ops.gt_visibility(batch["test"], batch["large"], edited(inst, *e), params)
    for e in bad_par:
        with pytest.raises(ValueError):
            ops.gt_visibility(batch["test"], batch["large"], inst, edited(params, *e))
    with pytest.raises(ValueError, match="device"):
        ops.gt_visibility(batch["test"].cpu(), batch["large"], inst, params)
    with pytest.raises(ValueError, match="device"):
        ops.gt_visibility(batch["test"], batch["large"].cpu(), inst, params)
    with pytest.raises(ValueError):
        ops.gt_visibility(batch["test"], batch["large"][:4], inst, params)
    with pytest.raises(ValueError):
        ops.gt_visibility(batch["test"], batch["large"][:0], inst[:0], params[:0])
    with pytest.raises(ValueError):
        ops.gt_visibility(batch["test"], batch["large"], torch.from_numpy(inst).cuda(), params)
    assert _raw(batch, out, mask, visib, scratch) == 0               # and the good call still goes through
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().astype(np.int64), batch["rows"])
