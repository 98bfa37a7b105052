"""fp_mask_boxes and fp_proposal_crops (ops.mask_boxes, ops.proposal_crops) against their fp64 restatement
(tests/proposal_ref.py) on the smallest shapes at which they can go wrong: two images of 37 x 53 and crops of 28 -- a wide, a tall, a 3 x 2
and a one-pixel blob, a mask on all four borders, a mask with holes, an empty one -- and one box of 200 x 131 in a larger image (scale > 7,
several LDS chunks of source rows per band).  The bound: values in [0, 1], weights summing to 1, at most 2 sup + 1 <= 17 taps per axis, one
fp32 rounding of a weight and one of an fma per tap and axis: < 80 roundings of 2^-24 = 4.8e-6 < 1e-5."""
import numpy as np
import pytest
import torch

from foundpose_amd import ops
from tests import proposal_ref as pr

pytestmark = pytest.mark.gpu
H, W, S = 37, 53, 28
BOUND = 1e-5


def _masks():
    m = np.zeros((7, H, W), np.uint8)
    m[0, 10:19, 2:52] = 1                      # wide: 9 x 50
    m[0, 12, 20] = 0
    m[1, 1:36, 30:39] = 1                      # tall: 35 x 9
    m[2, 20:23, 7:9] = 1                       # 3 x 2 (h x w): upscaled
    m[3, 36, 52] = 7                           # one pixel, in the last corner; any non-zero byte counts
    m[4, 0, 5] = m[4, 36, 40] = m[4, 17, 0] = m[4, 9, 52] = 1   # touches all four borders: the box is the image
    m[4, 5:30, 8:45] = 1
    m[5, 4:30, 6:40] = 1                       # holes: zeros inside the box keep their weight
    m[5, 8:15, 10:20] = 0
    m[5, 20:22, 30:39] = 0
    return m                                   # m[6] stays empty


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(5)
    images = rng.random((2, H, W, 3)).astype(np.float32)
    masks = _masks()
    index = np.array([0, 1, 0, 1, 0, 1, 0], np.int32)
    dm, di, dx = torch.from_numpy(masks).cuda(), torch.from_numpy(images).cuda(), torch.from_numpy(index).cuda()
    boxes, area = ops.mask_boxes(dm)
    crops, status = ops.proposal_crops(di, dm, boxes, S, dx)
    ref_boxes, ref_area = pr.mask_boxes(masks)
    ref = [pr.proposal_crop(images[index[p]], masks[p], ref_boxes[p], S) for p in range(len(masks))]
    return dict(images=images, masks=masks, index=index, dm=dm, di=di, dx=dx, boxes=boxes, area=area, crops=crops, status=status,
                ref_boxes=ref_boxes, ref_area=ref_area, ref=ref)


def test_boxes_and_areas_are_exact(small):
    assert small["boxes"].cpu().numpy().tolist() == small["ref_boxes"].tolist()
    assert small["area"].cpu().numpy().tolist() == small["ref_area"].tolist()
    assert small["ref_boxes"][4].tolist() == [0, 0, W, H] and small["ref_boxes"][3].tolist() == [52, 36, 53, 37]
    assert small["ref_boxes"][6].tolist() == [0, 0, 0, 0] and small["ref_area"][6] == 0
    # the 16-byte path and the byte path agree: the same masks behind an odd offset, and a 16-byte-aligned stack of 16 x 16
    shifted = torch.zeros(7 * H * W + 1, dtype=torch.uint8, device="cuda")
    shifted[1:] = small["dm"].flatten()
    b2, a2 = ops.mask_boxes(shifted[1:].view(7, H, W))
    assert torch.equal(b2, small["boxes"]) and torch.equal(a2, small["area"])
    rng = np.random.default_rng(1)
    m = (rng.random((3, 16, 16)) < 0.05).astype(np.uint8)
    b3, a3 = ops.mask_boxes(torch.from_numpy(m).cuda())
    rb, ra = pr.mask_boxes(m)
    assert b3.cpu().numpy().tolist() == rb.tolist() and a3.cpu().numpy().tolist() == ra.tolist()


def test_crops_match_the_restatement(small):
    crops, status = small["crops"].cpu().numpy(), small["status"].cpu().numpy()
    assert status.tolist() == [0, 0, 0, 0, 0, 0, 2] == [s for _, s in small["ref"]]
    for p, (want, _) in enumerate(small["ref"]):
        err = float(np.abs(crops[p] - want).max())
        print(f"proposal {p}: box {small['ref_boxes'][p].tolist()} max |device - fp64| = {err:.3g}")
        assert err <= BOUND, p
        if status[p] == 0:
            wo, ho, ox, oy = pr.crop_window(small["ref_boxes"][p], S)
            outside = np.ones((S, S), bool)
            outside[oy:oy + ho, ox:ox + wo] = False
            assert not crops[p][:, outside].any(), p                 # exact zeros outside the window
            assert crops[p].min() >= 0.0 and crops[p].max() <= 1.0 + 1e-6
    assert not crops[6].any()                                        # status 2: all zero
    assert np.abs(crops[3] - small["images"][1, 36, 52][:, None, None]).max() <= BOUND   # one pixel fills the crop
    # holes: the restatement with the holes FILLED differs, so the zeros did enter with their weight
    filled = small["masks"][5].copy()
    filled[4:30, 6:40] = 1
    assert np.abs(pr.proposal_crop(small["images"][1], filled, small["ref_boxes"][5], S)[0] - crops[5]).max() > 1e-2


def test_the_background_does_not_change_a_bit(small):
    rng = np.random.default_rng(9)
    other = rng.random((2, H, W, 3)).astype(np.float32)
    for p in range(7):                                               # keep the image only under each proposal's own mask
        on = small["masks"][p] != 0
        other[small["index"][p]][on] = small["images"][small["index"][p]][on]
    # (proposals of one image overlap in places; a pixel under ANY of them keeps its value, which is all a proposal may read through its mask)
    crops, status = ops.proposal_crops(torch.from_numpy(other).cuda(), small["dm"], small["boxes"], S, small["dx"])
    assert torch.equal(crops, small["crops"]) and torch.equal(status, small["status"])


def test_alone_and_at_another_position_gives_the_same_bits(small):
    for p in (0, 2, 5):
        c, s = ops.proposal_crops(small["di"], small["dm"][p:p + 1].contiguous(), small["boxes"][p:p + 1].contiguous(), S, small["dx"][p:p + 1].contiguous())
        assert torch.equal(c[0], small["crops"][p]) and int(s[0]) == 0
    perm = torch.tensor([5, 6, 0, 3, 1, 4, 2], device="cuda")
    c, s = ops.proposal_crops(small["di"], small["dm"][perm].contiguous(), small["boxes"][perm].contiguous(), S, small["dx"][perm].contiguous())
    assert torch.equal(c, small["crops"][perm]) and torch.equal(s, small["status"][perm])
    # image_index = None: proposal p reads image p
    c, s = ops.proposal_crops(small["di"], small["dm"][:2].contiguous(), small["boxes"][:2].contiguous(), S)
    assert torch.equal(c, small["crops"][:2])


def test_bad_tables_give_status_2_and_zeros(small):
    idx = small["dx"].clone()
    idx[0], idx[1] = 2, -1                                           # outside the table of two images
    boxes = small["boxes"].clone()
    boxes[2] = torch.tensor([7, 20, 9, 38], dtype=torch.int32)       # leaves the image at the bottom
    boxes[4] = torch.tensor([-1, 0, 10, 10], dtype=torch.int32)
    boxes[5] = torch.tensor([6, 4, 6, 30], dtype=torch.int32)        # no width
    c, s = ops.proposal_crops(small["di"], small["dm"], boxes, S, idx)
    assert s.cpu().tolist() == [2, 2, 2, 0, 2, 2, 2]
    assert not c[[0, 1, 2, 4, 5, 6]].any() and torch.equal(c[3], small["crops"][3])
    with pytest.raises(ValueError):
        ops.proposal_crops(small["di"], small["dm"], small["boxes"], 0, small["dx"])
    with pytest.raises(ValueError):
        ops.proposal_crops(small["di"], small["dm"], small["boxes"], 1025, small["dx"])


def test_a_box_of_200_by_131_scales_down_by_more_than_7():
    rng = np.random.default_rng(11)
    Hb, Wb = 210, 140
    image = rng.random((1, Hb, Wb, 3)).astype(np.float32)
    mask = np.zeros((1, Hb, Wb), np.uint8)
    mask[0, 4:204, 6:137] = rng.random((200, 131)) < 0.7
    mask[0, 4, 6] = mask[0, 203, 136] = 1
    dm = torch.from_numpy(mask).cuda()
    boxes, area = ops.mask_boxes(dm)
    assert boxes.cpu().tolist() == [[6, 4, 137, 204]] and int(area[0]) == int(mask.sum())
    crops, status = ops.proposal_crops(torch.from_numpy(image).cuda(), dm, boxes, S)
    want, _ = pr.proposal_crop(image[0], mask[0], (6, 4, 137, 204), S)
    assert pr.crop_window((6, 4, 137, 204), S) == (18, 28, 5, 0) and pr.max_taps(200, 28) <= 2 * 200 / 28 + 1
    err = float(np.abs(crops[0].cpu().numpy() - want).max())
    print(f"200 x 131 -> 28 x 18: max |device - fp64| = {err:.3g}")
    assert int(status[0]) == 0 and err <= BOUND
    # a larger crop than the box (upscaling by 4) and a crop size that is no multiple of the band
    small_mask = np.ascontiguousarray(mask[:, :60, :70])
    small_image = np.ascontiguousarray(image[:, :60, :70])
    sb, _ = ops.mask_boxes(torch.from_numpy(small_mask).cuda())
    c3, s3 = ops.proposal_crops(torch.from_numpy(small_image).cuda(), torch.from_numpy(small_mask).cuda(), sb, 203)
    want3, _ = pr.proposal_crop(small_image[0], small_mask[0], sb.cpu().numpy()[0], 203)
    err3 = float(np.abs(c3[0].cpu().numpy() - want3).max())
    print(f"56 x 64 -> 203: max |device - fp64| = {err3:.3g}")
    assert int(s3[0]) == 0 and err3 <= BOUND
