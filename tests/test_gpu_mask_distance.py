"""GPU: ops.mask_distance (csrc/mask_refine.hip, fp_mask_distance) is EQUAL to the numpy restatement
tests/mask_refine_ref.mask_distance -- which tests/test_mask_refine_cpu.py holds to the definition and to scipy -- at sizes that are
ragged in waves and rows, on empty, full, one-pixel, checkerboard and blob masks, with set bytes 1 and 255."""

import functools

import numpy as np
import pytest
import torch

from foundpose_amd import ops
from tests import mask_refine_ref as mr

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (1, 70), (70, 1), (48, 64), (37, 131), (65, 129)]


def _contents(H, W):
    """The masks of one size: [(name, uint8 [H, W])]."""
    rng = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[:H, :W]
    corner = np.zeros((H, W), np.uint8)
    corner[H - 1, W - 1] = 255
    blobs = np.zeros((H, W), np.uint8)
    for value in (1, 255, 1):
        cy, cx, r = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(0.5, max(H, W) / 4 + 0.5)
        blobs[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = value
    return [("empty", np.zeros((H, W), np.uint8)), ("full", np.full((H, W), 255, np.uint8)), ("corner", corner),
            ("checkerboard", ((yy + xx) % 2).astype(np.uint8)), ("blobs", blobs)]


@functools.lru_cache(maxsize=None)
def _case(H, W):
    """-> (masks uint8 [5, H, W], the restatement int32 [5, H, W]).  Shared: leave unchanged."""
    masks = np.stack([m for _, m in _contents(H, W)])
    return masks, np.stack([mr.mask_distance(m) for m in masks]).astype(np.int32)


def _gpu(masks):
    out = ops.mask_distance(torch.from_numpy(np.ascontiguousarray(masks)).cuda())
    assert out.dtype == torch.int32 and tuple(out.shape) == masks.shape
    return out.cpu().numpy()


@pytest.mark.parametrize("H,W", SIZES)
def test_equal_to_the_restatement(H, W):
    masks, ref = _case(H, W)
    assert set(np.unique(masks)) == {0, 1, 255} or H * W == 1
    got = _gpu(masks)
    for (name, _), g, r in zip(_contents(H, W), got, ref):
        assert np.array_equal(g, r), name
    assert (got[0] == 1 << 30).all() and (got[1] == 0).all()


@pytest.mark.parametrize("H,W", [(37, 131), (65, 129)])
def test_a_batch_equals_each_mask_alone_and_the_reversed_batch(H, W):
    masks, ref = _case(H, W)
    batch = _gpu(masks)
    assert np.array_equal(batch, ref)
    assert np.array_equal(_gpu(masks[::-1])[::-1], batch)
    for i in range(len(masks)):
        assert np.array_equal(_gpu(masks[i:i + 1])[0], batch[i]), i


def test_what_is_refused():
    m = torch.zeros(2, 5, 7, dtype=torch.uint8)
    with pytest.raises(ValueError, match="on the device"):
        ops.mask_distance(m)
    with pytest.raises(ValueError, match="uint8"):
        ops.mask_distance(m.cuda().to(torch.int32))
    with pytest.raises(ValueError, match="uint8"):
        ops.mask_distance(m.cuda()[0])
    assert tuple(ops.mask_distance(m.cuda()[:0]).shape) == (0, 5, 7)
