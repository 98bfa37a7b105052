"""fp_pnp_ransac_keyed (pnp_util.solve_pnp_ransac_batch(..., pair_keys=)): RANSAC whose sampler is keyed by the caller, so that a pair's
hypotheses -- and with them its pose -- do not depend on where in a launch the pair sits.  The reference is the
unkeyed entry, which keys a pair by its index in the launch: with pair_keys[i] == i both are the same bits; a permuted batch that carries
its keys along gives the permuted outputs; and other keys give other hypotheses (the key is really read).

B = 4 detections x n = 2 slots, K = 64, 30 % gross outliers and 1 px noise on the inliers (so that two different minimal samples give two
different models); pair (3, 1) has 5 correspondences -- fewer than min_corresp -- and fails in every call."""
import numpy as np
import pytest
import torch

from foundpose_amd import pnp_util
from tests.test_gpu_pnp import CAM, _batch, _scene

pytestmark = pytest.mark.gpu
B, N, K = 4, 2, 64
FIELDS = ("success", "R", "t", "quality", "inliers", "ransac_pose")


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(21)
    scenes = [_scene(rng, 64, 19, 1.0) for _ in range(B * N - 1)] + [_scene(rng, 5, 0, 0.0)]
    c2, c3, cnt = _batch(scenes, K)                                   # [8, 1, K, .]: pair p = detection p // 2, slot p % 2
    return c2.reshape(B, N, K, 2), c3.reshape(B, N, K, 3), cnt.reshape(B, N)


def _solve(inp, seed=7, keys=None, perm=None):
    c2, c3, cnt = inp if perm is None else tuple(x[perm].contiguous() for x in inp)
    out = pnp_util.solve_pnp_ransac_batch(c2, c3, cnt, [CAM] * B, 400, 10.0, 0.99, True, seed=seed, return_ransac_pose=True, pair_keys=keys)
    return {k: out[k].cpu().numpy() for k in FIELDS}


@pytest.fixture(scope="module")
def unkeyed(inputs):
    return _solve(inputs)


def test_index_keys_reproduce_the_unkeyed_entry_bit_for_bit(inputs, unkeyed):
    assert unkeyed["success"].tolist() == [[True, True]] * 3 + [[True, False]]
    for keys in (torch.arange(B * N, dtype=torch.int64).reshape(B, N), torch.arange(B * N, dtype=torch.int64).reshape(B, N).cuda(),
                 [[b * N + j for j in range(N)] for b in range(B)]):      # host tensor, device tensor, nested lists
        got = _solve(inputs, keys=keys)
        for k in FIELDS:
            assert np.array_equal(got[k], unkeyed[k]), k
    with pytest.raises(ValueError, match="shape"):
        _solve(inputs, keys=torch.arange(B * N, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        _solve(inputs, keys=torch.arange(B * N, dtype=torch.int32).reshape(B, N))


def test_a_permuted_batch_with_its_own_keys_gives_the_permuted_outputs(inputs, unkeyed):
    perm = torch.tensor([2, 0, 3, 1])
    keys = torch.arange(B * N, dtype=torch.int64).reshape(B, N)[perm]
    got = _solve(inputs, keys=keys, perm=perm.cuda())
    for k in FIELDS:
        assert np.array_equal(got[k], unkeyed[k][perm.numpy()]), k
    # ... which the unkeyed entry does not do: there the hypotheses follow the position (the reason the key exists)
    moved = _solve(inputs, perm=perm.cuda())
    assert not np.array_equal(moved["ransac_pose"], unkeyed["ransac_pose"][perm.numpy()])


def test_other_keys_give_other_hypotheses(inputs, unkeyed):
    # the precondition, on the reference (the unkeyed kernel): these scenes are not so clean that the sample does not matter
    other_seed = _solve(inputs, seed=8)
    assert not np.array_equal(other_seed["ransac_pose"][:2], unkeyed["ransac_pose"][:2])
    keys = torch.arange(B * N, dtype=torch.int64).reshape(B, N)[torch.tensor([1, 0, 2, 3])]     # detections 0 and 1 swap their keys
    got = _solve(inputs, keys=keys)
    assert not np.array_equal(got["ransac_pose"][:2], unkeyed["ransac_pose"][:2])               # all four pairs there have outliers
    for k in FIELDS:                                                                            # the others kept their keys: untouched
        assert np.array_equal(got[k][2:], unkeyed[k][2:]), k
    # keys are 64-bit: a key above 2^32 is another key than its low half
    big = torch.arange(B * N, dtype=torch.int64).reshape(B, N) + (1 << 32)
    assert not np.array_equal(_solve(inputs, keys=big)["ransac_pose"][:3], unkeyed["ransac_pose"][:3])
