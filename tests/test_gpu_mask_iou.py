"""GPU: fp_mask_pack, fp_group_mask_iou and fp_group_box_iou (csrc/coco_eval.hip) against numpy: integers by equality,
overlaps by bit pattern."""

import numpy as np
import pytest
import torch

from tests import coco_ref as cr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def np_pack(masks):
    """uint8 [N, H, W] -> (uint64 [N, H, Wq], area): numpy's little-endian packbits, padded to whole words."""
    m = np.asarray(masks) != 0
    N, H, W = m.shape
    Wq = (W + 63) // 64
    pad = np.zeros((N, H, Wq * 64), bool)
    pad[:, :, :W] = m
    return np.packbits(pad, axis=2, bitorder="little").view("<u8").reshape(N, H, Wq), m.reshape(N, -1).sum(1).astype(np.int32)


def random_masks(rng, N, H, W, fill=0.4):
    m = (rng.random((N, H, W)) < fill).astype(np.uint8)
    m *= rng.choice(np.array([1, 2, 255], np.uint8), size=m.shape)       # any non-zero byte is set
    m[:, :, W - 1] = np.where(np.arange(H)[None, :] % 2 == 0, 255, m[:, :, W - 1])   # set pixels in the row's last, partial word
    return m


def words_of(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 129, 200, 80, 640])
@pytest.mark.parametrize("H", [1, 3, 50])
def test_mask_pack_matches_numpy(H, W):
    from foundpose_amd import ops
    rng = np.random.default_rng(1000 * H + W)
    m = random_masks(rng, 3, H, W)
    m[2] = 0                                                               # an empty mask
    want_w, want_a = np_pack(m)
    assert np.array_equal(want_w[0], cr.pack_bits(m[0]))                  # the helper against the restatement's loop
    words, area = ops.mask_pack(torch.from_numpy(m).to(DEV))
    assert words.shape == (3, H, (W + 63) // 64) and words.dtype == torch.int64
    assert np.array_equal(words_of(words), want_w) and np.array_equal(area.cpu().numpy(), want_a)
    # the same bytes from a storage that starts one byte off 16-byte alignment, and for every mask alone
    base = torch.zeros(m.size + 1, dtype=torch.uint8, device=DEV)
    base[1:] = torch.from_numpy(m).to(DEV).flatten()
    off = base[1:].view(3, H, W)
    assert off.data_ptr() % 16 == 1 and off.is_contiguous()
    w2, a2 = ops.mask_pack(off)
    assert torch.equal(w2, words) and torch.equal(a2, area)
    for i in range(3):
        w1, a1 = ops.mask_pack(torch.from_numpy(m[i:i + 1].copy()).to(DEV))
        assert torch.equal(w1[0], words[i]) and int(a1[0]) == int(area[i])


def test_mask_pack_refuses_bad_input():
    from foundpose_amd import ops
    with pytest.raises(ValueError):
        ops.mask_pack(torch.zeros(2, 4, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.mask_pack(torch.zeros(2, 4, 8, dtype=torch.uint8, device=DEV)[:, :, ::2])
    with pytest.raises(ValueError):
        ops.mask_pack(torch.zeros(2, 0, 4, dtype=torch.uint8, device=DEV))
    w, a = ops.mask_pack(torch.zeros(0, 4, 4, dtype=torch.uint8, device=DEV))
    assert w.shape == (0, 4, 1) and a.shape == (0,)


# ---------------------------------------------------------------------------------------------------------- overlaps of groups
H, W = 90, 200     # L = 90 * 4 = 360 words: more than one stride of the 256-thread workgroup, and no multiple of it
SHAPES = [(0, 3), (2, 0), (1, 1), (37, 9), (5, 4), (4, 8), (3, 3), (9, 1), (6, 2)]   # 37 x 9: more than one 4 x 4 tile both ways, neither a multiple; 9 x 1: 4 x 1 tiles


@pytest.fixture(scope="module")
def groups():
    """The masks of all groups, the tables and the numpy reference, computed once."""
    rng = np.random.default_rng(7)
    A = [random_masks(rng, E, H, W, 0.3) for E, _ in SHAPES]
    B = [random_masks(rng, G, H, W, 0.3) for _, G in SHAPES]
    A[3][5], B[3][2] = 0, 0                                                # two empty masks meet: status 2
    B[3][3] = A[3][7]                                                      # identical masks: exactly 1
    A[3][9][:, 100:], B[3][4][:, :100] = 0, 0                              # disjoint masks: 0
    A[6][:], B[6][:] = 0, 0
    A[6][0][10:20, 60:70] = 1                                              # (3, 3): mostly empty masks
    est_off = np.cumsum([0] + [E for E, _ in SHAPES])
    gt_off = np.cumsum([0] + [G for _, G in SHAPES])
    pair_off = np.cumsum([0] + [E * G for E, G in SHAPES])
    ref = []
    for a, b in zip(A, B):
        fa, fb = (a != 0).reshape(len(a), H * W).astype(np.int64), (b != 0).reshape(len(b), H * W).astype(np.int64)
        inter = fa @ fb.T
        union = fa.sum(1)[:, None] + fb.sum(1)[None, :] - inter
        ov = np.where(union > 0, inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64), 0.0)
        ref.append((inter.reshape(-1), union.reshape(-1), ov.reshape(-1), np.where(union > 0, 0, 2).reshape(-1)))
    return A, B, est_off, gt_off, pair_off, ref


def run_groups(A, B, est_off, gt_off, pair_off):
    from foundpose_amd import ops
    wa, _ = ops.mask_pack(torch.from_numpy(np.concatenate(A)).to(DEV))
    wb, _ = ops.mask_pack(torch.from_numpy(np.concatenate(B)).to(DEV))
    t = [torch.from_numpy(np.asarray(x, np.int32)).to(DEV) for x in (est_off, gt_off, pair_off)]
    counts, overlap, status = ops.group_mask_iou(wa, wb, *t, int(pair_off[-1]))
    return counts.cpu().numpy(), overlap.cpu().numpy(), status.cpu().numpy()


def test_group_mask_iou_matches_numpy(groups):
    A, B, est_off, gt_off, pair_off, ref = groups
    counts, overlap, status = run_groups(A, B, est_off, gt_off, pair_off)
    for g, (inter, union, ov, st) in enumerate(ref):
        sl = slice(pair_off[g], pair_off[g + 1])
        assert np.array_equal(counts[sl, 0], inter) and np.array_equal(counts[sl, 1], union), g
        assert np.array_equal(overlap[sl].view(np.int64), ov.view(np.int64)) and np.array_equal(status[sl], st), g
    G = SHAPES[3][1]
    p = pair_off[3]
    assert status[p + 5 * G + 2] == 2 and overlap[p + 5 * G + 2] == 0.0 and counts[p + 5 * G + 2].tolist() == [0, 0]
    assert overlap[p + 7 * G + 3] == 1.0 and status[p + 7 * G + 3] == 0
    assert overlap[p + 9 * G + 4] == 0.0 and status[p + 9 * G + 4] == 0
    a, b = A[3][1] != 0, B[3][1] != 0
    assert (int(counts[p + G + 1, 0]), int(counts[p + G + 1, 1]), float(overlap[p + G + 1]), int(status[p + G + 1])) == cr.mask_iou(a, b)


def test_a_group_alone_and_permuted_groups_give_the_same_bytes(groups):
    A, B, est_off, gt_off, pair_off, _ = groups
    counts, overlap, status = run_groups(A, B, est_off, gt_off, pair_off)
    for g, (E, G) in enumerate(SHAPES):
        if E == 0 or G == 0:
            continue
        c1, o1, s1 = run_groups([A[g]], [B[g]], [0, E], [0, G], [0, E * G])
        sl = slice(pair_off[g], pair_off[g + 1])
        assert np.array_equal(c1, counts[sl]) and np.array_equal(o1.view(np.int64), overlap[sl].view(np.int64)) and np.array_equal(s1, status[sl])
    perm = [4, 0, 8, 6, 3, 7, 1, 5, 2]
    sh = [SHAPES[i] for i in perm]
    po = np.cumsum([0] + [E * G for E, G in sh])
    c2, o2, s2 = run_groups([A[i] for i in perm], [B[i] for i in perm], np.cumsum([0] + [E for E, _ in sh]), np.cumsum([0] + [G for _, G in sh]), po)
    for k, i in enumerate(perm):
        a, b = slice(po[k], po[k + 1]), slice(pair_off[i], pair_off[i + 1])
        assert np.array_equal(c2[a], counts[b]) and np.array_equal(o2[a].view(np.int64), overlap[b].view(np.int64)) and np.array_equal(s2[a], status[b])


@pytest.mark.parametrize("third", ["1x1", "1x2", "5x1"])
@pytest.mark.parametrize("num_groups", [257, 600])
def test_tile_table_across_the_scan_chunks(num_groups, third):
    """The tile table is a scan in chunks of 256 groups with a carry: 257 groups put one entry into the second chunk, 600 cross two seams.
    Groups of 1 x 1 on masks of 2 x 70 (L = 4 words, the last one partial); every third group is `third` instead.  1 x 2 still takes one
    tile (4 x 4 tiles), 5 x 1 takes two, so only the last variant makes the tile counts differ between groups.  The reference is numpy's
    popcount of the packed words."""
    from foundpose_amd import ops
    rng = np.random.default_rng(num_groups)
    E3, G3 = (int(v) for v in third.split("x"))
    shapes = [(E3, G3) if g % 3 == 2 else (1, 1) for g in range(num_groups)]
    est_off, gt_off = np.cumsum([0] + [E for E, _ in shapes]), np.cumsum([0] + [G for _, G in shapes])
    pair_off = np.cumsum([0] + [E * G for E, G in shapes])
    a, b = random_masks(rng, int(est_off[-1]), 2, 70), random_masks(rng, int(gt_off[-1]), 2, 70)
    a[est_off[4]], b[gt_off[4]] = 0, 0                                     # group 4 (1 x 1): union 0
    wa, wb = (np_pack(m)[0].reshape(len(m), 4) for m in (a, b))
    pop = lambda w: np.unpackbits(np.ascontiguousarray(w).view(np.uint8).reshape(len(w), -1), axis=1).sum(1).astype(np.int64)
    rows_a = np.concatenate([np.repeat(np.arange(est_off[g], est_off[g + 1]), G) for g, (_, G) in enumerate(shapes)])
    rows_b = np.concatenate([np.tile(np.arange(gt_off[g], gt_off[g + 1]), E) for g, (E, _) in enumerate(shapes)])
    inter = pop(wa[rows_a] & wb[rows_b])
    union = pop(wa[rows_a]) + pop(wb[rows_b]) - inter
    want = np.where(union > 0, inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64), 0.0)
    counts, overlap, status = run_groups([a], [b], est_off, gt_off, pair_off)
    assert np.array_equal(counts[:, 0], inter) and np.array_equal(counts[:, 1], union)
    assert np.array_equal(overlap.view(np.int64), want.view(np.int64)) and np.array_equal(status, np.where(union > 0, 0, 2))
    assert status[pair_off[4]] == 2 and (union > 0).sum() == len(union) - 1 and (inter > 0).any()


def test_offsets_beyond_the_arrays_are_clamped(groups):
    """Tables that the host would refuse: the kernel clamps them into the arrays, writes only rows that exist and nothing faults."""
    A, B, *_ = groups
    from foundpose_amd import ops
    wa, _ = ops.mask_pack(torch.from_numpy(A[4][:3]).to(DEV))             # 3 rows of a
    wb, _ = ops.mask_pack(torch.from_numpy(B[4][:2]).to(DEV))             # 2 rows of b
    t = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    counts, overlap, status = ops.group_mask_iou(wa, wb, t([-5, 1000, 2000]), t([0, 1000, 4000]), t([0, 9, 1 << 30]), 5)
    torch.cuda.synchronize()
    want = run_groups([A[4][:2]], [B[4][:2]], [0, 2], [0, 2], [0, 4])      # 3 x 2 does not fit 5 rows: the group is cut to 2 x 2
    assert np.array_equal(counts.cpu().numpy()[:4], want[0]) and np.array_equal(status.cpu().numpy()[:4], want[2])
    assert counts.cpu().numpy()[4].tolist() == [0, 0] and int(status[4]) == 2     # no group owns the last row
    ov, st = ops.group_box_iou(torch.ones(3, 4, dtype=torch.float64, device=DEV), torch.ones(2, 4, dtype=torch.float64, device=DEV),
                               t([-5, 1000, 2000]), t([0, 1000, 4000]), t([0, 9, 1 << 30]), 5)
    torch.cuda.synchronize()
    assert ov.cpu().numpy().tolist() == [1.0, 1.0, 1.0, 1.0, 0.0] and st.cpu().numpy().tolist() == [0, 0, 0, 0, 2]


def test_group_box_iou_matches_the_restatement_bit_for_bit():
    from foundpose_amd import ops
    rng = np.random.default_rng(11)
    shapes = [(3, 2), (0, 4), (40, 7), (1, 1), (300, 1)]
    fr = np.array([0.0, 0.25, 1.0 / 3.0, 0.5, 0.1, 0.7])
    make = lambda n: np.concatenate([rng.integers(0, 30, (n, 2)) + fr[rng.integers(0, 6, (n, 2))], rng.integers(1, 25, (n, 2)) + fr[rng.integers(0, 6, (n, 2))]], 1)
    A, B = [make(E) for E, _ in shapes], [make(G) for _, G in shapes]
    A[0][0], B[0][0] = [2.5, 3.0, 4.0, 2.0], [6.5, 3.0, 1.0, 2.0]         # touching boxes: overlap 0, scored
    A[0][1], B[0][1] = [1.0, 1.0, 0.0, 5.0], [1.0, 1.0, 0.0, 5.0]         # zero-area boxes: status 2
    A[0][2] = B[0][0]                                                      # identical: exactly 1
    est_off, gt_off = np.cumsum([0] + [E for E, _ in shapes]), np.cumsum([0] + [G for _, G in shapes])
    pair_off = np.cumsum([0] + [E * G for E, G in shapes])
    t = [torch.from_numpy(np.asarray(x, np.int32)).to(DEV) for x in (est_off, gt_off, pair_off)]
    ov, st = ops.group_box_iou(torch.from_numpy(np.concatenate(A)).to(DEV), torch.from_numpy(np.concatenate(B)).to(DEV), *t, int(pair_off[-1]))
    ov, st = ov.cpu().numpy(), st.cpu().numpy()
    for g, (E, G) in enumerate(shapes):
        for e in range(E):
            for j in range(G):
                want = cr.box_iou(A[g][e], B[g][j])
                q = pair_off[g] + e * G + j
                assert (np.float64(ov[q]).view(np.int64), int(st[q])) == (np.float64(want[0]).view(np.int64), want[1]), (g, e, j)
    assert (ov[0], st[0]) == (0.0, 0) and (ov[1 * 2 + 1], st[1 * 2 + 1]) == (0.0, 2) and ov[2 * 2 + 0] == 1.0
    with pytest.raises(ValueError):
        ops.group_box_iou(torch.zeros(3, 4, device=DEV), torch.zeros(2, 4, dtype=torch.float64, device=DEV), *t, 0)
