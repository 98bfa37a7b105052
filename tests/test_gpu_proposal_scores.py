"""fp_proposal_scores, fp_proposal_rank and fp_box_iou (ops.proposal_scores / proposal_rank / box_iou) against
tests/proposal_ref.py.  The similarities are read back from the library's own canonical chain (the scratch fp_cosine_topk leaves) and agree
with fp64 within D 2^-24 (unit rows: every partial sum is at most 1 in magnitude, D roundings of half an ulp of 1); GIVEN those
similarities the scores, the best object, its score and its template are numpy's bit for bit, the fp32 adds in the stated order.
Objects of 1, 7, 70 and 0 templates (fewer than k, just above k, more than one key per lane, none) and a fifth that repeats the second
(equal scores: the lower object wins); duplicated template rows (equal similarities: the lower template id comes first)."""
import numpy as np
import pytest
import torch

from foundpose_amd import ops
from tests import proposal_ref as pr

pytestmark = pytest.mark.gpu
COUNTS = [1, 7, 70, 0, 7]
P = 5


def _unit(x):
    return ops.normalize_rows(torch.from_numpy(x.astype(np.float32)).cuda())


def _case(D):
    rng = np.random.default_rng(D)
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
    bank = rng.standard_normal((int(off[-1]), D))
    bank[off[2] + 40] = bank[off[2] + 3]          # a duplicated row inside the 70-template object
    bank[off[2] + 41] = bank[off[2] + 3]
    bank[off[1] + 5] = bank[off[1] + 2]           # ... and inside the 7-template one
    bank[off[4]:off[5]] = bank[off[1]:off[2]]     # object 4 repeats object 1
    desc = rng.standard_normal((P, D))
    desc[1] = bank[off[2] + 3] + 0.05 * rng.standard_normal(D)   # close to the duplicated rows: the tie is among the best
    desc[2] = bank[off[1] + 2]                                   # equal to a row of objects 1 and 4
    return _unit(desc), _unit(bank), off


def _sims32(sims, off):
    """[O, P, maxT] as the device left it -> fp32 [P, N], each object's columns cut to its template count."""
    s = sims.cpu().numpy()
    return np.concatenate([s[o, :, :off[o + 1] - off[o]] for o in range(len(off) - 1)], 1)


@pytest.mark.parametrize("D", [20, 128])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_scores_are_numpys_on_the_chains_similarities(D, k):
    desc_n, bank_n, off = _case(D)
    d_off = torch.from_numpy(off).cuda()
    scores, bo, bs, bt, sims = ops.proposal_scores(desc_n, bank_n, d_off, max(COUNTS), k, return_sims=True)
    s32 = _sims32(sims, off)
    err = float(np.abs(s32.astype(np.float64) - pr.similarities64(desc_n.cpu().numpy(), bank_n.cpu().numpy())).max())
    print(f"D = {D}, k = {k}: max |chain - fp64| = {err:.3g} (bound {D * 2.0 ** -24:.3g})")
    assert err <= D * 2.0 ** -24
    want = pr.proposal_scores(s32, off, k)
    got = (scores.cpu().numpy(), bo.cpu().numpy(), bs.cpu().numpy(), bt.cpu().numpy())
    for name, g, w in zip(("scores", "best_obj", "best_score", "best_template"), got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, g, w)
    assert np.isneginf(got[0][:, 3]).all() and not (got[1] == 3).any()        # the empty object scores -inf and is never best
    assert got[1][2] == 1                                                       # objects 1 and 4 tie on proposal 2: the lower one
    assert (got[0][:, 1].tobytes() == got[0][:, 4].tobytes())
    if k == 1:
        assert got[3][2] == 2                                                   # rows 2 and 5 of object 1 are equal: template 2 is v_1
        assert got[1][1] == 2 and got[3][1] == 3                                # rows 3, 40, 41 of object 2 are equal: template 3


@pytest.mark.parametrize("D", [20, 128])
def test_a_proposal_alone_or_elsewhere_gets_the_same_bits(D):
    desc_n, bank_n, off = _case(D)
    d_off = torch.from_numpy(off).cuda()
    full = ops.proposal_scores(desc_n, bank_n, d_off, max(COUNTS), 5)
    for p in (1, 4):
        one = ops.proposal_scores(desc_n[p:p + 1].contiguous(), bank_n, d_off, max(COUNTS), 5)
        for a, b in zip(one, full):
            assert torch.equal(a[0], b[p])
    perm = torch.tensor([3, 0, 4, 2, 1], device="cuda")
    moved = ops.proposal_scores(desc_n[perm].contiguous(), bank_n, d_off, max(COUNTS), 5)
    for a, b in zip(moved, full):
        assert torch.equal(a, b[perm])
    big = ops.proposal_scores(desc_n.repeat(9, 1), bank_n, d_off, max(COUNTS), 5)   # 45 rows: more than one 32-row chunk per object
    for a, b in zip(big, full):
        assert torch.equal(a[40:45], b)


def test_no_object_with_templates_gives_minus_one():
    desc_n, bank_n, off = _case(20)
    none = torch.zeros(3, dtype=torch.int32, device="cuda")
    scores, bo, bs, bt = ops.proposal_scores(desc_n, bank_n, none, 1, 3)
    assert torch.isneginf(scores).all() and bo.cpu().tolist() == [-1] * P and bt.cpu().tolist() == [-1] * P and torch.isneginf(bs).all()
    # offsets that leave the bank or decrease are clamped before anything is read through them
    wild = torch.tensor([-5, 3, 1, 10 ** 6], dtype=torch.int32, device="cuda")
    scores, bo, bs, bt, sims = ops.proposal_scores(desc_n, bank_n, wild, 100, 2, return_sims=True)
    clamped = np.array([0, 3, 3, int(bank_n.shape[0])], np.int32)
    want = pr.proposal_scores(_sims32(sims, clamped), clamped, 2)
    assert scores.cpu().numpy().tobytes() == want[0].tobytes() and bo.cpu().numpy().tolist() == want[1].tolist()
    with pytest.raises(ValueError):
        ops.proposal_scores(desc_n, bank_n, none, 1, 17)


# ---------------------------------------------------------------------------------------------------- overlaps and the layout
BOXES = [(0, 0, 4, 4), (0, 0, 4, 4), (1, 1, 3, 3), (4, 0, 8, 4), (0, 0, 0, 5), (7, 7, 7, 7), (0, 0, 5, 2), (0, 1, 5, 3), (10, 10, 2010, 3010),
         (1010, 10, 3010, 3010)]
PAIRS = [(0, 1), (0, 2), (2, 0), (0, 3), (4, 5), (4, 0), (6, 7), (8, 9), (0, 10), (-1, 0), (3, 3)]


def test_box_overlaps_are_exact():
    boxes = torch.tensor(BOXES, dtype=torch.int32, device="cuda")
    pairs = torch.tensor(PAIRS, dtype=torch.int32, device="cuda")
    ov, st = ops.box_iou(boxes, pairs)
    want_ov, want_st = pr.box_iou(BOXES, PAIRS)
    assert ov.cpu().numpy().tobytes() == want_ov.tobytes() and st.cpu().numpy().tolist() == want_st.tolist()
    got = dict(zip(PAIRS, zip(ov.cpu().tolist(), st.cpu().tolist())))
    assert got[(0, 1)] == (1.0, 0)            # identical
    assert got[(0, 2)] == (0.25, 0) == got[(2, 0)]   # nested: 4 of 16, exactly the threshold
    assert got[(0, 3)] == (0.0, 0)            # touching: no common pixel
    assert got[(4, 5)] == (0.0, 2)            # both degenerate: union 0
    assert got[(4, 0)] == (0.0, 0)            # one degenerate: scored, nothing in common
    assert got[(6, 7)] == (5 / 15, 0)
    assert got[(0, 10)] == (0.0, 2) and got[(-1, 0)] == (0.0, 2)   # an index outside the table
    assert got[(8, 9)] == (3.0e6 / 9.0e6, 0)  # 6e6-pixel boxes: products beyond 2^31 stay exact in int64
    empty = ops.box_iou(boxes, torch.zeros(0, 2, dtype=torch.int32, device="cuda"))
    assert empty[0].numel() == 0 and empty[1].numel() == 0


def test_the_pair_at_exactly_the_threshold_conflicts():
    """Three boxes in rank order: box 2 is nested in box 0 at overlap exactly 0.25; box 3 only touches box 0."""
    boxes = torch.tensor([BOXES[0], BOXES[2], BOXES[3]], dtype=torch.int32, device="cuda")
    pairs = torch.tensor([(0, 1), (0, 2), (1, 2)], dtype=torch.int32, device="cuda")
    ov, st = ops.box_iou(boxes, pairs)
    off = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    keep, by = ops.pose_nms_greedy(off(0, 3), off(0, 3), pairs, ov, st, 3, 0.25)
    assert keep.cpu().tolist() == [1, 0, 1] and by.cpu().tolist() == [-1, 0, -1]
    keep, by = ops.pose_nms_greedy(off(0, 3), off(0, 3), pairs, ov, st, 3, float(np.nextafter(0.25, 1.0)))
    assert keep.cpu().tolist() == [1, 1, 1]


def _rank_case(seed, n, num_obj):
    rng = np.random.default_rng(seed)
    obj = rng.integers(-1, num_obj + 1, n).astype(np.int32)          # -1 and num_obj: no object
    score = rng.random(n).astype(np.float32)
    score[3] = score[2] = score[11]                                  # equal scores: input order
    score[5] = np.nan
    score[6] = -np.inf
    obj[2] = obj[3] = obj[11] = 1
    area = rng.integers(0, 40, n).astype(np.int32)
    status = (rng.random(n) < 0.1).astype(np.int32) * 2
    xy = rng.integers(0, 30, (n, 2))
    boxes = np.concatenate([xy, xy + rng.integers(1, 25, (n, 2))], 1).astype(np.int32)
    return obj, score, area, status, boxes


@pytest.mark.parametrize("n,num_obj,max_group", [(60, 3, 256), (60, 3, 4), (1, 1, 256), (300, 2, 256)])
def test_decisions_layout_and_pairs(n, num_obj, max_group):
    obj, score, area, status, boxes = _rank_case(n, max(n, 12), num_obj)
    n = len(obj)
    dev = lambda a: torch.from_numpy(a).cuda()
    decision, order, group_off, pair_off, pairs, ranked = ops.proposal_rank(dev(obj), dev(score), dev(area), dev(status), dev(boxes), num_obj, 8, 0.3, max_group)
    names, want_order, want_off = pr.decide(obj, score, area, status, num_obj, 8, 0.3, max_group)
    assert [pr.DECISIONS[d] for d in decision.cpu().tolist()] == names
    assert group_off.cpu().tolist() == want_off
    assert order.cpu().tolist() == want_order + [-1] * (n - len(want_order))
    want_pairs, want_pair_off = pr.group_pairs(want_off)
    assert pair_off.cpu().tolist() == want_pair_off
    got_pairs = pairs.cpu().numpy()
    assert got_pairs.shape[0] == n * (max_group - 1) // 2
    assert got_pairs[:len(want_pairs)].tolist() == want_pairs.tolist() and (got_pairs[len(want_pairs):] == -1).all()
    rk = ranked.cpu().numpy()
    assert rk[:len(want_order)].tolist() == boxes[want_order].tolist() and not rk[len(want_order):].any()
    # ... and through the overlaps and the suppression: the restated selection
    ov, st = ops.box_iou(ranked, pairs)
    assert (st.cpu().numpy()[len(want_pairs):] == 2).all()
    keep, by = ops.pose_nms_greedy(group_off, pair_off, pairs, ov, st, n, 0.25)
    want_keep, want_by = pr.nms_greedy(boxes[want_order] if want_order else np.zeros((0, 4), np.int32), want_off, 0.25)
    assert keep.cpu().numpy()[:len(want_order)].astype(bool).tolist() == want_keep.tolist()
    assert by.cpu().numpy()[:len(want_order)].tolist() == want_by.tolist()
