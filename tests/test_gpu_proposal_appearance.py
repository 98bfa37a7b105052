"""fp_proposal_patch_cover and fp_proposal_appearance (ops.proposal_patch_cover, ops.proposal_appearance) against
their restatement (tests/appearance_ref.py).  Coverage is exact.  A similarity is an fp32 fmaf chain over D products of unit vectors: it
lies within D 2^-24 of the fp64 dot product (section 23's bar), so does the maximum, and the fp64 similarity at the device's argmax lies
within the same bound of the fp64 maximum.  Everything behind the similarities is replayed in fp32 from the device's own best_sim and must
agree by bit pattern.  Shapes: 7 proposals; 1, 16, 130 (one full 128-row tile and a ragged one) and 256 patches; 20 and 384 words; objects
of 1, 5 and 0 templates and a fourth object whose bank rows and coverage are copies of the second's."""
import numpy as np
import pytest
import torch

from foundpose_amd import _lib, ops
from tests import appearance_ref as ar

pytestmark = pytest.mark.gpu
PS, MIN_COVER = 14, 98
OBJ_OFF = [0, 1, 6, 6, 11]           # objects of 1, 5, 0 templates and a copy of the second: rows 6 .. 10 are rows 1 .. 5 (Case.__init__)
N_BANK, N_OBJ = 11, 4
BEST = [(0, 0), (1, 2), (1, 2), (3, 4), (1, 0), (3, 0), (1, 4)]   # (object, template) of the 7 proposals; 1 and 2 share a template


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------------------------ coverage
H, W = 215, 150
BOXES = [(3, 2, 53, 11), (5, 4, 14, 54), (149, 214, 150, 215), (20, 30, 48, 58), (7, 9, 138, 209),   # (h, w) = 9x50, 50x9, 1x1, 28x28, 200x131
         (0, 0, 0, 0), (10, 10, 40, 40), (100, 100, 151, 120)]                                        # empty; bad image_index; leaves the image
IMAGE_INDEX = [0, 1, 0, 1, 0, 1, 2, 0]
N_IMG = 2


@pytest.mark.parametrize("S", [28, 56, 42])
def test_coverage_is_exact(S):
    rng = np.random.default_rng(S)
    masks = ((rng.random((len(BOXES), H, W)) < 0.6) * rng.integers(1, 256, (len(BOXES), H, W))).astype(np.uint8)
    masks[2, 214, 149] = 9                  # the one-pixel box is set; any non-zero byte counts
    boxes, index = np.array(BOXES, np.int32), np.array(IMAGE_INDEX, np.int32)
    want = np.stack([ar.patch_cover(masks[p], BOXES[p], S, PS, IMAGE_INDEX[p], N_IMG) for p in range(len(BOXES))])
    assert not want[5:].any() and all(want[p].any() for p in range(5))
    got = ops.proposal_patch_cover(_dev(masks), _dev(boxes), S, PS, _dev(index), N_IMG)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(BOXES), (S // PS) ** 2)
    assert got.cpu().numpy().tolist() == want.tolist()
    # the same masks behind an odd byte offset
    shifted = torch.zeros(masks.size + 1, dtype=torch.uint8, device="cuda")
    shifted[1:] = _dev(masks).flatten()
    got2 = ops.proposal_patch_cover(shifted[1:].view(len(BOXES), H, W), _dev(boxes), S, PS, _dev(index), N_IMG)
    assert torch.equal(got2, got)
    # alone and without an index table (proposal p reads image p): a row depends on its own data only
    for p in (0, 4):
        alone = ops.proposal_patch_cover(_dev(masks[p:p + 1]), _dev(boxes[p:p + 1]), S, PS)
        assert torch.equal(alone[0], got[p])


def test_coverage_refusals():
    m, b = torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda"), torch.zeros(1, 4, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="multiple"):
        ops.proposal_patch_cover(m, b, 30, 14)
    out = torch.zeros(1, 4, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.FoundPoseNativeError, match="multiple"):
        _lib.call("fp_proposal_patch_cover", _lib.ptr(m), 1, 8, 8, None, _lib.ptr(b), 1, 30, 14, _lib.ptr(out), _lib.stream())


# ------------------------------------------------------------------------------------------------ the score
class Case:
    """Random unit rows, random coverage, one device call and its fp64 reference -- made once per shape and left unchanged."""

    def __init__(self, Np, D):
        rng = np.random.default_rng(1000 * Np + D)
        P = len(BEST)
        self.Np, self.D, self.P = Np, D, P
        self.q = ops.normalize_rows(_dev(rng.standard_normal((P * Np, D)).astype(np.float32))).view(P, Np, D)
        self.bank = ops.normalize_rows(_dev(rng.standard_normal((N_BANK * Np, D)).astype(np.float32))).view(N_BANK, Np, D)
        self.q_cover = rng.integers(0, 197, (P, Np)).astype(np.int32)
        self.bank_cover = rng.integers(0, 197, (N_BANK, Np)).astype(np.int32)
        self.q_cover[:, 0] = 150          # every row has a valid patch
        self.bank_cover[:, Np - 1] = 150
        self.bank[6:11] = self.bank[1:6]  # the fourth object is a copy of the second: descriptors and coverage
        self.bank_cover[6:11] = self.bank_cover[1:6]
        self.best_obj = np.array([o for o, _ in BEST], np.int32)
        self.best_tpl = np.array([t for _, t in BEST], np.int32)
        self.best_score = rng.random(P).astype(np.float32)
        self.rows = ar.template_rows(OBJ_OFF, N_BANK, self.best_obj, self.best_tpl)
        self.out = self.run()
        self.sim64 = ar.similarities_f64(self.q.cpu().numpy(), self.bank.cpu().numpy(), self.rows)

    def run(self, sel=None, q=None, bank=None, q_cover=None, bank_cover=None, obj_off=OBJ_OFF, best_obj=None, best_tpl=None):
        sel = list(range(self.P)) if sel is None else sel
        pick = lambda x: _dev(np.asarray(x)[sel])
        q = self.q if q is None else q
        out = ops.proposal_appearance(q[sel].contiguous(), pick(self.q_cover if q_cover is None else q_cover), self.bank if bank is None else bank,
                                      _dev(self.bank_cover if bank_cover is None else bank_cover), _dev(np.array(obj_off, np.int32)),
                                      pick(self.best_obj if best_obj is None else best_obj), pick(self.best_tpl if best_tpl is None else best_tpl),
                                      pick(self.best_score), MIN_COVER)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]   # score, appearance, n_valid, status, best_sim, best_patch


_CASES = {}


def case(Np, D):
    if (Np, D) not in _CASES:
        _CASES[(Np, D)] = Case(Np, D)
    return _CASES[(Np, D)]


SHAPES = [(Np, D) for Np in (1, 16, 130, 256) for D in (20, 384)]


@pytest.mark.parametrize("Np,D", SHAPES)
def test_best_similarities_are_within_the_chain_bound(Np, D):
    c = case(Np, D)
    score, app, n_valid, status, best_sim, best_patch = c.out
    bound = D * 2.0 ** -24
    assert c.rows == [0, 3, 3, 10, 1, 6, 5] and status.tolist() == [0] * c.P
    worst = 0.0
    for p, r in enumerate(c.rows):
        qv, tv = c.q_cover[p] >= MIN_COVER, c.bank_cover[r] >= MIN_COVER
        assert (best_patch[p][~qv] == -1).all() and not best_sim[p][~qv].any()
        masked = np.where(tv[None, :], c.sim64[p], -np.inf)
        top = masked.max(1)
        js = np.nonzero(qv)[0]
        assert tv[best_patch[p, js]].all() and (best_patch[p, js] >= 0).all()
        e1 = np.abs(best_sim[p, js].astype(np.float64) - top[js]).max()
        e2 = np.abs(c.sim64[p, js, best_patch[p, js]] - top[js]).max()
        worst = max(worst, e1, e2)
        assert n_valid[p] == qv.sum()
    print(f"Np {Np} D {D}: max |device - fp64| of the best similarity and of the similarity at the device's argmax = {worst:.3g} (bound {bound:.3g})")
    assert worst <= bound


@pytest.mark.parametrize("Np,D", SHAPES)
def test_a_copy_of_an_object_gives_the_same_bits(Np, D):
    """Query row t sent to template t of the second object and to template t of its copy: other rows of the bank, the same bytes."""
    c = case(Np, D)
    assert torch.equal(c.bank[6:11], c.bank[1:6]) and (c.bank_cover[6:11] == c.bank_cover[1:6]).all()
    assert not torch.equal(c.bank[1], c.bank[2])                      # ... and the templates of an object differ from one another
    props = [t for t in range(5) for _ in (0, 1)]
    best_obj = np.array([1, 3] * 5, np.int32)
    best_tpl = np.array(props, np.int32)
    assert ar.template_rows(OBJ_OFF, N_BANK, best_obj, best_tpl) == [1, 6, 2, 7, 3, 8, 4, 9, 5, 10]
    out = ops.proposal_appearance(c.q[props].contiguous(), _dev(c.q_cover[props]), c.bank, _dev(c.bank_cover), _dev(np.array(OBJ_OFF, np.int32)),
                                  _dev(best_obj), _dev(best_tpl), _dev(c.best_score[props]), MIN_COVER)
    score, app, n_valid, status, best_sim, best_patch = (o.cpu().numpy() for o in out)
    assert status.tolist() == [0] * 10
    for o in (score, app, n_valid, status, best_sim, best_patch):
        assert o[0::2].tobytes() == o[1::2].tobytes()
    assert c.rows[6] == 5 and c.rows[3] == 10                          # best (1, 4) is row 5, best (3, 4) row 10: checked against fp64 above


@pytest.mark.parametrize("Np,D", SHAPES)
def test_the_rest_replays_bit_for_bit(Np, D):
    c = case(Np, D)
    score, app, n_valid, status, best_sim, best_patch = c.out
    w_app, w_nv, w_st, w_score = ar.replay_from_best(best_sim, c.q_cover, c.bank_cover, c.rows, c.best_score, MIN_COVER)
    assert app.tobytes() == w_app.tobytes() and score.tobytes() == w_score.tobytes()
    assert n_valid.tolist() == w_nv.tolist() and status.tolist() == w_st.tolist()
    assert np.isfinite(app).all() and (np.abs(app) <= 1 + 1e-5).all()


@pytest.mark.parametrize("Np,D", [(16, 20), (130, 384), (256, 20)])
def test_the_whole_replay_from_fp64_similarities_names_the_same_patches(Np, D):
    """The device's own chain differs from fp64 by less than the bound; where the two best candidates are further apart than twice the
    bound the argmax must be the restatement's."""
    c = case(Np, D)
    best_sim, best_patch = c.out[4], c.out[5]
    w_sim, w_patch = ar.replay(c.sim64, c.q_cover, c.bank_cover, c.rows, c.best_score, MIN_COVER)[:2]
    bound = D * 2.0 ** -24
    for p, r in enumerate(c.rows):
        tv = c.bank_cover[r] >= MIN_COVER
        srt = np.sort(np.where(tv[None, :], c.sim64[p], -np.inf), 1)
        clear = (srt[:, -1] - (srt[:, -2] if Np > 1 else -np.inf) > 2 * bound) & (c.q_cover[p] >= MIN_COVER)
        assert (best_patch[p][clear] == w_patch[p][clear]).all()
        assert (best_patch[p][c.q_cover[p] < MIN_COVER] == -1).all() and (w_patch[p][c.q_cover[p] < MIN_COVER] == -1).all()
    assert np.abs(best_sim.astype(np.float64) - w_sim.astype(np.float64)).max() <= 2 * bound


@pytest.mark.parametrize("Np,D", [(16, 20), (130, 384)])
def test_an_exact_tie_goes_to_the_lower_patch(Np, D):
    c = case(Np, D)
    bank, q = c.bank.clone(), c.q.clone()
    cover = c.bank_cover.copy()
    row = c.rows[0]
    pairs = [(2, 5)] + ([(1, 129), (3, 128)] if Np > 129 else [])   # two lanes of one tile; one lane of two tiles; two lanes of two tiles
    for k, (lo, hi) in enumerate(pairs):
        bank[row, hi] = bank[row, lo]                              # identical bytes
        q[0, k] = bank[row, lo]                                    # ... and the query patch that matches them best
        cover[row, lo] = cover[row, hi] = 150
    q_cover = c.q_cover.copy()
    q_cover[0, :len(pairs)] = 150
    out = c.run(q=q, bank=bank, bank_cover=cover, q_cover=q_cover)
    for k, (lo, hi) in enumerate(pairs):
        assert out[5][0, k] == lo and out[4][0, k] >= 1 - D * 2.0 ** -24
    # and when the lower twin is invalid the upper one wins
    cover[row, pairs[0][0]] = 0
    assert c.run(q=q, bank=bank, bank_cover=cover, q_cover=q_cover)[5][0, 0] == pairs[0][1]


@pytest.mark.parametrize("Np,D", [(16, 20), (130, 384)])
def test_a_nan_never_wins(Np, D):
    c = case(Np, D)
    bank = c.bank.clone()
    cover = c.bank_cover.copy()
    row, bad = c.rows[0], 7
    bank[row, bad, 0] = float("nan")
    cover[row, bad] = 150
    out = c.run(bank=bank, bank_cover=cover)
    score, app, n_valid, status, best_sim, best_patch = out
    assert (best_patch[0] != bad).all() and np.isfinite(best_sim[0]).all() and np.isfinite(app[0]) and status[0] == 0
    keep = cover[row] >= MIN_COVER
    keep[bad] = False
    top = np.where(keep[None, :], c.sim64[0], -np.inf).max(1)
    js = np.nonzero(c.q_cover[0] >= MIN_COVER)[0]
    assert np.abs(best_sim[0, js] - top[js]).max() <= D * 2.0 ** -24
    for o_new, o_old in zip(out, c.out):                              # the other proposals read other templates: not a bit changes
        assert o_new[1:].tobytes() == o_old[1:].tobytes()


@pytest.mark.parametrize("Np,D", [(16, 20), (130, 384)])
def test_an_invalid_template_patch_never_wins(Np, D):
    c = case(Np, D)
    bank, cover = c.bank.clone(), c.bank_cover.copy()
    row, planted = c.rows[0], Np - 2
    bank[row, planted] = c.q[0, 0]            # similarity 1 with query patch 0 of proposal 0: the largest of its row
    cover[row, planted] = MIN_COVER - 1       # ... one pixel short of valid
    out = c.run(bank=bank, bank_cover=cover)
    assert out[5][0, 0] != planted and out[4][0, 0] < 0.9 and (out[5][0] != planted).all()
    cover[row, planted] = MIN_COVER           # ... and with that pixel it wins
    out = c.run(bank=bank, bank_cover=cover)
    assert out[5][0, 0] == planted and out[4][0, 0] >= 1 - D * 2.0 ** -24


@pytest.mark.parametrize("Np,D", [(16, 20), (130, 384)])
def test_a_row_is_the_same_bits_alone_permuted_and_embedded(Np, D):
    c = case(Np, D)
    for p in (1, 3):
        alone = c.run(sel=[p])
        for a, full in zip(alone, c.out):
            assert a[0].tobytes() == full[p].tobytes()
    perm = [4, 2, 6, 0, 5, 1, 3]
    for a, full in zip(c.run(sel=perm), c.out):
        assert a.tobytes() == full[perm].tobytes()
    emb = [5, 5, 1, 0, 3, 6, 6, 2, 4, 1]
    for a, full in zip(c.run(sel=emb), c.out):
        assert a.tobytes() == full[emb].tobytes()


@pytest.mark.parametrize("Np,D", [(16, 20), (130, 384)])
def test_statuses(Np, D):
    c = case(Np, D)
    # object -1 and O; a template beyond its object's count (object 0 has one, object 2 none); the rest as before
    best_obj = np.array([-1, N_OBJ, 0, 2, 1, 3, 1], np.int32)
    best_tpl = np.array([0, 0, 1, 0, 0, -1, 4], np.int32)
    q_cover, bank_cover = c.q_cover.copy(), c.bank_cover.copy()
    rows = ar.template_rows(OBJ_OFF, N_BANK, best_obj, best_tpl)
    assert rows == [-1, -1, -1, -1, 1, -1, 5]
    wild = [-5, 1, 6, 2, 99]                  # out of range and decreasing: clamped to OBJ_OFF before anything is read
    assert ar.template_rows(wild, N_BANK, best_obj, best_tpl) == rows
    for off in (OBJ_OFF, wild):
        score, app, n_valid, status, best_sim, best_patch = c.run(obj_off=off, best_obj=best_obj, best_tpl=best_tpl)
        assert status.tolist() == [2, 2, 2, 2, 0, 2, 0] and n_valid[:4].tolist() == [0] * 4 and n_valid[5] == 0
        for p in (0, 1, 2, 3, 5):
            assert app[p] == 0 and not best_sim[p].any() and (best_patch[p] == -1).all()
            assert score[p] == np.float32(c.best_score[p] * np.float32(0.5))
        w = ar.replay_from_best(best_sim, q_cover, bank_cover, rows, c.best_score, MIN_COVER)
        assert app.tobytes() == w[0].tobytes() and score.tobytes() == w[3].tobytes()
        assert best_sim[6].tobytes() == c.out[4][6].tobytes() and best_patch[6].tobytes() == c.out[5][6].tobytes()   # proposal 6 kept its template
    # status 1: no valid query patch; status 3: the template has no valid patch; both: 1
    q_cover[0] = MIN_COVER - 1
    q_cover[4] = 0
    bank_cover[c.rows[1]] = MIN_COVER - 1     # proposals 1 and 2 share this template
    bank_cover[c.rows[4]] = 0
    score, app, n_valid, status, best_sim, best_patch = c.run(q_cover=q_cover, bank_cover=bank_cover)
    assert status.tolist() == [1, 3, 3, 0, 1, 0, 0]
    assert n_valid.tolist() == [0] + [(c.q_cover[p] >= MIN_COVER).sum() for p in (1, 2, 3)] + [0] + [(c.q_cover[p] >= MIN_COVER).sum() for p in (5, 6)]
    for p in (0, 1, 2, 4):
        assert app[p] == 0 and not best_sim[p].any() and (best_patch[p] == -1).all() and score[p] == np.float32(c.best_score[p] * np.float32(0.5))
    for p in (3, 5, 6):
        assert best_sim[p].tobytes() == c.out[4][p].tobytes() and score[p] == c.out[0][p]
    # -inf stays -inf
    c2 = ops.proposal_appearance(c.q[:1].contiguous(), _dev(c.q_cover[:1]), c.bank, _dev(c.bank_cover), _dev(np.array(OBJ_OFF, np.int32)),
                                 _dev(np.array([-1], np.int32)), _dev(np.array([-1], np.int32)), _dev(np.array([-np.inf], np.float32)), MIN_COVER)
    assert c2[0].cpu().numpy()[0] == -np.inf and int(c2[3][0]) == 2


def test_refused_shapes():
    i32 = torch.int32

    def call(P, Np, D, min_cover=1):
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
        return ops.proposal_appearance(z(P, Np, D), z(P, Np, dt=i32), z(2, Np, D), z(2, Np, dt=i32), torch.tensor([0, 2], dtype=i32, device="cuda"),
                                       z(P, dt=i32), z(P, dt=i32), z(P), min_cover)
    for P, Np, D in ((1, 4, 18), (1, 4, 4100), (1, 0, 4), (1, 8193, 4), (65536, 1, 4)):
        with pytest.raises(ValueError, match="proposal_appearance"):
            call(P, Np, D)
    with pytest.raises(ValueError, match="min_cover"):
        call(1, 4, 4, 0)
    assert call(0, 4, 4)[0].numel() == 0      # no proposal: no launch
    # the library refuses them itself
    z = torch.zeros(64, dtype=torch.float32, device="cuda")
    zi = torch.zeros(64, dtype=i32, device="cuda")
    for Np, D, mc in ((4, 6, 1), (8193, 4, 1), (4, 4, 0)):
        with pytest.raises(_lib.FoundPoseNativeError, match="proposal_appearance"):
            _lib.call("fp_proposal_appearance", _lib.ptr(z), _lib.ptr(zi), 1, Np, D, _lib.ptr(z), _lib.ptr(zi), 1, _lib.ptr(zi), 1, _lib.ptr(zi), _lib.ptr(zi),
                      _lib.ptr(z), mc, _lib.ptr(z), _lib.ptr(zi), _lib.ptr(z), _lib.ptr(zi), _lib.ptr(zi), _lib.ptr(z), _lib.stream())
