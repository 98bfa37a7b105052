"""tests/pnp_ref.py -- the numpy restatement of fp_pnp_ransac / fp_pnp_ransac_keyed -- checked on its own, and the fixtures of
tests/test_gpu_pnp_restatement.py built and their conditions asserted, all without a GPU: the sampler against index quadruples written out
as literals (they were cross-checked once against a C++ transcription of the kernel's loop), its distinctness and uniformity, the exact path
on noise-free samples, the interval replay against the plain one and against hand-made count sequences, and for every fixture that it is
decided, identifiable and within the fragile cap."""

import numpy as np
import pytest

from tests import pnp_ref as pr

FRAGILE_CAP = 0.05


# ------------------------------------------------------------------------------------------------------------------------- the sampler
@pytest.mark.parametrize("seed, key, h, N, ids", [
    (0, 0, 0, 40, [15, 33, 16, 6]),
    (7, 3, 299, 40, [16, 28, 30, 20]),
    ((1 << 63) + 12345, 5, 17, 300, [36, 4, 113, 139]),                  # seed >= 2^63
    (11, (1 << 63) + 5, 1023, 64, [15, 42, 26, 12]),                     # a key with the top bit set
    ((1 << 64) - 1, (1 << 64) - 1, 4095, 4096, [1677, 1862, 2916, 3408]),
    (1, 2, 3, 4, [3, 0, 1, 2]),                                          # N = 4: a permutation
    ((1 << 63) + 1, 1 << 40, 0, 4, [0, 1, 2, 3]),
    (5, 2047, 0, 7, [0, 1, 2, 6]),
])
def test_sampler_literals(seed, key, h, N, ids):
    assert pr.sample4(pr.hyp_key(pr.pair_base(seed, key), h), N) == ids


def test_an_int64_key_is_read_as_its_uint64_bits():
    as_int64 = int(np.array([-(1 << 63) + 5], np.int64)[0])
    assert pr.pair_base(11, as_int64) == pr.pair_base(11, (1 << 63) + 5)
    assert pr.pair_base(11, -1) == pr.pair_base(11, (1 << 64) - 1)
    # every part of the seed and of the key is read (the two are combined by xor: varied one at a time)
    parts = (0, 1, 1 << 31, 1 << 32, 1 << 63)
    assert len({pr.pair_base(s, 9) for s in parts}) == len(parts) and len({pr.pair_base(9, k) for k in parts}) == len(parts)


def test_sampler_draws_distinct_indices_uniformly():
    hist = np.zeros(7, np.int64)
    base = pr.pair_base(3, 1)
    for h in range(20000):
        ids = pr.sample4(pr.hyp_key(base, h), 7)
        assert len(set(ids)) == 4
        hist[ids] += 1
    assert np.all(np.abs(hist / (20000 * 4 / 7) - 1.0) < 0.05), hist


# --------------------------------------------------------------------------------------------------------------------- the exact path
def test_exact_path_reprojects_noise_free_samples():
    rng = np.random.default_rng(4)
    worst, fragile = 0.0, 0
    for i in range(2000):
        X, uv, _ = pr.scene(rng, 4, 0, 0.0, pr.CAM_A, as_float32=False)
        H = pr.hypothesis(pr.hyp_key(pr.pair_base(0, i), 0), X.astype(np.float64), uv, pr.CAM_A)
        if H.fragile:
            fragile += 1
            continue
        assert H.pose is not None, i
        worst = max(worst, float(H.err.max()))
        assert H.counts(pr.THRESH) == (4, 4)
    print(f"2000 noise-free four-point samples: {fragile} fragile, the others re-project to {worst:.3e} px")
    assert worst < 1e-6 and fragile <= FRAGILE_CAP * 2000


def test_runner_up_rule():
    assert not pr.runner_up_is_close(np.array([1.0]), [1e-6])
    assert pr.runner_up_is_close(np.array([1.0, 1.0 + 7e-6]), [1e-6, 1e-6])          # within 4 x (1e-6 + 1e-6)
    assert not pr.runner_up_is_close(np.array([1.0 + 9e-6, 1.0]), [1e-6, 1e-6])
    assert pr.runner_up_is_close(np.array([100.0, 300.0, 101.0]), [0.2, 1e-6, 0.1])  # the runner-up is the third


# -------------------------------------------------------------------------------------------------------------------------- the replay
def _as_intervals(cnt, asked=None):
    def get(h):
        if asked is not None:
            asked.append(h)
        return cnt[h], cnt[h], False
    return get


def test_interval_replay_reduces_to_the_plain_replay():
    rng = np.random.default_rng(8)
    for trial in range(200):
        N = int(rng.integers(6, 60))
        cnt = rng.integers(0, N + 1, size=int(rng.integers(1, 400))).tolist()
        conf = float(rng.choice([0.5, 0.9, 0.99]))
        plain = pr.replay_counts(cnt, N, conf)
        best, best_c, niters, _ = pr.replay(_as_intervals(cnt), len(cnt), N, conf)
        assert (best, best_c, niters) == plain


def test_replay_rules_on_hand_made_counts():
    # the first best wins; the tie later in the sequence does not
    cnt = [0, 5, 3, 9, 9, 4] + [0] * 94
    assert pr.replay_counts(cnt, 40, 0.99)[:2] == (3, 9)
    assert pr.replay(_as_intervals(cnt), 100, 40, 0.99)[:2] == (3, 9)
    # 30 of 40 inliers at h = 0: log(0.01) / log(1 - 0.75^4) = 12.1 -> a budget of 12; the better model at h = 12 is never visited,
    # the one at h = 11 is
    cnt = [30] + [0] * 99
    cnt[12] = 40
    asked = []
    assert pr.replay(_as_intervals(cnt, asked), 100, 40, 0.99) == (0, 30, 12, True)
    assert asked == list(range(12))
    assert pr.replay_counts(cnt, 40, 0.99) == (0, 30, 12)
    cnt[11] = 40
    assert pr.replay_counts(cnt, 40, 0.99)[:2] == (11, 40) and pr.replay(_as_intervals(cnt), 100, 40, 0.99)[:2] == (11, 40)
    # no count exceeds 3: no model
    assert pr.replay_counts([3, 0, 2, 3], 40, 0.99) == (-1, 3, 4)
    assert pr.replay(_as_intervals([3, 0, 2, 3]), 4, 40, 0.99) == (-1, 3, 4, True)
    # an arg-max over the whole budget would have taken the later, higher count
    cnt = [0, 28, 0, 0] + [0] * 20 + [33] + [0] * 75      # 28 of 40 at h = 1: a budget of 17
    assert pr.replay_counts(cnt, 40, 0.99)[:2] == (1, 28) and int(np.argmax(cnt)) == 24


def test_replay_decidedness():
    iv = [(0, 0, False), (10, 10, False), (0, 9, True), (5, 12, False), (0, 10, True)]
    get = lambda seq: (lambda h: seq[h])
    assert pr.replay(get(iv[:3]), 3, 40, 0.99)[3]                 # a fragile hypothesis that cannot beat the best: still decided
    assert not pr.replay(get(iv[:4]), 4, 40, 0.99)[3]             # an interval that straddles the best count
    assert pr.replay(get(iv[:3] + iv[4:]), 4, 40, 0.99)[3]        # cnt_hi == best_c does not beat it (strict >)
    assert not pr.replay(get([(0, 11, True)]), 1, 40, 0.99)[3]    # a fragile hypothesis that could
    assert not pr.replay(get([(7, 7, True)]), 1, 40, 0.99)[3]


# ------------------------------------------------------------------------------------------------------- the GPU tests' fixtures
def test_sweep_fixture_leaves_out_at_most_five_percent():
    fix = pr.sweep_fixture()
    hyps = pr.sweep_hypotheses(fix)
    fragile = sum(H.fragile for H in hyps)
    open_counts = sum((not H.fragile) and H.counts(fix["thresh"])[0] != H.counts(fix["thresh"])[1] for H in hyps)
    models = sum((not H.fragile) and H.counts(fix["thresh"])[0] > 3 for H in hyps)
    print(f"hypothesis sweep: {fragile} of {len(hyps)} fragile, {open_counts} with an open count interval, {models} certain models")
    assert fragile + open_counts <= FRAGILE_CAP * len(hyps)
    assert models >= 0.2 * len(hyps)      # 0.7^4 of the samples are all inliers


def test_four_point_fixture():
    fix = pr.four_point_fixture(1024)    # (the GPU test builds all 4 096)
    hyps = pr.four_point_hypotheses(fix)
    fragile = sum(H.fragile for H in hyps)
    print(f"four-point sweep: {fragile} of {len(hyps)} fragile")
    assert fragile <= FRAGILE_CAP * len(hyps)
    for H in hyps:
        assert H.fragile or (H.pose is not None and H.counts(fix["thresh"]) == (4, 4))


@pytest.fixture(scope="module")
def replay_fix():
    return pr.replay_fixture()


@pytest.mark.parametrize("keyed", [False, True])
def test_replay_fixture_is_decided_and_identifiable(replay_fix, keyed):
    fix, cache = replay_fix, {}
    keys = pr.REPLAY_KEYS if keyed else None
    assert fix["seed"] >= 1 << 63 and fix["counts"].tolist() == [40, 0, 5, 57, 6, 40] and fix["cams"][0] != fix["cams"][1]
    assert min(min(r) for r in pr.REPLAY_KEYS) < 0     # keys with the top bit set
    winners = []
    for conf in (0.99, 0.5):
        ref = pr.run_ref_on(fix, conf, keys, refine=False, cache=cache)
        assert pr.fixture_conditions(fix, ref) == []
        assert ref["success"].tolist() == [True, False, False, True, True, False]        # the last pair is all outliers
        assert ref["quality"][3] <= 40 and ref["quality"][4] == 6
        winners.append(ref["best_h"].tolist())
        # the noisy pair's count climbs in several steps
        steps, best_c = 0, 3
        for h in range(int(ref["best_h"][0]) + 1):
            lo, _ = ref["hyps"][0][h].counts(fix["thresh"])
            if lo > best_c:
                best_c, steps = lo, steps + 1
        assert steps >= 2 and len(ref["history"][0]) == steps, steps
        assert len(ref["hyps"][5]) == 300       # no model: the whole budget is visited, the hypothesis loop's second trip included
    if keyed:
        assert winners[0] != winners[1]         # the confidence decides where the replay stops ...
        assert pr.budget_is_tight(fix, ref, 0, keys)   # ... (ref: confidence 0.5) and a budget a little shorter or longer gives another winner
        assert fix["counts"][0] >= 6 and fix["counts"][3] >= 6 and keys[0][0] < 0 and keys[1][0] < 0    # top-bit keys on pairs that are solved
    swapped = pr.run_ref_on(fix, 0.99, keys, cams=fix["cams"][::-1], refine=False)
    for p in (0, 3, 4):
        assert not (np.array_equal(swapped["ransac_R"][p], ref["ransac_R"][p]) and np.array_equal(swapped["inliers"][p], ref["inliers"][p]))


def test_late_winner_fixture():
    fix = pr.late_winner_fixture()
    ref = pr.run_ref_on(fix, refine=False)
    assert pr.fixture_conditions(fix, ref, gap_factor=2.0) == []
    assert ref["best_h"][0] >= 256 and ref["quality"][0] == 16 and ref["niters"][0] == 1024


def test_lds_limit_fixture():
    fix = pr.lds_fixture()
    assert fix["K"] == 4096 and fix["iters"] == 4096 and fix["counts"].tolist() == [4096, 4196]
    ref = pr.run_ref_on(fix, pair_keys=pr.LDS_KEYS, refine=False)
    assert pr.fixture_conditions(fix, ref) == []
    assert ref["success"].all() and np.all(ref["quality"] >= 2048) and np.all(ref["niters"] < 100)
