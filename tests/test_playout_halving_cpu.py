"""CPU: the statement of tarok_playout_cards_halving (tests/playout_halving_model.py) against brute force and against the
uniform models it is built on, the mutants of the survivor rule it kills, the argument checks of the two new C calls
(before any HIP call) and the rules of playout.card_player(halving=...).  No GPU involved."""
import ctypes
import inspect

import numpy as np
import pytest

import playout_det_model as DM
import playout_halving_model as HM
import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

SEED, SALT = 23, 5


def brute(values, alive):
    """max(1, ceil(k / 2)) survivors by counting, for every rank, the alive ranks that beat it."""
    keep = max(1, -(-len(alive) // 2))
    return [j for j in alive if sum(1 for i in alive if values[i] > values[j] or (values[i] == values[j] and i < j)) < keep]


def test_the_survivor_rule_equals_brute_force_with_planted_ties():
    rnd = np.random.RandomState(1)
    for k in range(1, 13):
        for trial in range(200):
            alive = sorted(rnd.choice(12, k, replace=False).tolist())
            v = rnd.randint(-3, 4, 12) if trial % 2 else rnd.randint(-10 ** 6, 10 ** 6, 12)
            got = HM.survivors(v, alive)
            assert got == brute(v, alive) and len(got) == max(1, (k + 1) // 2) and set(got) <= set(alive)
    assert HM.survivors(np.zeros(12), list(range(12))) == [0, 1, 2, 3, 4, 5]          # ties to the lower rank


def chain(nlegal, round_worlds, samples=1, seed=0, rule=HM.survivors):
    rnd = np.random.RandomState(seed)
    scores = rnd.randint(-70, 71, (12, sum(round_worlds), samples, 4)).astype(np.int64)
    scores[nlegal:] = 0
    return scores, HM.halve(scores, nlegal, 1, round_worlds, samples, rule)


def test_the_chains_and_the_counts():
    for nlegal, sizes in ((12, [12, 6, 3, 2]), (5, [5, 3, 2, 1]), (1, [1]), (2, [2, 1]), (3, [3, 2, 1])):
        scores, (sums, count, alive) = chain(nlegal, (2, 2, 4, 8))
        ends = [2, 4, 8, 16]
        played = sorted(count[:nlegal].tolist(), reverse=True)
        want = []
        for r, k in enumerate(sizes):
            if r > 0 and k == 1:                                    # down to one card: it plays no further round
                want.append(ends[r - 1])
                break
            want += [ends[r]] * (k - (sizes[r + 1] if r + 1 < len(sizes) else 0))
        assert played == sorted(want, reverse=True), (nlegal, played, want)
        assert not count[nlegal:].any() and not sums[nlegal:].any()
        assert len(alive) == sizes[-1]
        for j in range(nlegal):                                     # the row-by-count prefix property
            assert (sums[j] == scores[j, :count[j]].sum(axis=(0, 1))).all()


def test_one_round_is_the_uniform_model_and_the_final_card_is_alive():
    for gidx, cards in ((0, 0), (1, 5), (2, 13), (3, 34), (4, 46), (5, 22)):
        g = O.Game.synth(SEED, gidx, 0, S.MIX_BOT)
        key = O.game_key(SEED, gidx, 0)
        for q in range(cards):
            g.step(O.policy_action(key, q, g.legal()))
        lanes = g.lanes()
        scores = DM.playout_scores(lanes, 0, SEED, SALT, gidx, 15, 4, 2)
        sums, count, card = HM.playout_cards_halving("det", lanes, 0, SEED, SALT, gidx, 15, (4,), 2, scores=scores)
        want, want_card = DM.playout_cards(lanes, 0, SEED, SALT, gidx, 15, 4, 2)
        nl = len(PM.cards_of(g.legal()))
        assert (sums == want).all() and card == want_card and count[:nl].tolist() == [8] * nl and not count[nl:].any()
        sums, count, card = HM.playout_cards_halving("det", lanes, 0, SEED, SALT, gidx, 15, (1, 1, 2), 2, scores=scores)
        legal = PM.cards_of(g.legal())
        assert card in legal and count[legal.index(card)] == count.max()
        for j in range(nl):
            assert int(count[j]) in (2, 4, 8) and (sums[j] == DM.sums_of(scores, int(count[j]) // 2, 2)[j]).all()
        z = HM.playout_cards_halving("det", lanes, 0, SEED, SALT, gidx, 0, (1, 1), 1)
        assert not z[0].any() and not z[1].any() and z[2] == PM.card_of(lanes, SEED, gidx, 0, 0, z[0])


def test_three_mutants_of_the_rule_are_killed():
    """The mutants replace the MODEL's rule and are told apart from it on the model's own chains.  The device rule is not
    run here: tests/test_halving_host.py ties halve_alive to the model's sort, so a device rule with one of these faults
    fails there."""
    def higher(values, alive):                                 # ties to the HIGHER rank
        keep = max(1, (len(alive) + 1) // 2)
        return sorted(sorted(alive, key=lambda j: (-int(values[j]), -j))[:keep])

    def floor(values, alive):                                  # floor instead of ceil
        return sorted(sorted(alive, key=lambda j: (-int(values[j]), j))[:max(1, len(alive) // 2)])

    class Stale:                                               # compares the sums of the round before
        def __init__(self):
            self.seen = None

        def __call__(self, values, alive):
            old, self.seen = self.seen, np.array(values).copy()
            return HM.survivors(values if old is None else old, alive)
    killed = {"higher": 0, "floor": 0, "stale": 0}
    for seed in range(40):
        nlegal = 12 if seed % 2 else 5
        scores = np.random.RandomState(seed).randint(-70, 71, (12, 8, 1, 4)).astype(np.int64)
        scores[nlegal:] = 0
        scores[:, :, :, 1] //= 24                              # few distinct values in the mover's column: ties
        s0, c0, a0 = HM.halve(scores, nlegal, 1, (1, 1, 2, 4), 1)
        for name, rule in (("higher", higher), ("floor", floor), ("stale", Stale())):
            s1, c1, a1 = HM.halve(scores, nlegal, 1, (1, 1, 2, 4), 1, rule)
            killed[name] += int((c1 != c0).any() or a1 != a0)
    assert all(v >= 5 for v in killed.values()), killed


def test_the_counts_target_reference_and_its_bound():
    sums = np.zeros((3, 12, 4), np.int64)
    counts = np.zeros((3, 12), np.int64)
    word = (0b10110 | (2 << 54))                               # three legal cards 1, 2, 4; seat 2
    sums[0, :3, 2], counts[0, :3] = (40, 90, 10), (2, 4, 0)
    sums[1, :3, 2], counts[1, :3] = (30, 30, 99), (4, 4, 2)
    q, has, card, big = HM.targets_counts_reference(sums, counts, [word] * 3, 8.0, 15)
    e = np.exp((np.array([20.0, 22.5]) - 22.5) / 8.0)
    assert np.allclose(q[0, [1, 2]], e / e.sum()) and q[0, 4] == 0 and abs(q[0].sum() - 1) < 1e-12 and big[0] == 22.5
    assert card.tolist() == [2, 1, 255] and has.all() and not q[2].any()
    q0 = HM.targets_counts_reference(sums, counts, [word] * 3, 0.0, 15)[0]
    assert q0[0, 2] == 1 and q0[1, 1] == 1 and q0.sum() == 2
    b = HM.targets_counts_bound(q, big, 8.0)
    assert (b[q == 0] == 0).all() and (b[q > 0] < q[q > 0] * 2.0 ** -7).all() and (b[q > 0] > q[q > 0] * 2.0 ** -8).all()


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- before the dlopen: one HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_both_calls_validate_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough."""
    z = ctypes.c_void_p(0)
    env = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    out = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    arr = lambda *w: (ctypes.c_int * len(w))(*w)
    f = L.tarok_playout_cards_halving
    ok = (0, z, 2, arr(2, 2), 1, 0, 15, z, out, out, out, z)

    def call(env_=env, **kw):
        a = list(ok)
        for k, v in kw.items():
            a[("kind", "words", "rounds", "round_worlds", "samples", "salt", "seats", "spg", "sum", "count", "action").index(k)] = v
        return f(env_, *a)
    assert call(None) == -1
    for kw in (dict(rounds=0), dict(rounds=5, round_worlds=arr(1, 1, 1, 1, 1)), dict(round_worlds=z), dict(round_worlds=arr(2, 0)),
               dict(round_worlds=arr(2, -1)), dict(round_worlds=arr(32, 33)), dict(rounds=1, round_worlds=arr(65)), dict(kind=3), dict(kind=-1),
               dict(kind=1), dict(kind=2), dict(kind=0, words=out), dict(samples=0), dict(samples=1025), dict(seats=16), dict(seats=-1),
               dict(sum=z, count=z, action=z)):
        assert call(**kw) == -1, kw
    g = L.tarok_playout_targets_counts
    assert g(None, out, out, out, 1.0, 15, z, out, z) == -1
    for hole in range(4):
        a = [out, out, out, 1.0, 15, z, out, z]
        a[(0, 1, 2, 6)[hole]] = z
        assert g(env, *a) == -1
    for tau in (-1.0, float("nan"), float("inf"), 1e-45):
        assert g(env, out, out, out, tau, 15, z, out, z) == -1
    for seats in (-1, 16):
        assert g(env, out, out, out, 1.0, seats, z, out, z) == -1


def test_the_card_player_rules_and_the_surface():
    from tarok_amd import _native, karte
    from tarok_amd import evaluate as EV
    from tarok_amd import playout as P
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.selfplay import SelfPlay
    assert karte.PLAYOUT_MAX_ROUNDS == 4
    assert "tarok_playout_cards_halving" in _native.SYMBOLS and "tarok_playout_targets_counts" in _native.SYMBOLS
    sig = inspect.signature(TarokVecEnv.playout_cards_halving).parameters
    assert list(sig)[1:] == ["round_worlds", "samples", "voids", "hidden", "words", "salt", "seats", "seats_per_game", "sum_out", "count_out",
                             "action_out"]
    assert list(inspect.signature(TarokVecEnv.playout_targets_counts).parameters)[1:] == ["sums", "counts", "obs_words", "tau", "seats",
                                                                                          "seats_per_game", "target_out"]
    assert inspect.signature(EV.evaluate_playout_vs_bot).parameters["halving"].default is None
    assert inspect.signature(SelfPlay.evaluate).parameters["playout_halving"].default is None
    p = P.card_player(2, halving=(1, 2, 4), hidden=True, salt=3)
    assert (p.kind, p.worlds, p.samples, p.halving, p.salt, p.net, p.needs_history) == ("hidden", 7, 2, (1, 2, 4), 3, False, True)
    assert P.card_player(None, 7, halving=[1, 2, 4]).kind == "det" and P.card_player(1, 0, voids=True, halving=(3,)).kind == "voids"
    assert P.card_player(2, 3) == P.CardPlayer("det", 3, 2, False, 15, None, 70.0, 0) and P.card_player(2, 3).halving is None
    for kw in (dict(halving=()), dict(halving=(1, 1, 1, 1, 1)), dict(halving=(0, 2)), dict(halving=(2.0, 1)), dict(halving=(True, 1)), dict(halving=3),
               dict(halving=(32, 33)), dict(halving=(1, 2), worlds=4), dict(halving=(1, 2), net=True, worlds=3, samples=None),
               dict(halving=(1, 2), front=True), dict(halving=(1, 2), voids=True, hidden=True), dict(halving=(1, 2), hidden=True, history=False)):
        with pytest.raises(ValueError):
            P.card_player(**{"samples": 1, **kw})
    with pytest.raises(ValueError):
        EV.evaluate_playout_vs_bot(1, 8, 1, halving=(1, 2), exchange=2)
    with pytest.raises(ValueError):
        EV.evaluate_playout_vs_bot(1, 8, 1, halving=(1, 2), bidding=(2, 1))
    with pytest.raises(ValueError):
        EV.evaluate_playout_vs_bot(1, 8, 1, halving=(1, 2), worlds=2)
