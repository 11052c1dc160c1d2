"""CPU-side checks of the determinized Monte-Carlo playouts (tarok_playout_cards_det): the model of
tests/playout_det_model.py — what a world keeps, the team rule case by case, the uniformity of the walk, the prefix
property — and the argument validation of the entry point, which makes no HIP call and so runs without a GPU."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

import playout_det_model as DM
import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

SEED = 23
SALT = 6


def played_on(gidx, episode, mix, cards):
    """The synthetic game (SEED, gidx, episode) after `cards` Bot cards (or its end, if that comes first)."""
    g = O.Game.synth(SEED, gidx, episode, mix)
    key = O.game_key(SEED, gidx, episode)
    for q in range(cards):
        if g.done:
            break
        g.step(O.policy_action(key, q, g.legal()))
    return g


def hands(game):
    return [int(game.g.hand[s]) for s in range(4)]


def popcount(m):
    return bin(int(m)).count("1")


@pytest.mark.parametrize("cards", [0, 1, 2, 3, 5, 22, 46])
def test_a_world_keeps_everything_the_mover_can_see(cards):
    contracts, differ = set(), 0
    for gidx in range(120):
        g = played_on(gidx, 1, S.MIX_ALL, cards)
        if g.done:
            continue
        contracts.add(int(g.g.contract))
        seat = g.seat()
        before = g.lanes()
        for w in range(3):
            x = DM.world_of(g, DM.world_key(SEED, SALT, gidx, 1, int(g.g.trick_no) * 4 + int(g.g.n_in_trick), w))
            assert (g.lanes() == before).all()                               # the game itself is not touched
            h0, h1 = hands(g), hands(x)
            assert [popcount(m) for m in h1] == [popcount(m) for m in h0]    # the hand sizes
            pool0 = pool1 = 0
            for o in DM.others_of(seat):
                pool0 |= h0[o]
                pool1 |= h1[o]
            assert pool1 == pool0                                            # the union of the other hands
            assert all(h1[a] & h1[b] == 0 for a, b in itertools.combinations(range(4), 2))
            assert h1[seat] == h0[seat]                                      # the mover's hand,
            la, lb = g.lanes(), x.lanes()
            assert (la[4:9] == lb[4:9]).all()                                # the piles and the talon ids,
            team_field = np.uint64(15 << 42)
            assert (la[9] & ~team_field) == (lb[9] & ~team_field)            # and all of the rest but the team
            assert x.legal() == g.legal() and x.seat() == seat
            differ += h1 != h0
    assert len(contracts) >= (8 if cards < 22 else 5)                        # (the Beracs thin out as cards are played)
    if cards < 46:
        assert differ > 100


def king_case(g):
    """Where the called king of a game in play lies, as the team rule tells the cases apart."""
    if g.g.king < 0:
        return "no king"
    kb = 1 << (8 * int(g.g.king) + 7)
    seat = g.seat()
    if int(g.g.hand[seat]) & kb:
        return "mover"
    if any(int(g.g.hand[o]) & kb for o in DM.others_of(seat)):
        return "pool"
    if any((int(g.g.talon[i]) == 8 * int(g.g.king) + 7) for i in range(6)) and not any(int(g.g.pile[s]) & kb for s in range(4)):
        return "talon"
    return "played"


def test_the_team_rule_in_each_of_its_cases():
    seen = dict.fromkeys(("pool", "mover", "played", "talon", "no king"), 0)
    changed = 0
    for cards in (0, 6, 17, 30, 45):
        for gidx in range(150):
            g = played_on(gidx, 0, S.MIX_ALL if gidx % 3 == 0 else S.MIX_NAVADNA3, cards)
            if g.done:
                continue
            case = king_case(g)
            seen[case] += 1
            played = int(g.g.trick_no) * 4 + int(g.g.n_in_trick)
            for w in range(2):
                x = DM.world_of(g, DM.world_key(SEED, SALT, gidx, 0, played, w))
                if case == "pool":
                    kb = 1 << (8 * int(g.g.king) + 7)
                    (holder,) = [o for o in DM.others_of(g.seat()) if int(x.g.hand[o]) & kb]
                    assert int(x.g.team) == (1 << int(g.g.declarer)) | (1 << holder)
                    assert 1 <= popcount(x.g.team) <= 2
                    changed += int(x.g.team) != int(g.g.team)
                else:
                    assert int(x.g.team) == int(g.g.team), case
    assert all(v >= 10 for v in seen.values()), seen
    assert changed >= 50


def test_with_one_card_left_the_pool_is_empty_and_the_sum_is_the_score():
    seen = 0
    for gidx in range(16):
        g = played_on(gidx, 0, S.MIX_ALL, 47)
        if g.done:
            continue
        seen += 1
        assert sum(popcount(m) for m in hands(g)) == 1
        end = PM.copy_of(g)
        (card,) = PM.cards_of(end.legal())
        end.step(card)
        assert end.done
        for worlds, samples in ((1, 1), (5, 3)):
            sums, got = DM.playout_cards(g.lanes(), 0, SEED, SALT, gidx, 15, worlds, samples)
            assert sums[0].tolist() == [worlds * samples * x for x in end.scores] and not sums[1:].any() and got == card
    assert seen >= 8


def test_the_walk_is_uniform_over_the_arrangements():
    """Three unseen cards, capacities 1/1/1 (a game played to 44 cards): each of the 6 arrangements within 5 sigma of
    N / 6 over N = 6,000 (gidx, w) pairs, sigma^2 = N * (1/6) * (5/6).  Deterministic: it ran once and stays."""
    g = None
    for gidx in range(20):
        g = played_on(gidx, 0, S.MIX_FIXED + S.KLOP, 44)
        if not g.done:
            break
    assert [popcount(m) for m in hands(g)] == [1, 1, 1, 1]
    seat = g.seat()
    oth = DM.others_of(seat)
    counts = {}
    n = 0
    for gidx in range(100):
        for w in range(60):
            x = DM.world_of(g, DM.world_key(SEED, SALT, gidx, 0, 44, w))
            key = tuple(int(x.g.hand[o]) for o in oth)
            counts[key] = counts.get(key, 0) + 1
            n += 1
    assert n == 6000 and len(counts) == 6
    sigma = (n * (1 / 6) * (5 / 6)) ** 0.5
    assert all(abs(c - n / 6) <= 5 * sigma for c in counts.values()), counts


def test_uneven_capacities_come_out_in_proportion():
    """Six cards into a game the other seats hold unequal hands: over 2,000 (gidx, w) pairs the lowest card of the pool
    goes to each seat in proportion to its capacity, within 5 sigma of the binomial."""
    g = played_on(1, 0, S.MIX_FIXED + S.SOLO_BREZ, 6)
    seat = g.seat()
    oth = DM.others_of(seat)
    caps = [popcount(g.g.hand[o]) for o in oth]
    assert len(set(caps)) > 1
    pool = 0
    for o in oth:
        pool |= int(g.g.hand[o])
    low = PM.cards_of(pool)[0]
    n, got = 2000, [0, 0, 0]
    for w in range(n):
        masks = DM.deal_pool(pool, caps, DM.world_key(SEED, SALT, w // 64, 0, 6, w % 64))
        assert [popcount(m) for m in masks] == caps
        got[[i for i in range(3) if (masks[i] >> low) & 1][0]] += 1
    for i in range(3):
        p = caps[i] / sum(caps)
        assert abs(got[i] - n * p) <= 5 * (n * p * (1 - p)) ** 0.5, (got, caps)


def test_worlds_and_samples_are_prefixes_and_the_keys_are_apart():
    g = played_on(7, 1, S.MIX_ALL, 5)
    lanes = g.lanes()
    sc = DM.playout_scores(lanes, 1, SEED, 9, 7, 15, 4, 3)
    assert sc.shape == (12, 4, 3, 4)
    for worlds, samples in ((1, 1), (2, 3), (4, 2), (4, 3)):
        sums, _ = DM.playout_cards(lanes, 1, SEED, 9, 7, 15, worlds, samples)
        assert (sums == DM.sums_of(sc, worlds, samples)).all()
        assert (sums == sc[:, :worlds, :samples].reshape(12, -1, 4).sum(axis=1)).all()
    assert (sc[:, 0] != sc[:, 1]).any()                                       # the worlds are not one world
    keys = {DM.playout_key(SEED, salt, gidx, ep, played, card, w, k)
            for salt in (0, 1) for gidx in (0, 1) for ep in (0, 1) for played in (0, 1) for card in (0, 1) for w in (0, 1) for k in (0, 1)}
    keys |= {DM.world_key(SEED, salt, gidx, ep, played, w)
             for salt in (0, 1) for gidx in (0, 1) for ep in (0, 1) for played in (0, 1) for w in (0, 1)}
    assert len(keys) == 128 + 32
    # bits 63..61: 011 a deal's episode never has, 100 the open-hand playouts, 110 these playouts, 111 the worlds
    assert DM.playout_key(SEED, 0, 3, 0, 0, 0, 0, 0) not in (S.game_key(SEED, 3, 0), PM.playout_key(SEED, 0, 3, 0, 0, 0, 0))
    assert DM.world_key(SEED, 0, 3, 0, 0, 0) not in (S.game_key(SEED, 3, 0), PM.playout_key(SEED, 0, 3, 0, 0, 0, 0),
                                                     DM.playout_key(SEED, 0, 3, 0, 0, 0, 0, 0))
    assert DM.world_key(SEED ^ 6, 6, 3, 2, 11, 5) == DM.world_key(SEED, 0, 3, 2, 11, 5)          # seed ^ salt
    # the largest fields do not run into one another: k = 1023 and w = 63 against their neighbours
    assert DM.playout_key(SEED, 0, 3, 2, 47, 53, 63, 1023) != DM.playout_key(SEED, 0, 3, 2, 47, 53, 63, 1022)
    assert DM.playout_key(SEED, 0, 3, 2, 47, 53, 63, 1023) != DM.playout_key(SEED, 0, 3, 2, 47, 53, 62, 1023)


def test_the_model_is_blind_to_the_hidden_hands():
    """Swapping two unseen cards between two other seats changes neither sums nor card (the GPU test does this at
    scale; here on the model itself, so a model that peeked would fail before a GPU is involved)."""
    done = 0
    for gidx in range(12):
        g = played_on(gidx, 0, S.MIX_NAVADNA3, 9)
        seat = g.seat()
        a, b = DM.others_of(seat)[:2]
        ca, cb = PM.cards_of(g.g.hand[a])[0], PM.cards_of(g.g.hand[b])[-1]
        twin = PM.copy_of(g)
        twin.g.hand[a] = (int(g.g.hand[a]) & ~(1 << ca)) | (1 << cb)
        twin.g.hand[b] = (int(g.g.hand[b]) & ~(1 << cb)) | (1 << ca)
        x = DM.playout_cards(g.lanes(), 0, SEED, SALT, gidx, 15, 3, 1)
        y = DM.playout_cards(twin.lanes(), 0, SEED, SALT, gidx, 15, 3, 1)
        assert (x[0] == y[0]).all() and x[1] == y[1]
        done += 1
    assert done == 12


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- before the dlopen: one HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_abi_list_and_python_surface_have_the_determinized_playouts():
    from tarok_amd import _native, karte as K
    from tarok_amd import evaluate as EV
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.selfplay import SelfPlay
    assert "tarok_playout_cards_det" in _native.SYMBOLS
    assert K.PLAYOUT_MAX_WORLDS == 64 == DM.MAX_WORLDS
    sig = inspect.signature(TarokVecEnv.playout_cards_det).parameters
    assert list(sig)[1:] == ["worlds", "samples", "salt", "seats", "seats_per_game", "sum_out", "action_out"]
    assert sig["salt"].default == 0 and sig["seats"].default == 15
    assert inspect.signature(EV.evaluate_playout_vs_bot).parameters["worlds"].default is None
    assert inspect.signature(EV._playout_passes).parameters["worlds"].default is None
    assert inspect.signature(SelfPlay.evaluate).parameters["playout_worlds"].default is None


def test_playout_cards_det_validates_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough."""
    z = ctypes.c_void_p(0)
    stand_in = ctypes.create_string_buffer(1 << 16)
    env = ctypes.cast(stand_in, ctypes.c_void_p)
    out = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    f = L.tarok_playout_cards_det
    assert f(None, 4, 4, 0, 15, z, out, out, z) == -1
    assert f(env, 0, 4, 0, 15, z, out, out, z) == -1
    assert f(env, 65, 4, 0, 15, z, out, out, z) == -1
    assert f(env, -2, 4, 0, 15, z, out, out, z) == -1
    assert f(env, 4, 0, 0, 15, z, out, out, z) == -1
    assert f(env, 4, 1025, 0, 15, z, out, out, z) == -1
    assert f(env, 4, -3, 0, 15, z, out, out, z) == -1
    assert f(env, 4, 4, 0, 16, z, out, out, z) == -1
    assert f(env, 4, 4, 0, -1, z, out, out, z) == -1
    assert f(env, 4, 4, 0, 15, z, z, z, z) == -1
