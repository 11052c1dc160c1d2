"""CPU-side checks of tarok_played_cards / tarok_playout_cards_hidden: the model of tests/playout_hidden_model.py — what a
world keeps, the discards, equality with the determinized world where nothing more is hidden, the fallback, the team
rule, uniformity on hand-made positions, the prefix property — and the argument validation of the two entry points, which
make no HIP call and so run without a GPU."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

import playout_det_model as DM
import playout_exchange_model as XM
import playout_hidden_model as HM
import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

SEED = 29
SALT = 6
KLOP, TRI, DVE, BERAC, SOLO_BREZ = 0, 1, 2, 7, 8


def popcount(m):
    return bin(int(m)).count("1")


def hands(game):
    return [int(game.g.hand[s]) for s in range(4)]


def piles(game):
    return [int(game.g.pile[s]) for s in range(4)]


def talon(game):
    return [int(game.g.talon[i]) for i in range(6)]


def count_of(game):
    return int(game.g.trick_no) * 4 + int(game.g.n_in_trick)


def same_world(x, y):
    return (x.lanes() == y.lanes()).all()


@pytest.mark.parametrize("cards", [0, 1, 4, 5, 20, 23, 24, 30])
def test_what_a_klop_world_keeps(cards):
    moved = 0
    for gidx in range(60):
        g, word = HM.bot_game(SEED, gidx, 1, S.MIX_FIXED + KLOP, cards)
        assert not g.done and popcount(word) == cards
        seat, tl = g.seat(), int(g.g.talon_left)
        assert tl == max(0, 6 - cards // 4)
        oth = DM.others_of(seat)
        before = g.lanes()
        for w in range(3):
            x = HM.world_for(g, DM.world_key(SEED, SALT, gidx, 1, cards, w), word)
            assert (g.lanes() == before).all()                               # the game itself is not touched
            h0, h1 = hands(g), hands(x)
            assert [popcount(m) for m in h1] == [popcount(m) for m in h0]    # the sizes,
            assert h1[seat] == h0[seat] and piles(x) == piles(g)             # the mover's hand, the piles,
            assert talon(x)[tl:] == talon(g)[tl:] and int(x.g.talon_left) == tl      # the slots given away
            pool0 = HM.mask_of(talon(g)[:tl]) | h0[oth[0]] | h0[oth[1]] | h0[oth[2]]
            pool1 = HM.mask_of(talon(x)[:tl]) | h1[oth[0]] | h1[oth[1]] | h1[oth[2]]
            assert pool1 == pool0 and len(set(talon(x)[:tl])) == tl          # a permutation of hands plus remaining talon
            assert all(h1[a] & h1[b] == 0 for a, b in itertools.combinations(range(4), 2))
            assert not HM.mask_of(talon(x)[:tl]) & (h1[0] | h1[1] | h1[2] | h1[3])
            la, lb = g.lanes(), x.lanes()
            assert la[9] == lb[9] and x.legal() == g.legal() and x.seat() == seat
            moved += talon(x) != talon(g)
            if tl == 0:
                assert same_world(x, DM.world_of(g, DM.world_key(SEED, SALT, gidx, 1, cards, w)))
    assert (moved > 100) == (cards < 24)


@pytest.mark.parametrize("cards", [0, 1, 3, 22, 46])
@pytest.mark.parametrize("contract", [1, 2, 3, 4, 5, 6])
def test_discards_are_discardable_and_the_pool_is_preserved(contract, cards):
    hidden = moved = 0
    for gidx in range(40):
        g, word = HM.bot_game(SEED, gidx, 2, S.MIX_FIXED + contract, cards)
        assert not g.done
        seat, d, gs = g.seat(), int(g.g.declarer), S.GROUP_SIZE[contract]
        oth = DM.others_of(seat)
        disc = HM.hidden_discards(g, seat, word)
        for w in range(3):
            wkey = DM.world_key(SEED, SALT, gidx, 2, cards, w)
            x = HM.world_for(g, wkey, word)
            if seat == d:
                assert disc == 0 and same_world(x, DM.world_of(g, wkey))
                continue
            h0, h1, p0, p1 = hands(g), hands(x), piles(g), piles(x)
            assert [popcount(m) for m in h1] == [popcount(m) for m in h0] and h1[seat] == h0[seat]
            assert talon(x) == talon(g) and all(p1[s] == p0[s] for s in range(4) if s != d)
            if not disc:                                                     # the rare fallback: the discards stay seen
                assert same_world(x, DM.world_of(g, wkey))
                continue
            hidden += 1
            new = p1[d] & ~(p0[d] & ~disc)
            assert p1[d] & ~new == p0[d] & ~disc                             # the piles minus D,
            assert popcount(new) == gs and not new & ~S.DISCARDABLE          # D' is discardable and of the group's size,
            assert new | h1[oth[0]] | h1[oth[1]] | h1[oth[2]] == disc | h0[oth[0]] | h0[oth[1]] | h0[oth[2]]     # the pool
            assert all(h1[a] & h1[b] == 0 for a, b in itertools.combinations(range(4), 2)) and not new & (h1[0] | h1[1] | h1[2] | h1[3])
            team_field = np.uint64(15 << 42)
            assert (g.lanes()[9] & ~team_field) == (x.lanes()[9] & ~team_field)
            assert x.legal() == g.legal() and x.seat() == seat
            moved += new != disc
    assert hidden > 40 and moved > (hidden * 2) // 3 if cards < 46 else hidden > 40


def test_equality_with_the_determinized_world_where_nothing_more_is_hidden():
    seen = 0
    for contract, cards in ((BERAC, 3), (SOLO_BREZ, 5), (9, 1), (KLOP, 24), (KLOP, 41)):
        for gidx in range(40):
            g, word = HM.bot_game(SEED, gidx, 0, S.MIX_FIXED + contract, cards)
            if g.done:
                continue
            for w in range(2):
                wkey = DM.world_key(SEED, SALT, gidx, 0, count_of(g), w)
                assert same_world(HM.world_for(g, wkey, word), DM.world_of(g, wkey))
                seen += 1
    for gidx in range(40):                                                   # games waiting for the exchange
        g = XM.deferred_game(SEED, gidx, 0, S.MIX_NAVADNA3)
        assert XM.waiting(g)
        wkey = DM.world_key(SEED, SALT, gidx, 0, 0, 1)
        for viewer in range(4):
            assert same_world(HM.world_for(g, wkey, 0, viewer=viewer), XM.world_for(g, viewer, wkey))
            seen += 1
    assert seen > 350


def hand_made(contract, declarer, hand_cards, pile=0, talon_ids=(0, 0, 0, 0, 0, 0), talon_left=0, king=-1, team=0):
    """A game in play with seat 0 to lead and the given one-card hands."""
    game = O.Game()
    g = game.g
    for s in range(4):
        g.hand[s] = hand_cards[s]
    g.pile[declarer] = pile
    for i in range(6):
        g.talon[i] = talon_ids[i]
    g.contract, g.declarer, g.king, g.team, g.talon_left, g.choice = contract, declarer, king, team, talon_left, 0
    g.trick_no, g.phase = 11, PM.PHASE_PLAY
    return game


def test_the_fallback_when_the_discards_hold_a_tarok_that_is_not_discardable():
    skis, c = 53, 1 << 2
    g = hand_made(DVE, 1, [1 << 40, 1 << 41, 1 << 10, 1 << 20], pile=(1 << skis) | c, team=2)
    assert HM.hidden_discards(g, 0, 0) == 0
    for w in range(8):
        wkey = DM.world_key(SEED, SALT, 0, 0, 44, w)
        assert same_world(HM.world_for(g, wkey, 0), DM.world_of(g, wkey))
    g.g.pile[1] = c | (1 << 3)                                                # two discardable cards: now they are hidden
    assert HM.hidden_discards(g, 0, 0) == c | (1 << 3)
    assert any(piles(HM.world_for(g, DM.world_key(SEED, SALT, 0, 0, 44, w), 0))[1] != c | (1 << 3) for w in range(8))
    assert HM.hidden_discards(g, 0, c) == 0                                   # one of them played: the count is wrong
    assert HM.hidden_discards(g, 1, 0) == 0                                   # the declarer sees its own


def test_the_team_rule_with_the_king_in_the_pool_and_with_it_picked_up():
    pool = picked = changed = 0
    for gidx in range(300):
        g, word = HM.bot_game(SEED, gidx, 0, S.MIX_FIXED + TRI, 5)
        seat, d = g.seat(), int(g.g.declarer)
        kb = 1 << (8 * int(g.g.king) + 7)
        for w in range(2):
            x = HM.world_for(g, DM.world_key(SEED, SALT, gidx, 0, 5, w), word)
            assert piles(x)[d] & kb == piles(g)[d] & kb                       # the called king is never laid down
            if any(int(g.g.hand[o]) & kb for o in DM.others_of(seat)):
                (holder,) = [o for o in DM.others_of(seat) if int(x.g.hand[o]) & kb]
                assert int(x.g.team) == (1 << d) | (1 << holder)
                pool += 1
                changed += int(x.g.team) != int(g.g.team)
                # picked up from the talon, the king is one more card of the declarer's hidden hand: the same rule
                picked += bool(int(g.g.hand[d]) & kb) and bool(kb & HM.mask_of(talon(g)))
            else:
                assert int(x.g.team) == int(g.g.team)
    assert pool > 100 and changed > 30 and picked >= 4, (pool, changed, picked)


def test_klop_worlds_are_uniform_over_hands_and_ordered_talon_slots():
    """Hands 1/1/1 and two talon cards left: 5 cards on 5 ordered places, 120 arrangements; over 24,000 (gidx, w) pairs
    each within 5 sigma of 200, sigma^2 = N (1/120) (119/120).  Deterministic: it ran once and stays."""
    g = hand_made(KLOP, 0, [1 << 40, 1 << 5, 1 << 17, 1 << 33], talon_ids=(50, 9, 1, 2, 3, 4), talon_left=2)
    counts = {}
    n = 0
    for gidx in range(400):
        for w in range(60):
            x = HM.world_for(g, DM.world_key(SEED, SALT, gidx, 0, 44, w), 0)
            key = (hands(x)[1], hands(x)[2], hands(x)[3]) + tuple(talon(x)[:2])
            assert talon(x)[2:] == [1, 2, 3, 4]
            counts[key] = counts.get(key, 0) + 1
            n += 1
    assert n == 24000 and len(counts) == 120
    sigma = (n * (1 / 120) * (119 / 120)) ** 0.5
    assert all(abs(c - 200) <= 5 * sigma for c in counts.values()), (min(counts.values()), max(counts.values()))


def test_dve_worlds_are_uniform_over_discards_and_hands():
    """Hands 1/1/1 (one of them a king, which cannot be laid down) and two discards: C(4, 2) discard sets x 3! hands = 36
    consistent worlds; over 7,200 (gidx, w) pairs each within 5 sigma of its share of 200."""
    king = 1 << 15
    g = hand_made(DVE, 1, [1 << 40, king, 1 << 17, 1 << 34], pile=(1 << 2) | (1 << 9), team=2)
    counts = {}
    n = 0
    for gidx in range(120):
        for w in range(60):
            x = HM.world_for(g, DM.world_key(SEED, SALT, gidx, 0, 44, w), 0)
            key = (hands(x)[1], hands(x)[2], hands(x)[3], piles(x)[1])
            assert not key[3] & king and popcount(key[3]) == 2
            counts[key] = counts.get(key, 0) + 1
            n += 1
    assert n == 7200 and len(counts) == 36
    sigma = (n * (1 / 36) * (35 / 36)) ** 0.5
    assert all(abs(c - 200) <= 5 * sigma for c in counts.values()), (min(counts.values()), max(counts.values()))


def test_worlds_and_samples_are_prefixes_and_the_new_draws_are_apart():
    for contract, gidx in ((KLOP, 3), (DVE, 4)):
        g, word = HM.bot_game(SEED, gidx, 1, S.MIX_FIXED + contract, 5)
        lanes = g.lanes()
        sc = HM.playout_scores(lanes, 1, SEED, 9, gidx, 15, 4, 3, word)
        for worlds, samples in ((1, 1), (2, 3), (4, 2), (4, 3)):
            sums, _ = HM.playout_cards(lanes, 1, SEED, 9, gidx, 15, worlds, samples, word)
            assert (sums == sc[:, :worlds, :samples].reshape(12, -1, 4).sum(axis=1)).all()
        assert (sc[:, 0] != sc[:, 1]).any()
        assert (sc != DM.playout_scores(lanes, 1, SEED, 9, gidx, 15, 4, 3)).any()   # not the determinized launch's worlds
    # draw numbers under a world key: the walks' 0..41, the void-aware launch's 64, 65 and 128..163, then 256.. and 320..
    assert HM.DRAW_DISCARD > 128 + 35 and HM.DRAW_DISCARD + 38 < HM.DRAW_SLOT
    wkey = DM.world_key(SEED, 0, 3, 0, 0, 0)
    draws = [S.rng32(wkey, i) for i in list(range(42)) + [64, 65] + list(range(128, 164)) + list(range(256, 295)) + list(range(320, 326))]
    assert len(set(draws)) == len(draws)


def test_the_model_is_blind_to_the_talon_and_the_discards():
    """Swapping a hidden hand card with a Klop's talon card, or with a discard, changes neither sums nor card; the
    determinized model is not blind to it (counted here, so the GPU test's seed is known to show it)."""
    det_differs = 0
    for gidx in range(8):
        g, word = HM.bot_game(SEED, gidx, 0, S.MIX_FIXED + KLOP, 4)
        o = DM.others_of(g.seat())[0]
        c, t = PM.cards_of(g.g.hand[o])[0], int(g.g.talon[0])
        twin = PM.copy_of(g)
        twin.g.hand[o] = (int(g.g.hand[o]) & ~(1 << c)) | (1 << t)
        twin.g.talon[0] = c
        x = HM.playout_cards(g.lanes(), 0, SEED, SALT, gidx, 15, 3, 1, word)
        y = HM.playout_cards(twin.lanes(), 0, SEED, SALT, gidx, 15, 3, 1, word)
        assert (x[0] == y[0]).all() and x[1] == y[1]
        det_differs += (DM.playout_cards(g.lanes(), 0, SEED, SALT, gidx, 15, 3, 1)[0]
                        != DM.playout_cards(twin.lanes(), 0, SEED, SALT, gidx, 15, 3, 1)[0]).any()
    done = 0
    for gidx in range(16):
        g, word = HM.bot_game(SEED, gidx, 0, S.MIX_FIXED + DVE, 5)
        seat, d = g.seat(), int(g.g.declarer)
        disc = HM.hidden_discards(g, seat, word)
        o = [q for q in DM.others_of(seat)][0]
        cand = PM.cards_of(int(g.g.hand[o]) & S.DISCARDABLE)
        if not disc or not cand:
            continue
        c, t = cand[0], PM.cards_of(disc)[0]
        twin = PM.copy_of(g)
        twin.g.hand[o] = (int(g.g.hand[o]) & ~(1 << c)) | (1 << t)
        twin.g.pile[d] = (int(g.g.pile[d]) & ~(1 << t)) | (1 << c)
        x = HM.playout_cards(g.lanes(), 0, SEED, SALT, gidx, 15, 3, 1, word)
        y = HM.playout_cards(twin.lanes(), 0, SEED, SALT, gidx, 15, 3, 1, word)
        assert (x[0] == y[0]).all() and x[1] == y[1]
        det_differs += (DM.playout_cards(g.lanes(), 0, SEED, SALT, gidx, 15, 3, 1)[0]
                        != DM.playout_cards(twin.lanes(), 0, SEED, SALT, gidx, 15, 3, 1)[0]).any()
        done += 1
    assert done >= 6 and det_differs >= 8


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- before the dlopen: one HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_abi_list_and_python_surface():
    from tarok_amd import _native
    from tarok_amd import evaluate as EV
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.selfplay import SelfPlay
    assert "tarok_played_cards" in _native.SYMBOLS and "tarok_playout_cards_hidden" in _native.SYMBOLS
    sig = inspect.signature(TarokVecEnv.playout_cards_hidden).parameters
    assert list(sig)[1:] == ["worlds", "samples", "salt", "seats", "seats_per_game", "played", "sum_out", "action_out"]
    assert sig["salt"].default == 0 and sig["seats"].default == 15 and sig["played"].default is None
    assert inspect.signature(EV.evaluate_playout_vs_bot).parameters["hidden"].default is False
    assert inspect.signature(SelfPlay.evaluate).parameters["playout_hidden"].default is False
    with pytest.raises(ValueError):
        EV.evaluate_playout_vs_bot(2, 8, 1, worlds=2, voids=True, hidden=True)
    with pytest.raises(ValueError):
        EV.evaluate_playout_vs_bot(2, 8, 1, hidden=True)


def test_both_calls_validate_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough —
    and being zeroed it is an env without history, which tarok_played_cards refuses."""
    z = ctypes.c_void_p(0)
    stand_in = ctypes.create_string_buffer(1 << 16)
    env = ctypes.cast(stand_in, ctypes.c_void_p)
    out = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    assert L.tarok_played_cards(None, out, z) == -1
    assert L.tarok_played_cards(env, z, z) == -1
    assert L.tarok_played_cards(env, out, z) == -1
    f = L.tarok_playout_cards_hidden
    assert f(None, 4, 4, 0, 15, z, out, out, out, z) == -1
    assert f(env, 4, 4, 0, 15, z, z, out, out, z) == -1                       # played must not be NULL
    for worlds, samples, seats in ((0, 4, 15), (65, 4, 15), (-2, 4, 15), (4, 0, 15), (4, 1025, 15), (4, -3, 15), (4, 4, 16), (4, 4, -1)):
        assert f(env, worlds, samples, 0, seats, z, out, out, out, z) == -1
    assert f(env, 4, 4, 0, 15, z, out, z, z, z) == -1                         # both outputs NULL
