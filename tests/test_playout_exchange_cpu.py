"""No GPU: the definition of tarok_playout_exchange (include/tarok_env.h) as tests/playout_exchange_model.py states it
on the CPU oracle — the candidates' discards, what a world keeps and the team rule with the DECLARER as the viewer, that
exchange and re-deal commute, the prefix property, key separation, the tie rule — and the C call's argument checks."""
import ctypes
import inspect

import numpy as np
import pytest

import playout_det_model as DM
import playout_exchange_model as XM
import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

SEED, EPISODE, SALT = 17, 4, 6
EXCHANGE_CODES = (S.TRI, S.DVE, S.ENA, S.SOLO_TRI, S.SOLO_DVE, S.SOLO_ENA)
pop = lambda m: bin(int(m)).count("1")


def game_of(code, gidx, seed=SEED):
    g = XM.deferred_game(seed, gidx, EPISODE, S.MIX_FIXED + code)
    assert XM.waiting(g)
    return g


@pytest.mark.parametrize("code", EXCHANGE_CODES)
def test_a_candidates_discards_are_legal_for_the_exchange(code):
    gs, ngroups = S.GROUP_SIZE[code], 6 // S.GROUP_SIZE[code]
    for gidx in range(40):
        g = game_of(code, gidx)
        for i in range(ngroups):
            for d in range(3):
                disc = XM.discards_under(g, i, XM.candidate_key(SEED, SALT, gidx, EPISODE, i, d))
                hand = int(g.g.hand[int(g.g.declarer)]) | XM.group_mask(g, i)
                assert len(disc) == len(set(disc)) == gs and all((hand >> c) & 1 and (S.DISCARDABLE >> c) & 1 for c in disc)
                h = PM.copy_of(g)
                assert h.exchange(i, disc) == 0 and not h.g.error and int(h.g.choice) == i
                assert pop(h.g.hand[int(g.g.declarer)]) == 12 and int(h.g.pile[int(g.g.declarer)]) == sum(1 << c for c in disc)


def test_a_hand_with_fewer_discardable_cards_than_the_group_falls_back_to_the_whole_hand():
    """Hand-made: the declarer of a Tri holds the four kings, the trula and six high taroks beside ONE discardable card;
    the talon group brings a second one: two discardable cards for three discards, so the sampler draws from all 15."""
    kings, trula = [7, 15, 23, 31], [32, 52, 53]
    hand = kings + trula + [0, 40, 41, 42, 43]                           # card 0 is the one discardable card
    talon = [1, 44, 45, 46, 47, 48]                                      # group 0 = {1, 44, 45}: card 1 is discardable
    rest = [c for c in range(54) if c not in hand + talon]
    g = O.Game(hand + rest + talon, S.TRI, 0, 0)
    assert XM.waiting(g) and pop((int(g.g.hand[0]) | XM.group_mask(g, 0)) & S.DISCARDABLE) == 2
    seen = set()
    for d in range(8):
        disc = XM.discards_under(g, 0, XM.candidate_key(SEED, SALT, 0, EPISODE, 0, d))
        assert len(set(disc)) == 3 and all(c in hand + talon[:3] for c in disc)
        seen |= set(disc)
        h = PM.copy_of(g)
        assert h.exchange(0, disc) == 0                                   # legal for to_exchange, kings and all
    assert seen - {0, 1}, "the fallback draws from the whole hand"
    disc = XM.discards_under(g, 1, XM.candidate_key(SEED, SALT, 0, EPISODE, 1, 0))   # group 1 = {46, 47, 48}: one discardable
    assert len(set(disc)) == 3


@pytest.mark.parametrize("code", EXCHANGE_CODES)
def test_group_0_under_the_games_own_key_is_the_bots_exchange(code):
    for gidx in range(60):
        g = game_of(code, gidx)
        disc = XM.discards_under(g, 0, S.game_key(SEED, gidx, EPISODE))
        assert g.exchange(0, disc) == 0
        bot = O.Game.synth(SEED, gidx, EPISODE, S.MIX_FIXED + code)       # the oracle's own Bot exchange
        assert (g.lanes() == bot.lanes()).all()
        waits = XM.deferred_game(SEED, gidx, EPISODE, S.MIX_FIXED + code)
        assert XM.choice_of(waits.lanes(), SEED, SALT, gidx, EPISODE, 0, np.zeros((6, 4), np.int64), 1) == (0, XM.padded(disc))


@pytest.mark.parametrize("code", EXCHANGE_CODES)
def test_what_a_world_keeps(code):
    moved = 0
    for gidx in range(40):
        g = game_of(code, gidx)
        declarer = int(g.g.declarer)
        for w in range(3):
            x = XM.world_for(g, declarer, XM.world_key(SEED, SALT, gidx, EPISODE, w))
            assert int(x.g.hand[declarer]) == int(g.g.hand[declarer])
            assert list(x.g.talon) == list(g.g.talon) and [int(p) for p in x.g.pile] == [0, 0, 0, 0]
            assert [pop(x.g.hand[s]) for s in range(4)] == [12] * 4
            pool = lambda y: sum(int(y.g.hand[s]) for s in range(4) if s != declarer)
            assert pool(x) == pool(g)
            for f in ("contract", "declarer", "king", "phase", "choice", "leader", "trick_no", "n_in_trick", "talon_left", "error"):
                assert getattr(x.g, f) == getattr(g.g, f)
            moved += any(int(x.g.hand[s]) != int(g.g.hand[s]) for s in range(4))
    assert moved > 100


def test_the_team_rule_with_the_king_in_the_pool_in_the_declarers_hand_and_in_the_talon():
    seen = dict(pool=0, own=0, talon=0, moved=0)
    for gidx in range(400):
        g = game_of(S.TRI + gidx % 3, gidx)
        declarer, kb = int(g.g.declarer), 1 << (8 * int(g.g.king) + 7)
        talon = sum(1 << int(c) for c in g.g.talon)
        for w in range(2):
            x = XM.world_for(g, declarer, XM.world_key(SEED, SALT, gidx, EPISODE, w))
            if int(g.g.hand[declarer]) & kb:
                seen["own"] += 1
                assert int(x.g.team) == int(g.g.team) == 1 << declarer
            elif talon & kb:
                seen["talon"] += 1
                assert int(x.g.team) == int(g.g.team) == 1 << declarer
            else:
                seen["pool"] += 1
                (holder,) = [s for s in range(4) if int(x.g.hand[s]) & kb]
                assert holder != declarer and int(x.g.team) == (1 << declarer) | (1 << holder)
                seen["moved"] += int(x.g.team) != int(g.g.team)
    assert seen["pool"] > 300 and seen["own"] > 50 and seen["talon"] > 20 and seen["moved"] > 100
    solo = game_of(S.SOLO_DVE, 3)
    x = XM.world_for(solo, int(solo.g.declarer), XM.world_key(SEED, SALT, 3, EPISODE, 0))
    assert int(x.g.team) == int(solo.g.team) == 1 << int(solo.g.declarer)


@pytest.mark.parametrize("code", EXCHANGE_CODES)
def test_exchange_then_world_equals_world_then_exchange(code):
    for gidx in range(30):
        g = game_of(code, gidx)
        declarer = int(g.g.declarer)
        i = gidx % (6 // S.GROUP_SIZE[code])
        disc = XM.discards_under(g, i, XM.candidate_key(SEED, SALT, gidx, EPISODE, i, 1))
        wkey = XM.world_key(SEED, SALT, gidx, EPISODE, 1)
        a = XM.world_for(g, declarer, wkey)
        assert a.exchange(i, disc) == 0
        b = PM.copy_of(g)
        assert b.exchange(i, disc) == 0
        b = XM.world_for(b, declarer, wkey)
        assert (a.lanes() == b.lanes()).all()


def test_the_prefix_property_in_worlds_samples_and_discard_sets():
    for code, gidx in ((S.TRI, 1), (S.ENA, 2), (S.SOLO_DVE, 3)):
        lanes = game_of(code, gidx).lanes()
        big = XM.playout_scores(lanes, EPISODE, SEED, SALT, gidx, 15, 3, 2, 3)
        assert big.any()
        for worlds, samples, sets in ((1, 1, 1), (2, 1, 3), (3, 2, 2), (1, 2, 3)):
            small = XM.playout_scores(lanes, EPISODE, SEED, SALT, gidx, 15, worlds, samples, sets)
            assert (small == big[:, :sets, :worlds, :samples]).all()
            assert (XM.sums_of(big, worlds, samples, sets) == XM.sums_of(small, worlds, samples, sets)).all()
        rows = XM.sums_of(big, 3, 2, 3)
        ngroups = 6 // S.GROUP_SIZE[code]
        assert rows.shape == (18, 4) and rows[:3 * ngroups].any() and not rows[3 * ngroups:].any()


def test_games_that_do_not_take_part():
    g = game_of(S.DVE, 5)
    lanes, declarer = g.lanes(), int(g.g.declarer)
    assert XM.playout_scores(lanes, EPISODE, SEED, SALT, 5, 1 << declarer, 2, 1, 2).any()
    assert not XM.playout_scores(lanes, EPISODE, SEED, SALT, 5, 15 & ~(1 << declarer), 2, 1, 2).any()
    for mix in (S.MIX_FIXED + S.KLOP, S.MIX_FIXED + S.BERAC, S.MIX_FIXED + S.SOLO_BREZ):
        k = XM.deferred_game(SEED, 5, EPISODE, mix)
        assert not XM.waiting(k)
        sums, choice, disc = XM.playout_exchange(k.lanes(), EPISODE, SEED, SALT, 5, 15, 2, 1, 2)
        assert not sums.any() and choice == -1 and disc == [255] * 3
    played = O.Game.synth(SEED, 5, EPISODE, S.MIX_FIXED + S.DVE)            # already in play
    assert XM.playout_exchange(played.lanes(), EPISODE, SEED, SALT, 5, 15, 2, 1, 2)[1:] == (-1, [255] * 3)


def test_the_keys_are_apart_from_the_card_launches_at_0_cards_played():
    """Same seed, salt, game, episode: the exchange's world / playout keys (63 in the cards-played field) against the
    determinized card launch's at 0 cards played, over every w, and every (card, k) / (i, d, k); the candidate keys
    (tag 101) against all of them and the game's own key."""
    args = (SEED, SALT, 11, EPISODE)
    card_worlds = {DM.world_key(*args, 0, w) for w in range(64)}
    my_worlds = {XM.world_key(*args, w) for w in range(64)}
    card_playouts = {DM.playout_key(*args, 0, c, w, k) for c in range(54) for w in range(4) for k in range(4)}
    my_playouts = {XM.playout_key(*args, i, d, w, k) for i in range(6) for d in range(8) for w in range(4) for k in range(4)}
    cands = {XM.candidate_key(*args, i, d) for i in range(6) for d in range(8)}
    open_hand = {PM.playout_key(*args, 0, c, k) for c in range(54) for k in range(4)}
    assert len(my_worlds) == 64 and len(my_playouts) == 6 * 8 * 16 and len(cands) == 48
    sets = [card_worlds, my_worlds, card_playouts, my_playouts, cands, open_hand, {S.game_key(SEED, 11, EPISODE)}]
    for a in range(len(sets)):
        for b in range(a + 1, len(sets)):
            assert not sets[a] & sets[b], (a, b)
    # and as counters: the episode words themselves differ, not only their hashes
    assert (7 << 61) | (EPISODE << 28) | (63 << 22) != (7 << 61) | (EPISODE << 28) | (0 << 22)
    assert (8 * 5 + 7) < 64                                               # (8 i + d) fits the six-bit card field


def test_the_tie_rule_is_the_smallest_candidate():
    g = game_of(S.DVE, 8)                                                 # three groups
    lanes, declarer = g.lanes(), int(g.g.declarer)
    sums = np.zeros((6, 4), np.int64)
    pick = lambda: XM.choice_of(lanes, SEED, SALT, 8, EPISODE, 15, sums, 2)
    key = lambda i, d: XM.padded(XM.discards_under(g, i, XM.candidate_key(SEED, SALT, 8, EPISODE, i, d)))
    assert pick() == (0, key(0, 0))                                       # all equal: candidate (0, 0)
    sums[3][declarer] = sums[5][declarer] = 9                             # rows 3 = (1, 1) and 5 = (2, 1) tie: the smaller
    assert pick() == (1, key(1, 1))
    sums[4][declarer] = 10
    assert pick() == (2, key(2, 0))
    sums[1][(declarer + 1) & 3] = 99                                      # another seat's column does not count
    assert pick() == (2, key(2, 0))
    sums[:] = -5
    sums[2][declarer] = -4
    assert pick() == (1, key(1, 0))


def test_replay_pass_0_is_the_bot_everywhere():
    for gidx in range(30):
        want = DM.replay_pass(0, S.MIX_BOT, gidx, 0, 0, 2, 1)
        got = XM.replay_pass(0, S.MIX_BOT, gidx, 0, 0, 2, 1, 2)
        assert (got[2], got[3]) == want
        assert XM.replay_pass(0, S.MIX_BOT, gidx, 0, 0, 2, 1, 2, cards=True)[2:] == want


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- before the dlopen: one HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_abi_list_and_python_surface_have_the_exchange():
    from tarok_amd import _native, karte as K
    from tarok_amd import evaluate as EV
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.selfplay import SelfPlay
    assert "tarok_playout_exchange" in _native.SYMBOLS
    assert K.EXCHANGE_MAX_SETS == 8 == XM.MAX_SETS
    sig = inspect.signature(TarokVecEnv.playout_exchange).parameters
    assert list(sig)[1:] == ["worlds", "samples", "discard_sets", "salt", "seats", "seats_per_game", "sum_out", "choice_out", "discards_out"]
    assert sig["discard_sets"].default == 4 and sig["salt"].default == 0 and sig["seats"].default == 15
    sig = inspect.signature(EV.evaluate_exchange_vs_bot).parameters
    assert list(sig) == ["worlds", "samples", "discard_sets", "n_games", "episodes", "seed", "mix", "device", "salt", "inspect"]
    assert inspect.signature(EV.evaluate_playout_vs_bot).parameters["exchange"].default is None
    assert inspect.signature(EV._playout_passes).parameters["exchange"].default is None
    assert inspect.signature(SelfPlay.evaluate).parameters["playout_exchange"].default is None


def test_playout_exchange_validates_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough."""
    assert L.tarok_abi_version() == 5
    z = ctypes.c_void_p(0)
    stand_in = ctypes.create_string_buffer(1 << 16)
    env = ctypes.cast(stand_in, ctypes.c_void_p)
    out = ctypes.cast(ctypes.create_string_buffer(1024), ctypes.c_void_p)
    f = L.tarok_playout_exchange
    assert f(None, 4, 4, 4, 0, 15, z, out, out, out, z) == -1
    for worlds in (0, 65, -2):
        assert f(env, worlds, 4, 4, 0, 15, z, out, out, out, z) == -1
    for samples in (0, 1025, -3):
        assert f(env, 4, samples, 4, 0, 15, z, out, out, out, z) == -1
    for sets in (0, 9, -1):
        assert f(env, 4, 4, sets, 0, 15, z, out, out, out, z) == -1
    for seats in (16, -1):
        assert f(env, 4, 4, 4, 0, seats, z, out, out, out, z) == -1
