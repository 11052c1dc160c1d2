"""CPU-side checks of the open-hand Monte-Carlo playouts (tarok_playout_cards): the per-game model of
tests/playout_model.py on positions that can be checked by hand, the pure-torch helper playout_values against a loop,
and the argument validation of the entry point, which makes no HIP call and so runs without a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

SEED = 23


def played_on(gidx, episode, mix, cards):
    """The synthetic game (SEED, gidx, episode) after `cards` Bot cards (or its end, if that comes first)."""
    g = O.Game.synth(SEED, gidx, episode, mix)
    key = O.game_key(SEED, gidx, episode)
    for q in range(cards):
        if g.done:
            break
        g.step(O.policy_action(key, q, g.legal()))
    return g


def test_one_card_left_in_every_hand_gives_samples_times_the_final_scores():
    seen = 0
    for gidx in range(12):
        g = played_on(gidx, 0, S.MIX_ALL, 44)
        if g.done:                                       # a Berac that ended early
            continue
        seen += 1
        lanes = g.lanes()
        assert all(bin(int(lanes[s])).count("1") == 1 for s in range(4))
        end = PM.copy_of(g)
        while not end.done:                              # every card is forced
            (card,) = PM.cards_of(end.legal())
            end.step(card)
        for samples in (1, 7):
            sums, card = PM.playout_cards(lanes, 0, SEED, 5, gidx, 15, samples)
            assert sums[0].tolist() == [samples * x for x in end.scores]
            assert not sums[1:].any()
            assert [card] == PM.cards_of(g.legal())
    assert seen >= 6


def test_finished_game_and_bot_seat_give_zeros():
    g = played_on(3, 0, S.MIX_FIXED + S.KLOP, 48)
    assert g.done
    sums, card = PM.playout_cards(g.lanes(), 0, SEED, 0, 3, 15, 4)
    assert not sums.any() and card == PM.NO_CARD == 255
    # a game in play whose mover is outside the set: no playout, the Bot's card under the game's own key
    g = played_on(4, 2, S.MIX_FIXED + S.TRI, 9)
    seat, legal = g.seat(), g.legal()
    sums, card = PM.playout_cards(g.lanes(), 2, SEED, 0, 4, 15 & ~(1 << seat), 4)
    assert not sums.any()
    assert card == S.policy_action(S.game_key(SEED, 4, 2), 9, legal)
    # and inside it: rows of the legal cards only
    sums, card = PM.playout_cards(g.lanes(), 2, SEED, 0, 4, 1 << seat, 4)
    k = len(PM.cards_of(legal))
    assert not sums[k:].any() and (legal >> card) & 1


def test_the_chosen_card_is_the_lowest_ranked_maximiser():
    g = played_on(0, 0, S.MIX_FIXED + S.KLOP, 0)         # seat 0 leads a Klop: the whole hand is legal
    seat, cards = g.seat(), PM.cards_of(g.legal())
    assert len(cards) >= 11
    sums = np.zeros((12, 4), np.int64)
    sums[:, seat] = [-40, -12, -30, -12, -12, -50, -13, -12, -90, -20, -12, -12]
    sums[:, (seat + 1) & 3] = np.arange(12) * 100        # other seats' sums do not matter
    assert PM.card_of(g.lanes(), SEED, 0, 0, 15, sums) == cards[1]
    sums[0, seat] = -12
    assert PM.card_of(g.lanes(), SEED, 0, 0, 15, sums) == cards[0]
    sums[:, seat] = 0                                    # all equal (as with zero sums): the lowest legal card
    assert PM.card_of(g.lanes(), SEED, 0, 0, 15, sums) == cards[0]
    sums[len(cards) - 1, seat] = 1                       # the single maximum on the last rank
    assert PM.card_of(g.lanes(), SEED, 0, 0, 15, sums) == cards[-1]


def test_samples_are_prefixes_and_the_key_separates_everything():
    g = played_on(7, 1, S.MIX_ALL, 5)
    lanes = g.lanes()
    sc = PM.playout_scores(lanes, 1, SEED, 9, 7, 15, 6)
    for samples in (1, 3, 6):
        sums, _ = PM.playout_cards(lanes, 1, SEED, 9, 7, 15, samples)
        assert (sums == PM.sums_of(sc, samples)).all()
    keys = {PM.playout_key(SEED, salt, gidx, ep, played, card, k)
            for salt in (0, 1) for gidx in (0, 1) for ep in (0, 1) for played in (0, 1) for card in (0, 1) for k in (0, 1)}
    assert len(keys) == 64
    assert PM.playout_key(SEED, 0, 3, 0, 0, 0, 0) != S.game_key(SEED, 3, 0)          # bit 63: never a deal's key
    assert PM.playout_key(SEED ^ 6, 6, 3, 2, 11, 40, 5) == PM.playout_key(SEED, 0, 3, 2, 11, 40, 5)   # seed ^ salt


def test_playout_values_against_a_loop():
    import torch
    from tarok_amd.env import playout_values
    rnd = np.random.RandomState(3)
    n = 500
    words = np.zeros(n, np.uint64)
    for i in range(n):
        k = rnd.randint(0, 13)                           # 0 legal cards too: a row of -inf
        for c in rnd.choice(54, k, replace=False):
            words[i] |= np.uint64(1) << np.uint64(c)
        words[i] |= np.uint64(rnd.randint(0, 4)) << np.uint64(54)
        words[i] |= np.uint64(rnd.randint(0, 48)) << np.uint64(56)
        words[i] |= np.uint64(rnd.randint(0, 2)) << np.uint64(63)
    for samples in (1, 3, 1024):
        sums = rnd.randint(-300 * samples, 300 * samples + 1, (n, 12, 4)).astype(np.int32)
        got = playout_values(torch.from_numpy(sums), torch.from_numpy(words.view(np.int64)), samples)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, 54)
        want = PM.playout_values_loop(sums, words, samples)
        assert (got.numpy().view(np.uint32) == want.view(np.uint32)).all()


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- before the dlopen: one HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_abi_list_and_python_surface_have_the_playouts():
    from tarok_amd import _native, karte as K
    from tarok_amd import evaluate as EV
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.selfplay import SelfPlay
    assert "tarok_playout_cards" in _native.SYMBOLS
    assert K.PLAYOUT_RANKS == 12 == PM.RANKS and K.PLAYOUT_MAX_SAMPLES == 1024 == PM.MAX_SAMPLES
    sig = inspect.signature(TarokVecEnv.playout_cards).parameters
    assert list(sig)[1:] == ["samples", "salt", "seats", "seats_per_game", "sum_out", "action_out"]
    assert sig["salt"].default == 0 and sig["seats"].default == 15
    sig = inspect.signature(EV.evaluate_playout_vs_bot).parameters
    assert list(sig)[:3] == ["samples", "n_games", "episodes"] and sig["mix"].default == K.MIX_BOT and "inspect" in sig
    assert inspect.signature(SelfPlay.evaluate).parameters["versus_playout"].default is None


def test_playout_cards_validates_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough."""
    z = ctypes.c_void_p(0)
    stand_in = ctypes.create_string_buffer(1 << 16)
    env = ctypes.cast(stand_in, ctypes.c_void_p)
    out = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    assert L.tarok_playout_cards(None, 4, 0, 15, z, out, out, z) == -1
    assert L.tarok_playout_cards(env, 0, 0, 15, z, out, out, z) == -1
    assert L.tarok_playout_cards(env, 1025, 0, 15, z, out, out, z) == -1
    assert L.tarok_playout_cards(env, -3, 0, 15, z, out, out, z) == -1
    assert L.tarok_playout_cards(env, 4, 0, 16, z, out, out, z) == -1
    assert L.tarok_playout_cards(env, 4, 0, -1, z, out, out, z) == -1
    assert L.tarok_playout_cards(env, 4, 0, 15, z, z, z, z) == -1
