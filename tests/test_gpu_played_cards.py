"""GPU: tarok_played_cards (the cards of every game's play history as one word per game) against the history read back
with tarok_get_history and the canonical lanes (tests/playout_hidden_model.played_of_lanes).  The output sits inside
guard bands (tests/guarded.py).

Run on the GPU box:  python -m pytest tests/test_gpu_played_cards.py -m gpu -q
"""
import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = 41, 1000, 3               # tests/test_gpu_playout_det.py's: the same games
U = np.uint64
POSITIONS = (0, 1, 4, 5, 47)


def played(env):
    """One tarok_played_cards launch into a guarded array: [n] u64, every row written."""
    import torch
    from guarded import Guarded, assert_guards_intact
    from tarok_amd import _native
    g = Guarded("played_out", 1, env.n, np.uint64, device="cuda")
    with torch.cuda.device(env.device):
        _native.check(env.L.tarok_played_cards(env._h, g.ptr, env._stream()))
        torch.cuda.synchronize()
    assert_guards_intact([g], env.n)
    vals, written = g.host()
    assert written.all(), "a word of played_out was not written"
    return vals[0]


def model(env):
    import playout_hidden_model as HM
    lanes, hist = env.state(), env.get_history().cpu().numpy()
    return np.array([HM.played_of_lanes(lanes[:, g], hist[:, g]) for g in range(env.n)], np.uint64)


def popcounts(words):
    return np.array([bin(int(w)).count("1") for w in words])


@pytest.mark.parametrize("n", [64, 1, 300])
def test_every_word_against_the_history(T, n):
    """64 games of TAROK_MIX_BOT after 0, 1, 4, 5 and 47 cards (finished games beside games in play at 47); one game; 300
    games: a ragged last workgroup."""
    from oracle import tarok_spec as S
    env = T.TarokVecEnv(n, seed=SEED, mix=S.MIX_BOT, game_offset=OFFSET, history=True)
    try:
        env.reset(episode=EPISODE)
        at = 0
        for cards in POSITIONS:
            while at < cards:
                env.step_random(auto_reset=False)
                at += 1
            before = (env.state().copy(), env.get_history().cpu().numpy().copy())
            got, want = played(env), model(env)
            assert (got == want).all(), (cards, np.nonzero(got != want)[0][:8])
            assert (got >> U(54) == 0).all()
            m = env.state()[9]
            count = ((m >> U(29)) & U(15)) * U(4) + ((m >> U(24)) & U(7))
            assert (popcounts(got) == count.astype(int)).all()                 # every card once: as many bits as cards played
            assert (before[0] == env.state()).all() and (before[1] == env.get_history().cpu().numpy()).all()   # read-only
            assert (env.played_cards().cpu().numpy().view(np.uint64) == got).all()
        env.step_random(auto_reset=False)                                       # card 48: every game finished
        got = played(env)
        assert (got == model(env)).all() and (((env.state()[9] >> U(52)) & U(3)) == 3).all()
        if n > 1:
            assert (popcounts(got) == 48).sum() > n // 2                        # (a Berac may end early)
    finally:
        env.close()


def test_a_game_renewed_by_auto_reset_starts_from_an_empty_word(T):
    """Several cards per launch through the games' ends: a renewed game's history column still holds the finished game's
    cards beyond its own `played`, and none of them may show up in its word."""
    from oracle import tarok_spec as S
    env = T.TarokVecEnv(256, seed=SEED, mix=S.MIX_ALL, game_offset=OFFSET, history=True)
    try:
        env.reset(episode=EPISODE)
        fresh = 0
        for cards in (4, 7, 12, 12, 12, 5, 12, 12, 12, 3):
            env.krog_random(cards=cards, auto_reset=True)
            got, want = played(env), model(env)
            assert (got == want).all(), (cards, np.nonzero(got != want)[0][:8])
            ep, _ = env.counters()
            fresh += int(((np.asarray(ep) > EPISODE) & (popcounts(got) < 12)).sum())
        assert fresh > 64
    finally:
        env.close()


def test_games_waiting_for_the_exchange_and_an_env_without_history(T):
    import ctypes
    import torch
    from oracle import tarok_spec as S
    env = T.TarokVecEnv(96, seed=SEED, mix=S.MIX_ALL, game_offset=OFFSET, history=True)
    try:
        env.reset(episode=EPISODE, defer_exchange=True)
        phases = (env.state()[9] >> U(52)) & U(3)
        assert (phases == 1).sum() >= 8
        assert not played(env).any()
    finally:
        env.close()
    env = T.TarokVecEnv(96, seed=SEED, mix=S.MIX_ALL, game_offset=OFFSET)
    try:
        env.reset(episode=EPISODE)
        out = torch.zeros(96, dtype=torch.int64, device=env.device)
        assert env.L.tarok_played_cards(env._h, ctypes.c_void_p(out.data_ptr()), env._stream()) == -1
        assert env.L.tarok_played_cards(env._h, None, env._stream()) == -1
        with pytest.raises(ValueError):
            env.played_cards()
        with pytest.raises(ValueError):
            env.playout_cards_hidden(2, 1)
    finally:
        env.close()
