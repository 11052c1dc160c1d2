"""GPU: tarok_shown_voids (the voids the play of every game has shown, one word per game) against the model of
tests/playout_voids_model.py, which rebuilds every word from the env's history and canonical lanes on the CPU oracle.
The output sits inside guard bands (tests/guarded.py).

Run on the GPU box:  python -m pytest tests/test_gpu_shown_voids.py -m gpu -q
"""
import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = 41, 1000, 3               # tests/test_gpu_playout_det.py's: the same games
U = np.uint64
N = 256
POSITIONS = (0, 1, 4, 5, 13, 22, 34, 46, 47)


def shown(env):
    """One tarok_shown_voids launch into a guarded array: [n] u32, every row written."""
    import torch
    from guarded import Guarded, assert_guards_intact
    from tarok_amd import _native
    g = Guarded("voids_out", 1, env.n, np.uint32, device="cuda")
    with torch.cuda.device(env.device):
        _native.check(env.L.tarok_shown_voids(env._h, g.ptr, env._stream()))
        torch.cuda.synchronize()
    assert_guards_intact([g], env.n)
    vals, written = g.host()
    assert written.all(), "a word of voids_out was not written"
    return vals[0]


def model(env):
    import playout_voids_model as VM
    lanes, hist = env.state(), env.get_history().cpu().numpy()
    return np.array([VM.voids_of_lanes(lanes[:, g], hist[:, g]) for g in range(env.n)], np.uint32)


def sound(env, words):
    """No seat of any game holds a card of a class its bits mark void."""
    import playout_voids_model as VM
    lanes = env.state()
    for g in range(env.n):
        for s in range(4):
            assert not int(lanes[s, g]) & VM.class_cards((int(words[g]) >> (5 * s)) & 31), (g, s)


@pytest.mark.parametrize("mix", ["all", "bot", 0, 3, 7, 8])
def test_every_word_against_the_model_one_card_at_a_time(T, mix):
    from oracle import tarok_spec as S
    code = {"all": S.MIX_ALL, "bot": S.MIX_BOT}.get(mix, S.MIX_FIXED + mix if isinstance(mix, int) else None)
    env = T.TarokVecEnv(N, seed=SEED, mix=code, game_offset=OFFSET, history=True)
    try:
        env.reset(episode=EPISODE)
        at, nonzero = 0, 0
        for cards in POSITIONS:
            while at < cards:
                env.step_random(auto_reset=False)
                at += 1
            before = (env.state().copy(), env.get_history().cpu().numpy().copy())
            got, want = shown(env), model(env)
            assert (got == want).all(), (mix, cards, np.nonzero(got != want)[0][:8])
            assert (got >> 20 == 0).all()
            sound(env, got)
            phases = (env.state()[9] >> U(52)) & U(3)
            assert not got[phases != 2].any()                                  # finished games: 0
            assert (before[0] == env.state()).all() and (before[1] == env.get_history().cpu().numpy()).all()   # read-only
            if cards <= 1:
                assert not got.any()
            nonzero += int((got != 0).sum())
        assert nonzero > N
    finally:
        env.close()


def test_multi_card_launches_through_auto_resets_do_not_leak_the_finished_game(T):
    """tarok_krog_random, several cards per launch, through the games' ends: a renewed game's history holds the finished
    game's cards beyond its own `played`, and none of them may show up in its word (the model reads the entries below
    `played` alone, so a kernel that read a stale one would differ)."""
    from oracle import tarok_spec as S
    env = T.TarokVecEnv(N, seed=SEED, mix=S.MIX_ALL, game_offset=OFFSET, history=True)
    try:
        env.reset(episode=EPISODE)
        renewed = 0
        for cards in (4, 7, 12, 12, 12, 5, 12, 12, 12, 3):
            env.krog_random(cards=cards, auto_reset=True)
            got, want = shown(env), model(env)
            assert (got == want).all(), (cards, np.nonzero(got != want)[0][:8])
            sound(env, got)
            ep, _ = env.counters()
            renewed = max(renewed, int((np.asarray(ep) > EPISODE).sum()))
        assert renewed > N // 2
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
        assert not shown(env).any()
        assert (env.shown_voids().cpu().numpy().view(np.uint32) == shown(env)).all()
    finally:
        env.close()
    env = T.TarokVecEnv(96, seed=SEED, mix=S.MIX_ALL, game_offset=OFFSET)
    try:
        env.reset(episode=EPISODE)
        out = torch.zeros(96, dtype=torch.int32, device=env.device)
        assert env.L.tarok_shown_voids(env._h, ctypes.c_void_p(out.data_ptr()), env._stream()) == -1
        with pytest.raises(ValueError):
            env.shown_voids()
        with pytest.raises(ValueError):
            env.playout_cards_voids(2, 1)
    finally:
        env.close()
