"""GPU: tarok_playout_cards (open-hand Monte-Carlo playouts from the env's current positions) and the surface built on
it, checked exactly — integers against integers — against the per-game model of tests/playout_model.py, which plays
every playout on the CPU oracle.  Outputs sit inside guard bands (tests/guarded.py): a stray store or a row that was
not written fails the test.

Run on the GPU box:  python -m pytest tests/test_gpu_playout.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

SEED = 41
OFFSET = 1000                            # game offset of the envs: gidx = OFFSET + g
EPISODE = 3                              # episode the envs are reset to: the key's episode field is not zero
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)


def launch(env, samples, salt=0, seats=15, per_game=None, want=("sum", "action")):
    """One tarok_playout_cards launch into guarded outputs: (sum [n,12,4] i32 or None, action [n] u8 or None)."""
    return H.launch_det(env, None, samples, salt, seats, per_game, want)


def model_scores(env, salt, sets, samples, seed=SEED):
    """Per game: (lanes, episode, set, the model's scores [12, samples, 4]) of the env's current positions."""
    import playout_model as PM
    lanes = env.state()
    ep, _ = env.counters()
    out = []
    for g in range(env.n):
        s = int(sets[g]) & 15
        out.append((lanes[:, g].copy(), int(ep[g]), s, PM.playout_scores(lanes[:, g], int(ep[g]), seed, salt, OFFSET + g, s, samples)))
    return out


def expected(model, samples, seed=SEED):
    import playout_model as PM
    sums = np.stack([PM.sums_of(sc, samples) for _, _, _, sc in model])
    acts = np.array([PM.card_of(lanes, seed, OFFSET + g, ep, s, sums[g]) for g, (lanes, ep, s, _) in enumerate(model)], np.uint8)
    return sums, acts


def check(env, model, samples, salt=0, seats=15, per_game=None, tag=None):
    want_sum, want_act = expected(model, samples)
    got_sum, got_act = launch(env, samples, salt, seats, per_game)
    H.assert_cards_equal(got_sum, want_sum, got_act, want_act, tag)
    return got_sum, got_act


@pytest.mark.parametrize("cards", [0, 1, 2, 3, 5, 22, 46, 47])
def test_every_row_against_the_model(T, cards):
    """300 games (two workgroups at one sample, a ragged tail at every team width) of every contract after `cards` Bot
    cards: all four places in a trick, finished games, Berac games that ended early.  Samples 1 and 5: sample k of a card
    is the same playout whatever `samples`, so one model run at 5 serves both launches."""
    from oracle import tarok_spec as S
    env = make_env(T, 300, S.MIX_ALL, cards)
    try:
        model = model_scores(env, 7, np.full(300, 15), 5)
        phases = (env.state()[9] >> np.uint64(52)) & np.uint64(3)
        if cards >= 22:
            assert (phases == 3).any() and (phases == 2).any()           # finished games beside games in play
        for samples in (1, 5):
            got_sum, got_act = check(env, model, samples, salt=7, tag=(cards, samples))
            assert (got_act[phases == 3] == 255).all() and not got_sum[phases == 3].any()
            assert got_sum[phases == 2].any()
        # one output at a time: the same bytes
        s_only, _ = launch(env, 5, 7, want=("sum",))
        _, a_only = launch(env, 5, 7, want=("action",))
        assert (s_only == got_sum).all() and (a_only == got_act).all()
    finally:
        env.close()


@pytest.mark.parametrize("cards", [23, 36])
def test_more_samples_than_one_team_of_lanes(T, cards):
    """64 and 80 samples at 70 games: more work items per game than the widest team has lanes (one model run at 80)."""
    from oracle import tarok_spec as S
    env = make_env(T, 70, S.MIX_ALL, cards)
    try:
        model = model_scores(env, 0, np.full(70, 15), 80)
        for samples in (64, 80):
            check(env, model, samples, tag=(cards, samples))
    finally:
        env.close()


def test_a_single_game(T):
    from oracle import tarok_spec as S
    for cards in (0, 6):
        env = make_env(T, 1, S.MIX_ALL, cards)
        try:
            check(env, model_scores(env, 2, [15], 3), 3, salt=2, tag=("n=1", cards))
        finally:
            env.close()


@pytest.mark.parametrize("code", [0, 7, 3, 8])
def test_fixed_contracts(T, code):
    """Klop (talon gifts), Berac (early ends), Ena (called king, exchange) and Solo_brez, 64 games, after 0 and 7 cards."""
    from oracle import tarok_spec as S
    for cards in (0, 7):
        env = make_env(T, 64, S.MIX_FIXED + code, cards)
        try:
            check(env, model_scores(env, 0, np.full(64, 15), 2), 2, tag=(code, cards))
        finally:
            env.close()


def test_games_waiting_for_the_exchange_give_zeros_and_255(T):
    from oracle import tarok_spec as S
    env = make_env(T, 96, S.MIX_ALL, 0, defer_exchange=True)
    try:
        phases = (env.state()[9] >> np.uint64(52)) & np.uint64(3)
        waiting = phases == 1
        assert waiting.sum() >= 8 and (phases == 2).sum() >= 8
        got_sum, got_act = check(env, model_scores(env, 0, np.full(96, 15), 2), 2, tag="deferred exchange")
        assert not got_sum[waiting].any() and (got_act[waiting] == 255).all()
    finally:
        env.close()


def test_seat_sets(T):
    """seats = 0: tarok_policy_random's bytes and no playout; a per-game array mixing 0, 1, 6 and 15 (bits 4..7 are
    ignored) against the model."""
    from oracle import tarok_spec as S
    env = make_env(T, 300, S.MIX_ALL, 5)
    try:
        bot = env.policy_random(env.legal_actions()).cpu().numpy().copy()
        got_sum, got_act = launch(env, 4, seats=0)
        assert not got_sum.any() and (got_act == bot).all()
        assert (bot != 255).sum() > 200
        per = np.array([0, 1, 6, 15], np.uint8)[np.arange(300) % 4] | ((np.arange(300) % 3) << 4).astype(np.uint8)
        model = model_scores(env, 11, per, 2)
        got_sum, got_act = check(env, model, 2, salt=11, seats=9, per_game=per, tag="per-game sets")
        movers = ((env.legal_actions().words.cpu().numpy().view(np.uint64) >> np.uint64(54)) & np.uint64(3)).astype(np.int64)
        out = ((per.astype(np.int64) >> movers) & 1) == 0
        assert out.sum() > 50 and (~out).sum() > 50
        assert not got_sum[out].any() and (got_act[out] == bot[out]).all()
    finally:
        env.close()


def test_read_only_and_deterministic(T):
    import torch
    from oracle import tarok_spec as S
    envs = [T.TarokVecEnv(300, seed=SEED, mix=S.MIX_ALL, game_offset=OFFSET, history=True) for _ in range(2)]
    env, twin = envs
    try:
        for e in envs:
            e.reset(episode=EPISODE)
            e.set_play_mode(0.5, 0.25)
            for _ in range(9):
                e.step_random(auto_reset=True)
        snap = lambda: (env.state().copy(), env.counters(), env.get_history().cpu().numpy().copy(), env.play_mode)
        before = snap()
        s1, a1 = launch(env, 3)
        after = snap()
        assert (before[0] == after[0]).all() and (before[2] == after[2]).all() and before[3] == after[3]
        assert (before[1][0] == after[1][0]).all() and (before[1][1] == after[1][1]).all()
        s2, a2 = launch(env, 3)
        assert (s1 == s2).all() and (a1 == a2).all()
        s3, _ = launch(env, 3, salt=1)
        assert (s3 != s1).any()
        for e in envs:                                   # the twin never ran a playout: the same games from here on
            e.run_random(96, auto_reset=True)
        torch.cuda.synchronize()
        assert (env.state() == twin.state()).all()
        ce, ct = env.counters(), twin.counters()
        assert (ce[0] == ct[0]).all() and (ce[1] == ct[1]).all()
        assert (env.get_history().cpu().numpy() == twin.get_history().cpu().numpy()).all()
    finally:
        for e in envs:
            e.close()


def test_playout_values_on_the_device(T):
    from oracle import tarok_spec as S
    import playout_model as PM
    from tarok_amd.env import playout_values
    env = make_env(T, 64, S.MIX_ALL, 6)
    try:
        words = env.legal_actions().words
        sums, _ = env.playout_cards(3)
        got = playout_values(sums, words, 3).cpu().numpy()
        want = PM.playout_values_loop(sums.cpu().numpy(), words.cpu().numpy().view(np.uint64), 3)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
    finally:
        env.close()


def test_evaluate_playout_vs_bot_replays_on_the_oracle(T):
    """24 deals, 2 samples: every card of every pass and the returned dict equal a replay on the oracle with the
    model's cards."""
    import playout_model as PM
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    seen = []
    got = EV.evaluate_playout_vs_bot(2, 24, 1, seed=5, inspect=seen)
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS)
    scores = np.zeros((5, 24, 4), np.int32)
    for p, rec in enumerate(seen):
        for i in range(24):
            actions, sc = PM.replay_pass(5, S.MIX_BOT, i, 0, rec["seats"], 2)
            assert rec["actions"][:, i].tolist() == actions, (p, i)
            assert rec["scores"][i].tolist() == sc, (p, i)
            scores[p, i] = sc
    want = EV.duplicate_advantage(scores)
    assert got == want or (np.isnan(got["stderr"]) and np.isnan(want["stderr"]))


SANITY_SUM = 11671       # = advantage 5.69873046875 points per game over 4 * 512 paired scores (stderr 0.49)


def test_the_playout_player_beats_the_bot(T):
    """Sanity, not a bar on play strength: on 512 deals (seed 0, MIX_BOT) with 8 samples the playout player's summed
    duplicate advantage over the Bot is positive.  SANITY_SUM is that sum as the CPU model ALONE gives it for these very
    arguments (tests/playout_model.replay_pass over the five passes: sum over deals d and seats k of
    score(player on k)[d, k] - score(Bot everywhere)[d, k]); the GPU must equal it."""
    from tarok_amd import evaluate as EV
    got = EV.evaluate_playout_vs_bot(8, 512, 1, seed=0)
    assert SANITY_SUM > 0
    assert got["deals"] == 512 and got["advantage"] == SANITY_SUM / 2048.0
    assert got["policy_mean"] == 0.67626953125 and got["bot_mean"] == -5.0224609375      # (the model's, likewise)
