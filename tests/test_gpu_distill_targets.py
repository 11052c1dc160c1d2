"""GPU: tarok_playout_targets — a playout launch's sums as target rows — against tests/distill_model.targets_reference on
real env states and on hand-made sums.  Outputs sit inside guard bands (tests/guarded.py).  The sums come from
playout_cards_det(3, 2), which tests/test_gpu_playout_det.py pins: they are inputs here.

Run on the GPU box:  python -m pytest tests/test_gpu_distill_targets.py -m gpu -q
"""
import functools
import numpy as np
import pytest

import distill_model as DM
import gpu_harness as H
from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = 41, 1000, 3               # tests/test_gpu_playout_det.py's: the same games
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)
U = np.uint64


def targets(env, sums, words, playouts, tau, seats=15, per_game=None):
    """One launch into a guarded output: [n,64] float64 of the bf16 rows, and their raw 16-bit words."""
    import torch
    from guarded import Guarded, assert_guards_intact
    from tarok_amd import _native
    n = env.n
    out = Guarded("target_out", 1, n, np.uint16, inner=(64,), device="cuda")
    per_dev = None if per_game is None else torch.from_numpy(np.asarray(per_game, np.uint8)).cuda()
    s = torch.as_tensor(np.ascontiguousarray(sums, np.int32)).cuda()
    w = torch.as_tensor(np.ascontiguousarray(np.asarray(words).astype(np.uint64).view(np.int64))).cuda()
    with torch.cuda.device(env.device):
        _native.check(env.L.tarok_playout_targets(env._h, env._p(s), env._p(w), int(playouts), float(tau), int(seats), env._p(per_dev),
                                                  out.ptr, env._stream()))
        torch.cuda.synchronize()
    assert_guards_intact([out], (n, playouts, tau, seats))
    raw, written = out.host()
    assert written.all(), "a row of target_out was not written"
    raw = raw[0]
    vals = torch.from_numpy(raw.astype(np.int16)).view(torch.bfloat16).double().numpy()
    return vals, raw


def judge(got, raw, sums, words, playouts, tau, sets, acts=None):
    q, has, card = DM.targets_reference(sums, words, playouts, tau, sets)
    assert (got[~has] == 0).all() and (raw[~has] == 0).all(), "a game without a teacher has a non-zero row"
    if tau == 0:
        assert np.array_equal(got, q), "one-hot rows differ"
        if acts is not None:
            assert (card[has] == acts[has]).all(), "the one-hot card is not the playout launch's"
        return 0.0
    b = DM.target_bound(q)
    err = np.abs(got - q)
    assert (err[b == 0] == 0).all(), "a column outside the legal cards is not zero"
    ratio = float((err[b > 0] / b[b > 0]).max(initial=0.0))
    assert ratio <= 1.0, ("target rows outside their bound", tau, ratio)
    return ratio


@pytest.mark.parametrize("cards", [0, 1, 3, 22, 47])
def test_rows_on_real_env_states(T, cards):
    """773 games (a partial last workgroup) of every contract after `cards` Bot cards, without auto-reset: finished games
    stand beside games in play from 22 cards on.  Seat sets 15, 0, 6 and a per-game cycle; tau in {0.5, 8, 64} within the
    bound, tau = 0 equal bytes and the launch's card.  The zero rows are exactly the games the playout launch left zero."""
    from oracle import tarok_spec as S
    from gpu_harness import launch_det as launch
    env = make_env(T, 773, S.MIX_ALL, cards)
    try:
        words = env.legal_actions().words.cpu().numpy().view(np.uint64)
        phases = (env.state()[9] >> U(52)) & U(3)
        cycle = (np.arange(773) % 16).astype(np.uint8)
        worst = 0.0
        for seats, per_game in ((15, None), (0, None), (6, None), (15, cycle)):
            sets = np.full(773, seats) if per_game is None else per_game
            sums, acts = launch(env, 3, 2, 5, seats, per_game)
            # the playout launch's rule on the env's state: in the play phase and the seat to move in the set (a game
            # that takes part can have all-zero sums — every playout scored 0 for everyone — so the sums alone do not say)
            took_part = (phases == 2) & (((sets.astype(np.int64) >> ((words >> U(54)) & U(3)).astype(np.int64)) & 1) == 1)
            assert not sums[~took_part].any() and (acts[phases == 2] != 255).all() and (acts[phases != 2] == 255).all()
            for tau in (0.5, 8.0, 64.0, 0.0):
                got, raw = targets(env, sums, words, 6, tau, seats, per_game)
                worst = max(worst, judge(got, raw, sums, words, 6, tau, sets, acts))
                assert np.array_equal(raw.any(1), took_part), "zero rows are not the games the playout launch left zero"
                assert not raw[phases != 2].any()
                again, raw2 = targets(env, sums, words, 6, tau, seats, per_game)
                assert np.array_equal(raw, raw2)
            if seats == 0:
                assert not took_part.any()
        if cards >= 22:
            assert (phases == 3).any() and (phases == 2).any()
        print("target rows after %d cards: largest error / bound %.3f" % (cards, worst))
    finally:
        env.close()


def test_games_waiting_for_the_exchange_and_games_renewed_by_auto_reset(T):
    """Deferred exchange: every game that waits has a zero row and zero sums.  Auto-reset: a word that describes the slot's
    NEXT game keeps TAROK_OBS_DONE, the playout launch plays that game, and the row is its teacher's."""
    from oracle import tarok_spec as S
    from gpu_harness import launch_det as launch
    env = make_env(T, 300, S.MIX_ALL, 0, defer_exchange=True)
    try:
        words = env.legal_actions().words.cpu().numpy().view(np.uint64)
        phases = (env.state()[9] >> U(52)) & U(3)
        assert (phases != 2).any() and (phases == 2).any()
        sums, acts = launch(env, 3, 2, 5)
        got, raw = targets(env, sums, words, 6, 8.0)
        judge(got, raw, sums, words, 6, 8.0, np.full(300, 15))
        assert not raw[phases != 2].any() and raw[phases == 2].any(1).all() and not sums[phases != 2].any()
    finally:
        env.close()
    env = make_env(T, 300, S.MIX_ALL, 0)
    try:
        obs = None
        for _ in range(47):
            obs = env.step_random(auto_reset=True)
        obs = env.step_random(auto_reset=True)
        words = (obs[0] if isinstance(obs, tuple) else obs).words.cpu().numpy().view(np.uint64)
        renewed = (words >> U(62)) & U(1) == 1
        assert renewed.any()
        sums, acts = launch(env, 3, 2, 5)
        got, raw = targets(env, sums, words, 6, 8.0)
        judge(got, raw, sums, words, 6, 8.0, np.full(300, 15))
        assert raw.any(1).all() and (acts != 255).all()
        got, raw = targets(env, sums, words, 6, 0.0)
        judge(got, raw, sums, words, 6, 0.0, np.full(300, 15), acts)
    finally:
        env.close()


def test_one_game_and_hand_made_sums(T):
    env = T.TarokVecEnv(1, seed=3)
    try:
        env.reset()
        word = np.array([0b10110 | (1 << 54)], np.uint64)
        sums = np.zeros((1, 12, 4), np.int32)
        sums[0, :3, 1] = 7                                    # all ranks equal: a uniform row
        got, raw = targets(env, sums, word, 4, 2.0)
        assert got[0].nonzero()[0].tolist() == [1, 2, 4] and (raw[0, [1, 2, 4]] == raw[0, 1]).all()
        judge(got, raw, sums, word, 4, 2.0, [15])
        sums[0, :3, 1] = (-(1 << 20), 1 << 20, -(1 << 20))    # a spread of 2^21 at tau = 0.5: the losers underflow, no NaN
        got, raw = targets(env, sums, word, 4, 0.5)
        assert got[0, 2] == 1.0 and got[0, 1] == 0.0 and got[0, 4] == 0.0 and np.isfinite(got).all()
        judge(got, raw, sums, word, 4, 0.5, [15])
    finally:
        env.close()
