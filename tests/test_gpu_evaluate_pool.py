"""GPU: evaluate.evaluate_vs_pool / SelfPlay.evaluate(opponent=[...]) — the duplicate evaluation against K networks on
ONE env of K blocks, one tarok_policy_step_pool launch per lock-step.  256 games per opponent, one episode.

Run on the GPU box:  python -m pytest tests/test_gpu_evaluate_pool.py -m gpu -q
"""
import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

GAMES, EPISODES, SEED = 256, 1, 12


@pytest.fixture(scope="module")
def nets(T):
    from policy_step_cases import make_weights
    return [make_weights(T, s) for s in (0, 1, 2)]


def test_a_pool_of_copies_of_the_weights_scores_exactly_zero(T, nets):
    from tarok_amd import evaluate as EV
    A = nets[0]
    res = EV.evaluate_vs_pool(A, [[w.clone() for w in A] for _ in range(3)], GAMES, EPISODES, seed=SEED)
    assert len(res) == 3
    for r in res:
        assert r["advantage"] == 0.0 and r["stderr"] == 0.0 and r["by_seat"] == [0.0] * 4 and r["deals"] == GAMES * EPISODES
        assert r["policy_mean"] == r["bot_mean"]


def test_a_pool_of_one_is_evaluate_vs_policy(T, nets):
    from tarok_amd import evaluate as EV
    A, B, _ = nets
    for mode in (dict(), dict(temperature=0.0, epsilon=0.25)):
        assert EV.evaluate_vs_pool(A, [B], GAMES, EPISODES, seed=SEED, **mode) == [EV.evaluate_vs_policy(A, B, GAMES, EPISODES, seed=SEED, **mode)]


def test_every_dict_is_the_statistic_of_its_own_block(T, nets):
    """K = 2 different opponents: dict k is duplicate_advantage of the scores of block k's slots [256 k, 256 k + 256), taken
    from the passes' inspect hook; the two dicts differ; block 0 (the deals of evaluate_vs_policy) is that call's dict."""
    from tarok_amd import evaluate as EV
    A, B, C = nets
    record = []
    res = EV.evaluate_vs_pool(A, [B, C], GAMES, EPISODES, seed=SEED, inspect=record)
    assert [(r["episode"], r["seats"]) for r in record] == [(0, s) for s in EV.PASS_SEATS]
    assert all(r["scores"].shape == (2 * GAMES, 4) for r in record)
    for k in range(2):
        block = np.stack([r["scores"][k * GAMES:(k + 1) * GAMES] for r in record])           # [5, 256, 4]
        assert res[k] == EV.duplicate_advantage(block), k
        assert res[k]["deals"] == GAMES
    assert res[0] != res[1]
    assert res[0] == EV.evaluate_vs_policy(A, B, GAMES, EPISODES, seed=SEED)
    assert EV.evaluate_vs_pool(A, [B, C], GAMES, EPISODES, seed=SEED) == res
    # the opponent of a block is its own: with the two swapped, block 1 (the same deals) now meets B
    swapped = EV.evaluate_vs_pool(A, [C, B], GAMES, EPISODES, seed=SEED)
    assert swapped[1] != res[1] and swapped[0] != res[0]
    # n_games that is no multiple of 256: whole step groups are played, the first n_games slots of a block count
    part = EV.evaluate_vs_pool(A, [B, C], 100, EPISODES, seed=SEED)
    assert part[0] == EV.evaluate_vs_policy(A, B, 100, EPISODES, seed=SEED) and part[1]["deals"] == 100


def test_selfplay_evaluate_against_a_list(T):
    import torch
    from oracle import tarok_spec as S
    from tarok_amd import selfplay as SP
    env = T.TarokVecEnv(512, seed=8, mix=S.MIX_ALL)
    try:
        sp = SP.SelfPlay(env, hidden=256, seed=0)
        snap = sp.snapshot()
        before = env.state().copy()
        res = sp.evaluate(n_games=GAMES, episodes=EPISODES, opponent=[snap, sp.snapshot()])
        assert isinstance(res, list) and len(res) == 2
        assert all(r["advantage"] == 0.0 and r["deals"] == GAMES for r in res)
        assert (env.state() == before).all()          # on an env of its own
        with pytest.raises(ValueError):
            sp.evaluate(n_games=GAMES, episodes=EPISODES, opponent=[])
    finally:
        env.close()
