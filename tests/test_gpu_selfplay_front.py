"""GPU: SelfPlay(front=...) — the bid and exchange heads on the games a training rollout swaps in.
n = 512, T = 16: the captured rollout against the eager one, the empty seat set against front=None, the statistics of
iterate() against a recount from get_lines(), and one iterate() through the fused learner.  Bytes and integers only.

Run on the GPU box:  python -m pytest tests/test_gpu_selfplay_front.py -m gpu -q
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, T_STEPS, SEED = 512, 16, 5
KEYS = ("obs", "words", "act", "logp", "val", "done", "reward")


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import tarok_amd
    tarok_amd.build()
    return tarok_amd


def heads():
    from test_gpu_front_lines import random_weights
    return dict(bid=random_weights(11, 4.0), exchange=random_weights(12, 4.0), scale=70.0, contracts=0x3FF)


def run(T, front, use_graph, rollouts=2, **kw):
    """`rollouts` collect(T_STEPS) of a fresh SelfPlay: (the buffers of each as bytes, the lines at the end, the object).
    The captured path plays a warm-up rollout of two lock-steps before its capture: the eager one plays it too."""
    import torch
    from tarok_amd import karte as K
    from tarok_amd.selfplay import SelfPlay
    env = T.TarokVecEnv(N, seed=SEED, mix=K.MIX_BOT)
    sp = SelfPlay(env, seed=1, use_graph=use_graph, front=front, **kw)
    out = []
    if not use_graph:
        sp.collect(2)
    for _ in range(rollouts):
        buf = sp.collect(T_STEPS)
        torch.cuda.synchronize()
        out.append({k: buf[k].cpu().numpy().copy() for k in KEYS})
    return out, env.get_lines(), sp, env


def same(a, b):
    return all((x[k].view(np.uint8) == y[k].view(np.uint8)).all() for x, y in zip(a, b) for k in KEYS)


def test_captured_rollout_equals_the_eager_one(T):
    eager, lines_e, _, env_e = run(T, heads(), False)
    graph, lines_g, _, env_g = run(T, heads(), True)
    assert same(eager, graph) and (lines_e == lines_g).all()
    env_e.close()
    env_g.close()


def test_empty_seat_set_equals_front_none(T):
    snap = [t.clone() for t in heads()["bid"]]
    seated, lines, _, env_s = run(T, heads(), True, opponent=snap, learner_seats=0)
    versus, _, _, env_v = run(T, None, True, opponent=snap, learner_seats=0)
    assert same(seated, versus), "no seat for the heads: the Bot's fronts, the rollout of front=None"
    tag = lines[:, :, 5]
    assert ((tag >> np.uint64(32)) != 0).any(), "... and the lines are marked all the same"
    for e in (env_s, env_v):
        e.close()


def test_statistics_are_a_recount_of_the_lines(T):
    import torch
    from tarok_amd import karte as K
    from tarok_amd.selfplay import SelfPlay
    env = T.TarokVecEnv(N, seed=SEED, mix=K.MIX_BOT)
    sp = SelfPlay(env, seed=1, front=heads())
    first = sp.iterate(T_STEPS)
    assert first["fronted"] == 0, "the start fronted all fourteen lines of every slot and no game has ended yet"
    before = env.get_lines()
    unmarked = (before[:, :, 5] >> np.uint64(32)) != (before[:, :, 5] & np.uint64(0xFFFFFFFF))
    ep = env.counters()[0]
    nep = (before[:, :, 5] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    valid = (nep > ep[:, None]) & (nep <= ep[:, None] + 14)
    stats = sp.iterate(T_STEPS)                           # its front_lines call takes exactly the valid, unmarked lines
    assert stats["fronted"] == int((unmarked & valid).sum()) > 0
    # those lines were dealt during the first rollout, thirteen games ahead or more: the second rollout cannot have reached them
    after, lanes = env.get_lines(lanes=True)
    took = unmarked & valid
    assert (after[:, :, 5][took] & np.uint64(0xFFFFFFFF) == before[:, :, 5][took] & np.uint64(0xFFFFFFFF)).all()
    assert ((after[:, :, 5][took] >> np.uint64(32)) == (after[:, :, 5][took] & np.uint64(0xFFFFFFFF))).all()
    hist = np.bincount(((lanes[9][took] >> np.uint64(33)) & np.uint64(15)).astype(np.int64), minlength=10)
    assert stats["front_contract_share"] == [int(c) / max(1, stats["fronted"]) for c in hist]
    assert stats["env_errors"] == 0 and np.isfinite(stats["loss"]), "one iterate() through the fused learner"
    env.close()
