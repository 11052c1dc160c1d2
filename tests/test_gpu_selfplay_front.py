"""GPU: SelfPlay(front=...) — the bid and exchange heads on the games a training rollout swaps in.
n = 512, T = 16: the captured rollout against the eager one, the empty seat set against front=None, the statistics of
iterate() against a recount from get_lines(), and one iterate() through the fused learner; then front= with an opponent
pool, self-play groups and learner seats — alone, with GAE, with a teacher — whose rollouts are replayed on the oracle
model (tests/oracle_model.py) from the twin chain's game starts.  Bytes and integers only.

Run on the GPU box:  python -m pytest tests/test_gpu_selfplay_front.py -m gpu -q
"""
import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

N, T_STEPS, SEED = 512, 16, 5
KEYS = ("obs", "words", "act", "logp", "val", "done", "reward")


def heads():
    from front_lines_cases import random_weights
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


# ---- front= composed with what it is trained with: an opponent pool with self-play groups, GAE, a teacher.  The rollout's
# act / done / reward (and words) arrays are replayed on tests/oracle_model.SlotModel: the card is the network's and only has
# to be accepted; every game — the first too — starts as the twin chain's game of its (slot, episode) under the seat sets
# SelfPlay hands to front_lines (front_lines_cases.twin_chain: neither front_lines nor a step kernel is in it).
POOL = dict(self_play_groups=0.5, learner_seats=5)


def pool():
    from front_lines_cases import random_weights
    return [random_weights(31), random_weights(32)]


def play(T, use_graph, rollouts=2, iterate=False, **kw):
    """run() with the warm-up rollout kept: (every buffer in order — the eager path's two warm-up lock-steps first —, the
    lines at the end, the stats of iterate(), the object, the env)."""
    import torch
    from tarok_amd import karte as K
    from tarok_amd.selfplay import SelfPlay
    env = T.TarokVecEnv(N, seed=SEED, mix=K.MIX_BOT)
    sp = SelfPlay(env, seed=1, use_graph=use_graph, front=heads(), opponent=pool(), **dict(POOL, **kw))
    copy = lambda buf: {k: buf[k].cpu().numpy().copy() for k in KEYS}
    out, stats = [], None
    if not use_graph:
        out.append(copy(sp.collect(2)))
    for _ in range(rollouts):
        if iterate:
            stats = sp.iterate(T_STEPS)
            buf = sp._buf
        else:
            buf = sp.collect(T_STEPS)
        torch.cuda.synchronize()
        out.append(copy(buf))
    return out, env.get_lines(), stats, sp, env


def replay(T, sp, bufs):
    """Every slot of the buffers on the oracle model; returns (games ended, games started that differ from the Bot's line)."""
    import front_lines_model as FM
    from oracle import oracle as O
    from oracle import tarok_spec as S
    from oracle_model import SlotModel
    from front_lines_cases import twin_chain
    f = sp.front
    kw = dict(bid=sp._front_w["bid"], exchange=sp._front_w["exchange"], scale=f["scale"], contracts=f["contracts"], margin=f["margin"],
              playouts=f["playouts"], pass_value=f["pass_value"], seats_per_game=sp._seats)
    chains, started = {}, []

    def hook(index, ep):
        if ep not in chains:
            chains[ep] = twin_chain(T, ep, kw, n=N, seed=SEED, offset=0)[0]
        if ep > 0:
            started.append((index, ep))
        return O.Game.from_lanes(chains[ep][:, index]), S.game_key(SEED, index, ep)
    models = [SlotModel(SEED, j, S.MIX_BOT, game_of=hook) for j in range(N)]
    first = bufs[0]["words"][0].view(np.uint64)
    assert all(int(first[j]) == m.g.obs_word(False) for j, m in enumerate(models)), "the first observation"
    ended = 0
    for r, buf in enumerate(bufs):
        words = buf["words"].view(np.uint64)
        for t in range(buf["act"].shape[0]):
            for j, m in enumerate(models):
                row = m.card(int(buf["act"][t, j]), auto=True)
                assert not row.rejected, ("the rollout's card is not accepted", r, t, j, int(buf["act"][t, j]))
                assert int(buf["done"][t, j]) == row.done, ("done", r, t, j)
                assert buf["reward"][t, j].tolist() == (row.reward if row.done else [0, 0, 0, 0]), ("reward", r, t, j)
                assert int(words[t + 1, j]) == row.obs, ("words", r, t, j)
                ended += row.done
    differ = sum(1 for j, ep in started if (chains[ep][:, j] != FM.bot_line(SEED, j, ep, S.MIX_BOT).lanes()).any())
    return ended, differ


def test_pool_composition_replays_on_the_oracle(T):
    """front= with a pool of two snapshots, self_play_groups = 0.5 and learner_seats = 5: the captured rollouts equal the
    eager ones byte for byte, and both rollouts (behind the two warm-up lock-steps) replay on the model."""
    eager, lines_e, _, sp, env_e = play(T, False)
    graph, lines_g, _, _, env_g = play(T, True)
    try:
        seats = sp._seats.cpu().numpy()
        assert (seats[:256] == 15).all() and (seats[256:] == 5).all(), "a self-play group, and a group whose seats 0 and 2 learn"
        assert same(eager[1:], graph) and (lines_e == lines_g).all()
        ended, differ = replay(T, sp, eager)
        assert ended > 0 and differ > 0, "games ended, and games began that are not the Bot's"
    finally:
        env_e.close()
        env_g.close()


@pytest.mark.parametrize("extra", [dict(gamma=0.99, gae_lambda=0.95), dict(teacher=dict(worlds=1, samples=1, tau=1.0, every=8), distill_coef=0.5)],
                         ids=["gae", "teacher"])
def test_pool_composition_through_one_iterate(T, extra):
    """The same composition with GAE, and with a playout teacher (distillation), through one iterate() of the fused learner:
    no env error, a finite loss, the captured rollout equal to the eager one, and the rollout replays on the model."""
    eager, _, stats_e, sp, env_e = play(T, False, rollouts=1, iterate=True, **extra)
    graph, _, stats_g, _, env_g = play(T, True, rollouts=1, iterate=True, **extra)
    try:
        for stats in (stats_e, stats_g):
            assert stats["env_errors"] == 0 and np.isfinite(stats["loss"])
        assert same(eager[1:], graph)
        ended, differ = replay(T, sp, eager)
        assert ended > 0 and differ > 0
    finally:
        env_e.close()
        env_g.close()
