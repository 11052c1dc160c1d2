"""GPU: SelfPlay against a POOL of frozen opponents (opponent=[snapshot, ...]: tarok_policy_step_pool in the captured
rollout, the learner path as for one opponent), on 1,024 games = four step groups, T = 16, two iterations.

Run on the GPU box:  python -m pytest tests/test_gpu_selfplay_pool.py -m gpu -q
"""
import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

N, TN, ITERS = 1024, 16, 2


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


@pytest.fixture(scope="module")
def snaps(T):
    """Two different frozen networks (make_weights of the versus test: PolicyNet(256), parameters x 3)."""
    from policy_step_cases import make_weights
    return make_weights(T, 11), make_weights(T, 12)


def train(T, S, opponent, swap=None, **kw):
    """ITERS iterations of a fresh SelfPlay on a fresh env (mid-game start, so that games end inside the rollouts);
    swap = (weights, index): set_opponent before the second iteration.  Returns (the final parameters, the recorded
    cards of every iteration [ITERS, T, N], the stats, the last rollout's host arrays, the object's seat sets and groups)."""
    import torch
    from tarok_amd import selfplay as SP
    env = T.TarokVecEnv(N, seed=8, mix=S.MIX_ALL)
    try:
        sp = SP.SelfPlay(env, hidden=256, seed=0, opponent=opponent, **kw)
        obs = env.legal_actions()
        for _ in range(34):
            obs, _, _ = env.step(env.policy_random(obs), auto_reset=True)
        sp.obs_words.copy_(obs.words)
        acts, stats = [], []
        for it in range(ITERS):
            if swap is not None and it == 1:
                sp.set_opponent(swap[0], index=swap[1]) if swap[1] is not None else sp.set_opponent(swap[0])
            stats.append(sp.iterate(T=TN))
            acts.append(sp._buf["act"].cpu().numpy().copy())
        torch.cuda.synchronize()
        last = {k: sp._buf[k].cpu().numpy().copy() for k in ("reward", "done", "words")}
        seats = sp._seats.cpu().numpy().copy()
        groups = None if sp._group_net is None else sp._group_net.cpu().numpy().copy()
        return sp.flat.detach().cpu().clone(), np.stack(acts), stats, last, seats, groups
    finally:
        env.close()


def test_a_pool_of_copies_trains_to_the_bits_of_the_single_opponent(T, S, snaps):
    import torch
    s, _ = snaps
    one = train(T, S, s)
    pool = train(T, S, [s, s, s])
    assert torch.equal(one[0].view(torch.int32), pool[0].view(torch.int32))
    assert (one[1] == pool[1]).all()
    assert [x["learner_samples"] for x in one[2]] == [x["learner_samples"] for x in pool[2]]
    assert one[2][-1]["learner_samples"] > 0
    assert pool[5].tolist() == [0, 1, 2, 0] and len(pool[2][-1]["learner_mean_score_by_opponent"]) == 3
    assert "learner_mean_score_self" not in pool[2][-1] and "learner_mean_score_by_opponent" not in one[2][-1]


def test_set_opponent_by_index_changes_that_entrys_groups_only(T, S, snaps):
    """Four groups on a pool of three: group g meets g % 3, so the groups on entry 1 are those with g % 3 == 1 — group 1
    alone here; group 3 is back on entry 0.  Iteration 0 is the same in both runs; after set_opponent(w, index=1) the
    cards of group 1 change and those of groups 0, 2 and 3 do not (the learner's update is the same up to there, and a
    slot's cards depend on its own group's networks only)."""
    s, w = snaps
    kept = train(T, S, [s, s, s])
    swapped = train(T, S, [s, s, s], swap=(w, 1))
    group = np.arange(N) // 256
    assert (kept[1][0] == swapped[1][0]).all()                                   # before the swap: the same rollout
    touched = group % 3 == 1
    assert (kept[1][1][:, ~touched] == swapped[1][1][:, ~touched]).all()
    assert (kept[1][1][:, touched] != swapped[1][1][:, touched]).any()
    from tarok_amd import selfplay as SP
    env = T.TarokVecEnv(N, seed=8, mix=S.MIX_ALL)
    try:
        sp = SP.SelfPlay(env, hidden=256, seed=0, opponent=[s, s, s])
        with pytest.raises(ValueError):
            sp.set_opponent(w)                        # a pool needs index=
        with pytest.raises(ValueError):
            sp.set_opponent(w, index=3)
    finally:
        env.close()


def test_self_play_groups_learn_on_all_four_seats_and_the_scores_by_opponent(T, S, snaps):
    """self_play_groups = 0.25 on four groups: the period is 4, so group 0 is plain self-play (index K = 2, seat sets 15)
    and groups 1, 2, 3 meet opponents 1, 0, 1.  learner_samples counts all four seats of group 0's slots;
    learner_mean_score_by_opponent / _self equal a NumPy recomputation from the recorded rewards."""
    s, w = snaps
    _, acts, stats, last, seats, groups = train(T, S, [s, w], self_play_groups=0.25)
    assert groups.tolist() == [2, 1, 0, 1]
    group = np.arange(N) // 256
    assert (seats[group == 0] == 15).all()
    assert (seats[group != 0] == (1 << (np.arange(N) % 4))[group != 0]).all()
    words = last["words"][:TN].view(np.uint64)
    mover = ((words >> np.uint64(54)) & np.uint64(3)).astype(np.int64)
    mine = ((seats[None, :].astype(np.int64) >> mover) & 1).astype(bool)
    st = stats[-1]
    # every one of the learner's samples whose game ended inside the rollout is known to the Monte-Carlo returns; group 0
    # contributes on all four seats: more than any single-seat count could give
    done = last["done"].astype(bool)
    ends_later = np.flip(np.maximum.accumulate(np.flip(done, 0), 0), 0)          # a game end at or after lock-step t
    known = mine & ends_later
    assert st["learner_samples"] == int(known.sum())
    assert int(known[:, group == 0].sum()) == int(ends_later[:, group == 0].sum()) > 0
    assert int(known[:, group == 1].sum()) < int(ends_later[:, group == 1].sum())
    # the scores by opponent
    own = ((seats[:, None].astype(np.int64) >> np.arange(4)) & 1).astype(np.float64)         # [N, 4]
    wgt = done[:, :, None].astype(np.float64) * own[None]
    rew = last["reward"].astype(np.float64)
    net = np.minimum(groups, 2)[group]
    for k in range(2):
        m = net == k
        want = (rew[:, m] * wgt[:, m]).sum() / max(1.0, wgt[:, m].sum())
        assert st["learner_mean_score_by_opponent"][k] == want, k
    m = net == 2
    assert st["learner_mean_score_self"] == (rew[:, m] * wgt[:, m]).sum() / max(1.0, wgt[:, m].sum())
    assert len(st["learner_mean_score_by_opponent"]) == 2 and wgt[:, m].sum() > 0
