"""GPU: tarok_playout_exchange_net_list (the exchange's net playouts on a compacted item list) checked exactly — bytes
against bytes: the three outputs against tarok_playout_exchange_net (depth None / 13) and tarok_playout_exchange_net_value
(depths 12, 1, 3) on random bf16 weights and on the exactly summable integer sets of tests/playout_net_value_cases.py, at
net_seats 15, 1 and 0 (there also tarok_playout_exchange); the list read back from the scratch against the dense grid; empty
lists; each output alone; determinism; salt; batch independence; a captured graph; the learner and the evaluation.  Every
launch writes into guard bands (tests/guarded.py) over a guarded scratch of exactly the header's size and leaves the env and
its counters as they were.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_exchange_net_list.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import front_list_cases as F
import gpu_harness as H
import playout_front_net_value_cases as C
from gpu_harness import T, random_net  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
make_env = functools.partial(H.make_env, seed=C.X_SEED, offset=C.X_OFFSET, episode=C.X_EPISODE, defer_exchange=True)
DEPTHS = (None, 13, 12, 1, 3)
NAMES = ("sums", "choices", "discards")


@pytest.fixture(scope="module")
def nets(T):
    """The integer set R as a kernel set, and one random bf16 set."""
    import policy_exact_ref as PE
    return dict(R=PE.kernel_weights(T, C.weight_sets()["R"]), random=random_net(T, 17))


def assert_same(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        assert g.tobytes() == w.tobytes(), (tag, name, np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0][:8])


def both(env, kw, worlds, sets, net_seats, depth, tag, check_list=True, **kw_launch):
    """The list launch and the dense launch of the same arguments: equal outputs, and the list is the dense grid compacted."""
    a, b = [], []
    want = F.exchange_dense(env, kw, worlds, sets, net_seats, depth, scratch_out=a, **kw_launch)
    got = F.exchange_list(env, kw, worlds, sets, net_seats, depth, scratch_out=b, **kw_launch)
    assert_same(got, want, tag)
    total = None
    if check_list:
        bound = F.exchange_bound(env.n, worlds, sets)
        total, on, base, counts = F.assert_list_is_the_dense_grid_compacted(b[0], a[0], bound, bound, 6 * env.n)
        assert (on == 0).sum() + (on == (1 << sets) - 1).sum() == on.size
        assert (base == np.concatenate([[0], np.cumsum(counts * worlds)[:-1]])).all(), "base is the exclusive prefix sum"
    return got, total


@pytest.mark.parametrize("n,worlds,sets", [(5, 3, 2), (1, 3, 2), (43, 2, 2)])
def test_bytes_of_the_dense_launches_on_the_bots_mix(T, nets, n, worlds, sets):
    """n = 5 (at most 180 live items: a full and a partial play tile), n = 1, n = 43 (258 units: across the 256-unit scan
    block) at every depth and net_seats 15, 1, 0, on both weight sets; at net_seats = 0 also tarok_playout_exchange."""
    from oracle import tarok_spec as S
    env = make_env(T, n, S.MIX_BOT)
    try:
        some = 0
        for k, depth in enumerate(DEPTHS):
            for net_seats in (15, 1, 0):
                kw = nets["R" if (k + net_seats) & 1 else "random"]
                got, total = both(env, kw, worlds, sets, net_seats, depth, (n, depth, net_seats))
                some += int(got[0].any())
                assert total > 0 and (n == 1 or total < F.exchange_bound(n, worlds, sets))
                if net_seats == 0 and F.to_the_end(depth):
                    assert_same(got, H.launch_exchange_bot(env, worlds, 1, sets, salt=3), ("bot", n, depth))
        assert some >= 10
    finally:
        env.close()


@pytest.mark.parametrize("mix", ["tri", "dve", "ena", "solo_ena"])
def test_single_contract_envs(T, nets, mix):
    """A Tri has 2 groups, a Dve 3, an Ena 6: the list holds 1/3, 1/2 and all of the grid."""
    n, worlds, sets = 5, 3, 2
    env = make_env(T, n, C.X_MIXES[mix])
    try:
        for depth, net_seats, name in ((None, 15, "random"), (1, 1, "R"), (3, 0, "random"), (12, 15, "R"), (13, 0, "R")):
            got, total = both(env, nets[name], worlds, sets, net_seats, depth, (mix, depth, net_seats))
            groups = dict(tri=2, dve=3, ena=6, solo_ena=6)[mix]
            assert total == n * groups * sets * worlds and got[0].any()
    finally:
        env.close()


def test_seat_sets_games_that_do_not_wait_and_empty_lists(T, nets):
    """Declarers outside the set (zero sums, the Bot's own exchange), per-game sets, a Klop that does not wait; then the
    empty seat set and an env where no game waits for the exchange: total 0 and the dense launch's outputs."""
    from oracle import tarok_spec as S
    n, worlds, sets = 5, 3, 2
    env = make_env(T, n, S.MIX_BOT)
    try:
        per = np.array([15, 0, 2, 13, 15], np.uint8) | np.uint8(0x30)
        for depth in (None, 3):
            for seats, per_game in ((5, None), (0, per), (10, None)):
                both(env, nets["random"], worlds, sets, 15, depth, ("sets", depth, seats), salt=9, seats=seats, per_game=per_game)
            got, total = both(env, nets["R"], worlds, sets, 15, depth, ("empty set", depth), seats=0)
            assert total == 0 and not got[0].any() and (got[1] >= -1).all()
    finally:
        env.close()
    env = H.make_env(T, n, S.MIX_BOT, seed=C.X_SEED, offset=C.X_OFFSET, episode=C.X_EPISODE)      # the exchange not deferred: nobody waits
    try:
        got, total = both(env, nets["random"], worlds, sets, 15, 1, "nobody waits")
        assert total == 0 and not got[0].any() and (got[1] == -1).all() and (got[2] == 255).all()
    finally:
        env.close()


def test_each_output_alone_determinism_salt_and_batch_independence(T, nets):
    from oracle import tarok_spec as S
    worlds, sets, kw = 3, 2, nets["random"]
    env, two = make_env(T, 5, S.MIX_BOT), make_env(T, 2, S.MIX_BOT)
    try:
        outs = ("sum", "choice", "discards")
        a, b = [], []
        full = F.exchange_list(env, kw, worlds, sets, 15, 3, scratch_out=a)
        again = F.exchange_list(env, kw, worlds, sets, 15, 3, scratch_out=b)
        assert_same(again, full, "twice")
        assert a[0].tobytes() == b[0].tobytes(), "the whole scratch"
        for i, one in enumerate(outs):
            alone = F.exchange_list(env, kw, worlds, sets, 15, 3, want=(one,))
            assert alone[i].tobytes() == full[i].tobytes() and all(x is None for j, x in enumerate(alone) if j != i), one
        salted = F.exchange_list(env, kw, worlds, sets, 15, 3, salt=4)
        assert salted[0].tobytes() != full[0].tobytes()
        assert_same(salted, F.exchange_dense(env, kw, worlds, sets, 15, 3, salt=4), "salt")
        first = F.exchange_list(two, kw, worlds, sets, 15, 3)
        assert_same(first, [x[:2] for x in full], "the first two games")
    finally:
        env.close()
        two.close()


def test_a_captured_launch_replays_with_the_weights_in_place(T, nets):
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 37, S.MIX_BOT)
    try:
        kw, other = [t.clone() for t in nets["random"]], random_net(T, 23)
        env.playout_exchange_net_list_scratch(2, 2)                # allocated before the capture
        outs = [torch.zeros((37, 12, 4), dtype=torch.int32, device="cuda"), torch.zeros(37, dtype=torch.int8, device="cuda"),
                torch.zeros((37, 3), dtype=torch.uint8, device="cuda")]
        eager = lambda w: [t.cpu() for t in env.playout_exchange_net_value(w, 2, 2, 2, 0.5, salt=4)]
        first = eager(kw)
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_exchange_net_list(kw, 2, 2, 2, 0.5, salt=4, sum_out=outs[0], choice_out=outs[1], discards_out=outs[2])
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.cpu(), x) for o, x in zip(outs, first))
        for t, o in zip(kw, other):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        second = eager(other)
        assert all(torch.equal(o.cpu(), x) for o, x in zip(outs, second)) and not torch.equal(second[0], first[0])
    finally:
        env.close()


def test_the_python_surface_the_learner_and_the_evaluation(T, nets):
    """playout_exchange_net_list equals the direct C call and depth=None the plain launch; ExchangeLearner(net_list=True)
    collects the eager list launch's rows and steps; evaluate_exchange_net_vs_bot(net_list=True) returns the numbers of
    net_list=False."""
    import torch
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    from tarok_amd.exchange import ExchangeLearner
    kw = nets["random"]
    env = make_env(T, 5, S.MIX_BOT)
    try:
        want = F.exchange_list(env, kw, 3, 2, 10, 2, scale=0.5, salt=2)
        got = env.playout_exchange_net_list(kw, 3, 2, 2, 0.5, net_seats=10, salt=2)
        assert all((g.cpu().numpy() == w).all() for g, w in zip(got, want))
        assert all(torch.equal(a, b) for a, b in zip(env.playout_exchange_net(kw, 3, 2, salt=2), env.playout_exchange_net_list(kw, 3, 2, salt=2)))
        with pytest.raises(ValueError):
            env.playout_exchange_net_list(kw, 3, 2, 14)
    finally:
        env.close()
    env, twin = T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT), T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT)
    try:
        xl = ExchangeLearner(env, worlds=2, discard_sets=2, seed=5, net=kw, net_seats=15, net_list=True)
        fw, sums, cands, playouts = xl.collect(3)
        twin.reset(episode=3, defer_exchange=True)
        assert playouts == 2 and sums.any() and torch.equal(sums, twin.playout_exchange_net_list(kw, 2, 2, net_seats=15, salt=5)[0])
        assert torch.equal(sums, twin.playout_exchange_net(kw, 2, 2, net_seats=15, salt=5)[0])
        assert np.isfinite(xl.step(fw, sums, cands, playouts))
    finally:
        env.close()
        twin.close()
    for depth in (None, 2):
        a = EV.evaluate_exchange_net_vs_bot(kw, 2, 2, 32, 1, seed=3, net_list=True, net_depth=depth)
        b = EV.evaluate_exchange_net_vs_bot(kw, 2, 2, 32, 1, seed=3, net_list=False, net_depth=depth)
        assert a == b, depth
