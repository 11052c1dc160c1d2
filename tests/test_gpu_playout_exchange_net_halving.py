"""GPU: tarok_playout_exchange_net_halving (sequential halving over a game's exchange candidates, on the compacted item list)
checked exactly.  One round against tarok_playout_exchange_net_list byte for byte; the schedules (1,1,2), (2,2,4,8), (4,4,4,4)
and (1,3) against an expectation built from list launches at the cumulative ends and walked by
tests/playout_front_halving_model.py — sums, counts, choice and discards —, with the inputs ASSERTED to hold a tie at a cut, a
game that leaves early and a final choice that differs from the uniform launch's; shapes, seat sets, empty lists; the guarded
scratch of exactly the header's size and one 16-byte step short; each output alone, determinism, salt, batch independence; a
captured first call; the learner and the evaluation.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_exchange_net_halving.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import front_halving_cases as FH
import front_list_cases as F
import gpu_harness as H
import playout_front_halving_model as M
import playout_front_net_value_cases as C
from gpu_harness import T, random_net  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
make_env = functools.partial(H.make_env, seed=C.X_SEED, offset=C.X_OFFSET, episode=C.X_EPISODE, defer_exchange=True)
SCHEDULES = ((1, 1, 2), (2, 2, 4, 8), (4, 4, 4, 4), (1, 3))
NAMES = FH.X_NAMES


@pytest.fixture(scope="module")
def nets(T):
    """The integer set R as a kernel set, and one random bf16 set."""
    import policy_exact_ref as PE
    return dict(R=PE.kernel_weights(T, C.weight_sets()["R"]), random=random_net(T, 17))


def assert_same(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        assert g.tobytes() == np.ascontiguousarray(w, g.dtype).tobytes(), (tag, name, np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0][:8])


@pytest.mark.parametrize("n", [1, 17])
def test_one_round_is_the_list_launch(T, nets, n):
    """(W,) against tarok_playout_exchange_net_list at worlds = W: depths None, 13, 12, 1, net_seats 15, 1 and 0."""
    from oracle import tarok_spec as S
    env = make_env(T, n, S.MIX_BOT)
    try:
        for k, depth in enumerate((None, 13, 12, 1)):
            for net_seats in (15, 1, 0):
                kw = nets["R" if (k + net_seats) & 1 else "random"]
                want = F.exchange_list(env, kw, 3, 2, net_seats, depth)
                got = FH.exchange_halving(env, kw, (3,), 2, net_seats, depth)
                assert_same((got[0], got[2], got[3]), want, (n, depth, net_seats))
                live = want[0].any(axis=2) | (got[1] != 0)
                assert (got[1][live] == 3).all() and set(np.unique(got[1]).tolist()) <= {0, 3}, (n, depth, net_seats)
    finally:
        env.close()


def test_schedules_against_the_walk_over_list_launches(T, nets):
    """Every schedule at depth None and 1 on 17 games of the Bot's mix, and a Tri-only env at D = 1 (two candidates: every game
    leaves after round 0); the inputs hold each case the rule has."""
    from oracle import tarok_spec as S
    tally = FH.Tally()
    env, tri = make_env(T, 17, S.MIX_BOT), make_env(T, 5, C.X_MIXES["tri"])
    try:
        for schedule in SCHEDULES:
            for depth, name, net_seats in ((None, "random", 15), (1, "R", 15), (1, "random", 5)):
                want = FH.expect_exchange(env, nets[name], schedule, 2, net_seats, depth, tally)
                got = FH.exchange_halving(env, nets[name], schedule, 2, net_seats, depth)
                assert_same(got, want, (schedule, depth, net_seats))
            early = FH.Tally()
            want = FH.expect_exchange(tri, nets["random"], schedule, 1, 15, None, early)
            got = FH.exchange_halving(tri, nets["random"], schedule, 1, 15, None)
            assert_same(got, want, ("tri", schedule))
            assert early.units == 5 and early.early == 5 and (got[1].max(axis=1) == schedule[0]).all()
        print(tally)
        assert tally.ties > 0 and tally.early > 0 and tally.differs > 0, tally      # (on the Bot's mix alone)
    finally:
        env.close()
        tri.close()


def test_shapes_seat_sets_and_empty_lists(T, nets):
    """n = 300 (1,800 units: across the 256-unit scan block), seat sets and per-game sets, the empty set, an env where nobody
    waits."""
    from oracle import tarok_spec as S
    tally = FH.Tally()
    env = make_env(T, 300, S.MIX_BOT)
    try:
        want = FH.expect_exchange(env, nets["random"], (1, 3), 2, 15, 1, tally)
        assert_same(FH.exchange_halving(env, nets["random"], (1, 3), 2, 15, 1), want, "300")
    finally:
        env.close()
    env = make_env(T, 5, S.MIX_BOT)
    try:
        per = np.array([15, 0, 2, 13, 15], np.uint8) | np.uint8(0x30)
        for seats, per_game in ((5, None), (0, per), (10, None), (0, None)):
            want = FH.expect_exchange(env, nets["R"], (2, 2, 4, 8), 2, 15, 3, tally, salt=9, seats=seats, per_game=per_game)
            got = FH.exchange_halving(env, nets["R"], (2, 2, 4, 8), 2, 15, 3, salt=9, seats=seats, per_game=per_game)
            assert_same(got, want, ("sets", seats))
        assert not got[0].any() and not got[1].any() and (got[2] >= -1).all()
    finally:
        env.close()
    env = H.make_env(T, 5, S.MIX_BOT, seed=C.X_SEED, offset=C.X_OFFSET, episode=C.X_EPISODE)      # the exchange not deferred: nobody waits
    try:
        got = FH.exchange_halving(env, nets["random"], (1, 1, 2), 2, 15, 1)
        assert not got[0].any() and not got[1].any() and (got[2] == -1).all() and (got[3] == 255).all()
    finally:
        env.close()


def test_the_scratch_each_output_alone_determinism_salt_and_batch_independence(T, nets):
    import torch
    from oracle import tarok_spec as S
    schedule, sets, kw = (2, 2, 4), 2, nets["random"]
    env, two = make_env(T, 5, S.MIX_BOT), make_env(T, 2, S.MIX_BOT)
    try:
        a, b = [], []
        full = FH.exchange_halving(env, kw, schedule, sets, 15, 3, scratch_out=a)          # (a guarded scratch of exactly the header's size)
        again = FH.exchange_halving(env, kw, schedule, sets, 15, 3, scratch_out=b)
        assert_same(again, full, "twice")
        assert a[0].tobytes() == b[0].tobytes(), "the whole scratch"
        for i, one in enumerate(NAMES):
            alone = FH.exchange_halving(env, kw, schedule, sets, 15, 3, want=(one,))
            assert alone[i].tobytes() == full[i].tobytes() and all(x is None for j, x in enumerate(alone) if j != i), one
        salted = FH.exchange_halving(env, kw, schedule, sets, 15, 3, salt=4)
        assert salted[0].tobytes() != full[0].tobytes()
        assert_same(FH.exchange_halving(two, kw, schedule, sets, 15, 3), [x[:2] for x in full], "the first two games")
        need = M.exchange_scratch(5, schedule, sets)
        scr = torch.empty(need, dtype=torch.uint8, device="cuda")
        out = torch.empty((5, 12, 4), dtype=torch.int32, device="cuda")
        rounds, arr = FH.schedule_args(schedule)
        p = env._p
        rc = lambda size, o: env.L.tarok_playout_exchange_net_halving(env._h, rounds, arr, sets, 0, 15, None, 15, 0, 70.0, *[p(t) for t in kw],
                                                                      p(scr), size, o, None, None, None, env._stream())
        assert rc(need - 16, p(out)) == -1 and rc(need, None) == -1 and rc(need, p(out)) == 0
        torch.cuda.synchronize()
    finally:
        env.close()
        two.close()


def test_a_captured_first_launch_replays_with_the_weights_in_place(T, nets):
    import torch
    from oracle import tarok_spec as S
    env, twin = make_env(T, 37, S.MIX_BOT), make_env(T, 37, S.MIX_BOT)
    try:
        kw, other = [t.clone() for t in nets["random"]], random_net(T, 23)
        env.playout_exchange_net_halving_scratch((1, 1, 2), 2)          # allocated before the capture
        outs = [torch.zeros((37, 12, 4), dtype=torch.int32, device="cuda"), torch.zeros((37, 12), dtype=torch.int32, device="cuda"),
                torch.zeros(37, dtype=torch.int8, device="cuda"), torch.zeros((37, 3), dtype=torch.uint8, device="cuda")]
        eager = lambda w: [t.cpu() for t in twin.playout_exchange_net_halving(w, (1, 1, 2), 2, 2, 0.5, salt=4)]
        for t, o in zip(kw, other):
            t.copy_(o)                                                   # the capture follows swapped weights
        first = eager(kw)
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_exchange_net_halving(kw, (1, 1, 2), 2, 2, 0.5, salt=4, sum_out=outs[0], count_out=outs[1], choice_out=outs[2],
                                                 discards_out=outs[3])
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.cpu(), x) for o, x in zip(outs, first))
        for t, o in zip(kw, nets["random"]):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        second = eager(kw)
        assert all(torch.equal(o.cpu(), x) for o, x in zip(outs, second)) and not torch.equal(second[0], first[0])
    finally:
        env.close()
        twin.close()


def test_the_learner_and_the_evaluation(T, nets):
    """ExchangeLearner(net=, net_halving=): collect() returns the launch's sums and counts, the targets are sum / count, one
    iterate gives a finite loss; evaluate_exchange_net_vs_bot(net_halving=(W,)) returns the numbers of net_list=True."""
    import torch
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    from tarok_amd.exchange import ExchangeLearner, exchange_targets
    kw = nets["random"]
    env, twin = T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT), T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT)
    try:
        xl = ExchangeLearner(env, discard_sets=2, seed=5, net=kw, net_halving=(1, 1, 2))
        fw, sums, cands, counts = xl.collect(3)
        twin.reset(episode=3, defer_exchange=True)
        want = twin.playout_exchange_net_halving(kw, (1, 1, 2), 2, salt=5)
        assert torch.equal(sums, want[0]) and torch.equal(counts, want[1]) and sums.any() and int(counts.max()) == 4 and int(counts[counts > 0].min()) < 4
        live, value, _, _ = exchange_targets(fw, sums, cands, counts, xl.reward_scale)
        w0 = fw[:, :6, 0]
        declarer = (((w0[:, 0] >> 55) & 1) + 2 * ((w0[:, 0] >> 56) & 1) + 3 * ((w0[:, 0] >> 57) & 1)).cpu().numpy()
        s, c, lv = sums.cpu().numpy().astype(np.float64), counts.cpu().numpy().astype(np.float64), live.cpu().numpy()
        for g in np.nonzero(lv.any(axis=1))[0][:16]:
            for i in np.nonzero(lv[g])[0]:
                mean = np.mean([s[g, i * 2 + d, declarer[g]] / c[g, i * 2 + d] for d in range(2)]) * xl.reward_scale
                assert abs(float(value[g, i]) - mean) <= 1e-5 * max(1.0, abs(mean)), (g, i)
        assert lv.any() and np.isfinite(xl.iterate())
    finally:
        env.close()
        twin.close()
    one = EV.evaluate_exchange_net_vs_bot(kw, 4, 2, 32, 1, seed=3, net_halving=(4,), net_depth=2)
    assert one == EV.evaluate_exchange_net_vs_bot(kw, 4, 2, 32, 1, seed=3, net_list=True, net_depth=2)


@pytest.mark.parametrize("schedule,depth,net_seats", [((1, 1, 2), 2, "own"), ((2, 2, 4, 8), None, 15)])
def test_the_evaluation_replayed_from_the_launchs_own_outputs(T, nets, schedule, depth, net_seats):
    """evaluate_exchange_net_vs_bot(net_halving=) on 32 games x 1 episode with a schedule of several rounds: on every pass the
    sums, the choice and the discards the evaluation handed to exchange() are those of the eager halving launch on a twin env
    in the inspected start state — the choice the first candidate at the maximum among the candidates its counts show alive at
    the end —, the halved choice differs from the uniform launch's somewhere, and pass 0 is the Bot-everywhere pass."""
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    kw, W = nets["random"], sum(schedule)
    seen, plain = [], []
    got = EV.evaluate_exchange_net_vs_bot(kw, None, 2, 32, 1, seed=5, salt=3, inspect=seen, net_seats=net_seats, net_halving=schedule,
                                          net_depth=depth)
    EV.evaluate_exchange_vs_bot(2, 1, 2, 32, 1, seed=5, salt=3, inspect=plain)
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS) and got["deals"] == 32
    twin = T.TarokVecEnv(32, seed=5, mix=S.MIX_BOT)
    try:
        from_bot = from_uniform = halved = 0
        for rec in seen:
            twin.reset(episode=0, defer_exchange=True)
            assert (twin.state() == rec["start"]).all()
            inner = rec["seats"] if net_seats == "own" else net_seats
            s, c, ch, di = [t.cpu().numpy() for t in twin.playout_exchange_net_halving(kw, schedule, 2, depth, net_seats=inner, salt=3,
                                                                                       seats=rec["seats"])]
            for name, w in (("sums", s), ("choice", ch), ("discards", di)):
                assert (rec[name] == w).all(), (rec["seats"], name)
            uniform = twin.playout_exchange_net_list(kw, W, 2, depth, net_seats=inner, salt=3, seats=rec["seats"])[1].cpu().numpy()
            cands = twin.exchange_candidates(2, salt=3).cpu().numpy().reshape(32, 12, 3)
            lanes = twin.state()
            for g in np.nonzero(c.any(axis=1))[0]:                       # the games that took part: the choice from the sums and counts
                declarer = int((int(lanes[9, g]) >> 37) & 3)
                alive = np.nonzero(c[g] == c[g].max())[0]
                best = min(alive.tolist(), key=lambda j: (-int(s[g, j, declarer]), j))
                assert rec["choice"][g] == best // 2 and (rec["discards"][g] == cands[g, best]).all(), (rec["seats"], g)
                halved += int(c[g][c[g] > 0].min() < W)
            from_uniform += int((rec["choice"] != uniform).sum())
            from_bot += int((rec["choice"] != seen[0]["choice"]).sum())
        assert halved > 0 and from_bot > 0, (halved, from_bot)
        print("choices that differ from the uniform launch's:", from_uniform)
    finally:
        twin.close()
    for name in ("start", "choice", "discards", "scores"):
        assert (seen[0][name] == plain[0][name]).all(), name
