"""GPU: tarok_playout_exchange_net (the talon exchange valued by playouts that a policy network plays) checked exactly —
integers against integers: net_seats = 0 against tarok_playout_exchange's bytes at samples = 1; exactly summable integer
weights against the model of tests/playout_front_net_model.py; random bf16 weights against a replay of every live item on
a twin env through the shipped greedy tarok_policy_step, result word by result word; a captured graph against the eager
launch after the weights changed in place; every TAROK_EINVAL; the learner and the evaluation built on the launch.  Every
case checks every row of all three outputs inside guard bands (tests/guarded.py), with the scratch between guards too, and
that the env's state is untouched.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_exchange_net.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T, U, item_arrays, nets, random_net  # noqa: F401  (T, nets: the module fixtures)

pytestmark = pytest.mark.gpu

SEED, OFFSET, EPISODE = 43, 2000, 5               # tests/test_gpu_playout_exchange.py's: the same games
LIVE = 0x8000800080008000
games_of = functools.partial(H.games_of, offset=OFFSET)
replay_on_a_twin = functools.partial(H.replay_on_a_twin, seed=SEED)
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE, defer_exchange=True)   # waiting for the exchange
bot_launch = H.launch_exchange_bot


def net_launch(env, kw, worlds, sets, net_seats, salt=0, seats=15, per_game=None, want=("sum", "choice", "discards"), scratch_out=None):
    """One launch into guarded outputs over a guarded scratch: (sum [n, 6 * sets, 4] i32, choice [n] i8, discards [n, 3] u8),
    None where not asked.  scratch_out: a list that receives the scratch's bytes after the launch."""
    return H.launch_exchange(env, "tarok_playout_exchange_net",
                             [int(worlds), int(sets), int(salt), int(seats), H.dev_u8(per_game), int(net_seats)] + list(kw), sets, want,
                             scratch=("tarok_playout_exchange_net_scratch", (int(worlds), int(sets)), env.n * 6 * sets * worlds * 48),
                             check_env_untouched=True, tag=(worlds, sets, net_seats, seats), scratch_out=scratch_out)


def check_model(env, W, kw, worlds, sets, net_seats, salt=0, seats=15, per_game=None, tag=None):
    import playout_front_net_model as FM
    want = FM.playout_exchange(games_of(env, per_game), SEED, salt, seats, worlds, sets, W, net_seats)
    got = net_launch(env, kw, worlds, sets, net_seats, salt, seats, per_game)
    for name, g, w in zip(("sums", "choices", "discards"), got, want):
        bad = np.nonzero((g != w).reshape(env.n, -1).any(axis=1))[0]
        assert bad.size == 0, (tag, name, "differ", bad[:8], g[bad[0]].tolist(), w[bad[0]].tolist())
    return got


@pytest.mark.parametrize("n,worlds,sets", [(5, 3, 2), (1, 1, 1)])
def test_no_net_seat_gives_the_bot_launch_bytes(T, nets, n, worlds, sets):
    """net_seats = 0: tarok_playout_exchange(worlds, 1, sets) to the byte, all three outputs.  n = 5, worlds = 3, sets = 2:
    180 item slots, one full tile of 128 and a partial one; n = 1: a single partial tile.  The five games are two Ena, a
    Tri, a Dve and a Klop (not waiting: -1 / 255); the seat set 5 leaves two declarers outside (the Bot's own exchange)."""
    from oracle import tarok_spec as S
    env = make_env(T, n, S.MIX_BOT)
    try:
        lanes = env.state()
        waiting = ((lanes[9] >> U(52)) & U(3)) == 1
        declarer = ((lanes[9] >> U(37)) & U(3)).astype(np.int64)
        if n == 5:
            assert waiting.sum() == 4 and sorted(declarer[waiting].tolist()) == [0, 1, 1, 2]
        per = np.array([15, 0, 2, 13, 15], np.uint8)[:n] | np.uint8(0x30)
        for salt, seats, per_game in ((0, 15, None), (9, 5, None), (9, 0, per), (9, 0, None)):
            want = bot_launch(env, worlds, 1, sets, salt, seats, per_game)
            got = net_launch(env, nets["R"][1], worlds, sets, 0, salt, seats, per_game)
            assert want[0].any() == (seats != 0 or per_game is not None)
            for w, g in zip(want, got):
                assert g.tobytes() == w.tobytes(), (salt, seats)
            assert (got[1][~waiting] == -1).all() and (got[2][~waiting] == 255).all() and (got[1][waiting] >= 0).all()
        for one in ("sum", "choice", "discards"):                        # one output at a time: the same bytes
            alone = dict(zip(("sum", "choice", "discards"), net_launch(env, nets["R"][1], worlds, sets, 0, 9, 5, want=(one,))))
            assert alone[one].tobytes() == dict(zip(("sum", "choice", "discards"), bot_launch(env, worlds, 1, sets, 9, 5)))[one].tobytes()
    finally:
        env.close()


@pytest.mark.parametrize("net_seats", [15, 1, 10])
@pytest.mark.parametrize("mix", ["tri", "dve", "ena", "solo_ena", "bot"])
def test_integer_weights_against_the_model(T, nets, mix, net_seats):
    """37 games, 2 worlds, 2 discard sets (up to 888 item slots: six full tiles and a partial one), weight set R (rounded
    H2, ties among the logits), on single-contract envs with 2, 3 and 6 groups and on the Bot's own mix."""
    from oracle import tarok_spec as S
    mixes = dict(tri=S.MIX_FIXED + S.TRI, dve=S.MIX_FIXED + S.DVE, ena=S.MIX_FIXED + S.ENA, solo_ena=S.MIX_FIXED + S.SOLO_ENA, bot=S.MIX_BOT)
    env = make_env(T, 37, mixes[mix])
    try:
        got_sum, got_ch, _ = check_model(env, *nets["R"], 2, 2, net_seats, salt=3, tag=(mix, net_seats))
        assert got_sum.any() and (got_ch > 0).any()
    finally:
        env.close()


def test_seat_sets_and_the_network_in_the_loop(T, nets):
    """The empty seat set (zero sums, the Bot's exchange everywhere), per-game sets (bits 4..7 ignored) against the model,
    and sums that differ between net_seats = 0 and 15 and between the two weight sets."""
    from oracle import tarok_spec as S
    env = make_env(T, 37, S.MIX_BOT)
    try:
        kw = nets["R"][1]
        s0, c0, d0 = net_launch(env, kw, 2, 2, 15, seats=0)
        bot = bot_launch(env, 2, 1, 2, seats=0)
        assert not s0.any() and c0.tobytes() == bot[1].tobytes() and d0.tobytes() == bot[2].tobytes()
        per = np.array([0, 1, 6, 15], np.uint8)[np.arange(37) % 4] | ((np.arange(37) % 3) << 4).astype(np.uint8)
        got_sum, _, _ = check_model(env, *nets["R"], 2, 2, 5, salt=11, seats=9, per_game=per, tag="per-game sets")
        declarer = ((env.state()[9] >> U(37)) & U(3)).astype(np.int64)
        out = ((per.astype(np.int64) >> declarer) & 1) == 0
        assert out.sum() > 4 and got_sum[~out].any() and not got_sum[out].any()
        sb, _, _ = net_launch(env, kw, 2, 2, 0)
        sr, _, _ = net_launch(env, kw, 2, 2, 15)
        sp, _, _ = check_model(env, *nets["P"], 2, 2, 15, tag="set P")
        assert (sb != sr).any() and (sr != sp).any()
    finally:
        env.close()


def test_random_weights_against_a_twin_replay(T):
    """Random bf16 weights, net_seats = 15, 6 games of the Bot's mix, 2 worlds, 2 discard sets.  Every live item — the
    model's world after the candidate's exchange — is played on a twin env by the greedy tarok_policy_step and must score
    what the item's result word says; the item's key in the scratch is the model's; every other slot's word is 0."""
    import playout_front_net_model as FM
    from oracle import tarok_spec as S
    kw = random_net(T, 17)
    n, worlds, sets = 6, 2, 2
    env = make_env(T, n, S.MIX_BOT)
    try:
        scr = []
        got_sum, _, _ = net_launch(env, kw, worlds, sets, 15, salt=1, scratch_out=scr)
        where, hs, keys = [], [], []
        for g, (lanes, ep, gidx, _) in enumerate(games_of(env)):
            for r, w, h, key in FM.exchange_items(lanes, ep, SEED, 1, gidx, 15, worlds, sets):
                where.append((g * 6 * sets + r) * worlds + w); hs.append(h); keys.append(key)
    finally:
        env.close()
    assert len(hs) >= 24
    items = n * 6 * sets * worlds
    ikey, ires, words = item_arrays(scr[0], items)
    final = replay_on_a_twin(T, kw, hs)
    where = np.array(where)
    assert (ikey[where] == np.array(keys, np.uint64)).all(), "an item's key"
    assert (ires[where] == final).all(), np.nonzero((ires[where] != final).any(axis=1))[0]
    rest = np.setdiff1d(np.arange(items), where)
    assert rest.size and (words[rest] == 0).all() and (words != U(LIVE)).all()
    want = np.zeros((n * 6 * sets, 4), np.int64)
    np.add.at(want, where // worlds, final)
    assert (got_sum.reshape(-1, 4) == want).all()


def test_a_captured_launch_replays_with_the_weights_in_place(T):
    """A launch captured into a graph, then the weights changed in place: the replay gives the eager launch's bytes for
    the NEW weights."""
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 37, S.MIX_BOT)
    try:
        kw, other = random_net(T, 1), random_net(T, 2)
        env.playout_exchange_net_scratch(2, 2)                    # allocated before the capture
        outs = [torch.zeros((37, 12, 4), dtype=torch.int32, device="cuda"), torch.zeros(37, dtype=torch.int8, device="cuda"),
                torch.zeros((37, 3), dtype=torch.uint8, device="cuda")]
        old = [t.cpu() for t in env.playout_exchange_net(kw, 2, 2, salt=4)]
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_exchange_net(kw, 2, 2, salt=4, sum_out=outs[0], choice_out=outs[1], discards_out=outs[2])
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.cpu(), x) for o, x in zip(outs, old))
        for t, o in zip(kw, other):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        new = [t.cpu() for t in env.playout_exchange_net(other, 2, 2, salt=4)]
        assert all(torch.equal(o.cpu(), x) for o, x in zip(outs, new))
        assert not torch.equal(new[0], old[0])
    finally:
        env.close()


def test_python_surface_and_arguments(T, nets):
    """playout_exchange_net equals the direct C call; the scratch is cached per shape; bad arguments are TAROK_EINVAL."""
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 5, S.MIX_BOT)
    try:
        kw = nets["R"][1]
        want = net_launch(env, kw, 3, 2, 10, salt=2)
        got = env.playout_exchange_net(kw, 3, 2, net_seats=10, salt=2)
        assert all((g.cpu().numpy() == w).all() for g, w in zip(got, want))
        assert tuple(env.playout_exchange_net(kw, 3, salt=2)[0].shape) == (5, 24, 4)                  # discard_sets defaults to 4
        assert env.playout_exchange_net_scratch(3, 2) is env.playout_exchange_net_scratch(3, 2)
        assert env.playout_exchange_net_scratch(2, 2) is not env.playout_exchange_net_scratch(3, 2)
        assert env.playout_exchange_net_scratch(3, 1) is not env.playout_exchange_net_scratch(3, 2)
        scr = env.playout_exchange_net_scratch(3, 2)
        p = env._p
        ok = dict(worlds=3, sets=2, seats=15, net=15, w=[p(t) for t in kw], scr=p(scr), size=scr.numel(), out=p(got[0]))

        def rc(**ch):
            a = dict(ok, **ch)
            return env.L.tarok_playout_exchange_net(env._h, a["worlds"], a["sets"], 0, a["seats"], None, a["net"], *a["w"], a["scr"],
                                                    a["size"], a["out"], None, None, env._stream())
        assert rc() == 0
        torch.cuda.synchronize()
        bad = [dict(worlds=0), dict(worlds=65), dict(sets=0), dict(sets=9), dict(seats=16), dict(seats=-1), dict(net=16), dict(net=-1),
               dict(scr=None), dict(size=scr.numel() - 1), dict(scr=scr.data_ptr() + 8), dict(out=None)]
        bad += [dict(w=ok["w"][:i] + [None] + ok["w"][i + 1:]) for i in range(6)]
        for ch in bad:
            assert rc(**ch) == -1, ch
        size = env.L.tarok_playout_exchange_net_scratch
        assert [size(env._h, 0, 2), size(env._h, 65, 2), size(env._h, 2, 0), size(env._h, 2, 9), size(None, 1, 1)] == [-1] * 5
        assert env.L.tarok_playout_exchange_net(None, 3, 2, 0, 15, None, 15, *ok["w"], ok["scr"], ok["size"], ok["out"], None, None, None) == -1
        with pytest.raises(ValueError):
            env.playout_exchange_net(kw, 2, 2, net_seats=16)
        with pytest.raises(ValueError):
            env.playout_exchange_net(kw, 0, 2)
        with pytest.raises(ValueError):
            env.playout_exchange_net(kw, 2, 9)
    finally:
        env.close()


def test_the_exchange_learner_with_a_net_teacher(T):
    """ExchangeLearner(net=...) at n = 64: one collect() gives the rows of the eager net launch on a twin env at playouts =
    worlds — not the Bot launch's —, and a step runs."""
    import torch
    from oracle import tarok_spec as S
    from tarok_amd.exchange import ExchangeLearner
    net = random_net(T, 3)
    env, twin = T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT), T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT)
    try:
        learner = ExchangeLearner(env, worlds=2, discard_sets=2, seed=5, net=net, net_seats=15)
        fw, sums, cands, playouts = learner.collect(3)
        assert playouts == 2 and tuple(sums.shape) == (64, 12, 4)
        twin.reset(episode=3, defer_exchange=True)
        want, _, _ = twin.playout_exchange_net(net, 2, 2, net_seats=15, salt=5)
        assert torch.equal(sums, want) and sums.any()
        assert not torch.equal(sums, twin.playout_exchange(2, 1, 2, salt=5)[0])
        assert torch.equal(cands, twin.exchange_candidates(2, salt=5))
        loss = learner.step(fw, sums, cands, playouts)
        assert np.isfinite(loss) and np.isfinite(learner.iterate())
    finally:
        env.close()
        twin.close()


def test_evaluate_exchange_net_vs_bot(T):
    """evaluate_exchange_net_vs_bot(net, ..., net_seats="own", cards=...) on 32 games x 1 episode: on every pass the front end's
    sums, choice and discards are those of the eager launch on a twin env in the inspected start state, and pass 0 — the
    empty set — is the Bot-everywhere pass of the plain call."""
    import torch
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    net = random_net(T, 4)
    seen, plain = [], []
    got = EV.evaluate_exchange_net_vs_bot(net, 2, 2, 32, 1, seed=5, salt=3, inspect=seen, net_seats="own", cards=net)
    EV.evaluate_exchange_vs_bot(2, 1, 2, 32, 1, seed=5, salt=3, inspect=plain)
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS) and got["deals"] == 32
    twin = T.TarokVecEnv(32, seed=5, mix=S.MIX_BOT)
    try:
        differs = 0
        for rec in seen:
            twin.reset(episode=0, defer_exchange=True)
            assert (twin.state() == rec["start"]).all()
            want = twin.playout_exchange_net(net, 2, 2, net_seats=rec["seats"], salt=3, seats=rec["seats"])
            for name, w in zip(("sums", "choice", "discards"), want):
                assert (rec[name] == w.cpu().numpy()).all(), (rec["seats"], name)
            differs += int((rec["choice"] != seen[0]["choice"]).sum())
        assert differs > 0, "the playout player exchanges otherwise than the Bot somewhere"
    finally:
        twin.close()
    for name in ("start", "choice", "discards", "scores"):
        assert (seen[0][name] == plain[0][name]).all(), name
    bots = []                                                        # the same front end, the Bot playing every card
    EV.evaluate_exchange_net_vs_bot(net, 2, 2, 32, 1, seed=5, salt=3, inspect=bots, net_seats="own")
    assert (bots[0]["scores"] == plain[0]["scores"]).all()
    assert all((bots[p]["choice"] == seen[p]["choice"]).all() for p in range(5))
    assert any((bots[p]["actions"] != seen[p]["actions"]).any() for p in range(1, 5)), "the network plays the pass's seats"
