"""GPU: tarok_playout_cards_net_value (net playouts stopped at the viewer's depth-th decision, the value head's estimate
in the viewer's column) checked exactly — integers against integers: depth 12 against the bytes of the three existing
launches; exactly summable integer weights at depths 1..3 against the model of tests/playout_net_value_model.py, over the
plan of tests/playout_net_value_cases.py; random weights at net_seats = 0 against tarok_policy_mlp's value_out on the
model's stop positions; a captured graph after the weights changed in place; every TAROK_EINVAL; the teacher inside the
captured rollout and the evaluation.  Every launch writes into guard bands (tests/guarded.py) over a guarded scratch and
leaves the env, its counters and its history as they were.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_net_value.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
import playout_net_value_cases as PC
import playout_net_value_model as VM
from gpu_harness import T, U, host_words, model_words, random_net, words_of  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = 41, 1000, 3               # tests/test_gpu_playout_det.py's: the same games
SEEN = dict(tags=set(), moved=0, cases=set())
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)
games_of = functools.partial(H.games_of, offset=OFFSET)


@pytest.fixture(scope="module")
def nets(T):
    """R, P and V of tests/playout_net_value_cases.weight_sets as (float64 set, kernel set)."""
    import policy_exact_ref as PE
    return {k: (W, PE.kernel_weights(T, W)) for k, W in PC.weight_sets().items()}


def value_launch(kind, env, kw, worlds, net_seats, depth, value_scale, words=None, salt=0, seats=15, per_game=None, want=("sum", "action")):
    """One launch of the kind into guarded outputs over a guarded scratch: (sum [n,12,4] i32 or None, action [n] u8 or None)."""
    return H.launch_net(kind, env, kw, worlds, net_seats, words, salt, seats, per_game, want, value=(depth, value_scale))


def existing_launch(kind, env, kw, worlds, net_seats, salt, seats, per_game):
    return H.launch_net(kind, env, kw, worlds, net_seats, None, salt, seats, per_game)


@pytest.mark.parametrize("kind", VM.KINDS)
@pytest.mark.parametrize("n,worlds,cards", [(5, 3, 0), (5, 3, 9), (5, 3, 24), (5, 3, 44), (1, 1, 0), (1, 1, 9), (1, 1, 24), (1, 1, 44)])
def test_depth_12_gives_the_existing_launch_bytes(T, nets, kind, n, worlds, cards):
    """depth = 12 never stops an item: the bytes of tarok_playout_cards_net / _net_voids / _net_hidden, with the integer
    set R and with random weights, at net_seats 15 and 0, for one seat set and for per-game sets, at any value_scale."""
    from oracle import tarok_spec as S
    env = make_env(T, n, S.MIX_ALL, cards, history=True)
    try:
        per = (np.array([15, 1, 6, 15, 9], np.uint8) | np.array([0, 16, 32, 64, 128], np.uint8))[:n]
        some = 0
        for kw, scale in ((nets["R"][1], 1.0), (random_net(T, 3 + cards), 1e9)):
            for net_seats in (15, 0):
                for salt, seats, per_game in ((3, 15, None), (9, 0, per)):
                    want_sum, want_act = existing_launch(kind, env, kw, worlds, net_seats, salt, seats, per_game)
                    got_sum, got_act = value_launch(kind, env, kw, worlds, net_seats, 12, scale, None, salt, seats, per_game)
                    some += int(want_sum.any())
                    assert got_sum.tobytes() == want_sum.tobytes() and got_act.tobytes() == want_act.tobytes(), (net_seats, salt, seats)
        assert some >= 4
    finally:
        env.close()


@pytest.mark.parametrize("kind,at", PC.CASES)
def test_integer_weights_against_the_model(T, nets, kind, at):
    """Depths 1, 2 and 3 with the exactly summable sets R, P and V, net_seats 15, 0 and a set without the viewer, at
    value_scale 1, 0.5 and 1e9: sum_out and action_out EQUAL the model, on the env's own words."""
    mix, cards = PC.POSITIONS[kind][at]
    for n, worlds, depth, name, choice in PC.plan(kind, at):
        W, kw = nets[name]
        env = make_env(T, n, mix, cards, history=True)
        try:
            games, objs = games_of(env), None
            words = None
            if kind != "det":
                words = model_words(kind, env)
                assert (host_words(kind, env) == words).all(), "the env's words are not the model's"
                words = [int(x) for x in words]
            from oracle import oracle as O
            net_seats = PC.net_seats_of(choice, [O.Game.from_lanes(games[0][0])])
            _, _, info = VM.playout_cards(kind, games, SEED, PC.SALT, 15, worlds, W, net_seats, depth, 1.0, words)
            _, full, _ = VM.playout_cards(kind, games, SEED, PC.SALT, 15, worlds, W, net_seats, 12, 1.0, words) if n > 1 else (0, None, 0)
            import playout_model as PM
            for scale in PC.SCALES:
                want_sum = PC.at_scale(n, worlds, info, scale)
                want_act = np.array([PM.card_of(lanes, SEED, gidx, ep, 15, want_sum[g]) for g, (lanes, ep, gidx, _) in enumerate(games)], np.uint8)
                got_sum, got_act = value_launch(kind, env, kw, worlds, net_seats, depth, scale, None, PC.SALT)
                tag = (kind, cards, n, depth, name, net_seats, scale)
                H.assert_cards_equal(got_sum, want_sum, got_act, want_act, tag)
                SEEN["tags"] |= VM.seen([(w, dict(d, V=VM.points(d["v"], scale) if d["stopped"] else None)) for w, d in info], scale)
                if full is not None and scale == 1.0:
                    SEEN["moved"] += int((got_act != full).sum())
        finally:
            env.close()
    SEEN["cases"].add((kind, at))


def test_the_comparison_was_not_vacuous():
    """Over the cases above (when all of them ran): stopped and finished items in one launch; positive, negative and
    differing V; a tie that half-even and half-away round differently; a clamped value; a game whose chosen card differs
    from the depth-12 card."""
    if SEEN["cases"] != set(PC.CASES):
        return                                        # (a partial run: the guard is the whole module's)
    assert SEEN["tags"] >= {"mixed", "signs", "tie", "clamped"}, SEEN["tags"]
    assert SEEN["moved"] >= 1


@pytest.mark.parametrize("kind,cards,depth", [("det", 0, 1), ("det", 9, 2), ("voids", 24, 1), ("hidden", 9, 2), ("det", 40, 1)])
def test_random_weights_give_policy_mlps_value_bits(T, kind, cards, depth):
    """Random bf16 weights, net_seats = 0, W = 1: the Bot plays, so the model's stop positions are exact for any weights.
    They go into a twin env through the canonical lanes; tarok_policy_mlp's value_out there, formed into V on the host
    in float32, plus the true scores of the finished items, IS the launch's sum — the viewer's column."""
    import torch
    from oracle import tarok_spec as S
    kw = random_net(T, 11 + cards)
    W0 = PC.weight_sets()["P"]                        # (any weights: with net_seats = 0 the model's positions do not read them)
    n, scale = 5, 70.0
    env = make_env(T, n, S.MIX_ALL, cards, history=True)
    try:
        games = games_of(env)
        words = None if kind == "det" else [int(x) for x in model_words(kind, env)]
        got_sum, _ = value_launch(kind, env, kw, 1, 0, depth, scale, None, PC.SALT)
    finally:
        env.close()
    _, _, info = VM.playout_cards(kind, games, SEED, PC.SALT, 15, 1, W0, 0, depth, scale, words)
    stops = [(where, d) for where, d in info if d["stopped"]]
    assert len(stops) >= 4
    twin = T.TarokVecEnv(len(stops), seed=SEED, mix=S.MIX_ALL)
    try:
        twin.reset()
        twin.set_state(np.stack([d["at"].lanes() for _, d in stops], axis=1))
        value = twin.policy_mlp(kw, twin.legal_actions().words)[2].cpu().numpy()
    finally:
        twin.close()
    want = np.zeros((n, 12, 4), np.int64)
    for (g, j, w), d in info:
        if not d["stopped"]:
            want[g, j] += d["scores"]
    Vs = set()
    for ((g, j, w), d), v in zip(stops, value):
        V = VM.points(v, scale)
        Vs.add(V)
        want[g, j, d["viewer"]] += V
    assert len(Vs) >= 3
    viewer = np.array([next((d["viewer"] for (g, _, _), d in info if g == k), 0) for k in range(n)])
    col = lambda a: np.take_along_axis(np.asarray(a, np.int64), viewer[:, None, None].repeat(12, 1), 2)
    assert (col(got_sum) == col(want)).all(), (col(got_sum) - col(want)).nonzero()
    assert (got_sum == want).all()                    # (and the other three columns: true scores and zeros)


@pytest.mark.parametrize("kind", VM.KINDS)
def test_a_captured_launch_replays_with_the_weights_in_place(T, nets, kind):
    """A launch captured into a graph, then the weights overwritten in place: the replay equals the eager launch with the
    new weights."""
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 5, S.MIX_ALL, 9, history=True)
    try:
        kw, other = [t.clone() for t in nets["V"][1]], nets["P"][1]
        arg = {} if kind == "det" else {kind: words_of(kind, env).clone()}
        env.playout_net_scratch(3)                                # allocated before the capture
        s_out = torch.zeros((5, 12, 4), dtype=torch.int32, device="cuda")
        a_out = torch.zeros(5, dtype=torch.uint8, device="cuda")
        eager = lambda w: [t.cpu() for t in env.playout_cards_net_value(w, 3, 2, 0.5, salt=3, **arg)]
        first = eager(kw)
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_cards_net_value(kw, 3, 2, 0.5, salt=3, sum_out=s_out, action_out=a_out, **arg)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_out.cpu(), first[0]) and torch.equal(a_out.cpu(), first[1])
        for t, o in zip(kw, other):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        second = eager(other)
        assert torch.equal(s_out.cpu(), second[0]) and torch.equal(a_out.cpu(), second[1])
        assert not torch.equal(second[0], first[0])
    finally:
        env.close()


def test_python_surface_and_arguments(T, nets):
    """playout_cards_net_value equals the direct C call for the three kinds; one output at a time gives the same bytes;
    every TAROK_EINVAL is returned."""
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 5, S.MIX_ALL, 24, history=True)
    try:
        kw = nets["V"][1]
        for num, kind in enumerate(VM.KINDS):
            want_sum, want_act = value_launch(kind, env, kw, 3, 10, 2, 0.5, salt=2)
            s_only, _ = value_launch(kind, env, kw, 3, 10, 2, 0.5, salt=2, want=("sum",))
            _, a_only = value_launch(kind, env, kw, 3, 10, 2, 0.5, salt=2, want=("action",))
            assert (s_only == want_sum).all() and (a_only == want_act).all()
            arg = {} if kind == "det" else {kind: True}
            sums, acts = env.playout_cards_net_value(kw, 3, 2, 0.5, net_seats=10, salt=2, **arg)
            assert (sums.cpu().numpy() == want_sum).all() and (acts.cpu().numpy() == want_act).all(), kind
            old = env.playout_cards_net(kw, 3, net_seats=10, salt=2, **arg)
            off = env.playout_cards_net_value(kw, 3, None, net_seats=10, salt=2, **arg)
            assert torch.equal(old[0], off[0]) and torch.equal(old[1], off[1])
            given = None if kind == "det" else words_of(kind, env)
            scr = env.playout_net_scratch(3)
            p = env._p
            ok = dict(env=env._h, worlds=3, seats=15, kind=num, words=p(given), net=15, depth=1, scale=70.0, w=[p(t) for t in kw], scr=p(scr),
                      size=scr.numel(), out=p(sums))

            def rc(**ch):
                a = dict(ok, **ch)
                return env.L.tarok_playout_cards_net_value(a["env"], a["worlds"], 0, a["seats"], None, a["kind"], a["words"], a["net"], a["depth"],
                                                           a["scale"], *a["w"], a["scr"], a["size"], a["out"], None, env._stream())
            assert rc() == 0
            torch.cuda.synchronize()
            bad = [dict(env=None), dict(worlds=0), dict(worlds=65), dict(seats=16), dict(seats=-1), dict(net=16), dict(net=-1), dict(scr=None),
                   dict(size=scr.numel() - 1), dict(scr=scr.data_ptr() + 8), dict(out=None), dict(kind=3), dict(kind=-1),
                   dict(words=p(scr) if kind == "det" else None), dict(depth=0), dict(depth=13), dict(depth=-1), dict(scale=0.0),
                   dict(scale=-70.0), dict(scale=float("inf")), dict(scale=float("nan"))]
            bad += [dict(w=ok["w"][:i] + [None] + ok["w"][i + 1:]) for i in range(6)]
            for ch in bad:
                assert rc(**ch) == -1, (kind, ch)
        with pytest.raises(ValueError):
            env.playout_cards_net_value(kw, 3, 0)
        with pytest.raises(ValueError):
            env.playout_cards_net_value(kw, 3, 1, voids=True, hidden=True)
    finally:
        env.close()


def test_a_value_teacher_in_the_captured_rollout(T):
    """SelfPlay(teacher=dict(net=True, worlds=2, depth=1)) on 256 games, T = 3: the captured graph records the bytes of
    the eager rollout; the teacher's rows are the targets of a direct playout_cards_net_value at (2, depth 1,
    1 / reward_scale) with the learner's rollout weights on a twin env, and differ from the full-depth teacher's; then one
    iterate() runs through the fused learner."""
    import torch
    from tarok_amd import selfplay as SP
    n, steps, tc = 256, 3, dict(worlds=2, net=True, depth=1, tau=8, salt=11)

    def make(use_graph):
        env = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_BOT)
        return env, SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True, teacher=tc, distill_coef=0.5, use_graph=use_graph)
    ea, a = make(True)
    eb, b = make(False)
    with torch.no_grad():
        b._alloc(steps)
        b._collect_body(2)                               # (SelfPlay.collect warms up with two lock-steps before it captures)
    bufa, bufb = a.collect(steps), b.collect(steps)
    torch.cuda.synchronize()
    for k in ("obs", "words", "act", "logp", "val", "done", "reward"):
        assert torch.equal(bufa[k], bufb[k]), k
    assert torch.equal(bufa["teach"].view(torch.int16), bufb["teach"].view(torch.int16))
    assert bufa["teach"].view(torch.int16).ne(0).any(-1).all()
    ec, c = make(False)
    buf = c.collect(steps)
    twin = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_BOT)
    twin.reset()
    torch.cuda.synchronize()
    differ = 0
    for t in range(steps):
        sums, _ = twin.playout_cards_net_value(c._w, 2, 1, 1.0 / c.reward_scale, salt=11)
        assert torch.equal(c._teach_sums, sums) or t < steps - 1      # (the recorded sums of the last lock-step are still in place)
        want = twin.playout_targets(sums, buf["words"][t], 2, 8.0)
        assert torch.equal(buf["teach"][t].view(torch.int16), want.view(torch.int16)), t
        full = twin.playout_targets(twin.playout_cards_net(c._w, 2, salt=11)[0], buf["words"][t], 2, 8.0)
        differ += int(buf["teach"][t].view(torch.int16).ne(full.view(torch.int16)).any(-1).sum())
        twin.step(buf["act"][t], auto_reset=True)
    assert differ > 0
    stats = a.iterate(T=steps, epochs=1, minibatches=1)
    assert np.isfinite(stats["loss"]) and np.isfinite(stats["distill_ce"]) and 0.0 <= stats["teacher_frac"] <= 1.0 + 1e-6
    for e in (ea, eb, ec, twin):
        e.close()


def replay_pass(W, seed, mix, gidx, episode, seats, worlds, depth, value_scale):
    """One game of one pass of evaluate_playout_vs_bot(net=, net_depth=) on the oracle, as tests/playout_det_model.replay_pass:
    the model's card at every move (the depth-limited player on `seats`, net_seats = 15, the Bot elsewhere)."""
    from oracle import oracle as O
    g = O.Game.synth(seed, gidx, episode, mix)
    actions = [255] * 48
    for t in range(48):
        if g.done:
            break
        _, cards, _ = VM.playout_cards("det", [(g.lanes(), episode, gidx, None)], seed, 0, seats, worlds, W, 15, depth, value_scale)
        actions[t] = int(cards[0])
        assert g.step(int(cards[0])) >= 0
    assert g.done
    return actions, g.scores


def test_evaluate_at_depth_1_replays_the_models_cards(T, nets):
    """evaluate_playout_vs_bot(None, worlds=2, net=V, net_depth=1, net_value_scale=0.5) on 3 deals: every card and every
    final score of the five passes are the model's replay, and the statistic is duplicate_advantage of those scores."""
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    W, kw = nets["V"]
    seen, n = [], 3
    got = EV.evaluate_playout_vs_bot(None, n, 1, seed=5, worlds=2, net=kw, net_depth=1, net_value_scale=0.5, inspect=seen)
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS)
    scores = np.zeros((5, n, 4), np.int32)
    for p, rec in enumerate(seen):
        for i in range(n):
            actions, sc = replay_pass(W, 5, S.MIX_BOT, i, 0, rec["seats"], 2, 1, 0.5)
            assert rec["actions"][:, i].tolist() == actions, (p, i)
            assert rec["scores"][i].tolist() == sc, (p, i)
            scores[p, i] = sc
    want = EV.duplicate_advantage(scores)
    assert got == want or (np.isnan(got["stderr"]) and np.isnan(want["stderr"]))
