"""GPU: tarok_playout_cards_net_versus and tarok_playout_cards_net_versus_halving (two networks seated relative to each item's
viewer) checked exactly — integers against integers: the byte equalities with the existing launches for the three world kinds
at depth 0, 1, 3 and 12; the mixed roles (1, 14), (14, 1) and (3, 8) with A != B against the model of
tests/playout_net_versus_model.py over the plan of tests/playout_net_versus_cases.py; the halving form against the dense
one; determinism and batch independence; a captured graph after B changed in place; the Python surface; the evaluation.
Every launch writes into guard bands (tests/guarded.py) over a guarded scratch and leaves the env, its counters and its
history as they were.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_net_versus.py -m gpu -q
"""
import ctypes
import functools

import numpy as np
import pytest

import gpu_harness as H
import playout_model as PM
import playout_net_value_cases as PC
import playout_net_value_model as VM
import playout_net_versus_cases as XC
import playout_net_versus_model as XM
from gpu_harness import T, host_words, model_words, random_net, words_of  # noqa: F401  (T: the module fixture)
from guarded import Guarded

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = XC.SEED, XC.OFFSET, XC.EPISODE
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)
games_of = functools.partial(H.games_of, offset=OFFSET)
SEEN = dict(both=0, stopped=0, cases=set())


@pytest.fixture(scope="module")
def nets(T):
    """A and B of tests/playout_net_versus_cases.weight_sets as (float64 set, kernel set)."""
    import policy_exact_ref as PE
    return {k: (W, PE.kernel_weights(T, W)) for k, W in XC.weight_sets().items()}


def versus_launch(kind, env, ka, kb, worlds, own, opp, depth, scale=70.0, salt=0, seats=15, per_game=None, want=("sum", "action")):
    """One tarok_playout_cards_net_versus into guarded outputs over a guarded scratch, the env compared before and after."""
    w = None if kind == "det" else words_of(kind, env)
    args = [int(worlds), int(salt), int(seats), H.dev_u8(per_game), VM.KINDS.index(kind), w, int(own), int(opp), int(depth), float(scale)]
    return H.launch_cards(env, "tarok_playout_cards_net_versus", args + list(ka) + list(kb if kb is not None else [None] * 6), want,
                          scratch=("tarok_playout_net_scratch", (int(worlds),), env.n * 12 * worlds * 48), check_env_untouched=True,
                          tag=(kind, worlds, own, opp, depth, seats))


def halving_size(n, schedule):
    bound = max(n * a * w for a, w in zip((12, 6, 3, 2), schedule))
    return (48 * bound + 252 * n + 4 * ((n + 255) // 256) + 4 + 15) // 16 * 16


def halving_launch(entry, kind, env, schedule, mid, tail, salt=0, seats=15):
    """One launch of a net halving entry — mid: what it takes between seats_per_game and (depth, value_scale); tail: those two
    — into guarded (sum, count, action) over a guarded scratch, the env compared before and after."""
    n = env.n
    arr = (ctypes.c_int * len(schedule))(*schedule)
    outs = [Guarded("sum_out", 1, n, np.int32, inner=(12, 4), device="cuda"), Guarded("count_out", 1, n, np.int32, inner=(12,), device="cuda"),
            Guarded("action_out", 1, n, np.uint8, device="cuda")]
    w = None if kind == "det" else words_of(kind, env)
    H._launch(env, entry, [VM.KINDS.index(kind), w, len(schedule), arr, int(salt), int(seats), None] + list(mid) + list(tail), outs,
              ("tarok_playout_net_halving_scratch_bytes", (len(schedule), arr), halving_size(n, schedule)), True, (entry, kind, schedule))
    return H.read_words(outs[0]), H.read_words(outs[1]), H.read_bytes(outs[2])


def versus_halving(kind, env, ka, kb, schedule, own, opp, depth, scale=70.0, salt=0, seats=15):
    return halving_launch("tarok_playout_cards_net_versus_halving", kind, env, schedule,
                          [int(own), int(opp)] + list(ka) + list(kb if kb is not None else [None] * 6), [int(depth), float(scale)], salt, seats)


def existing(kind, env, kw, worlds, net_seats, depth, scale, salt=0, seats=15, per_game=None):
    """The existing launch of the kind at the depth: depth 0 the plain one, else tarok_playout_cards_net_value."""
    return H.launch_net(kind, env, kw, worlds, net_seats, None, salt, seats, per_game, value=(depth, scale) if depth else None)


def bot_launch(kind, env, worlds, salt):
    if kind == "det":
        return H.launch_det(env, worlds, 1, salt)
    return H.launch_worlds(kind, env, worlds, 1, None, salt)


def same(got, want, tag):
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), tag


@pytest.mark.parametrize("kind", VM.KINDS)
@pytest.mark.parametrize("n,worlds,cards", [(5, 3, 0), (5, 3, 9), (5, 3, 24), (5, 3, 40), (5, 3, 44), (1, 1, 9)])
def test_the_byte_equalities_with_the_existing_launches(T, kind, n, worlds, cards):
    """At depth 0, 1, 3 and 12, with random weights: (15, 0) with any B is net_seats = 15 on A; (0, 15) is net_seats = 15 on B;
    (5, 10) with A and B equal copies in different tensors is net_seats = 15; (0, 0) is the Bot-played launch at samples = 1
    (where nothing stops: at depth > 0 the stop reads A's value head); for each v, seats = 1 << v with own_rel = an absolute
    set m rotated by v is the existing launch at seats = 1 << v, net_seats = m — compared over the union of the four."""
    from oracle import tarok_spec as S
    env = make_env(T, n, S.MIX_ALL, cards, history=True)
    try:
        ka, kb = random_net(T, 21 + cards), random_net(T, 22 + cards)
        copy = [t.clone() for t in ka]
        some = 0
        for depth in XC.BYTE_DEPTHS:
            scale, salt = (70.0, 3) if depth != 3 else (1e9, 9)
            on_a = existing(kind, env, ka, worlds, 15, depth, scale, salt)
            on_b = existing(kind, env, kb, worlds, 15, depth, scale, salt)
            some += int(on_a[0].any()) + int((on_a[0] != on_b[0]).any())
            same(versus_launch(kind, env, ka, kb, worlds, 15, 0, depth, scale, salt), on_a, (depth, "15, 0"))
            same(versus_launch(kind, env, ka, None, worlds, 15, 0, depth, scale, salt), on_a, (depth, "15, 0, no B"))
            same(versus_launch(kind, env, ka, kb, worlds, 0, 15, depth, scale, salt), on_b, (depth, "0, 15"))
            same(versus_launch(kind, env, ka, copy, worlds, 5, 10, depth, scale, salt), on_a, (depth, "5, 10"))
            if depth in (0, 12):
                same(versus_launch(kind, env, ka, kb, worlds, 0, 0, depth, scale, salt), bot_launch(kind, env, worlds, salt), (depth, "0, 0"))
            m = (6, 9, 1, 13)[XC.BYTE_DEPTHS.index(depth)]
            for v in range(4):
                same(versus_launch(kind, env, ka, kb, worlds, XC.rotate(m, v), 0, depth, scale, salt, seats=1 << v),
                     existing(kind, env, ka, worlds, m, depth, scale, salt, seats=1 << v), (depth, "rotated", m, v))
        assert some >= 2
    finally:
        env.close()


@pytest.mark.parametrize("kind,at", XC.CASES)
def test_mixed_roles_against_the_model(T, nets, kind, at):
    """(1, 14), (14, 1) and (3, 8) with the exactly summable sets A != B at depth 0, 1 and 3 and value_scale 1, 0.5 and 1e9, at
    (5 games, 3 worlds) and — one role and depth per case — at (1, 1): sum_out and action_out EQUAL the model, on the env's
    own words.  (1, 14) takes the viewer's stop value from A, (14, 1) from B."""
    mix, cards = XC.POSITIONS[kind][at]
    (WA, ka), (WB, kb) = nets["A"], nets["B"]
    k = VM.KINDS.index(kind) + at
    runs = [(5, 3, own, opp, depth) for own, opp in XC.MIXED for depth in XC.DEPTHS] + [(1, 1) + XC.MIXED[k % 3] + (XC.DEPTHS[(k // 3) % 3],)]
    envs = {}
    try:
        for n, worlds, own, opp, depth in runs:
            if n not in envs:
                env = make_env(T, n, mix, cards, history=True)
                words = None
                if kind != "det":
                    words = model_words(kind, env)
                    assert (host_words(kind, env) == words).all(), "the env's words are not the model's"
                    words = [int(x) for x in words]
                envs[n] = (env, games_of(env), words)
            env, games, words = envs[n]
            _, _, info = XM.playout_cards(kind, games, SEED, XC.SALT, 15, worlds, WA, WB, own, opp, depth, 1.0, words)
            SEEN["both"] += sum(d["both"] for _, d in info)
            SEEN["stopped"] += sum(d["stopped"] for _, d in info)
            for scale in (XC.SCALES if depth else XC.SCALES[:1]):
                want_sum = PC.at_scale(n, worlds, info, scale)
                want_act = np.array([PM.card_of(lanes, SEED, gidx, ep, 15, want_sum[g]) for g, (lanes, ep, gidx, _) in enumerate(games)], np.uint8)
                got_sum, got_act = versus_launch(kind, env, ka, kb, worlds, own, opp, depth, scale, XC.SALT)
                H.assert_cards_equal(got_sum, want_sum, got_act, want_act, (kind, cards, n, own, opp, depth, scale))
    finally:
        for env, _, _ in envs.values():
            env.close()
    SEEN["cases"].add((kind, at))


def test_the_comparison_was_not_vacuous():
    """Over the cases above (when all of them ran): items that met positions of both networks, and items that stopped."""
    if SEEN["cases"] != set(XC.CASES):
        return                                        # (a partial run: the guard is the whole module's)
    assert SEEN["both"] >= 100 and SEEN["stopped"] >= 100, SEEN


@pytest.mark.parametrize("kind,cards", [("det", 9), ("voids", 24), ("hidden", 0)])
def test_the_halving_form(T, nets, kind, cards):
    """A one-round schedule equals the dense versus launch; every row of a (2, 2) schedule equals the dense launch's row at the
    world count its count_out names; (15, 0) equals tarok_playout_cards_net_halving."""
    from oracle import tarok_spec as S
    ka, kb = nets["A"][1], nets["B"][1]
    env = make_env(T, 5, S.MIX_ALL, cards, history=True)
    try:
        for own, opp, depth in ((1, 14, 0), (14, 1, 3), (3, 8, 1)):
            dense = {e: versus_launch(kind, env, ka, kb, e, own, opp, depth, 0.5, 3) for e in (2, 3, 4)}
            s, c, a = versus_halving(kind, env, ka, kb, (3,), own, opp, depth, 0.5, 3)
            assert s.tobytes() == dense[3][0].tobytes() and a.tobytes() == dense[3][1].tobytes(), (own, opp, depth)
            assert set(np.unique(c)) <= {0, 3} and (c == 3).any()
            s, c, a = versus_halving(kind, env, ka, kb, (2, 2), own, opp, depth, 0.5, 3)
            assert set(np.unique(c)) <= {0, 2, 4} and (c == 4).any() and (c == 2).any()
            for g in range(5):
                for j in range(12):
                    want = dense[int(c[g, j])][0][g, j] if c[g, j] else np.zeros(4, np.int32)
                    assert (s[g, j] == want).all(), (own, opp, depth, g, j, int(c[g, j]))
            for d in (0, 3):
                old = halving_launch("tarok_playout_cards_net_halving", kind, env, (2, 2), [15] + list(ka), [d, 0.5], 3)
                new = versus_halving(kind, env, ka, kb, (2, 2), 15, 0, d, 0.5, 3)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(old, new)), (kind, d)
    finally:
        env.close()


def test_deterministic_and_batch_independent(T, nets):
    """Two launches give the same bytes; game 0's rows do not depend on the games beside it (5 games against 1) nor on the
    outputs asked for."""
    from oracle import tarok_spec as S
    ka, kb = nets["A"][1], nets["B"][1]
    five, one = make_env(T, 5, S.MIX_ALL, 9), make_env(T, 1, S.MIX_ALL, 9)
    try:
        for own, opp, depth in ((1, 14, 0), (3, 8, 3)):
            a = versus_launch("det", five, ka, kb, 3, own, opp, depth, 0.5, 3)
            b = versus_launch("det", five, ka, kb, 3, own, opp, depth, 0.5, 3)
            same(a, b, "twice")
            c = versus_launch("det", one, ka, kb, 3, own, opp, depth, 0.5, 3)
            assert (a[0][0] == c[0][0]).all() and a[1][0] == c[1][0]
            s_only, _ = versus_launch("det", five, ka, kb, 3, own, opp, depth, 0.5, 3, want=("sum",))
            _, a_only = versus_launch("det", five, ka, kb, 3, own, opp, depth, 0.5, 3, want=("action",))
            assert (s_only == a[0]).all() and (a_only == a[1]).all()
    finally:
        five.close(); one.close()


@pytest.mark.parametrize("halving", [None, (1, 2)])
def test_a_captured_launch_replays_with_b_overwritten_in_place(T, nets, halving):
    """A launch captured into a graph, then B overwritten in place: the replay equals the eager launch with the new B."""
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 5, S.MIX_ALL, 9)
    try:
        ka, kb, other = nets["A"][1], [t.clone() for t in nets["B"][1]], random_net(T, 77)
        more = dict(depth=2, value_scale=0.5, salt=3, halving=halving)
        if halving is None:
            env.playout_net_scratch(3)                               # allocated before the capture
        else:
            env.playout_net_halving_scratch(halving)
        outs = dict(sum_out=torch.zeros((5, 12, 4), dtype=torch.int32, device="cuda"), action_out=torch.zeros(5, dtype=torch.uint8, device="cuda"))
        if halving is not None:
            outs["count_out"] = torch.zeros((5, 12), dtype=torch.int32, device="cuda")
        eager = lambda b: [t.cpu() for t in env.playout_cards_net_versus(ka, b, 3, 14, 1, **more)]
        first = eager(kb)
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                captured = env.playout_cards_net_versus(ka, kb, 3, 14, 1, **more, **outs)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x.cpu(), y) for x, y in zip(captured, first))
        for t, o in zip(kb, other):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        second = eager(other)
        assert all(torch.equal(x.cpu(), y) for x, y in zip(captured, second))
        assert not torch.equal(second[0], first[0])
    finally:
        env.close()


def test_python_surface_and_arguments(T, nets):
    """playout_cards_net_versus equals the direct C calls for the three kinds, dense and halving; the refusals of a real env."""
    from oracle import tarok_spec as S
    env = make_env(T, 5, S.MIX_ALL, 24, history=True)
    try:
        ka, kb = nets["A"][1], nets["B"][1]
        for kind in VM.KINDS:
            arg = {} if kind == "det" else {kind: True}
            want = versus_launch(kind, env, ka, kb, 3, 3, 8, 2, 0.5, 2, seats=7)
            got = env.playout_cards_net_versus(ka, kb, 3, 3, 8, depth=2, value_scale=0.5, salt=2, seats=7, **arg)
            assert (got[0].cpu().numpy() == want[0]).all() and (got[1].cpu().numpy() == want[1]).all(), kind
            want = versus_launch(kind, env, ka, kb, 3, 1, 14, 0, 70.0, 2)
            got = env.playout_cards_net_versus(ka, kb, 3, salt=2, **arg)
            assert (got[0].cpu().numpy() == want[0]).all() and (got[1].cpu().numpy() == want[1]).all(), kind
            want = versus_halving(kind, env, ka, kb, (1, 2), 1, 14, 2, 0.5, 2)
            got = env.playout_cards_net_versus(ka, kb, None, depth=2, value_scale=0.5, salt=2, halving=(1, 2), **arg)
            assert len(got) == 3 and all((g.cpu().numpy() == w).all() for g, w in zip(got, want)), kind
        old = env.playout_cards_net(ka, 3, salt=2)
        new = env.playout_cards_net_versus(ka, None, 3, 15, 0, salt=2)
        assert all((x == y).all() for x, y in zip(old, new))
        for bad in (dict(own_rel=1, opp_rel=1), dict(own_rel=16), dict(depth=0), dict(voids=True, hidden=True)):
            with pytest.raises(ValueError):
                env.playout_cards_net_versus(ka, kb, 3, **bad)
        with pytest.raises(ValueError):
            env.playout_cards_net_versus(ka, None, 3)
    finally:
        env.close()


def replay_pass(WA, WB, seed, mix, n, episode, seats, worlds, depth, value_scale):
    """One pass of evaluate_playout_vs_bot(net=A, net_versus=(1, 14), net_opponent=B) on the oracle, all n games in lock-step: the
    model's card at every move (the versus player on `seats`, the Bot elsewhere).  Returns (actions [48, n], scores [n, 4])."""
    from oracle import oracle as O
    gs = [O.Game.synth(seed, i, episode, mix) for i in range(n)]
    actions = np.full((48, n), 255, np.uint8)
    for t in range(48):
        live = [i for i in range(n) if not gs[i].done]
        if not live:
            break
        _, cards, _ = XM.playout_cards("det", [(gs[i].lanes(), episode, i, None) for i in live], seed, 0, seats, worlds, WA, WB, 1, 14, depth,
                                       value_scale)
        for i, c in zip(live, cards):
            actions[t, i] = c
            assert gs[i].step(int(c)) >= 0
    assert all(g.done for g in gs)
    return actions, np.array([g.scores for g in gs], np.int32)


def test_evaluate_replays_the_models_cards(T, nets):
    """evaluate_playout_vs_bot(None, worlds=1, net=A, net_versus=(1, 14), net_opponent=B, net_depth=1, net_value_scale=0.5) on 64
    deals: every card and every final score of the five passes are the model's replay, and the statistic is
    duplicate_advantage of those scores."""
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    (WA, ka), (WB, kb) = nets["A"], nets["B"]
    seen, n = [], 64
    got = EV.evaluate_playout_vs_bot(None, n, 1, seed=5, worlds=1, net=ka, net_versus=(1, 14), net_opponent=kb, net_depth=1, net_value_scale=0.5,
                                     inspect=seen)
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS)
    scores = np.zeros((5, n, 4), np.int32)
    for p, rec in enumerate(seen):
        actions, sc = replay_pass(WA, WB, 5, S.MIX_BOT, n, 0, rec["seats"], 1, 1, 0.5)
        assert (np.asarray(rec["actions"]) == actions).all(), p
        assert (np.asarray(rec["scores"]) == sc).all(), p
        scores[p] = sc
    want = EV.duplicate_advantage(scores)
    assert got == want or (np.isnan(got["stderr"]) and np.isnan(want["stderr"]))
