"""GPU: tarok_playout_cards_net_sampled (the net playouts under a play mode per network, `samples` playouts per (card, world))
checked exactly — integers against integers — on 300 MIX_ALL games (168 full tiles of items and a last workgroup partly past
them at 2 worlds x 3 samples): the byte equalities with the existing launches for the three world kinds at depth 0, 1, 3 and
12; tempered play against the model of tests/playout_net_sampled_model.py over the plan of tests/playout_net_sampled_cases.py;
the contract (read-only, deterministic, batch-independent, the env's play mode untouched and unread, a captured graph after B
changed in place); the Python surface and the evaluation.  Every launch writes into guard bands (tests/guarded.py) over a
guarded scratch and leaves the env, its counters and its history as they were.

THE MARGIN.  A tempered draw picks the first legal card whose running sum of exp((l - max) / T) exceeds u * total.  The kernel
sums in float32, the model in float64; they can disagree only where u lies within the float32 rounding of a CDF edge.  NEAR =
1e-5 is the margin derived in tests/test_gpu_play_mode.py::test_temperature's docstring for this very sampler
(policy_sample<1>): inputs of the same kind — exact logits of the integer weight sets, at most 12 legal cards, so at most 12
float32 additions of terms in (0, 1] and one __expf each, a relative error of a few 2^-24 ~ 6e-8 per term and under 2e-6 on
a normalised edge, five times under NEAR.  The derivation does not depend on where the logits come from or on the key, so it
carries over unchanged.  A row (game, rank) is compared EXACTLY when every tempered draw of every one of its items has margin
>= NEAR in the model, and is left out otherwise; a game's card is compared when none of its rows is left out.  At most CAP =
10 % of the rows with a card left to choose may be left out (tests/test_playout_net_sampled_cpu.py holds the model alone to
that); after 44 cards nothing is.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_net_sampled.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
import playout_model as PM
import playout_net_sampled_cases as SC
import playout_net_sampled_model as SM
import playout_net_value_model as VM
from gpu_harness import T, host_words, model_words, random_net, words_of  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE, N = SC.SEED, SC.OFFSET, SC.EPISODE, SC.N
make_env = functools.partial(H.make_env, seed=SEED, episode=EPISODE)
GREEDY = (0.0, 0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def nets(T):
    """A and B of tests/playout_net_sampled_cases.weight_sets as (float64 set, kernel set)."""
    import policy_exact_ref as PE
    return {k: (W, PE.kernel_weights(T, W)) for k, W in SC.weight_sets().items()}


def mix_all():
    from oracle import tarok_spec as S
    return S.MIX_ALL


def sampled(kind, env, ka, kb, worlds, samples, own, opp, depth, modes, scale=70.0, salt=SC.SALT, seats=15, want=("sum", "action")):
    """One tarok_playout_cards_net_sampled into guarded outputs over a guarded scratch, the env compared before and after."""
    w = None if kind == "det" else words_of(kind, env)
    args = [int(worlds), int(samples), int(salt), int(seats), None, VM.KINDS.index(kind), w, int(own), int(opp), int(depth), float(scale)]
    args += [float(x) for x in modes]
    return H.launch_cards(env, "tarok_playout_cards_net_sampled", args + list(ka) + list(kb if kb is not None else [None] * 6), want,
                          scratch=("tarok_playout_cards_net_sampled_scratch", (int(worlds), int(samples)), env.n * 12 * worlds * samples * 48),
                          check_env_untouched=True, tag=(kind, worlds, samples, own, opp, depth, modes))


def versus(kind, env, ka, kb, worlds, own, opp, depth, scale=70.0, salt=SC.SALT):
    w = None if kind == "det" else words_of(kind, env)
    args = [int(worlds), int(salt), 15, None, VM.KINDS.index(kind), w, int(own), int(opp), int(depth), float(scale)]
    return H.launch_cards(env, "tarok_playout_cards_net_versus", args + list(ka) + list(kb), scratch=(
        "tarok_playout_net_scratch", (int(worlds),), env.n * 12 * worlds * 48), tag=(kind, worlds, own, opp, depth))


def bot_launch(kind, env, worlds, samples, salt=SC.SALT):
    if kind == "det":
        return H.launch_det(env, worlds, samples, salt)
    return H.launch_worlds(kind, env, worlds, samples, None, salt)


def same(got, want, tag):
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), tag


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("cards", SC.POSITIONS)
def test_the_byte_equalities_with_the_existing_launches(T, kind, cards):
    """At depth 0, 1, 3 and 12, with random weights A != B, 2 worlds: samples = 1 at temperature 0 and epsilon 0 on both is
    tarok_playout_cards_net_versus for (15, 0), (1, 14) and (3, 8); (0, 0) at any mode is the Bot-played launch at (worlds,
    samples) (where nothing stops: depth 0 and 12); epsilon 1 on both networks is (0, 0) at the same depth, whatever the roles
    and temperatures; (15, 0) at temperature 0 with 3 samples is 3 x the samples = 1 rows; A = B (equal copies in different
    tensors) under equal tempered modes gives (15, 0)'s rows for the splits (5, 10) and (1, 14)."""
    env = make_env(T, N, mix_all(), cards, history=True, offset=OFFSET)
    try:
        ka, kb = random_net(T, 31 + cards), random_net(T, 32 + cards)
        copy = [t.clone() for t in ka]
        W, S = SC.WORLDS, SC.SAMPLES
        some = 0
        for depth in SC.BYTE_DEPTHS:
            scale = 70.0 if depth != 3 else 1e9
            for own, opp in ((15, 0), (1, 14), (3, 8)):
                old = versus(kind, env, ka, kb, W, own, opp, depth, scale)
                same(sampled(kind, env, ka, kb, W, 1, own, opp, depth, GREEDY, scale), old, (depth, own, opp, "versus"))
                some += int(old[0].any())
            zero = sampled(kind, env, ka, kb, W, S, 0, 0, depth, (0.5, 0.25, 2.0, 0.0), scale)
            same(sampled(kind, env, ka, None, W, S, 0, 0, depth, (1.0, 0.0, 1.0, 0.0), scale), zero, (depth, "0, 0 at another mode"))
            if depth in (0, 12):
                same(zero, bot_launch(kind, env, W, S), (depth, "0, 0"))
            same(sampled(kind, env, ka, kb, W, S, 1, 14, depth, (0.5, 1.0, 2.0, 1.0), scale), zero, (depth, "epsilon 1, (1, 14)"))
            same(sampled(kind, env, ka, kb, W, S, 15, 0, depth, (0.0, 1.0, 1.0, 1.0), scale), zero, (depth, "epsilon 1, (15, 0)"))
            one = sampled(kind, env, ka, None, W, 1, 15, 0, depth, GREEDY, scale)
            three = sampled(kind, env, ka, None, W, S, 15, 0, depth, GREEDY, scale)
            assert (three[0] == S * one[0]).all() and (three[1] == one[1]).all(), (depth, "S x")
            mode = (0.5, 0.125, 0.5, 0.125)
            whole = sampled(kind, env, ka, None, W, S, 15, 0, depth, mode, scale)
            same(sampled(kind, env, ka, copy, W, S, 5, 10, depth, mode, scale), whole, (depth, "5, 10"))
            same(sampled(kind, env, ka, copy, W, S, 1, 14, depth, mode, scale), whole, (depth, "1, 14, A = B"))
            if cards < 44:
                assert (whole[0] != three[0]).any(), "the tempered rows are the greedy ones"
        assert some >= 2
    finally:
        env.close()


@pytest.mark.parametrize("at", range(len(SC.TEMPERED)))
def test_tempered_play_against_the_model(T, nets, at):
    """Every case of the plan on the env's own games and words: the rows of the model's games whose items all keep NEAR from
    every CDF edge EQUAL the model's, and so do the cards of the games with no row left out; at most CAP of the rows with a card
    left to choose are left out, none after 44 cards."""
    case = SC.TEMPERED[at]
    kind, cards, worlds, samples, (own, opp), ma, mb, depth = case
    (WA, ka), (WB, kb) = nets["A"], nets["B"]
    env = make_env(T, N, mix_all(), cards, history=True, offset=OFFSET)
    try:
        games = H.games_of(env, offset=OFFSET)
        words = None
        if kind != "det":
            words = model_words(kind, env)
            assert (host_words(kind, env) == words).all(), "the env's words are not the model's"
            words = [int(x) for x in words]
        scale = 0.5 if depth else 70.0
        want_sum, want_act, margin, info = SC.model_rows(case, games, words, dict(A=WA, B=WB), value_scale=scale)
        out, choice = SC.left_out(case, games, margin)
        got_sum, got_act = sampled(kind, env, ka, kb, worlds, samples, own, opp, depth, ma + mb, scale)
        print("case %s: %d rows with a choice, %d left out, %d tempered draws" % (case, choice.sum(), out.sum(), sum(d["draws"] for _, d in info)))
        assert out.sum() <= SC.CAP * choice.sum() and (cards < 44 or not out.any())
        only = np.array(SC.MODEL_GAMES)
        rows = ~out
        bad = np.argwhere((got_sum[only] != want_sum).any(-1) & rows)
        assert bad.size == 0, (case, "rows differ", bad[:6].tolist(), got_sum[only][tuple(bad[0])].tolist(), want_sum[tuple(bad[0])].tolist())
        whole = rows.all(1)
        assert (got_act[only][whole] == want_act[whole]).all(), (case, "cards differ")
        assert want_sum.any() and whole.sum() >= 0.5 * len(only)
        if depth and cards < 44:
            assert any(d["stopped"] for _, d in info)
    finally:
        env.close()


def test_the_contract(T, nets):
    """Two launches give equal bytes; a game's rows are the same in an env of 300 and in one holding the slice 140..159 of it,
    whatever outputs are asked for; the env's play mode is the same before and after, and changing it changes no byte.  (The
    env's state bytes before = after: every launch of this file, through the harness.)"""
    ka, kb = nets["A"][1], nets["B"][1]
    full = make_env(T, N, mix_all(), 24, offset=OFFSET)
    part = make_env(T, 20, mix_all(), 24, offset=OFFSET + 140)
    try:
        for own, opp, depth, modes in ((1, 14, 0, (1.0, 0.0, 0.5, 0.0)), (14, 1, 3, (2.0, 0.25, 1.0, 0.0))):
            assert full.play_mode == (1.0, 0.0)
            a = sampled("det", full, ka, kb, 2, 3, own, opp, depth, modes, 0.5)
            same(sampled("det", full, ka, kb, 2, 3, own, opp, depth, modes, 0.5), a, "twice")
            assert full.play_mode == (1.0, 0.0)
            c = sampled("det", part, ka, kb, 2, 3, own, opp, depth, modes, 0.5)
            assert (a[0][140:160] == c[0]).all() and (a[1][140:160] == c[1]).all() and c[0].any()
            s_only, _ = sampled("det", full, ka, kb, 2, 3, own, opp, depth, modes, 0.5, want=("sum",))
            _, a_only = sampled("det", full, ka, kb, 2, 3, own, opp, depth, modes, 0.5, want=("action",))
            assert (s_only == a[0]).all() and (a_only == a[1]).all()
            full.set_play_mode(0.25, 0.5)
            same(sampled("det", full, ka, kb, 2, 3, own, opp, depth, modes, 0.5), a, "under another env mode")
            assert full.play_mode == (0.25, 0.5)
            full.set_play_mode(1.0, 0.0)
    finally:
        full.close(); part.close()


def test_a_captured_launch_replays_with_b_overwritten_in_place(T, nets):
    """A launch captured into a graph, then B overwritten in place: the replay equals the eager launch with the new B."""
    import torch
    env = make_env(T, N, mix_all(), 24, offset=OFFSET)
    try:
        ka, kb, other = nets["A"][1], [t.clone() for t in nets["B"][1]], random_net(T, 77)
        more = dict(temperature=1.0, opp_temperature=0.5, opp_epsilon=0.125, depth=2, value_scale=0.5, salt=3)
        env.playout_net_sampled_scratch(2, 3)                        # allocated before the capture
        outs = dict(sum_out=torch.zeros((N, 12, 4), dtype=torch.int32, device="cuda"), action_out=torch.zeros(N, dtype=torch.uint8, device="cuda"))
        eager = lambda b: [t.cpu() for t in env.playout_cards_net_sampled(ka, b, 2, 3, 14, 1, **more)]
        first = eager(kb)
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                captured = env.playout_cards_net_sampled(ka, kb, 2, 3, 14, 1, **more, **outs)
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
    """playout_cards_net_sampled equals the direct C calls for the three kinds; opp_* default to A's mode; the refusals."""
    env = make_env(T, N, mix_all(), 24, history=True, offset=OFFSET)
    try:
        ka, kb = nets["A"][1], nets["B"][1]
        for kind in SC.KINDS:
            arg = {} if kind == "det" else {kind: True}
            want = sampled(kind, env, ka, kb, 2, 3, 3, 8, 2, (0.5, 0.25, 2.0, 0.0), 0.5, salt=2, seats=7)
            got = env.playout_cards_net_sampled(ka, kb, 2, 3, 3, 8, temperature=0.5, epsilon=0.25, opp_temperature=2.0, opp_epsilon=0.0, depth=2,
                                                value_scale=0.5, salt=2, seats=7, **arg)
            assert (got[0].cpu().numpy() == want[0]).all() and (got[1].cpu().numpy() == want[1]).all(), kind
            want = sampled(kind, env, ka, kb, 2, 3, 1, 14, 0, (0.5, 0.25, 0.5, 0.25), 70.0, salt=2)
            got = env.playout_cards_net_sampled(ka, kb, 2, 3, 1, 14, temperature=0.5, epsilon=0.25, salt=2, **arg)
            assert (got[0].cpu().numpy() == want[0]).all() and (got[1].cpu().numpy() == want[1]).all(), kind
        old = env.playout_cards_net(ka, 2, salt=2)
        new = env.playout_cards_net_sampled(ka, None, 2, 1, temperature=0.0, salt=2)
        assert all((x == y).all() for x, y in zip(old, new))
        for bad in (dict(own_rel=1, opp_rel=1), dict(own_rel=16), dict(depth=0), dict(voids=True, hidden=True), dict(temperature=-1.0),
                    dict(epsilon=1.5), dict(opp_temperature=1e7), dict(opp_epsilon=-0.5)):
            with pytest.raises(ValueError):
                env.playout_cards_net_sampled(ka, kb, 2, 3, **bad)
        for worlds, samples in ((0, 1), (2, 0), (2, 1025), (65, 1)):
            with pytest.raises(ValueError):
                env.playout_cards_net_sampled(ka, kb, worlds, samples)
        with pytest.raises(ValueError):
            env.playout_cards_net_sampled(ka, None, 2, 3, 1, 14)
    finally:
        env.close()


def replay_pass(WA, seed, mix, n, episode, seats, worlds, samples, depth, value_scale, mode):
    """One pass of evaluate_playout_vs_bot(net=A, net_samples=, net_temperature=) on the oracle, all n games in lock-step: the
    model's card at every move (the sampled player on `seats`, (15, 0), the Bot elsewhere).  Returns (actions [48, n], scores
    [n, 4], unsure [n]: the game met an item with a draw within NEAR of a CDF edge — its later cards are not the model's to say)."""
    from oracle import oracle as O
    gs = [O.Game.synth(seed, i, episode, mix) for i in range(n)]
    actions = np.full((48, n), 255, np.uint8)
    unsure = np.zeros(n, bool)
    for t in range(48):
        live = [i for i in range(n) if not gs[i].done]
        if not live:
            break
        _, cards, margin, _ = SM.playout_cards("det", [(gs[i].lanes(), episode, i, None) for i in live], seed, 0, seats, worlds, samples, WA, WA, 15,
                                               0, depth, value_scale, mode, mode)
        for i, c, m in zip(live, cards, margin.min(1)):
            unsure[i] |= m < SC.NEAR
            actions[t, i] = c
            assert gs[i].step(int(c)) >= 0
    assert all(g.done for g in gs)
    return actions, np.array([g.scores for g in gs], np.int32), unsure


def test_evaluate_replays_the_models_cards(T, nets):
    """evaluate_playout_vs_bot(None, worlds=1, net=A, net_samples=2, net_temperature=1.0, net_depth=1, net_value_scale=0.5) on 64
    deals: every card and every final score of the five passes are the model's replay, for the deals that met no ambiguous
    item (at most CAP of them are left out in a pass)."""
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    WA, ka = nets["A"]
    seen, n = [], 64
    EV.evaluate_playout_vs_bot(None, n, 1, seed=5, worlds=1, net=ka, net_samples=2, net_temperature=1.0, net_depth=1, net_value_scale=0.5,
                               inspect=seen)
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS)
    for p, rec in enumerate(seen):
        actions, sc, unsure = replay_pass(WA, 5, S.MIX_BOT, n, 0, rec["seats"], 1, 2, 1, 0.5, (1.0, 0.0))
        print("pass %d: %d of %d deals left out" % (p, unsure.sum(), n))
        assert unsure.sum() <= SC.CAP * n
        ok = ~unsure
        assert (np.asarray(rec["actions"])[:, ok] == actions[:, ok]).all(), p
        assert (np.asarray(rec["scores"])[ok] == sc[ok]).all(), p
