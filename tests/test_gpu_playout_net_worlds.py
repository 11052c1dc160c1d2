"""GPU: tarok_playout_cards_net_voids and tarok_playout_cards_net_hidden (the net-played card playouts in the void-aware
and the hidden-card worlds) checked exactly — integers against integers: net_seats = 0 against the Bot-played launches'
bytes; words that constrain nothing against tarok_playout_cards_net's bytes; exactly summable integer weights against
the model of tests/playout_net_worlds_model.py on the env's own words; a guard that those positions do constrain the
worlds; games that do not take part; a captured graph after the weights and the words changed in place; the teacher
inside the captured rollout.  Every launch writes into guard bands (tests/guarded.py) over a guarded scratch and leaves
the env and its history as they were.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_net_worlds.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T, U, host_words, model_words, nets, words_of  # noqa: F401  (T, nets: the module fixtures)

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = 41, 1000, 3               # tests/test_gpu_playout_det.py's: the same games
KLOP, DVE, BERAC, SOLO_BREZ = 0, 2, 7, 8
KINDS = ("voids", "hidden")
NET_FN = dict(voids="tarok_playout_cards_net_voids", hidden="tarok_playout_cards_net_hidden")
SHAPES = [(5, 3), (1, 1)]                         # 180 item slots: a full tile of 128 and a partial one; one partial tile
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)
games_of = functools.partial(H.games_of, offset=OFFSET)
det_net_launch = functools.partial(H.launch_net, "det")
net_launch = H.launch_net                         # (kind, env, kw, worlds, net_seats, words, salt, seats, per_game, want)


def bot_launch(kind, env, worlds, salt=0, seats=15, per_game=None):
    """tarok_playout_cards_voids / _hidden at (worlds, 1) on the env's own words, into guarded outputs."""
    return H.launch_worlds(kind, env, worlds, 1, None, salt, seats, per_game)


def check_model(kind, env, W, kw, worlds, net_seats, salt=0, seats=15, per_game=None, tag=None):
    """Both outputs of a launch on the env's own words against the model on the words rebuilt from the history."""
    import playout_net_worlds_model as WM
    words = model_words(kind, env)
    assert (host_words(kind, env) == words).all(), (tag, "the env's words are not the model's")
    want_sum, want_act = WM.playout_cards(kind, games_of(env, per_game), SEED, salt, seats, worlds, W, net_seats, [int(x) for x in words])
    got_sum, got_act = net_launch(kind, env, kw, worlds, net_seats, None, salt, seats, per_game)
    H.assert_cards_equal(got_sum, want_sum, got_act, want_act, tag)
    return got_sum, got_act


def positions(kind):
    """The (mix, cards) of the model comparison: fresh-ish, mid-game, last trick.  hidden: a Klop inside its first six
    tricks, then Dve games (non-declarers to move among them), then every contract."""
    from oracle import tarok_spec as S
    if kind == "voids":
        return [(S.MIX_ALL, 5), (S.MIX_ALL, 24), (S.MIX_ALL, 44)]
    return [(S.MIX_FIXED + KLOP, 5), (S.MIX_FIXED + DVE, 24), (S.MIX_ALL, 44)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,worlds,cards", [(5, 3, 0), (5, 3, 9), (5, 3, 24), (5, 3, 44), (1, 1, 0), (1, 1, 9)])
def test_no_net_seat_gives_the_bot_launch_bytes(T, nets, kind, n, worlds, cards):
    """net_seats = 0: tarok_playout_cards_voids(worlds, 1) / tarok_playout_cards_hidden(worlds, 1) to the byte, for one
    seat set and for per-game sets (bits 4..7 ignored)."""
    from oracle import tarok_spec as S
    env = make_env(T, n, S.MIX_ALL, cards, history=True)
    try:
        per = (np.array([15, 1, 6, 15, 9], np.uint8) | np.array([0, 16, 32, 64, 128], np.uint8))[:n]
        for salt, seats, per_game in ((0, 15, None), (9, 15, None), (9, 0, per)):
            want_sum, want_act = bot_launch(kind, env, worlds, salt, seats, per_game)
            got_sum, got_act = net_launch(kind, env, nets["R"][1], worlds, 0, None, salt, seats, per_game)
            assert per_game is not None or want_sum.any()
            assert got_sum.tobytes() == want_sum.tobytes() and got_act.tobytes() == want_act.tobytes(), (salt, seats)
        s_only, _ = net_launch(kind, env, nets["R"][1], worlds, 0, None, 9, 0, per, want=("sum",))   # one output at a time
        _, a_only = net_launch(kind, env, nets["R"][1], worlds, 0, None, 9, 0, per, want=("action",))
        assert (s_only == got_sum).all() and (a_only == got_act).all()
    finally:
        env.close()


@pytest.mark.parametrize("n,worlds", SHAPES)
def test_zero_void_words_give_the_net_launch_bytes(T, nets, n, worlds):
    from oracle import tarok_spec as S
    for cards in (9, 24):
        env = make_env(T, n, S.MIX_ALL, cards, history=True)
        try:
            want_sum, want_act = det_net_launch(env, nets["R"][1], worlds, 15, salt=3)
            got_sum, got_act = net_launch("voids", env, nets["R"][1], worlds, 15, np.zeros(n, np.uint32), salt=3)
            assert want_sum.any()
            assert got_sum.tobytes() == want_sum.tobytes() and got_act.tobytes() == want_act.tobytes(), cards
        finally:
            env.close()


@pytest.mark.parametrize("n,worlds", SHAPES)
def test_nothing_more_hidden_gives_the_net_launch_bytes(T, nets, n, worlds):
    """Berac, Solo_brez and a Klop whose talon is gone: every game's bytes are tarok_playout_cards_net's; Dve after 24
    cards: the games whose declarer is to move."""
    from oracle import tarok_spec as S
    for code, cards in ((BERAC, 3), (SOLO_BREZ, 5), (KLOP, 24)):
        env = make_env(T, n, S.MIX_FIXED + code, cards, history=True)
        try:
            want_sum, want_act = det_net_launch(env, nets["R"][1], worlds, 15, salt=3)
            got_sum, got_act = net_launch("hidden", env, nets["R"][1], worlds, 15, salt=3)
            assert want_sum.any()
            assert got_sum.tobytes() == want_sum.tobytes() and got_act.tobytes() == want_act.tobytes(), (code, cards)
        finally:
            env.close()
    env = make_env(T, n, S.MIX_FIXED + DVE, 24, history=True)
    try:
        m = env.state()[9]
        mover = (((m >> U(27)) & U(3)) + ((m >> U(24)) & U(7))) & U(3)
        own = mover == ((m >> U(37)) & U(3))
        assert own.sum() >= 1                                   # (games 0 and 1 of the five; game 0 of the one)
        want_sum, want_act = det_net_launch(env, nets["R"][1], worlds, 15, salt=3)
        got_sum, got_act = net_launch("hidden", env, nets["R"][1], worlds, 15, salt=3)
        assert want_sum[own].any() and (got_sum[own] == want_sum[own]).all() and (got_act[own] == want_act[own]).all()
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("net_seats", [15, 1, 10])
@pytest.mark.parametrize("at", [0, 1, 2])
def test_integer_weights_against_the_model(T, nets, kind, at, net_seats):
    """Weight set R (rounded H2, ties among the logits) on the env's own words, after 5, 24 and 44 cards, at both shapes."""
    mix, cards = positions(kind)[at]
    for n, worlds in SHAPES:
        env = make_env(T, n, mix, cards, history=True)
        try:
            got_sum, _ = check_model(kind, env, *nets["R"], worlds, net_seats, salt=3, tag=(kind, cards, net_seats, n))
            assert got_sum.any()
        finally:
            env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_positions_constrain_the_worlds(T, nets, kind):
    """The comparison above is not vacuous: among its positions a game has a void word for a seat other than the mover
    (voids), a non-empty hidden discard set and live Klop talon cards (hidden), and the launch's sums differ from
    tarok_playout_cards_net's somewhere."""
    import playout_net_worlds_model as WM
    from oracle import oracle as O
    seen, differ = set(), 0
    for mix, cards in positions(kind):
        env = make_env(T, 5, mix, cards, history=True)
        try:
            words, lanes = host_words(kind, env), env.state()
            seen |= {WM.constrains(kind, O.Game.from_lanes(lanes[:, g]), int(words[g])) for g in range(5)}
            new, _ = net_launch(kind, env, nets["R"][1], 3, 15, salt=3)
            old, _ = det_net_launch(env, nets["R"][1], 3, 15, salt=3)
            differ += int((new != old).any(axis=(1, 2)).sum())
        finally:
            env.close()
    assert seen >= ({"voids"} if kind == "voids" else {"discards", "talon"}), seen
    assert differ >= 1


@pytest.mark.parametrize("kind", KINDS)
def test_games_that_do_not_take_part(T, nets, kind):
    """Games waiting for the exchange, finished games and movers outside a per-game seat set: zero rows; card 255, or
    the Bot's card where the game is in play."""
    from oracle import tarok_spec as S
    env = make_env(T, 5, S.MIX_ALL, 0, history=True, defer_exchange=True)
    try:
        waiting = ((env.state()[9] >> U(52)) & U(3)) == 1
        assert waiting.sum() >= 1 and (~waiting).sum() >= 1
        got_sum, got_act = check_model(kind, env, *nets["R"], 3, 15, tag="deferred exchange")
        assert not got_sum[waiting].any() and (got_act[waiting] == 255).all() and got_sum[~waiting].any()
    finally:
        env.close()
    env = make_env(T, 5, S.MIX_ALL, 24, history=True)
    try:
        finished = ((env.state()[9] >> U(52)) & U(3)) == 3
        assert finished.sum() >= 1 and (~finished).sum() >= 3
        bot = env.policy_random(env.legal_actions()).cpu().numpy().copy()
        got_sum, got_act = net_launch(kind, env, nets["R"][1], 3, 15, seats=0)
        assert not got_sum.any() and (got_act[~finished] == bot[~finished]).all() and (got_act[finished] == 255).all()
        movers = ((env.legal_actions().words.cpu().numpy().view(U) >> U(54)) & U(3)).astype(np.int64)
        per = np.where(np.arange(5) % 2 == 0, 1 << movers, 15 ^ (1 << movers)).astype(np.uint8) | np.uint8(0x50)
        got_sum, got_act = check_model(kind, env, *nets["R"], 3, 5, salt=11, seats=9, per_game=per, tag="per-game sets")
        out = (np.arange(5) % 2 == 1) & ~finished
        assert out.sum() >= 1 and not got_sum[out | finished].any() and (got_act[out] == bot[out]).all()
        assert (got_act[finished] == 255).all() and got_sum[~(out | finished)].any()
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_captured_launch_replays_with_the_weights_and_the_words_in_place(T, nets, kind):
    """A launch captured into a graph on the caller's word tensor; the words, then the weights, change in place: every
    replay gives the eager launch's bytes for the values that are in place then."""
    import torch
    from oracle import tarok_spec as S
    mix, cards = positions(kind)[1]
    env = make_env(T, 5, mix, cards, history=True)
    try:
        kw, other = [t.clone() for t in nets["R"][1]], nets["P"][1]
        own = words_of(kind, env).clone()
        words = torch.zeros_like(own)
        arg = {kind: words}
        env.playout_net_scratch(3)                                # allocated before the capture
        s_out = torch.zeros((5, 12, 4), dtype=torch.int32, device="cuda")
        a_out = torch.zeros(5, dtype=torch.uint8, device="cuda")
        eager = lambda w, x: [t.cpu() for t in env.playout_cards_net(w, 3, salt=3, **{kind: x})]
        first = eager(kw, words)
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_cards_net(kw, 3, salt=3, sum_out=s_out, action_out=a_out, **arg)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_out.cpu(), first[0]) and torch.equal(a_out.cpu(), first[1])
        words.copy_(own)
        graph.replay()
        torch.cuda.synchronize()
        second = eager(nets["R"][1], own)
        assert torch.equal(s_out.cpu(), second[0]) and torch.equal(a_out.cpu(), second[1])
        assert not torch.equal(second[0], first[0])               # (zero words and the games' own: other worlds)
        for t, o in zip(kw, other):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        third = eager(other, own)
        assert torch.equal(s_out.cpu(), third[0]) and torch.equal(a_out.cpu(), third[1])
        assert not torch.equal(third[0], second[0])
    finally:
        env.close()


def test_python_surface_and_arguments(T, nets):
    """playout_cards_net(voids= / hidden=) equals the direct C call, with the env's own words (through a scratch tensor
    too) and with given ones, which need no history; every TAROK_EINVAL is returned."""
    import torch
    from oracle import tarok_spec as S
    env, plain = make_env(T, 5, S.MIX_ALL, 24, history=True), make_env(T, 5, S.MIX_ALL, 24)
    try:
        kw = nets["R"][1]
        for kind in KINDS:
            want_sum, want_act = net_launch(kind, env, kw, 3, 10, salt=2)
            given = words_of(kind, env)
            for e, arg in ((env, {kind: True}), (env, {kind: True, "words": torch.zeros_like(given)}), (env, {kind: given}),
                           (plain, {kind: given})):
                sums, acts = e.playout_cards_net(kw, 3, net_seats=10, salt=2, **arg)
                assert (sums.cpu().numpy() == want_sum).all() and (acts.cpu().numpy() == want_act).all(), (kind, list(arg))
            with pytest.raises(ValueError):
                plain.playout_cards_net(kw, 3, **{kind: True})
            scr = env.playout_net_scratch(3)
            p = env._p
            ok = dict(env=env._h, worlds=3, seats=15, words=p(given), net=15, w=[p(t) for t in kw], scr=p(scr), size=scr.numel(),
                      out=p(sums))
            def rc(**ch):
                a = dict(ok, **ch)
                return getattr(env.L, NET_FN[kind])(a["env"], a["worlds"], 0, a["seats"], None, a["words"], a["net"], *a["w"], a["scr"],
                                                    a["size"], a["out"], None, env._stream())
            assert rc() == 0
            torch.cuda.synchronize()
            bad = [dict(env=None), dict(worlds=0), dict(worlds=65), dict(seats=16), dict(seats=-1), dict(words=None), dict(net=16),
                   dict(net=-1), dict(scr=None), dict(size=scr.numel() - 1), dict(scr=scr.data_ptr() + 8), dict(out=None)]
            bad += [dict(w=ok["w"][:i] + [None] + ok["w"][i + 1:]) for i in range(6)]
            for ch in bad:
                assert rc(**ch) == -1, (kind, ch)
        with pytest.raises(ValueError):
            env.playout_cards_net(kw, 3, voids=True, hidden=True)
    finally:
        env.close()
        plain.close()


def test_a_void_aware_net_teacher_in_the_captured_rollout(T):
    """SelfPlay(teacher=dict(net=True, worlds=2, net_worlds="voids")) on 256 games, T = 4: the captured graph records the
    bytes of the eager rollout; the rows are the targets of an eager shown_voids + playout_cards_net(voids=...) with the
    learner's rollout weights on a twin env, and differ from the determinized net teacher's once voids have been shown;
    then one iterate() runs through the fused learner."""
    import torch
    from tarok_amd import selfplay as SP
    n, steps, tc = 256, 4, dict(worlds=2, net=True, net_worlds="voids", tau=8, salt=11)

    def make(use_graph):
        env = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_ALL, history=True)
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
    twin = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_ALL, history=True)
    twin.reset()
    torch.cuda.synchronize()
    differ = 0
    for t in range(steps):
        words = twin.shown_voids()
        sums, _ = twin.playout_cards_net(c._w, 2, salt=11, voids=words)
        want = twin.playout_targets(sums, buf["words"][t], 2, 8.0)
        assert torch.equal(buf["teach"][t].view(torch.int16), want.view(torch.int16)), t
        det = twin.playout_targets(twin.playout_cards_net(c._w, 2, salt=11)[0], buf["words"][t], 2, 8.0)
        differ += int(buf["teach"][t].view(torch.int16).ne(det.view(torch.int16)).any(-1).sum())
        twin.step(buf["act"][t], auto_reset=True)
    assert differ > 0
    stats = a.iterate(T=steps, epochs=1, minibatches=1)
    assert np.isfinite(stats["loss"]) and np.isfinite(stats["distill_ce"]) and stats["teacher_frac"] > 0
    for e in (ea, eb, ec, twin):
        e.close()
