"""GPU: tarok_playout_cards_net (determinized playouts played by a policy network) checked exactly — integers against
integers — four ways: net_seats = 0 against the det launch's bytes; exactly summable integer weights against the per-game
model of tests/playout_net_model.py; random bf16 weights against a replay of every playout on a twin env through the
shipped greedy tarok_policy_step; a captured graph against the eager launch after the weights changed in place.  Every
case checks every row of both outputs inside guard bands (tests/guarded.py), with the scratch between guards too, and
that the env's state is untouched.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_net.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T, U, nets, random_net  # noqa: F401  (T, nets: the module fixtures)
from gpu_harness import launch_det as det_launch

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = 41, 1000, 3               # tests/test_gpu_playout_det.py's: the same games
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)
games_of = functools.partial(H.games_of, offset=OFFSET)


def net_launch(env, kw, worlds, net_seats, salt=0, seats=15, per_game=None, want=("sum", "action")):
    """One launch into guarded outputs over a guarded scratch: (sum [n,12,4] i32 or None, action [n] u8 or None)."""
    return H.launch_net("det", env, kw, worlds, net_seats, None, salt, seats, per_game, want)


def check_model(env, W, kw, worlds, net_seats, salt=0, seats=15, per_game=None, tag=None):
    import playout_net_model as NM
    want_sum, want_act = NM.playout_cards(games_of(env, per_game), SEED, salt, seats, worlds, W, net_seats)
    got_sum, got_act = net_launch(env, kw, worlds, net_seats, salt, seats, per_game)
    H.assert_cards_equal(got_sum, want_sum, got_act, want_act, tag)
    return got_sum, got_act


@pytest.mark.parametrize("n,worlds,cards", [(5, 3, 0), (5, 3, 9), (1, 1, 0), (1, 1, 6)])
def test_no_net_seat_gives_the_det_launch_bytes(T, nets, n, worlds, cards):
    """net_seats = 0: tarok_playout_cards_det(worlds, 1) to the byte.  n = 5, worlds = 3: 180 item slots, one full tile of
    128 and a partial one; n = 1, worlds = 1: a single partial tile."""
    from oracle import tarok_spec as S
    env = make_env(T, n, S.MIX_ALL, cards)
    try:
        for salt in (0, 9):
            want_sum, want_act = det_launch(env, worlds, 1, salt)
            got_sum, got_act = net_launch(env, nets["R"][1], worlds, 0, salt)
            assert want_sum.any()
            assert got_sum.tobytes() == want_sum.tobytes() and got_act.tobytes() == want_act.tobytes()
        s_only, _ = net_launch(env, nets["R"][1], worlds, 0, 9, want=("sum",))       # one output at a time: the same bytes
        _, a_only = net_launch(env, nets["R"][1], worlds, 0, 9, want=("action",))
        assert (s_only == got_sum).all() and (a_only == got_act).all()
    finally:
        env.close()


@pytest.mark.parametrize("net_seats", [15, 1, 10])
@pytest.mark.parametrize("cards", [0, 5, 24, 44])
def test_integer_weights_against_the_model(T, nets, cards, net_seats):
    """37 mixed-contract games, 2 worlds (888 item slots: six full tiles and a partial one) at a fresh deal (12 legal
    cards, 47 cards to go), mid-trick, mid-game and at the last trick (one legal card), weight set R (rounded H2, ties
    among the logits)."""
    from oracle import tarok_spec as S
    env = make_env(T, 37, S.MIX_ALL, cards)
    try:
        got_sum, _ = check_model(env, *nets["R"], 2, net_seats, salt=3, tag=(cards, net_seats))
        assert got_sum.any()
    finally:
        env.close()


def test_the_network_changes_the_result(T, nets):
    """The sums at net_seats = 15 differ from net_seats = 0, and between the two weight sets: the network is in the loop."""
    from oracle import tarok_spec as S
    env = make_env(T, 37, S.MIX_ALL, 8)
    try:
        s0, _ = net_launch(env, nets["R"][1], 2, 0)
        sr, _ = net_launch(env, nets["R"][1], 2, 15)
        sp, _ = check_model(env, *nets["P"], 2, 15, tag="set P")
        assert (s0 != sr).any() and (sr != sp).any()
    finally:
        env.close()


@pytest.mark.parametrize("code", [0, 7])
def test_klop_and_berac(T, nets, code):
    """Single-family envs: Klop (talon gifts inside the playouts) and Berac (the playouts of one tile end at different
    cards, some with the candidate itself), 20 games after 0 and 6 cards."""
    from oracle import tarok_spec as S
    for cards in (0, 6):
        env = make_env(T, 20, S.MIX_FIXED + code, cards)
        try:
            check_model(env, *nets["R"], 2, 15, tag=(code, cards))
        finally:
            env.close()


def test_games_that_do_not_take_part(T, nets):
    """Games waiting for the exchange, a per-game seat set (bits 4..7 ignored) and, with it, movers outside the set: zero
    rows, 255 or the Bot's card."""
    from oracle import tarok_spec as S
    env = make_env(T, 48, S.MIX_ALL, 0, defer_exchange=True)
    try:
        phases = (env.state()[9] >> U(52)) & U(3)
        waiting = phases == 1
        assert waiting.sum() >= 4 and (phases == 2).sum() >= 8
        got_sum, got_act = check_model(env, *nets["R"], 2, 15, tag="deferred exchange")
        assert not got_sum[waiting].any() and (got_act[waiting] == 255).all()
    finally:
        env.close()
    env = make_env(T, 48, S.MIX_ALL, 6)
    try:
        bot = env.policy_random(env.legal_actions()).cpu().numpy().copy()
        got_sum, got_act = net_launch(env, nets["R"][1], 2, 15, seats=0)
        assert not got_sum.any() and (got_act == bot).all()
        per = np.array([0, 1, 6, 15], np.uint8)[np.arange(48) % 4] | ((np.arange(48) % 3) << 4).astype(np.uint8)
        got_sum, got_act = check_model(env, *nets["R"], 2, 5, salt=11, seats=9, per_game=per, tag="per-game sets")
        movers = ((env.legal_actions().words.cpu().numpy().view(U) >> U(54)) & U(3)).astype(np.int64)
        out = ((per.astype(np.int64) >> movers) & 1) == 0
        assert out.sum() > 8 and (~out).sum() > 8
        assert not got_sum[out].any() and (got_act[out] == bot[out]).all()
    finally:
        env.close()


@pytest.mark.parametrize("cards", [0, 22])
def test_random_weights_against_a_twin_replay(T, cards):
    """Random bf16 weights, net_seats = 15, 6 games, 2 worlds.  Every live item — the model's world with the candidate
    applied — is put into a twin env through the canonical lanes, and the twin is played to every game's end by the greedy
    tarok_policy_step (set_play_mode(0, 0)): the per-(game, rank) sums of its final scores are the launch's."""
    import torch
    import playout_net_model as NM
    from oracle import tarok_spec as S
    kw = random_net(T, 5 + cards)
    env = make_env(T, 6, S.MIX_ALL, cards)
    try:
        got_sum, _ = net_launch(env, kw, 2, 15, salt=1)
        where, hs = [], []
        for g, (lanes, ep, gidx, _) in enumerate(games_of(env)):
            for j, w, h, _key in NM.items_of(lanes, ep, SEED, 1, gidx, 15, 2):
                where.append((g, j)); hs.append(h)
    finally:
        env.close()
    m = len(hs)
    assert m >= 12
    want = np.zeros((6, 12, 4), np.int64)
    twin = T.TarokVecEnv(m, seed=SEED, mix=S.MIX_ALL)
    try:
        twin.reset()
        twin.set_state(np.stack([h.lanes() for h in hs], axis=1))
        twin.set_play_mode(0.0, 0.0)
        words = [twin.legal_actions().words.clone(), torch.zeros(m, dtype=torch.int64, device="cuda")]
        act = torch.zeros(m, dtype=torch.uint8, device="cuda")
        rew, dn = torch.zeros((m, 4), dtype=torch.int16, device="cuda"), torch.zeros(m, dtype=torch.uint8, device="cuda")
        final = np.zeros((m, 4), np.int64)
        finished = np.array([h.done for h in hs])
        for i, h in enumerate(hs):
            if h.done:
                final[i] = h.scores
        for t in range(48):
            if finished.all():
                break
            twin.policy_step(kw, words[t & 1], words[(t + 1) & 1], act, reward_out=rew, done_out=dn, auto_reset=False)
            d = dn.cpu().numpy().astype(bool) & ~finished
            final[d] = rew.cpu().numpy()[d]
            finished |= d
        assert finished.all()
    finally:
        twin.close()
    for (g, j), sc in zip(where, final):
        want[g, j] += sc
    assert (got_sum == want).all(), np.nonzero((got_sum != want).any(axis=(1, 2)))[0]


def test_a_captured_launch_replays_with_the_weights_in_place(T):
    """A launch captured into a graph, then the weights changed in place: the replay gives the eager launch's bytes for
    the NEW weights."""
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 37, S.MIX_ALL, 7)
    try:
        kw, other = random_net(T, 1), random_net(T, 2)
        env.playout_net_scratch(2)                                # allocated before the capture
        s_out = torch.zeros((37, 12, 4), dtype=torch.int32, device="cuda")
        a_out = torch.zeros(37, dtype=torch.uint8, device="cuda")
        old = [t.cpu() for t in env.playout_cards_net(kw, 2, salt=4)]
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_cards_net(kw, 2, salt=4, sum_out=s_out, action_out=a_out)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_out.cpu(), old[0]) and torch.equal(a_out.cpu(), old[1])
        for t, o in zip(kw, other):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        new = [t.cpu() for t in env.playout_cards_net(other, 2, salt=4)]
        assert torch.equal(s_out.cpu(), new[0]) and torch.equal(a_out.cpu(), new[1])
        assert not torch.equal(new[0], old[0])
    finally:
        env.close()


def test_python_surface_and_arguments(T, nets):
    """playout_cards_net equals the direct C call; the scratch is cached per `worlds`; bad arguments are TAROK_EINVAL."""
    import torch
    from oracle import tarok_spec as S
    from tarok_amd import _native
    env = make_env(T, 5, S.MIX_ALL, 3)
    try:
        kw = nets["R"][1]
        want_sum, want_act = net_launch(env, kw, 3, 10, salt=2)
        sums, acts = env.playout_cards_net(kw, 3, net_seats=10, salt=2)
        assert (sums.cpu().numpy() == want_sum).all() and (acts.cpu().numpy() == want_act).all()
        assert env.playout_net_scratch(3) is env.playout_net_scratch(3) and env.playout_net_scratch(2) is not env.playout_net_scratch(3)
        scr = env.playout_net_scratch(3)
        p = env._p
        ok = dict(worlds=3, seats=15, net=15, w=[p(t) for t in kw], scr=p(scr), size=scr.numel(), out=p(sums))
        def rc(**ch):
            a = dict(ok, **ch)
            return env.L.tarok_playout_cards_net(env._h, a["worlds"], 0, a["seats"], None, a["net"], *a["w"], a["scr"], a["size"],
                                                 a["out"], None, env._stream())
        assert rc() == 0
        torch.cuda.synchronize()
        bad = [dict(worlds=0), dict(worlds=65), dict(seats=16), dict(seats=-1), dict(net=16), dict(net=-1), dict(scr=None),
               dict(size=scr.numel() - 1), dict(scr=scr.data_ptr() + 8), dict(out=None)]
        bad += [dict(w=ok["w"][:i] + [None] + ok["w"][i + 1:]) for i in range(6)]
        for ch in bad:
            assert rc(**ch) == -1, ch
        assert env.L.tarok_playout_net_scratch(env._h, 0) == -1 and env.L.tarok_playout_net_scratch(env._h, 65) == -1
        assert env.L.tarok_playout_net_scratch(None, 1) == -1
        with pytest.raises(ValueError):
            env.playout_cards_net(kw, 2, net_seats=16)
        with pytest.raises(ValueError):
            env.playout_cards_net(kw, 0)
    finally:
        env.close()


def test_a_net_teacher_in_the_captured_rollout(T):
    """SelfPlay(teacher=dict(worlds=2, net=True)) on 256 games, T = 3: the captured graph records the bytes of the eager
    rollout; the rollout's env outputs are those of a rollout without a teacher; and the teacher's rows are the targets
    of an eager playout_cards_net with the learner's rollout weights on a twin env."""
    import torch
    from tarok_amd import selfplay as SP
    n, steps, tc = 256, 3, dict(worlds=2, net=True, net_seats=15, tau=8, salt=11)

    def make(use_graph, teacher=tc):
        env = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_BOT)
        return env, SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True, teacher=teacher, distill_coef=0.0, use_graph=use_graph)
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
    ed, d = make(False, None)
    buf, plain = c.collect(steps), d.collect(steps)
    for k in ("obs", "words", "act", "logp", "val", "done", "reward"):
        assert torch.equal(buf[k], plain[k]), k
    twin = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_BOT)
    twin.reset()
    torch.cuda.synchronize()
    differ = 0
    for t in range(steps):
        sums, _ = twin.playout_cards_net(c._w, 2, net_seats=15, salt=11)
        want = twin.playout_targets(sums, buf["words"][t], 2, 8.0)
        assert torch.equal(buf["teach"][t].view(torch.int16), want.view(torch.int16)), t
        bot = twin.playout_targets(twin.playout_cards_det(2, 1, salt=11)[0], buf["words"][t], 2, 8.0)
        differ += int(buf["teach"][t].view(torch.int16).ne(bot.view(torch.int16)).any(-1).sum())
        twin.step(buf["act"][t], auto_reset=True)
    assert differ > 0
    for e in (ea, eb, ec, ed, twin):
        e.close()
