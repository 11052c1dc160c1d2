"""GPU: tarok_playout_cards_net_halving — sequential-halving net playouts on a compacted item list — and the doors built on
it.  Every comparison is exact.  The expected values come from the EXISTING, already pinned net launches and the CPU rule:
tarok_playout_cards_net (or _voids / _hidden / _value) runs once per cumulative end, tests/playout_net_halving_model.py
walks the survivor rule over those rows on the host, and every row of sum, count and card is compared.  Outputs and the
scratch sit inside guard bands (tests/guarded.py), the scratch at exactly tarok_playout_net_halving_scratch_bytes; the
launch helpers are tests/gpu_harness.py's.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_net_halving.py -m gpu -q
"""
import ctypes
import functools

import numpy as np
import pytest

import gpu_harness as H
import playout_net_halving_model as NH
from guarded import Guarded
from gpu_harness import T, nets  # noqa: F401  (the module fixtures)

pytestmark = pytest.mark.gpu
U = np.uint64
KINDS = ("det", "voids", "hidden")
SEED, OFFSET, EPISODE = 43, 2000, 2
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)
POSITIONS = (0, 24, 44)
SCHEDULES = ((2, 2, 4, 8), (4, 4, 4, 4), (1, 1), (1, 2, 4))


def scratch_bytes(n, schedule):
    """The header's formula: 48 x B + 252 x n + 4 x ceil(n / 256) + 4 rounded up to 16, B = max_r n x a_r x W_r."""
    bound = max(n * a * int(w) for a, w in zip(NH.ALIVE_BOUNDS, schedule))
    return (48 * bound + 252 * n + 4 * ((n + 255) // 256) + 4 + 15) // 16 * 16


def launch(kind, env, kw, schedule, net_seats=15, depth=None, scale=70.0, words=None, salt=0, seats=15, per_game=None,
           want=("sum", "count", "action"), scratch_out=None):
    """One launch into guarded outputs over a guarded scratch of exactly scratch_bytes, the env compared before and after:
    (sum [n,12,4] i32, count [n,12] i32, action [n] u8), None where not asked for."""
    g_sum, g_act = H.card_outputs(env.n, want)
    g_cnt = Guarded("count_out", 1, env.n, np.int32, inner=(12,), device="cuda") if "count" in want else None
    w = None if kind == "det" else H.words_of(kind, env, words)
    rw = (ctypes.c_int * len(schedule))(*schedule)
    args = [KINDS.index(kind), w, len(schedule), rw, int(salt), int(seats), H.dev_u8(per_game), int(net_seats)] + list(kw) + \
        [0 if depth is None else int(depth), float(scale)]
    H._launch(env, "tarok_playout_cards_net_halving", args, [g_sum, g_cnt, g_act],
              ("tarok_playout_net_halving_scratch_bytes", (len(schedule), rw), scratch_bytes(env.n, schedule)), True,
              (kind, schedule, net_seats, depth), scratch_out)
    s, a = H.read_cards(g_sum, g_act)
    return s, None if g_cnt is None else H.read_words(g_cnt), a


def parent(kind, env, kw, worlds, net_seats=15, depth=None, scale=70.0, **more):
    """The existing net launch of the kind at `worlds`: (sum, action)."""
    return H.launch_net(kind, env, kw, worlds, net_seats, value=None if depth is None else (depth, scale), **more)


def position(env, seats=15, per_game=None):
    """(legal words [n] u64, takes_part [n] bool) of the env's games."""
    words = env.legal_actions().words.cpu().numpy().view(np.uint64)
    phase = (env.state()[9] >> U(52)) & U(3)
    mover = ((words >> U(54)) & U(3)).astype(np.int64)
    sets = np.full(env.n, seats, np.int64) if per_game is None else np.asarray(per_game, np.int64) & 15
    return words, (phase == 2) & (((sets >> mover) & 1) == 1)


def expect(kind, env, kw, schedule, net_seats=15, depth=None, scale=70.0, salt=0, seats=15, per_game=None, words=None):
    """The launch's three outputs rebuilt from the existing launch's rows at the cumulative ends, and per game the walk's
    flags and whether the card differs from the existing launch's at the first end."""
    ends = np.cumsum(schedule).tolist()
    rows = [parent(kind, env, kw, e, net_seats, depth, scale, words=words, salt=salt, seats=seats, per_game=per_game) for e in ends]
    legal, part = position(env, seats, per_game)
    s, c, a, flags = NH.launch([r[0] for r in rows], legal, part, schedule, rows[-1][1])
    differs = [bool(part[g]) and int(a[g]) != int(rows[0][1][g]) for g in range(env.n)]
    return (s, c, a), flags, differs


def check(kind, env, kw, schedule, tag=None, seen=None, **opts):
    want, flags, differs = expect(kind, env, kw, schedule, **opts)
    got = launch(kind, env, kw, schedule, **opts)
    H.assert_cards_equal(got[0], want[0], got[2], want[2], (tag, kind, schedule, opts.get("depth")))
    assert (got[1] == want[1]).all(), (tag, kind, schedule, "counts differ", np.nonzero((got[1] != want[1]).any(axis=1))[0][:8])
    if seen is not None:
        seen["tie"] += sum(bool(f and f["tie"]) for f in flags)
        seen["early"] += sum(bool(f and f["early"]) for f in flags)
        seen["differs"] += sum(differs)
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cards", POSITIONS)
def test_one_round_is_the_parent(T, nets, kind, cards):
    """(1,), (5,) and (16,) against the existing net launch at the same worlds, depth None, 1, 3 and 12: sum_out and
    action_out byte for byte, count_out = W on the legal ranks of the games that take part and 0 elsewhere."""
    from oracle import tarok_spec as S
    env = make_env(T, 96, S.MIX_BOT, cards, history=True)
    try:
        legal, part = position(env)
        nl = np.array([bin(int(w) & ((1 << 54) - 1)).count("1") for w in legal]) * part
        for worlds, depth in ((1, None), (5, None), (16, None), (5, 1), (16, 3), (1, 12), (5, 12)):
            kw = nets["P"][1] if depth in (None, 12) else nets["R"][1]
            s, c, a = launch(kind, env, kw, (worlds,), depth=depth, salt=3)
            p_sum, p_act = parent(kind, env, kw, worlds, depth=depth, salt=3)
            assert s.tobytes() == p_sum.tobytes() and a.tobytes() == p_act.tobytes(), (kind, cards, worlds, depth)
            assert (c == (np.arange(12)[None, :] < nl[:, None]) * worlds).all(), (kind, cards, worlds, depth)
        assert s.any()
    finally:
        env.close()


@pytest.mark.parametrize("kind", KINDS)
def test_schedules_against_the_rebuilt_expectation(T, nets, kind):
    """The four schedules on 96 games at the three positions, with both integer weight sets and a random one, to the last
    card and stopped at depth 2; (16, 16, 16, 16) on 16 games.  The walks seen include a cut decided by a tie, a game down
    to one card before the last round and a card that is not the existing launch's at the first end."""
    from oracle import tarok_spec as S
    seen = dict(tie=0, early=0, differs=0)
    sets = (nets["R"][1], nets["P"][1], H.random_net(T, 5))
    for cards in POSITIONS:
        env = make_env(T, 96, S.MIX_BOT, cards, history=True)
        try:
            for i, schedule in enumerate(SCHEDULES):
                check(kind, env, sets[(i + cards) % 3], schedule, tag=cards, seen=seen, salt=6)
            check(kind, env, sets[0], (1, 2, 4), tag=(cards, "depth"), seen=seen, salt=6, depth=2, scale=35.0)
        finally:
            env.close()
        env = make_env(T, 16, S.MIX_BOT, cards, history=True)
        try:
            check(kind, env, sets[1], (16, 16, 16, 16), tag=(cards, "W=64"), seen=seen, salt=6)
        finally:
            env.close()
    assert seen["tie"] >= 1 and seen["early"] >= 1 and seen["differs"] >= 1, seen


@pytest.mark.parametrize("n", [1, 17, 300])
def test_one_game_a_ragged_team_group_and_a_scan_across_blocks(T, nets, n):
    """n = 1; n = 17 (a ragged group of teams); n = 300 (the scan crosses a 256-game block, the items many 128-row tiles with
    a ragged last one)."""
    from oracle import tarok_spec as S
    env = make_env(T, n, S.MIX_BOT, 9, history=True)
    try:
        check("det", env, nets["P"][1], (2, 1, 2), tag=n, salt=2)
        check("hidden", env, nets["R"][1], (3, 2), tag=n, salt=2)
    finally:
        env.close()


def test_one_legal_card_everywhere_and_games_that_do_not_play(T, nets):
    """After 44 cards every game has one legal card: rounds 1 and later have no item at all, and every play workgroup leaves
    at its first vote.  Then a batch with finished and waiting games and seat sets that leave movers out: on = 0 between
    games that play."""
    from oracle import tarok_spec as S
    kw = nets["P"][1]
    env = make_env(T, 96, S.MIX_BOT, 44, history=True)
    try:
        legal, part = position(env)
        assert all(bin(int(w) & ((1 << 54) - 1)).count("1") == 1 for w in legal[part]) and part.sum() >= 48
        s, c, a = check("det", env, kw, (2, 2, 4, 8), tag="44 cards", salt=1)
        assert set(np.unique(c).tolist()) == {0, 2}
    finally:
        env.close()
    env = make_env(T, 96, S.MIX_ALL, 22, history=True)
    try:
        phases = (env.state()[9] >> U(52)) & U(3)
        assert (phases == 3).any() and (phases == 2).any()
        sets = np.random.RandomState(3).randint(0, 16, 96).astype(np.uint8)
        s, c, a = check("voids", env, kw, (1, 2, 2), tag="per game", salt=4, seats=0, per_game=sets)
        _, part = position(env, 0, sets)
        assert part.any() and (~part & (phases == 2)).any()
        assert (a[phases == 3] == 255).all() and not s[~part].any() and not c[~part].any()
        check("det", env, kw, (1, 2), tag="seats=5", salt=4, seats=5)
    finally:
        env.close()
    env = make_env(T, 96, S.MIX_ALL, 0, history=True, defer_exchange=True)
    try:
        phases = (env.state()[9] >> U(52)) & U(3)
        assert (phases == 1).sum() >= 8
        s, c, a = check("hidden", env, kw, (1, 1), tag="waiting", salt=4)
        assert (a[phases == 1] == 255).all() and not s[phases == 1].any() and not c[phases == 1].any()
    finally:
        env.close()


def test_net_seats_and_the_bot_played_halving_launch(T, nets):
    """net_seats 15, one seat and 0 against the rebuilt expectation; net_seats = 0 is
    tarok_playout_cards_halving(kind, schedule, samples = 1) to the byte on sum, count and action."""
    from oracle import tarok_spec as S
    env = make_env(T, 96, S.MIX_BOT, 13, history=True)
    try:
        for net_seats in (15, 4, 0):
            check("det", env, nets["R"][1], (1, 2, 4), tag=net_seats, salt=8, net_seats=net_seats)
        for kind in KINDS:
            got = launch(kind, env, nets["R"][1], (2, 1, 3), net_seats=0, salt=8)
            sums, counts, act = env.playout_cards_halving((2, 1, 3), 1, voids=kind == "voids", hidden=kind == "hidden", salt=8)
            bot = (sums.cpu().numpy(), counts.cpu().numpy(), act.cpu().numpy())
            assert got[0].any() and all(p.tobytes() == q.tobytes() for p, q in zip(got, bot)), kind
    finally:
        env.close()


def test_each_output_alone_determinism_salt_and_the_batch(T, nets):
    """Each output alone and each output NULL; the env unchanged (every launch here compares it); two calls give equal
    bytes, the whole scratch included; the salt changes the rows; a game's row in a batch of 96 equals its row alone."""
    from oracle import tarok_spec as S
    kw, schedule = nets["P"][1], (1, 2, 2)
    big, small = make_env(T, 96, S.MIX_BOT, 20, history=True), make_env(T, 1, S.MIX_BOT, 20, history=True)
    try:
        scr = []
        full = launch("hidden", big, kw, schedule, salt=5, scratch_out=scr)
        again = launch("hidden", big, kw, schedule, salt=5, scratch_out=scr)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(full, again)) and scr[0].tobytes() == scr[1].tobytes()
        assert scr[0].size == scratch_bytes(96, schedule)
        for i, name in enumerate(("sum", "count", "action")):
            alone = launch("hidden", big, kw, schedule, salt=5, want=(name,))
            assert alone[i].tobytes() == full[i].tobytes() and all(alone[k] is None for k in range(3) if k != i)
            rest = launch("hidden", big, kw, schedule, salt=5, want=tuple(k for k in ("sum", "count", "action") if k != name))
            assert rest[i] is None and all(rest[k].tobytes() == full[k].tobytes() for k in range(3) if k != i)
        assert (launch("hidden", big, kw, schedule, salt=6)[0] != full[0]).any()
        one = launch("hidden", small, kw, schedule, salt=5)
        assert all((p[:1] == q).all() for p, q in zip(full, one))
    finally:
        big.close()
        small.close()


def test_a_captured_graph_follows_the_weights(T):
    """The whole call — thirteen launches at three rounds — captured once and replayed twice, the weights changed in place
    between the replays."""
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 37, S.MIX_BOT, 6)
    try:
        kw, other = H.random_net(T, 1), H.random_net(T, 2)
        schedule = (1, 2, 2)
        env.playout_net_halving_scratch(schedule)                 # allocated before the capture
        outs = [torch.zeros((37, 12, 4), dtype=torch.int32, device="cuda"), torch.zeros((37, 12), dtype=torch.int32, device="cuda"),
                torch.zeros(37, dtype=torch.uint8, device="cuda")]
        old = [t.cpu() for t in env.playout_cards_net_halving(kw, schedule, salt=4)]
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_cards_net_halving(kw, schedule, salt=4, sum_out=outs[0], count_out=outs[1], action_out=outs[2])
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.cpu(), x) for o, x in zip(outs, old))
        for t, o in zip(kw, other):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        new = [t.cpu() for t in env.playout_cards_net_halving(other, schedule, salt=4)]
        assert all(torch.equal(o.cpu(), x) for o, x in zip(outs, new)) and not torch.equal(new[0], old[0])
    finally:
        env.close()


def test_evaluate_playout_vs_bot_net_halving_replays_from_the_launch(T):
    """64 deals, net_halving = (1, 2): every card of every pass is the launch's own on a twin env that replays the pass, and
    the returned dict is the statistic of the replayed scores."""
    import torch
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    kw = H.random_net(T, 3)
    seen = []
    got = EV.evaluate_playout_vs_bot(None, 64, 1, seed=5, inspect=seen, worlds=None, net=kw, net_halving=(1, 2))
    assert len(seen) == 5
    twin = T.TarokVecEnv(64, seed=5, mix=S.MIX_BOT)
    scores = np.zeros((5, 64, 4), np.int32)
    try:
        for p, rec in enumerate(seen):
            twin.reset(episode=rec["episode"], clear_counters=True)
            acts = torch.empty((48, 64), dtype=torch.uint8, device="cuda")
            for t in range(48):
                twin.playout_cards_net_halving(kw, (1, 2), seats=rec["seats"], action_out=acts[t])
                twin.step(acts[t], auto_reset=False)
            assert (acts.cpu().numpy() == rec["actions"]).all(), p
            scores[p] = twin.counters()[1]
            assert (scores[p] == rec["scores"]).all(), p
    finally:
        twin.close()
    assert got == EV.duplicate_advantage(scores)


def test_a_net_halving_teacher_in_the_captured_rollout(T):
    """SelfPlay(teacher=dict(net=True, net_halving=(1, 2), worlds=None)) on 512 games, T = 4: one captured iteration runs and
    records the eager rollout's bytes, and the target rows are playout_targets_counts on the launch's own sums and counts."""
    import torch
    from tarok_amd import selfplay as SP
    n, steps, tc = 512, 4, dict(net=True, net_halving=(1, 2), worlds=None, tau=8, salt=11)

    def make(use_graph):
        env = T.TarokVecEnv(n, seed=6, mix=T.karte.MIX_BOT)
        return env, SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True, teacher=tc, distill_coef=0.0, use_graph=use_graph)
    ea, a = make(True)
    eb, b = make(False)
    assert a.teacher["net_halving"] == (1, 2) and a.teacher["worlds"] == 3 and "halving" not in a.teacher
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
    for t in range(steps):
        sums, counts, _ = twin.playout_cards_net_halving(c._w, (1, 2), salt=11)
        want = twin.playout_targets_counts(sums, counts, buf["words"][t], 8.0)
        assert torch.equal(buf["teach"][t].view(torch.int16), want.view(torch.int16)), t
        twin.step(buf["act"][t], auto_reset=True)
    for e in (ea, eb, ec, twin):
        e.close()
