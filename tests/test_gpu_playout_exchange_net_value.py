"""GPU: tarok_playout_exchange_net_value (the exchange's net playouts stopped at the declarer's depth-th decision, the value
head's estimate in the declarer's column) checked exactly — integers against integers: depth 13 against the bytes of
tarok_playout_exchange_net, the final scratch included; exactly summable integer weights at depths 1, 2, 3 and 12 against
the model of tests/playout_front_net_value_model.py over the plan of tests/playout_front_net_value_cases.py; random weights
at net_seats = 0 against tarok_policy_mlp's value_out on the model's stop positions; a captured graph after the weights
changed in place; every TAROK_EINVAL.  Every launch writes into guard bands (tests/guarded.py) over a guarded scratch and
leaves the env and its counters as they were.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_exchange_net_value.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
import playout_front_net_value_cases as C
import playout_front_net_value_model as FV
from gpu_harness import T, U, random_net  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
make_env = functools.partial(H.make_env, seed=C.X_SEED, offset=C.X_OFFSET, episode=C.X_EPISODE, defer_exchange=True)
NAMES = ("sums", "choices", "discards")


@pytest.fixture(scope="module")
def nets(T):
    """R, P and V of tests/playout_net_value_cases.weight_sets as (float64 set, kernel set)."""
    import policy_exact_ref as PE
    return {k: (W, PE.kernel_weights(T, W)) for k, W in C.weight_sets().items()}


def scratch_of(env, worlds, sets):
    return ("tarok_playout_exchange_net_scratch", (int(worlds), int(sets)), env.n * 6 * sets * worlds * 48)


def value_launch(env, kw, worlds, sets, net_seats, depth, scale, salt=C.SALT, seats=15, per_game=None, want=("sum", "choice", "discards"),
                 scratch_out=None):
    """One launch into guarded outputs over a guarded scratch: (sum [n, 6 * sets, 4] i32, choice [n] i8, discards [n, 3] u8)."""
    return H.launch_exchange(env, "tarok_playout_exchange_net_value",
                             [int(worlds), int(sets), int(salt), int(seats), H.dev_u8(per_game), int(net_seats), int(depth), float(scale)] + list(kw),
                             sets, want, scratch=scratch_of(env, worlds, sets), check_env_untouched=True,
                             tag=(worlds, sets, net_seats, seats, depth, scale), scratch_out=scratch_out)


def existing_launch(env, kw, worlds, sets, net_seats, salt, seats, per_game, scratch_out):
    return H.launch_exchange(env, "tarok_playout_exchange_net", [int(worlds), int(sets), int(salt), int(seats), H.dev_u8(per_game), int(net_seats)] + list(kw),
                             sets, scratch=scratch_of(env, worlds, sets), check_env_untouched=True, tag=(worlds, sets, net_seats, seats),
                             scratch_out=scratch_out)


def assert_games(env, games):
    assert (env.state() == np.stack([g[0] for g in games], axis=1)).all(), "the env does not hold the plan's positions"


def assert_equal(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
        assert bad.size == 0, (tag, name, "differ", bad[:8], g[bad[0]].tolist(), w[bad[0]].tolist())


@pytest.mark.parametrize("n", [5, 1])
def test_depth_13_gives_the_existing_launch_bytes(T, nets, n):
    """depth = 13 never stops an item: the three outputs AND the final scratch of tarok_playout_exchange_net — the markers'
    viewer bits are gone once every item has its scores — with the integer set R and with random weights, at net_seats 15
    and 0, for one seat set and for per-game sets, at any value_scale."""
    from oracle import tarok_spec as S
    _, worlds, sets = C.X_SHAPE
    env = make_env(T, n, S.MIX_BOT)
    try:
        per = np.array([15, 0, 2, 13, 15], np.uint8)[:n] | np.uint8(0x30)
        some = 0
        for kw, scale in ((nets["R"][1], 1.0), (random_net(T, 5), 1e9)):
            for net_seats in (15, 0):
                for salt, seats, per_game in ((3, 15, None), (9, 0, per)):
                    a, b = [], []
                    want = existing_launch(env, kw, worlds, sets, net_seats, salt, seats, per_game, a)
                    got = value_launch(env, kw, worlds, sets, net_seats, 13, scale, salt, seats, per_game, scratch_out=b)
                    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), (net_seats, salt, seats)
                    assert a[0].tobytes() == b[0].tobytes(), "the final scratch"
                    some += int(want[0].any())
        assert some >= 4
    finally:
        env.close()


def check_model(env, nets, games, worlds, sets, depth, name, net_seats, info, tag):
    for scale in C.SCALES:
        want = FV.exchange_outputs(games, C.X_SEED, C.SALT, 15, worlds, sets, info, scale)
        got = value_launch(env, nets[name][1], worlds, sets, net_seats, depth, scale)
        assert_equal(got, want, tag + (scale,))
    return got


@pytest.mark.parametrize("mix", list(C.X_MIXES))
def test_integer_weights_against_the_model(T, nets, mix):
    """37 games, 2 worlds, 2 discard sets (up to 888 item slots) on the four single-contract envs and the Bot's mix: depths
    1, 2, 3 and 12 with the sets R, P and V, net_seats 15, 0 and a set without (game 0's) declarer, at value_scale 1, 0.5
    and 1e9 — sum_out, choice_out and discards_out EQUAL the model; the choice is the first row at the maximum of the
    declarer's summed V (tests/playout_front_net_model.exchange_choice inside the model)."""
    n, worlds, sets = C.X_WIDE
    env = make_env(T, n, C.X_MIXES[mix])
    try:
        assert_games(env, C.exchange_games(mix, n))
        for depth, name, choice in C.exchange_plan(mix):
            games, net_seats, info = C.exchange_model(mix, n, worlds, sets, depth, name, choice)
            got = check_model(env, nets, games, worlds, sets, depth, name, net_seats, info, (mix, depth, name, net_seats))
            assert got[0].any()
    finally:
        env.close()


def test_small_shapes_seat_sets_and_games_that_do_not_wait(T, nets):
    """n = 5, worlds = 3, sets = 2 (180 slots: a full tile and a partial one) and n = 1 on the Bot's mix — a Klop that does
    not wait among the five: -1 / 255 —; then per-game seat sets that leave declarers outside (zero sums, the Bot's own
    exchange) and the empty set, against the model."""
    from oracle import tarok_spec as S
    _, worlds, sets = C.X_SHAPE
    for n in (5, 1):
        env = make_env(T, n, S.MIX_BOT)
        try:
            assert_games(env, C.exchange_games("bot", n))
            for m, depth, name, choice in C.X_SMALL:
                if m == n:
                    games, net_seats, info = C.exchange_model("bot", n, worlds, sets, depth, name, choice)
                    got = check_model(env, nets, games, worlds, sets, depth, name, net_seats, info, (n, depth, name, net_seats))
            if n == 5:
                waiting = ((env.state()[9] >> U(52)) & U(3)) == 1
                assert waiting.sum() == 4 and (got[1][~waiting] == -1).all() and (got[2][~waiting] == 255).all() and (got[1][waiting] >= 0).all()
                per = np.array([15, 0, 2, 13, 15], np.uint8) | np.uint8(0x30)
                games = C.with_sets(C.exchange_games("bot", 5), per)
                W, kw = nets["V"]
                for seats, per_game, gs in ((0, per, games), (0, None, C.exchange_games("bot", 5))):
                    want = FV.playout_exchange(gs, C.X_SEED, 9, seats, worlds, sets, W, 15, 2, 0.5)[:3]
                    got = value_launch(env, kw, worlds, sets, 15, 2, 0.5, 9, seats, per_game)
                    assert_equal(got, want, ("sets", per_game is None))
                    declarer = np.array(C.declarers(gs))
                    out = ((per if per_game is not None else np.zeros(5, np.uint8)).astype(np.int64) >> declarer) & 1 == 0
                    assert not got[0][out].any() and (per_game is None or got[0][~out & waiting].any())
                outs = ("sum", "choice", "discards")
                full = dict(zip(outs, value_launch(env, kw, worlds, sets, 15, 2, 0.5, 9, 0, per)))
                for one in outs:                                         # one output at a time: the same bytes
                    alone = dict(zip(outs, value_launch(env, kw, worlds, sets, 15, 2, 0.5, 9, 0, per, want=(one,))))
                    assert alone[one].tobytes() == full[one].tobytes(), one
        finally:
            env.close()


@pytest.mark.parametrize("depth", [1, 3])
def test_random_weights_give_policy_mlps_value_bits(T, depth):
    """Random bf16 weights, net_seats = 0: the Bot plays, so the model's stop positions are exact for any weights.  They go
    into a twin env through the canonical lanes; tarok_policy_mlp's value_out there, formed into V on the host in float32,
    IS the launch's sum in the declarer's column, and the other three columns are 0 (every item stops)."""
    from oracle import tarok_spec as S
    kw = random_net(T, 11 + depth)
    n, worlds, sets = C.X_SHAPE
    scale = 70.0
    env = make_env(T, n, S.MIX_BOT)
    try:
        got, _, _ = value_launch(env, kw, worlds, sets, 0, depth, scale)
    finally:
        env.close()
    info = FV.exchange_info(C.exchange_games("bot", n), C.X_SEED, C.SALT, 15, worlds, sets, C.weight_sets()["P"], 0, depth)
    assert len(info) >= 24 and all(d["stopped"] for _, d in info)
    twin = T.TarokVecEnv(len(info), seed=C.X_SEED, mix=S.MIX_ALL)
    try:
        twin.reset()
        twin.set_state(np.stack([d["at"].lanes() for _, d in info], axis=1))
        value = twin.policy_mlp(kw, twin.legal_actions().words)[2].cpu().numpy()
    finally:
        twin.close()
    want, Vs = np.zeros((n, 6 * sets, 4), np.int64), set()
    for ((g, r, w), d), v in zip(info, value):
        V = FV.points(v, scale)
        Vs.add(V)
        want[g, r, d["viewer"]] += V
    assert len(Vs) >= 3 and (got == want).all(), np.nonzero(got != want)


def test_a_captured_launch_replays_with_the_weights_in_place(T, nets):
    """A launch captured into a graph, then the weights overwritten in place: the replay equals the eager launch with the
    new weights."""
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 37, S.MIX_BOT)
    try:
        kw, other = [t.clone() for t in nets["V"][1]], nets["P"][1]
        env.playout_exchange_net_scratch(2, 2)                    # allocated before the capture
        outs = [torch.zeros((37, 12, 4), dtype=torch.int32, device="cuda"), torch.zeros(37, dtype=torch.int8, device="cuda"),
                torch.zeros((37, 3), dtype=torch.uint8, device="cuda")]
        eager = lambda w: [t.cpu() for t in env.playout_exchange_net_value(w, 2, 2, 2, 0.5, salt=4)]
        first = eager(kw)
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_exchange_net_value(kw, 2, 2, 2, 0.5, salt=4, sum_out=outs[0], choice_out=outs[1], discards_out=outs[2])
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


def test_python_surface_and_arguments(T, nets):
    """playout_exchange_net_value equals the direct C call; depth=None IS playout_exchange_net; every TAROK_EINVAL."""
    import torch
    from oracle import tarok_spec as S
    env = make_env(T, 5, S.MIX_BOT)
    try:
        kw = nets["V"][1]
        want = value_launch(env, kw, 3, 2, 10, 2, 0.5, salt=2)
        got = env.playout_exchange_net_value(kw, 3, 2, 2, 0.5, net_seats=10, salt=2)
        assert all((g.cpu().numpy() == w).all() for g, w in zip(got, want))
        old, off = env.playout_exchange_net(kw, 3, 2, net_seats=10, salt=2), env.playout_exchange_net_value(kw, 3, 2, None, net_seats=10, salt=2)
        assert all(torch.equal(a, b) for a, b in zip(old, off))
        scr = env.playout_exchange_net_scratch(3, 2)
        p = env._p
        ok = dict(env=env._h, worlds=3, sets=2, seats=15, net=15, depth=1, scale=70.0, w=[p(t) for t in kw], scr=p(scr), size=scr.numel(),
                  out=p(got[0]))

        def rc(**ch):
            a = dict(ok, **ch)
            return env.L.tarok_playout_exchange_net_value(a["env"], a["worlds"], a["sets"], 0, a["seats"], None, a["net"], a["depth"], a["scale"],
                                                          *a["w"], a["scr"], a["size"], a["out"], None, None, env._stream())
        assert rc() == 0 and rc(depth=13) == 0
        torch.cuda.synchronize()
        bad = [dict(env=None), dict(worlds=0), dict(worlds=65), dict(sets=0), dict(sets=9), dict(seats=16), dict(seats=-1), dict(net=16),
               dict(net=-1), dict(scr=None), dict(size=scr.numel() - 1), dict(scr=scr.data_ptr() + 8), dict(out=None), dict(depth=0),
               dict(depth=14), dict(depth=-1), dict(scale=0.0), dict(scale=-70.0), dict(scale=float("inf")), dict(scale=float("nan"))]
        bad += [dict(w=ok["w"][:i] + [None] + ok["w"][i + 1:]) for i in range(6)]
        for ch in bad:
            assert rc(**ch) == -1, ch
        with pytest.raises(ValueError):
            env.playout_exchange_net_value(kw, 3, 2, 14)
    finally:
        env.close()
