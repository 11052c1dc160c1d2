"""GPU: tarok_playout_bids_net_value (every bid's — and the pass's — net playouts stopped at the viewer's depth-th decision,
the value head's estimate in the viewer's column) checked exactly — integers against integers: depth 13 against the bytes of
tarok_playout_bids_net and, with the pass at net_seats = 0, of tarok_playout_bids_pass(worlds, 1); exactly summable integer
weights at depths 1, 2, 3 and 12 against the model of tests/playout_front_net_value_model.py over the plan of
tests/playout_front_net_value_cases.py, with and without the pass; random bf16 weights at depth 13 with the pass against a
replay of every live item, row 19's included, on a twin env through the shipped greedy tarok_policy_step; a captured FIRST
call; every TAROK_EINVAL; the two learners with net_depth.  Every launch writes into guard bands (tests/guarded.py) over a
guarded scratch and leaves the env and its counters as they were.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_bids_net_value.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
import playout_front_net_value_cases as C
import playout_front_net_value_model as FV
from gpu_harness import T, U, item_arrays, random_net  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = C.B_SEED, C.B_OFFSET, C.B_EPISODE
LIVE = 0x8000800080008000
make_env = functools.partial(H.make_bid_env, seed=SEED, offset=OFFSET)   # (T, n, **kw): NOT reset, bidding comes first
replay_on_a_twin = functools.partial(H.replay_on_a_twin, seed=43)


@pytest.fixture(scope="module")
def nets(T):
    """R, P and V of tests/playout_net_value_cases.weight_sets as (float64 set, kernel set)."""
    import policy_exact_ref as PE
    return {k: (W, PE.kernel_weights(T, W)) for k, W in C.weight_sets().items()}


def value_launch(env, kw, worlds, net_seats, depth, scale, pass_value, contracts=C.DEFAULT, deals=None, salt=C.SALT, seats=15, per_game=None,
                 scratch_out=None):
    """One launch into a guarded sum_out [n, 4, 20] i32 over a guarded scratch."""
    from guarded import Guarded
    g_sum = Guarded("sum_out", 1, env.n, np.int32, inner=(4, 20), device="cuda")
    H._launch(env, "tarok_playout_bids_net_value",
              [int(EPISODE), H.dev_u8(deals), int(worlds), int(contracts), int(salt), int(seats), H.dev_u8(per_game), int(net_seats), int(depth),
               float(scale), int(pass_value)] + list(kw),
              [g_sum], ("tarok_playout_bids_net_scratch", (int(worlds),), env.n * 80 * worlds * 48 + env.n * 40), True,
              (worlds, contracts, net_seats, seats, depth, scale, pass_value), scratch_out)
    return H.read_words(g_sum)


def assert_sums(got, want, tag):
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, (tag, "sums differ", bad[:8], got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("n,worlds,contracts", [(2, 1, C.DEFAULT), (5, 3, C.ALL)])
def test_depth_13_gives_the_existing_launches_bytes(T, nets, n, worlds, contracts):
    """depth = 13 never stops an item.  pass_value = 0: tarok_playout_bids_net's bytes, the final scratch included, with the
    integer set R and with random weights at net_seats 15 and 0, at any value_scale.  pass_value = 1 at net_seats = 0:
    tarok_playout_bids_pass(worlds, 1)'s bytes, all twenty rows."""
    env = make_env(T, n)
    try:
        per = np.array([6, 0, 15, 9, 1], np.uint8)[:n] | np.uint8(0x50)
        passes = 0
        for kw, scale in ((nets["R"][1], 1.0), (random_net(T, 7), 1e9)):
            for salt, seats, per_game in ((0, 15, None), (9, 10, None), (9, 15, per), (9, 0, None)):
                for net_seats in (15, 0):
                    a, b = [], []
                    want = H.launch_bids_net(env, kw, worlds, net_seats, contracts, None, salt, seats, per_game, EPISODE, a)
                    got = value_launch(env, kw, worlds, net_seats, 13, scale, 0, contracts, None, salt, seats, per_game, b)
                    assert got.tobytes() == want.tobytes() and a[0].tobytes() == b[0].tobytes(), (salt, seats, net_seats)
                    assert want.any() == (seats != 0) and not got[:, :, 19].any()
                want = H.launch_bids(env, worlds, 1, contracts, None, salt, seats, per_game, episode=EPISODE, entry="tarok_playout_bids_pass")
                got = value_launch(env, kw, worlds, 0, 13, scale, 1, contracts, None, salt, seats, per_game)
                assert got.tobytes() == want.tobytes() and (seats != 0 or not got.any()), (salt, seats, "pass")
                passes += int(got[:, :, 19].any())
        assert passes >= 2                                           # (a pass often scores 0: the declarer's opponents do)
    finally:
        env.close()


@pytest.mark.parametrize("row", C.B_PLAN, ids=lambda r: "n%d-w%d-c%x-d%d-%s-s%d-p%d" % r)
def test_integer_weights_against_the_model(T, nets, row):
    """The plan's launches — n = 2, W = 1; n = 5, W = 3 with all ten contracts; n = 16 — at depths 1, 2, 3 and 12 with the
    sets R, P and V, with and without the pass, at value_scale 1, 0.5 and 1e9: sum_out EQUALS the model."""
    n, worlds, contracts, depth, name, net_seats, pass_value = row
    deals, info = C.bid_model(*row)
    env = make_env(T, n)
    try:
        for scale in C.SCALES:
            got = value_launch(env, nets[name][1], worlds, net_seats, depth, scale, pass_value, contracts)
            assert_sums(got, FV.bid_sums(n, info, scale), row + (scale,))
            assert pass_value or not got[:, :, 19].any()
        assert got[:, :, :13].any() and got[:, :, 19].any() == bool(pass_value)      # (at 1e9 every V that is not 0 is +-32767)
    finally:
        env.close()


def test_seat_sets_and_a_deals_array(T, nets):
    """The empty seat set (all zeros, the pass row too), per-game sets (bits 4..7 ignored) and a user `deals` array with one
    invalid row (zeros, no pass item), with the pass, against the model."""
    n = 8
    W, kw = nets["V"]
    env = make_env(T, n)
    try:
        assert not value_launch(env, kw, 2, 15, 2, 1.0, 1, seats=0).any()
        per = np.array([(5 * g + 3) & 15 for g in range(n)], np.uint8) | np.uint8(16)
        want, _ = FV.playout_bids(C.with_sets(C.bid_deals(n), per), SEED, 11, 9, 2, C.DEFAULT, W, 5, 2, 0.5, True)
        got = value_launch(env, kw, 2, 5, 2, 0.5, 1, salt=11, seats=9, per_game=per)
        assert_sums(got, want, "per-game sets")
        for g in range(n):
            for v in range(4):
                assert got[g, v].any() == bool((int(per[g]) >> v) & 1), (g, v)
        rng = np.random.default_rng(5)
        other = np.stack([rng.permutation(54) for _ in range(n)]).astype(np.uint8)
        other[3, 7] = other[3, 8]                                        # a card twice
        rows = [(other[g].tolist(), EPISODE, OFFSET + g, None) for g in range(n)]
        want, _ = FV.playout_bids(rows, SEED, 2, 15, 2, C.DEFAULT, W, 15, 1, 1.0, True)
        got = value_launch(env, kw, 2, 15, 1, 1.0, 1, deals=other, salt=2)
        assert_sums(got, want, "deals given")
        assert not got[3].any() and got[0].any() and got[4, :, 19].any()
    finally:
        env.close()


def test_random_weights_against_a_twin_replay(T):
    """Random bf16 weights, net_seats = 15, depth 13 with the pass, 3 deals, 2 worlds, all ten contracts.  Every live item —
    the option's game, and the pass item's game, on the model's world after the Bot's exchange — is played on a twin env
    by the greedy tarok_policy_step and must score what the item's result word says; the item's key in the scratch is the
    model's; every other slot's word is 0."""
    kw = random_net(T, 29)
    n, worlds = 3, 2
    env = make_env(T, n)
    try:
        scr = []
        got = value_launch(env, kw, worlds, 15, 13, 70.0, 1, C.ALL, salt=1, scratch_out=scr)
    finally:
        env.close()
    where, view, hs, keys = [], [], [], []
    for g, (perm, ep, gidx, _) in enumerate(C.bid_deals(n)):
        for v, r, w, h, key, viewer, _ in FV.bid_items(perm, ep, SEED, 1, gidx, 15, worlds, C.ALL, True):
            where.append(((g * 4 + v) * 20 + r) * worlds + w); view.append(viewer); hs.append(h); keys.append(key)
    assert len(hs) == n * 4 * 20 * worlds
    items = n * 80 * worlds
    ikey, ires, words = item_arrays(scr[0][:items * 48], items)
    final = replay_on_a_twin(T, kw, hs)
    where, view = np.array(where), np.array(view)
    assert (ikey[where] == np.array(keys, np.uint64)).all(), "an item's key"
    assert (ires[where] == final).all(), np.nonzero((ires[where] != final).any(axis=1))[0]
    assert (words & ~U(3) != U(LIVE)).all()
    want = np.zeros(n * 80, np.int64)
    np.add.at(want, where // worlds, final[np.arange(len(view)), view])
    assert (got.reshape(-1) == want).all() and got.any()
    env = make_env(T, n)                                             # without the pass: row 19's slots hold 0
    try:
        scr = []
        value_launch(env, kw, worlds, 15, 13, 70.0, 0, C.ALL, salt=1, scratch_out=scr)
    finally:
        env.close()
    _, _, words0 = item_arrays(scr[0][:items * 48], items)
    row19 = (np.arange(items) // worlds) % 20 == 19
    assert (words0[row19] == 0).all() and (words0[~row19] == words[~row19]).all()


def test_a_captured_first_launch_replays_with_the_weights_in_place(T, nets):
    """The FIRST launch of an env captured into a graph — nothing is allocated in the call —, then the weights changed in
    place: the replay gives the eager launch's bytes for the NEW weights."""
    import torch
    env, twin = make_env(T, 16), make_env(T, 16)
    try:
        kw, other = [t.clone() for t in nets["V"][1]], nets["P"][1]
        env.playout_bids_net_scratch(2)                           # allocated before the capture
        out = torch.zeros((16, 4, 20), dtype=torch.int32, device="cuda")
        old = twin.playout_bids_net_value(kw, EPISODE, 2, 2, 0.5, pass_value=True, salt=4).cpu()
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_bids_net_value(kw, EPISODE, 2, 2, 0.5, pass_value=True, salt=4, sum_out=out)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), old)
        for t, o in zip(kw, other):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        new = twin.playout_bids_net_value(other, EPISODE, 2, 2, 0.5, pass_value=True, salt=4).cpu()
        assert torch.equal(out.cpu(), new) and not torch.equal(new, old)
    finally:
        env.close()
        twin.close()


def test_python_surface_and_arguments(T, nets):
    """playout_bids_net_value equals the direct C call; depth=None IS playout_bids_net; every TAROK_EINVAL."""
    import torch
    env = make_env(T, 5)
    try:
        kw = nets["V"][1]
        want = value_launch(env, kw, 3, 10, 2, 0.5, 1, C.ALL, salt=2)
        got = env.playout_bids_net_value(kw, EPISODE, 3, 2, 0.5, pass_value=True, net_seats=10, contracts=C.ALL, salt=2)
        assert got.dtype == torch.int32 and tuple(got.shape) == (5, 4, 20) and (got.cpu().numpy() == want).all()
        assert torch.equal(env.playout_bids_net(kw, EPISODE, 3, net_seats=10, salt=2), env.playout_bids_net_value(kw, EPISODE, 3, None, net_seats=10, salt=2))
        scr = env.playout_bids_net_scratch(3)
        p = env._p
        ok = dict(env=env._h, worlds=3, contracts=C.ALL, seats=15, net=15, depth=1, scale=70.0, pas=1, w=[p(t) for t in kw], scr=p(scr),
                  size=scr.numel(), out=p(got))

        def rc(**ch):
            a = dict(ok, **ch)
            return env.L.tarok_playout_bids_net_value(a["env"], EPISODE, None, a["worlds"], a["contracts"], 0, a["seats"], None, a["net"], a["depth"],
                                                      a["scale"], a["pas"], *a["w"], a["scr"], a["size"], a["out"], env._stream())
        assert rc() == 0 and rc(depth=13, pas=0) == 0
        torch.cuda.synchronize()
        bad = [dict(env=None), dict(worlds=0), dict(worlds=65), dict(contracts=0), dict(contracts=0x400), dict(seats=16), dict(seats=-1),
               dict(net=16), dict(net=-1), dict(scr=None), dict(size=scr.numel() - 1), dict(scr=scr.data_ptr() + 8), dict(out=None),
               dict(depth=0), dict(depth=14), dict(depth=-1), dict(scale=0.0), dict(scale=-70.0), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(pas=2), dict(pas=-1)]
        bad += [dict(w=ok["w"][:i] + [None] + ok["w"][i + 1:]) for i in range(6)]
        for ch in bad:
            assert rc(**ch) == -1, ch
        with pytest.raises(ValueError):
            env.playout_bids_net_value(kw, EPISODE, 3, 14)
        with pytest.raises(ValueError):
            env.playout_bids_net_value(kw, EPISODE, 3, None, pass_value=True)
    finally:
        env.close()


def test_the_learners_with_a_value_teacher(T):
    """BidLearner(net=, net_depth=2, pass_value=True) and ExchangeLearner(net=, net_depth=2) at n = 64: one collect() gives
    the rows of the eager value launch on a twin env — not the full-depth launch's —, and a step runs."""
    import torch
    from oracle import tarok_spec as S
    from tarok_amd.bidding import BidLearner
    from tarok_amd.exchange import ExchangeLearner
    net = random_net(T, 3)
    env, twin = T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT), T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT)
    try:
        learner = BidLearner(env, worlds=2, seed=5, net=net, net_seats=15, net_depth=2, net_value_scale=35.0, pass_value=True)
        fw, sums, playouts = learner.collect(3)
        assert playouts == 2 and tuple(sums.shape) == (64, 4, 20)
        want = twin.playout_bids_net_value(net, 3, 2, 2, 35.0, pass_value=True, net_seats=15, salt=5)
        assert torch.equal(sums, want) and sums[:, :, 19].any()
        assert not torch.equal(sums, twin.playout_bids_net(net, 3, 2, net_seats=15, salt=5))
        loss = learner.step(fw, sums, playouts)
        assert np.isfinite(loss) and np.isfinite(learner.iterate())
        xl = ExchangeLearner(env, worlds=2, discard_sets=2, seed=5, net=net, net_seats=15, net_depth=2, net_value_scale=35.0)
        fw, sums, cands, playouts = xl.collect(3)
        twin.reset(episode=3, defer_exchange=True)
        want, _, _ = twin.playout_exchange_net_value(net, 2, 2, 2, 35.0, net_seats=15, salt=5)
        assert playouts == 2 and torch.equal(sums, want) and sums.any()
        assert not torch.equal(sums, twin.playout_exchange_net(net, 2, 2, net_seats=15, salt=5)[0])
        loss = xl.step(fw, sums, cands, playouts)
        assert np.isfinite(loss) and np.isfinite(xl.iterate())
    finally:
        env.close()
        twin.close()
