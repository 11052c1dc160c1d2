"""GPU: tarok_playout_bids_net (every bid valued by playouts that a policy network plays) checked exactly — integers
against integers: net_seats = 0 against tarok_playout_bids' bytes at samples = 1; exactly summable integer weights
against the model of tests/playout_front_net_model.py; random bf16 weights against a replay of every live item on a twin
env through the shipped greedy tarok_policy_step, result word by result word; a captured graph against the eager launch
after the weights changed in place; every TAROK_EINVAL; the learner and the evaluation built on the launch.  Every case
checks every row of sum_out inside guard bands (tests/guarded.py), with the scratch between guards too, and that the
env's state is untouched.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_bids_net.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T, U, dev_u8, item_arrays, nets, random_net  # noqa: F401  (T, nets: the module fixtures)

pytestmark = pytest.mark.gpu

SEED, OFFSET, EPISODE = 2, 3000, 4                # tests/test_gpu_playout_bids.py's: the same deals
DEFAULT, ALL = 0x00F, 0x3FF
LIVE = 0x8000800080008000
make_env = functools.partial(H.make_bid_env, seed=SEED, offset=OFFSET)   # (T, n, **kw): NOT reset, bidding comes first
perms_of = functools.partial(H.perms_of, seed=SEED, offset=OFFSET, episode=EPISODE)
replay_on_a_twin = functools.partial(H.replay_on_a_twin, seed=43)        # (the twin's seed of tests/test_gpu_playout_exchange_net.py)


def bot_launch(env, worlds, samples, contracts=DEFAULT, deals=None, salt=0, seats=15, per_game=None, episode=EPISODE):
    """One tarok_playout_bids into a guarded sum_out: [n, 4, 20] i32."""
    return H.launch_bids(env, worlds, samples, contracts, deals, salt, seats, per_game, episode=episode, entry="tarok_playout_bids")


def net_launch(env, kw, worlds, net_seats, contracts=DEFAULT, deals=None, salt=0, seats=15, per_game=None, episode=EPISODE,
               scratch_out=None):
    """One launch into a guarded sum_out [n, 4, 20] i32 over a guarded scratch.  scratch_out: a list that receives the
    scratch's bytes after the launch."""
    return H.launch_bids_net(env, kw, worlds, net_seats, contracts, deals, salt, seats, per_game, episode, scratch_out)


def deals_of(perms, per_game=None):
    return [(perms[g], EPISODE, OFFSET + g, None if per_game is None else int(per_game[g]) & 15) for g in range(len(perms))]


def check_model(env, W, kw, perms, worlds, net_seats, contracts=DEFAULT, salt=0, seats=15, per_game=None, deals=None, tag=None):
    import playout_front_net_model as FM
    want = FM.playout_bids(deals_of(perms, per_game), SEED, salt, seats, worlds, contracts, W, net_seats)
    got = net_launch(env, kw, worlds, net_seats, contracts, deals, salt, seats, per_game)
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, (tag, "sums differ", bad[:8], got[bad[0]].tolist(), want[bad[0]].tolist())
    return got


@pytest.mark.parametrize("n,worlds,contracts", [(2, 1, DEFAULT), (5, 3, ALL)])
def test_no_net_seat_gives_the_bot_launch_bytes(T, nets, n, worlds, contracts):
    """net_seats = 0: tarok_playout_bids(worlds, 1) to the byte.  n = 2, worlds = 1: 160 item slots, one full tile of 128
    and a partial one; n = 5, worlds = 3 with all ten contracts: 1,200 slots."""
    env = make_env(T, n)
    try:
        per = np.array([6, 0, 15, 9, 1], np.uint8)[:n] | np.uint8(0x50)
        for salt, seats, per_game in ((0, 15, None), (9, 10, None), (9, 15, per), (9, 0, None)):
            want = bot_launch(env, worlds, 1, contracts, None, salt, seats, per_game)
            got = net_launch(env, nets["R"][1], worlds, 0, contracts, None, salt, seats, per_game)
            assert want.any() == (seats != 0) and got.tobytes() == want.tobytes(), (salt, seats)
            assert not got[:, :, 19].any()
    finally:
        env.close()


@pytest.mark.parametrize("n,contracts,net_seats", [(16, DEFAULT, 15), (16, DEFAULT, 1), (16, DEFAULT, 10), (8, ALL, 15), (8, ALL, 10)])
def test_integer_weights_against_the_model(T, nets, n, contracts, net_seats):
    """16 deals at the default contracts (2,560 item slots, 1,664 live) and 8 deals with all ten (1,216 live: the Solos,
    the Beracs — playouts of one tile that end at different cards — and Solo_brez), 2 worlds, weight set R."""
    env = make_env(T, n)
    try:
        got = check_model(env, *nets["R"], perms_of(n), 2, net_seats, contracts, salt=3, tag=(n, contracts, net_seats))
        assert got[:, :, :13].any(axis=(0, 1)).all() and got[:, :, 13:19].any() == (contracts == ALL) and not got[:, :, 19].any()
    finally:
        env.close()


def test_seat_sets_deals_and_the_network_in_the_loop(T, nets):
    """The empty seat set (all zeros), per-game sets (bits 4..7 ignored), a user `deals` array with one invalid row, and
    sums that differ between net_seats = 0 and 15 and between the two weight sets."""
    n = 8
    perms = perms_of(n)
    env = make_env(T, n)
    try:
        kw = nets["R"][1]
        assert not net_launch(env, kw, 2, 15, seats=0).any()
        per = np.array([(5 * g + 3) & 15 for g in range(n)], np.uint8) | np.uint8(16)
        got = check_model(env, *nets["R"], perms, 2, 5, salt=11, seats=9, per_game=per, tag="per-game sets")
        for g in range(n):
            for v in range(4):
                assert got[g, v].any() == bool((int(per[g]) >> v) & 1), (g, v)
        rng = np.random.default_rng(5)
        other = np.stack([rng.permutation(54) for _ in range(n)]).astype(np.uint8)
        other[3, 7] = other[3, 8]                                        # a card twice
        got = check_model(env, *nets["R"], [other[g].tolist() for g in range(n)], 2, 15, salt=2, deals=other, tag="deals given")
        assert not got[3].any() and got[0].any() and got[4].any()
        sb = net_launch(env, kw, 2, 0)
        sr = net_launch(env, kw, 2, 15)
        sp = check_model(env, *nets["P"], perms, 2, 15, tag="set P")
        assert (sb != sr).any() and (sr != sp).any()
    finally:
        env.close()


def test_random_weights_against_a_twin_replay(T):
    """Random bf16 weights, net_seats = 15, 3 deals, 2 worlds, all ten contracts.  Every live item — the option's game on
    the model's world after the Bot's exchange — is played on a twin env by the greedy tarok_policy_step and must score
    what the item's result word says; the item's key in the scratch is the model's; every other slot's word is 0."""
    import playout_front_net_model as FM
    kw = random_net(T, 23)
    n, worlds = 3, 2
    env = make_env(T, n)
    try:
        scr = []
        got = net_launch(env, kw, worlds, 15, ALL, salt=1, scratch_out=scr)
    finally:
        env.close()
    where, view, hs, keys = [], [], [], []
    for g, (perm, ep, gidx, _) in enumerate(deals_of(perms_of(n))):
        for v, r, w, h, key in FM.bid_items(perm, ep, SEED, 1, gidx, 15, worlds, ALL):
            where.append(((g * 4 + v) * 20 + r) * worlds + w); view.append(v); hs.append(h); keys.append(key)
    assert len(hs) == n * 4 * 19 * worlds
    items = n * 80 * worlds
    ikey, ires, words = item_arrays(scr[0][:items * 48], items)
    final = replay_on_a_twin(T, kw, hs)
    where, view = np.array(where), np.array(view)
    assert (ikey[where] == np.array(keys, np.uint64)).all(), "an item's key"
    assert (ires[where] == final).all(), np.nonzero((ires[where] != final).any(axis=1))[0]
    rest = np.setdiff1d(np.arange(items), where)
    assert rest.size == n * 4 * worlds and (words[rest] == 0).all() and (words != U(LIVE)).all()
    want = np.zeros(n * 80, np.int64)
    np.add.at(want, where // worlds, final[np.arange(len(view)), view])
    assert (got.reshape(-1) == want).all()


def test_a_captured_launch_replays_with_the_weights_in_place(T):
    """The FIRST launch of an env captured into a graph — nothing is allocated in the call —, then the weights changed in
    place: the replay gives the eager launch's bytes for the NEW weights."""
    import torch
    env, twin = make_env(T, 16), make_env(T, 16)
    try:
        kw, other = random_net(T, 1), random_net(T, 2)
        env.playout_bids_net_scratch(2)                           # allocated before the capture
        out = torch.zeros((16, 4, 20), dtype=torch.int32, device="cuda")
        old = twin.playout_bids_net(kw, EPISODE, 2, salt=4).cpu()
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_bids_net(kw, EPISODE, 2, salt=4, sum_out=out)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), old)
        for t, o in zip(kw, other):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        new = twin.playout_bids_net(other, EPISODE, 2, salt=4).cpu()
        assert torch.equal(out.cpu(), new) and not torch.equal(new, old)
    finally:
        env.close()
        twin.close()


def test_python_surface_and_arguments(T, nets):
    """playout_bids_net equals the direct C call; the scratch is cached per `worlds`; bad arguments are TAROK_EINVAL."""
    import torch
    env = make_env(T, 5)
    try:
        kw = nets["R"][1]
        want = net_launch(env, kw, 3, 10, ALL, salt=2)
        got = env.playout_bids_net(kw, EPISODE, 3, net_seats=10, contracts=ALL, salt=2)
        assert got.dtype == torch.int32 and tuple(got.shape) == (5, 4, 20) and (got.cpu().numpy() == want).all()
        assert env.playout_bids_net_scratch(3) is env.playout_bids_net_scratch(3) and env.playout_bids_net_scratch(2) is not env.playout_bids_net_scratch(3)
        scr = env.playout_bids_net_scratch(3)
        p = env._p
        ok = dict(worlds=3, contracts=ALL, seats=15, net=15, w=[p(t) for t in kw], scr=p(scr), size=scr.numel(), out=p(got))

        def rc(**ch):
            a = dict(ok, **ch)
            return env.L.tarok_playout_bids_net(env._h, EPISODE, None, a["worlds"], a["contracts"], 0, a["seats"], None, a["net"], *a["w"],
                                                a["scr"], a["size"], a["out"], env._stream())
        assert rc() == 0
        torch.cuda.synchronize()
        bad = [dict(worlds=0), dict(worlds=65), dict(contracts=0), dict(contracts=0x400), dict(seats=16), dict(seats=-1), dict(net=16),
               dict(net=-1), dict(scr=None), dict(size=scr.numel() - 1), dict(scr=scr.data_ptr() + 8), dict(out=None)]
        bad += [dict(w=ok["w"][:i] + [None] + ok["w"][i + 1:]) for i in range(6)]
        for ch in bad:
            assert rc(**ch) == -1, ch
        size = env.L.tarok_playout_bids_net_scratch
        assert [size(env._h, 0), size(env._h, 65), size(None, 1)] == [-1] * 3
        assert env.L.tarok_playout_bids_net(None, EPISODE, None, 3, ALL, 0, 15, None, 15, *ok["w"], ok["scr"], ok["size"], ok["out"], None) == -1
        with pytest.raises(ValueError):
            env.playout_bids_net(kw, EPISODE, 2, net_seats=16)
        with pytest.raises(ValueError):
            env.playout_bids_net(kw, EPISODE, 0)
    finally:
        env.close()


def test_the_bid_learner_with_a_net_teacher(T):
    """BidLearner(net=...) at n = 64: one collect() gives the rows of the eager net launch on a twin env at playouts =
    worlds — not the Bot launch's —, and a step runs."""
    import torch
    from oracle import tarok_spec as S
    from tarok_amd.bidding import BidLearner
    net = random_net(T, 3)
    env, twin = T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT), T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT)
    try:
        learner = BidLearner(env, worlds=2, seed=5, net=net, net_seats=15)
        fw, sums, playouts = learner.collect(3)
        assert playouts == 2 and tuple(sums.shape) == (64, 4, 20)
        want = twin.playout_bids_net(net, 3, 2, net_seats=15, salt=5)
        assert torch.equal(sums, want) and sums.any()
        assert not torch.equal(sums, twin.playout_bids(3, 2, 1, salt=5))
        loss = learner.step(fw, sums, playouts)
        assert np.isfinite(loss) and np.isfinite(learner.iterate())
    finally:
        env.close()
        twin.close()


def test_evaluate_bidding_vs_bot_with_the_network(T):
    """evaluate_bidding_vs_bot(net=..., net_seats="own", cards=...) on 32 games x 1 episode: on every pass the front end's
    sums and its contract, declarer and king are those of the eager launches on a twin env, and pass 0 — the empty set —
    is the Bot-everywhere pass of the plain call."""
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    net = random_net(T, 4)
    seen, plain, bots = [], [], []
    got = EV.evaluate_bidding_vs_bot(2, None, 32, 1, seed=3, salt=2, inspect=seen, net=net, net_seats="own", cards=net)
    EV.evaluate_bidding_vs_bot(2, 1, 32, 1, seed=3, salt=2, inspect=plain)
    EV.evaluate_bidding_vs_bot(2, None, 32, 1, seed=3, salt=2, inspect=bots, net=net, net_seats="own")
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS) and got["deals"] == 32
    twin = T.TarokVecEnv(32, seed=3, mix=S.MIX_BOT)
    try:
        differs = 0
        for rec in seen:
            sums = twin.playout_bids_net(net, 0, 2, net_seats=rec["seats"], salt=2, seats=rec["seats"])
            assert (rec["sums"] == sums.cpu().numpy()).all(), rec["seats"]
            for name, w in zip(("contract", "declarer", "king_suit"), twin.bid_round(0, sums, 2, seats=rec["seats"])):
                assert (rec[name] == w.cpu().numpy()).all(), (rec["seats"], name)
            differs += int((rec["contract"] != seen[0]["contract"]).sum())
        assert differs > 0, "the playout bidder bids otherwise than the Bot somewhere"
    finally:
        twin.close()
    for name in ("start", "contract", "declarer", "king_suit", "scores"):
        assert (seen[0][name] == plain[0][name]).all(), name
    assert (bots[0]["scores"] == plain[0]["scores"]).all()
    assert all((bots[p]["contract"] == seen[p]["contract"]).all() for p in range(5))
    assert any((bots[p]["actions"] != seen[p]["actions"]).any() for p in range(1, 5)), "the network plays the pass's seats"
