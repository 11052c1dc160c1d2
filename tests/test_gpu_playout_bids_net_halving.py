"""GPU: tarok_playout_bids_net_halving (sequential halving over a viewer's bid rows, on the compacted item list) checked
exactly.  One round against tarok_playout_bids_net_list byte for byte, with and without the pass; the schedules (1,1,2),
(2,2,4,8), (4,4,4,4) and (1,3) against an expectation built from list launches at the cumulative ends and walked by
tests/playout_front_halving_model.py — sums, counts and value —, with the inputs ASSERTED to hold a tie at a cut, a unit that
leaves early and a best row that differs from the uniform launch's; Klop only, all ten contracts, seat sets, a deals array with
an invalid row, empty lists, n = 300; the guarded scratch of exactly the header's size and one 16-byte step short; each output
alone, determinism, salt, batch independence; a captured FIRST call; the learner and the evaluation.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_bids_net_halving.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import front_halving_cases as FH
import front_list_cases as F
import gpu_harness as H
import playout_front_halving_model as M
import playout_front_net_value_cases as C
from gpu_harness import T, random_net  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = C.B_SEED, C.B_OFFSET, C.B_EPISODE
make_env = functools.partial(H.make_bid_env, seed=SEED, offset=OFFSET)   # (T, n, **kw): NOT reset, bidding comes first
SCHEDULES = ((1, 1, 2), (2, 2, 4, 8), (4, 4, 4, 4), (1, 3))
NAMES = FH.B_NAMES


@pytest.fixture(scope="module")
def nets(T):
    """The integer set R as a kernel set, and one random bf16 set."""
    import policy_exact_ref as PE
    return dict(R=PE.kernel_weights(T, C.weight_sets()["R"]), random=random_net(T, 19))


def assert_same(got, want, tag):
    for name, g, w in zip(NAMES, got, want):
        assert g.tobytes() == np.ascontiguousarray(w, g.dtype).tobytes(), (tag, name, np.nonzero((g != w).any(axis=(1, 2)))[0][:8])


@pytest.mark.parametrize("n", [1, 17])
def test_one_round_is_the_list_launch(T, nets, n):
    """(W,) against tarok_playout_bids_net_list at worlds = W: depths None, 13, 12, 1, the pass both ways, net_seats 15, 10, 0:
    value_out = sum_out and the count is W on the live rows."""
    env = make_env(T, n)
    try:
        for k, depth in enumerate((None, 13, 12, 1)):
            for pass_value in (0, 1):
                for net_seats in (15, 10, 0):
                    kw = nets["R" if (k + pass_value + net_seats) & 1 else "random"]
                    want = F.bids_list(env, kw, EPISODE, 3, net_seats, depth, pass_value)
                    s, c, v = FH.bids_halving(env, kw, EPISODE, (3,), net_seats, depth, pass_value)
                    assert s.tobytes() == want.tobytes() and v.tobytes() == want.tobytes(), (n, depth, pass_value, net_seats)
                    rows = F.bid_rows(F.DEFAULT, pass_value)
                    assert (c == np.array([3 if (rows >> r) & 1 else 0 for r in range(20)], np.int32)).all(), (n, depth, pass_value)
    finally:
        env.close()


def test_schedules_against_the_walk_over_list_launches(T, nets):
    """Every schedule at depth None and 1, with and without the pass, on 5 deals; Klop only (one arm: one round played) and
    Klop with Solo_tri (two arms: the unit leaves after round 0), Tri alone (four arms: the unit leaves after round 1 where the
    schedule has a third); the inputs hold each case the rule has."""
    tally = FH.Tally()
    env = make_env(T, 5)
    try:
        for schedule in SCHEDULES:
            for depth, pass_value, name, net_seats in ((None, 0, "random", 15), (1, 1, "R", 15), (None, 1, "random", 10), (1, 0, "random", 15)):
                want = FH.expect_bids(env, nets[name], EPISODE, schedule, net_seats, depth, pass_value, tally)
                got = FH.bids_halving(env, nets[name], EPISODE, schedule, net_seats, depth, pass_value)
                assert_same(got, want, (schedule, depth, pass_value, net_seats))
                assert pass_value or not got[1][:, :, 19].any()
            for contracts in (0x001, 0x011):
                early = FH.Tally()
                want = FH.expect_bids(env, nets["random"], EPISODE, schedule, 15, 2, 1, early, contracts=contracts)
                got = FH.bids_halving(env, nets["random"], EPISODE, schedule, 15, 2, 1, contracts=contracts)
                assert_same(got, want, ("few arms", contracts, schedule))
                assert early.units == 20 and early.early == 20 and (got[1][:, :, 0] == schedule[0]).all() and (got[1][:, :, 19] == schedule[0]).all()
            four = FH.Tally()                                    # Tri alone: 4 arms -> 2 -> 1: the unit leaves before a third round
            want = FH.expect_bids(env, nets["R"], EPISODE, schedule, 15, 1, 0, four, contracts=0x002)
            assert_same(FH.bids_halving(env, nets["R"], EPISODE, schedule, 15, 1, 0, contracts=0x002), want, ("tri", schedule))
            assert four.units == 20 and four.early == (20 if len(schedule) > 2 else 0), (schedule, four)
        print(tally)
        # 13 arms stay above one through four rounds (13, 7, 4, 2): at the default contracts no unit can leave early, so that
        # case is asserted on the few-arm contracts above, each on its own; the ties and the changed best rows are the data's
        assert tally.ties > 0 and tally.early == 0 and tally.differs > 0, tally
    finally:
        env.close()


def test_contracts_seat_sets_a_deals_array_and_empty_lists(T, nets):
    """All ten contracts; seats 1 and 6, per-game sets; a `deals` array with an invalid row; the empty seat set; n = 300 (1,200
    units: across the 256-unit scan block)."""
    tally = FH.Tally()
    n, kw = 8, nets["random"]
    env = make_env(T, n)
    try:
        per = np.array([(5 * g + 3) & 15 for g in range(n)], np.uint8) | np.uint8(16)
        rng = np.random.default_rng(5)
        other = np.stack([rng.permutation(54) for _ in range(n)]).astype(np.uint8)
        other[3, 7] = other[3, 8]                                        # a card twice
        for kw_launch in (dict(contracts=F.ALL), dict(seats=1), dict(seats=6), dict(seats=9, per_game=per), dict(deals=other, salt=2), dict(seats=0)):
            want = FH.expect_bids(env, kw, EPISODE, (1, 1, 2), 15, 1, 1, tally, **kw_launch)
            got = FH.bids_halving(env, kw, EPISODE, (1, 1, 2), 15, 1, 1, **kw_launch)
            assert_same(got, want, sorted(kw_launch))
            if "deals" in kw_launch:
                assert not got[0][3].any() and not got[1][3].any() and got[1][0].any()
        assert not got[0].any() and not got[1].any() and not got[2].any()          # the empty seat set
    finally:
        env.close()
    env = make_env(T, 300)
    try:
        want = FH.expect_bids(env, nets["R"], EPISODE, (1, 3), 15, 1, 0, tally, seats=5)
        assert_same(FH.bids_halving(env, nets["R"], EPISODE, (1, 3), 15, 1, 0, seats=5), want, "300")
    finally:
        env.close()


def test_the_scratch_each_output_alone_determinism_salt_and_batch_independence(T, nets):
    import torch
    schedule, kw = (2, 2, 4), nets["random"]
    env, two = make_env(T, 5), make_env(T, 2)
    try:
        a, b = [], []
        full = FH.bids_halving(env, kw, EPISODE, schedule, 15, 1, 1, scratch_out=a)         # (a guarded scratch of exactly the header's size)
        again = FH.bids_halving(env, kw, EPISODE, schedule, 15, 1, 1, scratch_out=b)
        assert_same(again, full, "twice")
        assert a[0].tobytes() == b[0].tobytes(), "the whole scratch"
        for i, one in enumerate(NAMES):
            alone = FH.bids_halving(env, kw, EPISODE, schedule, 15, 1, 1, want=(one,))
            assert alone[i].tobytes() == full[i].tobytes() and all(x is None for j, x in enumerate(alone) if j != i), one
        salted = FH.bids_halving(env, kw, EPISODE, schedule, 15, 1, 1, salt=4)
        assert salted[0].tobytes() != full[0].tobytes()
        assert_same(FH.bids_halving(two, kw, EPISODE, schedule, 15, 1, 1), [x[:2] for x in full], "the first two games")
        need = M.bid_scratch(5, schedule, seats=1)
        assert 4 * max(M.bid_bounds(5, schedule, F.DEFAULT, 1, False, False)) == max(M.bid_bounds(5, schedule, F.DEFAULT, 15, False, False))
        scr = torch.empty(need, dtype=torch.uint8, device="cuda")
        out = torch.empty((5, 4, 20), dtype=torch.int32, device="cuda")
        rounds, arr = FH.schedule_args(schedule)
        p = env._p
        rc = lambda size, seats, o: env.L.tarok_playout_bids_net_halving(env._h, EPISODE, None, rounds, arr, F.DEFAULT, 0, seats, None, 15, 0, 70.0, 0,
                                                                         *[p(t) for t in kw], p(scr), size, o, None, None, env._stream())
        assert rc(need - 16, 1, p(out)) == -1 and rc(need, 3, p(out)) == -1 and rc(need, 1, None) == -1 and rc(need, 1, p(out)) == 0
        torch.cuda.synchronize()
    finally:
        env.close()
        two.close()


def test_a_captured_first_launch_replays_with_the_weights_in_place(T, nets):
    """The FIRST launch of an env captured into a graph, after the weights were swapped in place; then swapped back: each
    replay gives the eager launch's bytes for the weights in place."""
    import torch
    env, twin = make_env(T, 16), make_env(T, 16)
    try:
        kw, other = [t.clone() for t in nets["random"]], random_net(T, 31)
        env.playout_bids_net_halving_scratch((1, 1, 2), pass_value=True)      # allocated before the capture
        outs = [torch.zeros((16, 4, 20), dtype=torch.int32, device="cuda") for _ in range(3)]
        eager = lambda w: [t.cpu() for t in twin.playout_bids_net_halving(w, EPISODE, (1, 1, 2), 2, 0.5, pass_value=True, salt=4)]
        for t, o in zip(kw, other):
            t.copy_(o)
        first = eager(kw)
        stream = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                env.playout_bids_net_halving(kw, EPISODE, (1, 1, 2), 2, 0.5, pass_value=True, salt=4, sum_out=outs[0], count_out=outs[1],
                                             value_out=outs[2])
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.cpu(), x) for o, x in zip(outs, first))
        for t, o in zip(kw, nets["random"]):
            t.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        second = eager(kw)
        assert all(torch.equal(o.cpu(), x) for o, x in zip(outs, second)) and not torch.equal(second[0], first[0])
    finally:
        env.close()
        twin.close()


def test_the_learner_and_the_evaluation(T, nets):
    """BidLearner(net=, net_halving=, pass_value=True) without a depth: collect() returns the launch's sums and counts, the
    loss is bid_loss on sum / count over the counted rows, one iterate is finite; evaluate_bidding_vs_bot(net_halving=(W,))
    returns the numbers of net_list=True."""
    import torch
    import torch.nn.functional as TF
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    from tarok_amd.bidding import BidLearner
    kw = nets["random"]
    env, twin = T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT), T.TarokVecEnv(64, seed=8, mix=S.MIX_BOT)
    try:
        learner = BidLearner(env, seed=5, net=kw, net_halving=(1, 1, 2), pass_value=True)
        fw, sums, counts = learner.collect(3)
        want = twin.playout_bids_net_halving(kw, 3, (1, 1, 2), pass_value=True, salt=5)
        assert torch.equal(sums, want[0]) and torch.equal(counts, want[1]) and tuple(counts.shape) == (64, 4, 20)
        assert int(counts.max()) == 4 and int(counts[counts > 0].min()) == 1 and (counts[:, :, 19] == 4).all()
        with torch.no_grad():
            out = learner.outputs(fw)[:, :20].float()
            on = counts.reshape(-1, 20) > 0
            target = sums.reshape(-1, 20).double() / counts.reshape(-1, 20).clamp(min=1).double() * learner.reward_scale
            ref = TF.huber_loss(out[on].double(), target[on], reduction="mean", delta=1.0)
            assert abs(float(learner.loss(fw, sums, counts)) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
        assert np.isfinite(learner.iterate())
    finally:
        env.close()
        twin.close()
    one = EV.evaluate_bidding_vs_bot(4, None, 32, 1, seed=3, net=kw, net_halving=(4,), net_depth=2, pass_value=True)
    assert one == EV.evaluate_bidding_vs_bot(4, None, 32, 1, seed=3, net=kw, net_list=True, net_depth=2, pass_value=True)


@pytest.mark.parametrize("schedule,depth,pass_value,net_seats", [((1, 1, 2), None, True, "own"), ((2, 2, 4, 8), 2, False, 15)])
def test_the_evaluation_replayed_from_the_launchs_own_outputs(T, nets, schedule, depth, pass_value, net_seats):
    """evaluate_bidding_vs_bot(net=, net_halving=) on 32 games x 1 episode with a schedule of several rounds: on every pass the
    sums the round read are the eager halving launch's value_out on a twin env — rounded from sums over unequal counts —, and
    the contract, declarer and king are those of bid_round on that value_out at playouts = W; pass 0 is the Bot-everywhere
    pass."""
    from oracle import tarok_spec as S
    from tarok_amd import evaluate as EV
    kw, W = nets["random"], sum(schedule)
    seen, plain = [], []
    got = EV.evaluate_bidding_vs_bot(None, None, 32, 1, seed=3, salt=2, inspect=seen, net=kw, net_seats=net_seats,
                                     net_halving=schedule, net_depth=depth, pass_value=pass_value)
    EV.evaluate_bidding_vs_bot(2, 1, 32, 1, seed=3, salt=2, inspect=plain)
    assert [p["seats"] for p in seen] == list(EV.PASS_SEATS) and got["deals"] == 32
    twin = T.TarokVecEnv(32, seed=3, mix=S.MIX_BOT)
    try:
        differs = rounded = 0
        for rec in seen:
            inner = rec["seats"] if net_seats == "own" else net_seats
            s, c, v = twin.playout_bids_net_halving(kw, 0, schedule, depth, pass_value=pass_value, net_seats=inner, salt=2, seats=rec["seats"])
            assert (rec["sums"] == v.cpu().numpy()).all(), rec["seats"]
            sn, cn, vn = s.cpu().numpy(), c.cpu().numpy(), v.cpu().numpy()
            assert all(int(vn[i]) == M.value_of(sn[i], W, cn[i]) for i in zip(*np.nonzero(cn))) and not vn[cn == 0].any()
            rounded += int(((cn > 0) & (cn < W) & (vn != sn)).sum())
            for name, w in zip(("contract", "declarer", "king_suit"),
                               twin.bid_round(0, v, W, seats=rec["seats"], pass_value=pass_value)):
                assert (rec[name] == w.cpu().numpy()).all(), (rec["seats"], name)
            differs += int((rec["contract"] != seen[0]["contract"]).sum())
        assert differs > 0 and rounded > 0, (differs, rounded)
    finally:
        twin.close()
    for name in ("start", "contract", "declarer", "king_suit", "scores"):
        assert (seen[0][name] == plain[0][name]).all(), name
