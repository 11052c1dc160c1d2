"""CPU-side checks of the value-stopped net playouts for the exchange, the bid and the pass (tarok_playout_exchange_net_value,
tarok_playout_bids_net_value): the model of tests/playout_front_net_value_model.py against the models it is built from,
five mutants told apart from it ON THE GPU TESTS' POSITIONS (tests/playout_front_net_value_cases.py), the guards against a
vacuous comparison on those inputs, every ValueError of the wrappers, the learners and the evaluations, the evaluations'
default call lists against the golden record, and the new methods' parameter lists.  No GPU in here."""
import inspect
import json

import numpy as np
import pytest

import playout_bids_model as BM
import playout_front_net_model as FM
import playout_front_net_value_cases as C
import playout_front_net_value_model as FV
import playout_pass_model as PSM
from oracle import tarok_spec as S

BERACS = (S.BERAC, S.ODPRTI_BERAC)


@pytest.fixture(scope="module")
def W():
    return C.weight_sets()


@pytest.mark.parametrize("mix", ["tri", "dve", "ena", "solo_ena"])
def test_exchange_depth_13_is_the_net_model(W, mix):
    """Depth 13 never stops: sums, choice and discards of tests/playout_front_net_model.py, at any value_scale."""
    gs = C.exchange_games(mix, 3)
    want = FM.playout_exchange(gs, C.X_SEED, 7, 15, 2, 2, W["P"], 15)
    got = FV.playout_exchange(gs, C.X_SEED, 7, 15, 2, 2, W["P"], 15, 13, 1e9)
    assert all((g == w).all() for g, w in zip(got[:3], want)) and want[0].any()
    assert not any(d["stopped"] for _, d in got[3])


@pytest.mark.parametrize("contracts", [C.DEFAULT, C.ALL])
def test_bids_depth_13_is_the_net_model(W, contracts):
    ds = C.bid_deals(2)
    want = FM.playout_bids(ds, C.B_SEED, 5, 15, 2, contracts, W["P"], 15)
    got, info = FV.playout_bids(ds, C.B_SEED, 5, 15, 2, contracts, W["P"], 15, 13, 0.5, False)
    assert (got == want).all() and want.any() and not got[:, :, 19].any() and not any(d["stopped"] for _, d in info)


@pytest.mark.parametrize("depth", [1, 2, 5, 12])
def test_every_item_stops_below_depth_13(W, depth):
    """An item starts at 0 cards and a seat plays once per trick: at depths 1..12 every live item of a game that runs its
    twelve tricks stops, none finishes first, and at depth 1 the stop is within 4 card rounds.  (A Berac ends when its
    declarer takes a trick: those rows of the full contract mask, and only those, may finish first.)"""
    for mix in ("tri", "dve", "ena", "solo_ena"):
        info = FV.exchange_info(C.exchange_games(mix, 2), C.X_SEED, 1, 15, 2, 1, W["R"], 10, depth)
        assert info and all(d["stopped"] and d["rounds"] <= 4 * depth for _, d in info), (mix, depth)
    for contracts in (C.DEFAULT, C.ALL):
        info = FV.bid_info(C.bid_deals(1), C.B_SEED, 1, 15, 2, contracts, W["R"], 10, depth, True)
        early = [at for at, d in info if not d["stopped"]]
        assert all(at[2] < 19 and BM.row_option(at[2])[0] in BERACS for at in early), (contracts, depth, early)
        assert all(d["rounds"] <= 4 * depth for _, d in info if d["stopped"]) and (depth > 1 or not early)
        assert sum(1 for at, _ in info if at[2] == 19) == 4 * 2


def test_the_pass_row_without_a_net_seat_is_the_pass_model_at_one_sample(W):
    """net_seats = 0, depth 13, pass_value: all twenty rows are tests/playout_pass_model.pass_sums at samples = 1."""
    ds = C.bid_deals(2)
    got, _ = FV.playout_bids(ds, C.B_SEED, 5, 15, 2, C.ALL, W["R"], 0, 13, 1.0, True)
    for g, (perm, ep, gidx, _) in enumerate(ds):
        assert (got[g] == PSM.pass_sums(perm, ep, C.B_SEED, 5, gidx, 15, 2, 1, C.ALL)).all(), g
    assert got[:, :, 19].any()
    off, _ = FV.playout_bids(ds, C.B_SEED, 5, 15, 2, C.ALL, W["R"], 0, 13, 1.0, False)
    assert not off[:, :, 19].any() and (off[:, :, :19] == got[:, :, :19]).all()


X_ROWS = [("bot",) + C.X_SHAPE[:1] + C.X_SHAPE[1:] + row[1:] for row in C.X_SMALL if row[0] == 5]      # (mix, n, W, D, depth, set, seats)


def exchange_sums(row, rule, scale=1.0):
    games, _, info = C.exchange_model(*row, rule=rule)
    return FV.exchange_outputs(games, C.X_SEED, C.SALT, 15, row[2], row[3], info, scale, rule)[0]


def bid_sums(row, rule, scale=1.0):
    deals, info = C.bid_model(*row, rule=rule)
    return FV.bid_sums(len(deals), info, scale, rule)


def test_five_mutants_differ_on_the_gpu_tests_positions():
    """Each mutant gives other sums than the statement on launches the GPU tests make, so those tests can tell them apart."""
    x = {r[4]: r for r in X_ROWS}
    b = {(r[0], r[3]): r for r in C.B_PLAN}
    assert (exchange_sums(x[1], "late") != exchange_sums(x[1], "spec")).any()          # the stop one decision late
    assert (bid_sums(b[2, 1], "late") != bid_sums(b[2, 1], "spec")).any()
    passes = [r for r in C.B_PLAN if r[6]]
    for row in passes:                                                                 # the viewer of a pass item as its declarer
        spec, mut = bid_sums(row, "spec"), bid_sums(row, "declarer")
        assert (spec[:, :, :19] == mut[:, :, :19]).all()
    assert any((bid_sums(r, "spec")[:, :, 19] != bid_sums(r, "declarer")[:, :, 19]).any() for r in passes)
    spec, mut = exchange_sums(x[2], "spec"), exchange_sums(x[2], "all")                # V in every column
    assert (spec != mut).any()
    assert (exchange_sums(x[12], "never12") != exchange_sums(x[12], "spec")).any()     # depth 12 never stopping
    assert (bid_sums(b[2, 12], "never12") != bid_sums(b[2, 12], "spec")).any()
    for row in passes:                                                                 # the pass row left 0
        spec, mut = bid_sums(row, "spec"), bid_sums(row, "nopass")
        assert not mut[:, :, 19].any() and spec[:, :, 19].any() and (spec[:, :, :19] == mut[:, :, :19]).all()


def test_the_gpu_comparisons_are_not_vacuous():
    """On the GPU tests' own inputs, from the model alone: per launch family at least two distinct non-zero V of both signs
    (here: in most single launches too), a pass item whose declarer is not the viewer, a pass item that ends in Klop."""
    x_tags = [FV.seen(C.exchange_model(mix, *C.X_WIDE, *row)[2], 1.0) for mix in C.X_MIXES for row in C.exchange_plan(mix)]
    x_tags += [FV.seen(C.exchange_model(*row)[2], 0.5) for row in X_ROWS]
    assert sum("signs" in t for t in x_tags) >= len(x_tags) - 2
    b_tags = [FV.seen(C.bid_model(*row)[1], 1.0) for row in C.B_PLAN]
    assert sum("signs" in t for t in b_tags) >= len(b_tags) - 1
    for row, tags in zip(C.B_PLAN, b_tags):
        assert ({"pass_other", "pass_klop"} <= tags) == row[6], row
    assert {d for mix in C.X_MIXES for d, _, _ in C.exchange_plan(mix)} == set(C.DEPTHS) == {r[3] for r in C.B_PLAN} | {3, 12}
    assert {(r[4], r[6]) for r in C.B_PLAN} == {(s, p) for s in "RPV" for p in (True, False)}


def net_tensors():
    import torch
    return [torch.zeros(256, 256, dtype=torch.bfloat16), torch.zeros(256), torch.zeros(256, 256, dtype=torch.bfloat16), torch.zeros(256),
            torch.zeros(64, 256, dtype=torch.bfloat16), torch.zeros(64)]


def test_wrapper_learner_and_evaluation_arguments():
    """Every ValueError of the new surface, raised before an env or the GPU is touched."""
    from tarok_amd import _native, evaluate as EV, karte as K
    from tarok_amd.bidding import BidLearner
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.exchange import ExchangeLearner
    assert "tarok_playout_exchange_net_value" in _native.SYMBOLS and "tarok_playout_bids_net_value" in _native.SYMBOLS
    assert K.PLAYOUT_FRONT_MAX_DEPTH == 13 == FV.MAX_DEPTH
    net = net_tensors()

    class NoEnv:                            # the checks come before anything of the env is read
        pass
    X, B = TarokVecEnv.playout_exchange_net_value, TarokVecEnv.playout_bids_net_value
    calls = [lambda: X(NoEnv(), net, 2, 2, 0), lambda: X(NoEnv(), net, 2, 2, 14), lambda: X(NoEnv(), net, 2, 2, True),
             lambda: X(NoEnv(), net, 2, 2, 1.0), lambda: X(NoEnv(), net, 2, 2, 1, 0.0), lambda: X(NoEnv(), net, 2, 2, 1, float("inf")),
             lambda: X(NoEnv(), net, 2, 2, 1, float("nan")), lambda: X(NoEnv(), net, 2, 2, 1, net_seats=16),
             lambda: X(NoEnv(), net, 2, 2, None, net_seats=-1),
             lambda: B(NoEnv(), net, 0, 2, 0), lambda: B(NoEnv(), net, 0, 2, 14), lambda: B(NoEnv(), net, 0, 2, 1, -1.0),
             lambda: B(NoEnv(), net, 0, 2, 1, float("nan")), lambda: B(NoEnv(), net, 0, 2, 1, net_seats=16),
             lambda: B(NoEnv(), net, 0, 2, None, pass_value=True), lambda: B(NoEnv(), net, 0, 2, None, net_seats=16),
             lambda: ExchangeLearner(None, net_depth=1), lambda: ExchangeLearner(None, net=net, net_depth=0),
             lambda: ExchangeLearner(None, net=net, net_depth=14), lambda: ExchangeLearner(None, net=net, net_depth=1, net_value_scale=0),
             lambda: ExchangeLearner(None, net=net, net_depth=1, samples=2),
             lambda: BidLearner(None, net_depth=1), lambda: BidLearner(None, net=net, net_depth=0), lambda: BidLearner(None, net=net, net_depth=14),
             lambda: BidLearner(None, net=net, net_depth=2, net_value_scale=float("inf")), lambda: BidLearner(None, net=net, pass_value=True),
             lambda: BidLearner(None, pass_value=True, net_depth=2),
             lambda: EV.evaluate_exchange_net_vs_bot(net, 2, 2, 8, 1, net_depth=0), lambda: EV.evaluate_exchange_net_vs_bot(net, 2, 2, 8, 1, net_depth=14),
             lambda: EV.evaluate_exchange_net_vs_bot(net, 2, 2, 8, 1, net_depth=1, net_value_scale=0.0),
             lambda: EV.evaluate_bidding_vs_bot(2, 1, 8, 1, net_depth=1), lambda: EV.evaluate_bidding_vs_bot(2, None, 8, 1, net=net, net_depth=14),
             lambda: EV.evaluate_bidding_vs_bot(2, None, 8, 1, net=net, net_depth=1, net_value_scale=-1.0),
             lambda: EV.evaluate_bidding_vs_bot(2, 2, 8, 1, net=net, net_depth=1),
             lambda: EV.evaluate_bidding_vs_bot(2, None, 8, 1, net=net, pass_value=True)]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d did not raise" % i)
    a = BidLearner(None, net=net, net_depth=13, pass_value=True)
    b = ExchangeLearner(None, net=net, net_depth=1, net_value_scale=0.5)
    assert (a.net_depth, a.net_value_scale, a.pass_value, a.samples) == (13, 70.0, True, 1)
    assert (b.net_depth, b.net_value_scale, b.samples) == (1, 0.5, 1)
    assert (BidLearner(None, net=net).net_depth, ExchangeLearner(None).net_depth) == (None, None)


def test_parameter_lists():
    from tarok_amd import evaluate as EV
    from tarok_amd.bidding import BidLearner
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.exchange import ExchangeLearner
    sig = lambda f: inspect.signature(f).parameters
    assert list(sig(TarokVecEnv.playout_exchange_net_value)) == [
        "self", "weights", "worlds", "discard_sets", "depth", "value_scale", "net_seats", "salt", "seats", "seats_per_game", "sum_out",
        "choice_out", "discards_out"]
    assert list(sig(TarokVecEnv.playout_bids_net_value)) == [
        "self", "weights", "episode", "worlds", "depth", "value_scale", "pass_value", "net_seats", "contracts", "deals", "salt", "seats",
        "seats_per_game", "sum_out"]
    for f in (TarokVecEnv.playout_exchange_net_value, TarokVecEnv.playout_bids_net_value):
        assert sig(f)["value_scale"].default == 70.0 and sig(f)["net_seats"].default == 15
    assert sig(TarokVecEnv.playout_bids_net_value)["pass_value"].default is False
    assert list(sig(TarokVecEnv.playout_exchange_net)) == ["self", "weights", "worlds", "discard_sets", "net_seats", "salt", "seats",
                                                           "seats_per_game", "sum_out", "choice_out", "discards_out"]
    assert list(sig(TarokVecEnv.playout_bids_net)) == ["self", "weights", "episode", "worlds", "net_seats", "contracts", "deals", "salt",
                                                       "seats", "seats_per_game", "sum_out"]
    for f in (ExchangeLearner.__init__, BidLearner.__init__, EV.evaluate_exchange_net_vs_bot, EV.evaluate_bidding_vs_bot):
        assert list(sig(f))[-2:] == ["net_depth", "net_value_scale"]
        assert sig(f)["net_depth"].default is None and sig(f)["net_value_scale"].default == 70.0


def test_default_calls_are_the_golden_records_and_net_depth_changes_one_call():
    """The two evaluations with their defaults issue the call lists of tests/golden/evaluate_calls_v1.json; with a network,
    net_depth=None issues the calls of the call without it, and net_depth=D swaps the one launch (and, with pass_value, the
    round) and nothing else."""
    import evaluate_calls_cases as EC
    from tarok_amd import evaluate as EV
    with open(EC.FIXTURE) as f:
        golden = json.load(f)
    for name in ("exchange", "exchange_inspect", "bidding_pass_value_inspect"):
        trace, _, _ = EC.run_case(EV, name)
        assert trace.calls == EC.unpack(golden[name]["calls"]), name

    def calls(fn, args, **kw):
        EC.CASES["_probe"] = (fn, args, kw, False)
        try:
            return EC.run_case(EV, "_probe")[0].calls
        finally:
            del EC.CASES["_probe"]
    plain = calls("evaluate_exchange_net_vs_bot", ("W", 3, 2))
    assert calls("evaluate_exchange_net_vs_bot", ("W", 3, 2), net_depth=None, net_value_scale=1.0) == plain
    deep = calls("evaluate_exchange_net_vs_bot", ("W", 3, 2), net_depth=2, net_value_scale=0.5)
    assert len(deep) == len(plain) and [c.split("(")[0] for c in deep] == [c.split("(")[0].replace("exchange_net", "exchange_net_value") for c in plain]
    assert any(c.startswith("playout_exchange_net_value(W0, 3, 2, 2, 0.5, ") for c in deep)
    plain = calls("evaluate_bidding_vs_bot", (3, None), net="W")
    assert calls("evaluate_bidding_vs_bot", (3, None), net="W", net_depth=None) == plain
    deep = calls("evaluate_bidding_vs_bot", (3, None), net="W", net_depth=13, pass_value=True, threshold=2)
    assert [c.split("(")[0] for c in deep] == [c.split("(")[0].replace("bids_net", "bids_net_value") for c in plain]
    assert all("pass_value=True" in c for c in deep if c.startswith(("playout_bids_net_value(", "bid_round(")))
    assert any(c.startswith("playout_bids_net_value(W0, 0, 3, 13, 70.0, ") for c in deep)
