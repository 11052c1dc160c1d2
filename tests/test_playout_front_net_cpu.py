"""CPU-side checks of the net-played playouts for the exchange and the bid (tarok_playout_exchange_net,
tarok_playout_bids_net): the models of tests/playout_front_net_model.py against the Bot models at samples = 1 where no
seat is the network's, one mutant per model caught, and the argument validation of the Python wrappers, the learners and
the evaluations.  No GPU in here."""
import numpy as np
import pytest

import playout_bids_model as BM
import playout_exchange_model as XM
import playout_front_net_model as FM
from oracle import tarok_spec as S
from playout_net_cases import zero_net

SEED, EPISODE = 41, 3


def waiting_games(code, n, first=0):
    return [(XM.deferred_game(SEED, gidx, EPISODE, S.MIX_FIXED + code).lanes(), EPISODE, gidx, None) for gidx in range(first, first + n)]


def deals(n, first=0):
    return [(S.deal(S.game_key(SEED, gidx, EPISODE)), EPISODE, gidx, None) for gidx in range(first, first + n)]


@pytest.mark.parametrize("code", [S.TRI, S.DVE, S.ENA, S.SOLO_ENA])
def test_exchange_without_a_net_seat_is_the_bot_model_at_one_sample(code):
    """Tri (2 groups), Dve (3), Ena and Solo_ena (6): sums, choice and discards of the Bot model at (2, 1, 2)."""
    gs = waiting_games(code, 3)
    sums, choice, disc = FM.playout_exchange(gs, SEED, 7, 15, 2, 2, zero_net(np.zeros(54)), 0)
    ngroups = 6 // S.GROUP_SIZE[code]
    for g, (lanes, ep, gidx, _) in enumerate(gs):
        want_sum, want_ch, want_di = XM.playout_exchange(lanes, ep, SEED, 7, gidx, 15, 2, 1, 2)
        assert (sums[g] == want_sum).all() and int(choice[g]) == want_ch and disc[g].tolist() == want_di, (code, g)
        assert sums[g, :ngroups * 2].any() and not sums[g, ngroups * 2:].any()


def test_exchange_games_that_do_not_take_part():
    """A declarer outside the set: zero sums and the Bot's own exchange; a game in play: -1 and 255s."""
    gs = waiting_games(S.DVE, 2)
    declarer = [int((int(l[9]) >> 37) & 3) for l, _, _, _ in gs]
    per = [(l, ep, gidx, 15 & ~(1 << declarer[g])) for g, (l, ep, gidx, _) in enumerate(gs)]
    sums, choice, disc = FM.playout_exchange(per, SEED, 0, 15, 2, 1, zero_net(np.zeros(54)), 15)
    assert not sums.any() and (choice == 0).all() and (disc[:, :2] < 54).all() and (disc[:, 2] == 255).all()
    from oracle import oracle as O
    played = [(O.Game.synth(SEED, 5, EPISODE, S.MIX_FIXED + S.DVE).lanes(), EPISODE, 5, None)]
    sums, choice, disc = FM.playout_exchange(played, SEED, 0, 15, 2, 1, zero_net(np.zeros(54)), 15)
    assert not sums.any() and choice.tolist() == [-1] and (disc == 255).all()


@pytest.mark.parametrize("contracts", [BM.DEFAULT_CONTRACTS, BM.ALL_CONTRACTS])
def test_bids_without_a_net_seat_are_the_bot_model_at_one_sample(contracts):
    ds = deals(2)
    got = FM.playout_bids(ds, SEED, 5, 15, 2, contracts, zero_net(np.zeros(54)), 0)
    for g, (perm, ep, gidx, _) in enumerate(ds):
        assert (got[g] == BM.playout_bids(perm, ep, SEED, 5, gidx, 15, 2, 1, contracts)).all(), (contracts, g)
    assert got[:, :, :13].any(axis=(0, 1)).all() and not got[:, :, 19].any()
    assert got[:, :, 13:19].any() == (contracts == BM.ALL_CONTRACTS)


def test_bids_seat_sets_and_an_invalid_deal():
    ds = deals(2)
    bad = list(ds[1][0]); bad[3] = bad[4]
    got = FM.playout_bids([ds[0][:3] + (5,), (bad,) + ds[1][1:]], SEED, 0, 15, 1, 0x003, zero_net(np.zeros(54)), 15)
    assert got[0, 0].any() and got[0, 2].any() and not got[0, 1].any() and not got[0, 3].any() and not got[1].any()


def last_best(column):
    """MUTANT: the last row at the maximum."""
    column = np.asarray(column)
    return int(len(column) - 1 - np.argmax(column[::-1]))


def test_the_first_best_candidate_and_its_mutant():
    """With the network on every seat a playout has no draw in it, so two candidates of a group that lay down the same
    cards score the same in every world: ties at the maximum are common (a condition on the inputs, asserted on the
    model's own sums).  The rule takes the first of them; the mutant that takes the last names another candidate."""
    gs = waiting_games(S.ENA, 6)
    W = zero_net(np.linspace(1.0, 0.0, 54))
    sums, choice, disc = FM.playout_exchange(gs, SEED, 0, 15, 1, 8, W, 15)
    declarer = [int((int(l[9]) >> 37) & 3) for l, _, _, _ in gs]
    tied = [g for g in range(len(gs)) if (sums[g, :, declarer[g]] == sums[g, :, declarer[g]].max()).sum() > 1]
    assert tied, "the inputs must hold a tie at the maximum"
    for g, (lanes, ep, gidx, _) in enumerate(gs):                    # the rule as an argument IS the Bot model's rule
        assert FM.exchange_choice(lanes, SEED, 0, gidx, ep, 15, sums[g], 8) == XM.choice_of(lanes, SEED, 0, gidx, ep, 15, sums[g], 8)
    rows = lambda best: [FM.exchange_choice(gs[g][0], SEED, 0, gs[g][2], EPISODE, 15, sums[g], 8, best=best) for g in tied]
    first, last = rows(FM.first_best), rows(last_best)
    assert first == [(int(choice[g]), disc[g].tolist()) for g in tied]
    picked = lambda best: [best(sums[g, :, declarer[g]]) for g in tied]
    assert all(a < b for a, b in zip(picked(FM.first_best), picked(last_best)))
    _, ch_m, di_m = FM.playout_exchange(gs, SEED, 0, 15, 1, 8, W, 15, best=last_best)
    assert (ch_m != choice).any() or (di_m != disc).any(), "the mutant's outputs differ somewhere"


def declarers_score(v, game):
    """MUTANT: the declarer's seat instead of the viewer's."""
    return int(game.g.declarer)


def test_the_viewers_score_and_its_mutant():
    """A Klop's declarer is seat 0 whoever views it: the mutant that sums the declarer's score writes seat 0's score into
    the Klop row of viewers 1..3."""
    ds = deals(2)
    W = zero_net(np.linspace(0.0, 1.0, 54))
    want = FM.playout_bids(ds, SEED, 0, 15, 2, 0x003, W, 15)
    mutant = FM.playout_bids(ds, SEED, 0, 15, 2, 0x003, W, 15, scorer=declarers_score)
    assert (want[:, 0] == mutant[:, 0]).all() and (want[:, :, 1:] == mutant[:, :, 1:]).all()      # (v = declarer there)
    assert (want[:, 1:, 0] != mutant[:, 1:, 0]).any()
    assert (want != FM.playout_bids(ds, SEED, 0, 15, 2, 0x003, W, 0)).any()                       # (and the Bot plays other cards)


def net_tensors():
    import torch
    return [torch.zeros(256, 256, dtype=torch.bfloat16), torch.zeros(256), torch.zeros(256, 256, dtype=torch.bfloat16), torch.zeros(256),
            torch.zeros(64, 256, dtype=torch.bfloat16), torch.zeros(64)]


def test_wrapper_learner_and_evaluation_arguments():
    """Every ValueError of the new surface, raised before an env or the GPU is touched."""
    from tarok_amd import _native, evaluate as EV
    from tarok_amd.bidding import BidLearner
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.exchange import ExchangeLearner
    for name in ("tarok_playout_exchange_net", "tarok_playout_exchange_net_scratch", "tarok_playout_bids_net", "tarok_playout_bids_net_scratch"):
        assert name in _native.SYMBOLS
    net = net_tensors()

    class NoEnv:                            # the checks come before anything of the env is read
        pass
    for call in (lambda: TarokVecEnv.playout_exchange_net(NoEnv(), net, 2, 2, net_seats=16),
                 lambda: TarokVecEnv.playout_exchange_net(NoEnv(), net, 2, 2, net_seats=-1),
                 lambda: TarokVecEnv.playout_exchange_net_scratch(NoEnv(), 0, 2),
                 lambda: TarokVecEnv.playout_exchange_net_scratch(NoEnv(), 65, 2),
                 lambda: TarokVecEnv.playout_exchange_net_scratch(NoEnv(), 2, 0),
                 lambda: TarokVecEnv.playout_exchange_net_scratch(NoEnv(), 2, 9),
                 lambda: TarokVecEnv.playout_bids_net(NoEnv(), net, 0, 2, net_seats=16),
                 lambda: TarokVecEnv.playout_bids_net(NoEnv(), net, 0, 2, net_seats=-1),
                 lambda: TarokVecEnv.playout_bids_net_scratch(NoEnv(), 0),
                 lambda: TarokVecEnv.playout_bids_net_scratch(NoEnv(), 65),
                 lambda: ExchangeLearner(None, net=net, samples=2),
                 lambda: ExchangeLearner(None, net=net, net_seats=16),
                 lambda: ExchangeLearner(None, net=net[:5]),
                 lambda: BidLearner(None, net=net, samples=2),
                 lambda: BidLearner(None, net=net, net_seats=16),
                 lambda: BidLearner(None, net=net, pass_value=True),
                 lambda: BidLearner(None, net=net[:5]),
                 lambda: EV.evaluate_exchange_net_vs_bot(net, 2, 2, 8, 1, net_seats=16),
                 lambda: EV.evaluate_exchange_net_vs_bot(net, 2, 2, 8, 1, net_seats="mine"),
                 lambda: EV.evaluate_exchange_net_vs_bot(net[:5], 2, 2, 8, 1),
                 lambda: EV.evaluate_bidding_vs_bot(2, 2, 8, 1, net=net),
                 lambda: EV.evaluate_bidding_vs_bot(2, None, 8, 1, net=net, net_seats=16),
                 lambda: EV.evaluate_bidding_vs_bot(2, 1, 8, 1, net=net, pass_value=True)):
        with pytest.raises(ValueError):
            call()
    a, b = ExchangeLearner(None, net=net), BidLearner(None, net=net, samples=1)
    assert (a.samples, a.net_seats, b.samples, b.net_seats) == (1, 15, 1, 15) and all(x is y for x, y in zip(a.net_weights, net))
    assert (ExchangeLearner(None).samples, ExchangeLearner(None).net_weights, BidLearner(None).samples) == (2, None, 2)
