"""CPU-side checks of the policy-network playouts (tarok_playout_cards_net): the model of tests/playout_net_model.py
against the determinized model where no seat is the network's, two mutants of the card rule caught on a constructed
position, and the argument validation of the Python wrappers.  No GPU in here."""
import numpy as np
import pytest

import playout_det_model as DM
import playout_model as PM
import playout_net_model as NM
from oracle import oracle as O
from oracle import tarok_spec as S
from playout_net_cases import zero_net

SEED, EPISODE = 41, 3


def games(mix, n, cards, first=0):
    out = []
    for gidx in range(first, first + n):
        g = O.Game.synth(SEED, gidx, EPISODE, mix)
        key = O.game_key(SEED, gidx, EPISODE)
        for q in range(cards):
            if g.done:
                break
            assert g.step(O.policy_action(key, q, g.legal())) >= 0
        out.append((g.lanes(), EPISODE, gidx, None))
    return out


@pytest.mark.parametrize("cards", [0, 5, 30, 44])
def test_no_net_seat_is_the_determinized_model(cards):
    gs = games(S.MIX_ALL, 6, cards)
    got = NM.playout_scores(gs, SEED, 7, 15, 2, zero_net(np.zeros(54)), 0)
    for g, (lanes, ep, gidx, _) in enumerate(gs):
        want = DM.playout_scores(lanes, ep, SEED, 7, gidx, 15, 2, 1)[:, :, 0]
        assert (got[g] == want).all(), (cards, g)
    assert got.any()


def test_feature_words_are_the_state_the_network_sees():
    """The restated feature words on a position mid-trick: own hand, legal cards, table, taken cards and the flag bits."""
    g = O.Game.synth(SEED, 2, EPISODE, S.MIX_FIXED + 3)
    key = O.game_key(SEED, 2, EPISODE)
    for q in range(6):
        assert g.step(O.policy_action(key, q, g.legal())) >= 0
    w = NM.feature_words(g)
    seat, nt = g.seat(), int(g.g.n_in_trick)
    assert nt == 2 and w[0] & NM.DECK == int(g.g.hand[seat]) and w[1] & NM.DECK == g.legal()
    assert bin(w[2] & NM.DECK).count("1") == 2 and bin(w[3] & NM.DECK).count("1") >= 4
    assert (w[0] >> 54) == 1 << 3 and (w[1] >> (54 + 4)) & 15 == 1 << nt and (w[3] >> 54) == 1 and (w[2] >> 58) & 15 == 1
    x = NM.expand([w])
    assert x.shape == (1, 256) and x.sum() == sum(bin(v).count("1") for v in w)


def reversed_ties(logits, legal):
    cards = PM.cards_of(legal)
    top = max(logits[c] for c in cards)
    return max(c for c in cards if logits[c] == top)


def over_all_cards(logits, legal):
    return int(np.argmax(logits[:54]))


def test_the_card_rule_and_its_mutants_on_a_constructed_position():
    """A fresh Klop deal; logits equal on every card but one that the mover does NOT hold, which is higher.  The rule plays
    the lowest legal card; the tie rule reversed plays the highest — other playouts, other sums —, and the rule over all
    54 cards picks a card that is not legal, which the model's step rejects."""
    gs = games(S.MIX_FIXED + 0, 3, 0)
    lanes = gs[0][0]
    game = O.Game.from_lanes(lanes)
    legal = game.legal()
    outside = [c for c in range(54) if not (legal >> c) & 1][0]
    b3 = np.full(54, 0.25)
    b3[outside] = 1.0
    cards = PM.cards_of(legal)
    assert len(cards) >= 2
    assert NM.greedy(b3, legal) == cards[0] and reversed_ties(b3, legal) == cards[-1] and over_all_cards(b3, legal) == outside
    W = zero_net(b3)
    want = NM.playout_scores(gs, SEED, 0, 15, 2, W, 15)
    assert (want != NM.playout_scores(gs, SEED, 0, 15, 2, W, 15, pick=reversed_ties)).any()
    assert (want != NM.playout_scores(gs, SEED, 0, 15, 2, W, 0)).any()                  # (and the Bot plays other cards)
    with pytest.raises(AssertionError):
        NM.playout_scores(gs, SEED, 0, 15, 2, W, 15, pick=over_all_cards)


def test_wrapper_arguments():
    """evaluate_playout_vs_bot(net=...) and SelfPlay(teacher=dict(net=True)) reject what they do not build, before any
    env is made."""
    import torch
    from tarok_amd import _native, evaluate as EV, selfplay as SP
    assert "tarok_playout_cards_net" in _native.SYMBOLS and "tarok_playout_net_scratch" in _native.SYMBOLS
    net = [torch.zeros(256, 256, dtype=torch.bfloat16), torch.zeros(256), torch.zeros(256, 256, dtype=torch.bfloat16), torch.zeros(256),
           torch.zeros(64, 256, dtype=torch.bfloat16), torch.zeros(64)]
    for kw in (dict(), dict(worlds=2, voids=True), dict(worlds=2, hidden=True), dict(worlds=2, exchange=2), dict(worlds=2, bidding=(2, 1)),
               dict(worlds=2, net_seats=16), dict(worlds=2, net_seats="mine")):
        with pytest.raises(ValueError):
            EV.evaluate_playout_vs_bot(None, 8, 1, net=net, **kw)
    with pytest.raises(ValueError):
        EV.evaluate_playout_vs_bot(2, 8, 1, net=net, worlds=2)                          # samples is not taken

    class Env:
        history = False
    for tc in (dict(net=True), dict(net=True, worlds=0), dict(net=True, worlds=2, samples=2), dict(net=True, worlds=2, voids=True),
               dict(net=True, worlds=2, hidden=True), dict(net=True, worlds=2, net_seats=16), dict(worlds=2, samples=1, net_seats=3),
               dict(net=True, worlds=65)):
        with pytest.raises(ValueError):
            SP.SelfPlay(Env(), hidden=256, teacher=tc)
    with pytest.raises(ValueError):
        SP.SelfPlay(Env(), hidden=128, teacher=dict(net=True, worlds=2))
