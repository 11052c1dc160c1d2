"""TEST INFRASTRUCTURE — the CPU model of tarok_front_lines (include/tarok_env.h): which next-game lines a
call takes, and the game it writes into one, per (slot, episode).  Composes tests/bid_head_model.py, tests/playout_bids_model.py
/ tests/playout_pass_model.py (the round), tests/exchange_head_model.py and the oracle's deal, setup and exchange."""
import numpy as np

import bid_head_model as BH
import exchange_head_model as XH
import playout_bids_model as BM
import playout_exchange_model as XM
import playout_pass_model as PP
from oracle import oracle as O
from oracle import tarok_spec as S

AHEAD = 14
EMPTY = 0xFFFFFFFF


def takes(episode, b, nep, mark):
    """Line b of a slot at `episode`, holding tag nep and front mark `mark`, is taken by a call."""
    return episode < nep <= episode + AHEAD and nep % AHEAD == b and mark != nep


def call(episode, lines):
    """A call on one slot: lines = [(nep, mark)] * 14 -> (the lines after it, the line numbers taken)."""
    taken = [b for b, (nep, mark) in enumerate(lines) if takes(episode, b, nep, mark)]
    return [(nep, nep) if b in taken else (nep, mark) for b, (nep, mark) in enumerate(lines)], taken


def redeal(lines, episode):
    """A refill deals `episode` into its line: the tag changes, the mark keeps its bytes."""
    b = episode % AHEAD
    return [(episode, mark) if k == b else (nep, mark) for k, (nep, mark) in enumerate(lines)]


def bid_values_row(perm, W, scale, contracts, seats, pass_value):
    """[4, ROWS] int32: tarok_bid_values[_pass]' values of one deal."""
    words = np.array(BH.game_words(perm), np.uint64)
    y, _ = BH.forward(BH.expand(words), W, stores=True)
    keep = BH.keep(seats, contracts, BM.valid_perm(perm))
    if pass_value:
        for v in range(4):
            keep[v, BH.ROWS - 1] = bool((seats >> v) & 1) and BM.valid_perm(perm)
    return np.where(keep, BH.values(y[:, :BH.ROWS].astype(np.float32), scale), 0).astype(np.int32)


def bot_exchange(g, key):
    gs = XM.group_size(g)
    assert g.exchange(0, XM.discards_under(g, 0, key)[:gs]) == 0


def front_game(seed, gidx, nep, seats, mix, bid=None, exchange=None):
    """The oracle game a taken line holds.  bid: None or dict(W, scale, playouts, margin, contracts, pass_value);
    exchange: None or a weight set (float64 torch tensors, [out, in])."""
    key = S.game_key(seed, gidx, nep)
    perm = S.deal(key)
    if bid is not None:
        vals = bid_values_row(perm, bid["W"], bid["scale"], bid["contracts"], seats, bid["pass_value"])
        rnd = PP.bid_round if bid["pass_value"] else BM.bid_round
        contract, declarer, king = rnd(key, vals, bid["playouts"], bid["margin"], bid["contracts"], seats)
        g = O.Game(perm, contract, declarer, king if contract in BM.KING_CONTRACTS else -1)
    else:
        g = O.Game(perm, *S.sample_setup(key, mix))
    if XM.waiting(g):
        if exchange is not None and XM.takes_part(g, seats):
            _, choice, disc, _ = XH.exchange_values([g.lanes()], exchange, seed, gidx, nep, [seats])
            assert g.exchange(int(choice[0]), [int(c) for c in disc[0][:XM.group_size(g)]]) == 0
        else:
            bot_exchange(g, key)
    return g


def bot_line(seed, gidx, nep, mix):
    """The game deal_into_buffer writes: the env's mix under the key, the Bot's exchange."""
    key = S.game_key(seed, gidx, nep)
    g = O.Game(S.deal(key), *S.sample_setup(key, mix))
    if XM.waiting(g):
        bot_exchange(g, key)
    return g
