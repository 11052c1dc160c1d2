"""TEST INFRASTRUCTURE — the statements of tarok_playout_exchange_net and tarok_playout_bids_net (include/tarok_env.h) on
the CPU oracle.

tarok_playout_exchange and tarok_playout_bids at one playout per (candidate or option, world), with the cards played by a
policy network on the seats of `net_seats` and by the Bot on the others.  The worlds, the candidates, the Bot's exchange
inside a bid playout and every key are tests/playout_exchange_model.py's and tests/playout_bids_model.py's; the lock-step
play-out with the float64 forward and the greedy rule is tests/playout_net_model.py's.  An item is a Game at 0 cards
played with the Bot launch's playout key at sample 0.  Nothing comes from the code under test.

The rules the mutants of tests/test_playout_front_net_cpu.py replace are arguments: `best` (which candidate at the
maximum is chosen) and `scorer` (whose score a bid playout contributes).
"""
import numpy as np

import playout_bids_model as BM
import playout_exchange_model as XM
import playout_model as PM
import playout_net_model as NM
from oracle import oracle as O
from oracle import tarok_spec as S


# ---- the exchange
def exchange_items(lanes, episode, seed, salt, gidx, seats, worlds, sets):
    """The live items of one game: [(row r = i * sets + d, world w, the world's Game after the candidate's exchange, its
    playout key)]; none for a game that does not take part."""
    game = O.Game.from_lanes(lanes)
    if not XM.takes_part(game, seats):
        return []
    declarer = int(game.g.declarer)
    ws = [XM.world_for(game, declarer, XM.world_key(seed, salt, gidx, episode, w)) for w in range(worlds)]
    out = []
    for i in range(6 // XM.group_size(game)):
        for d in range(sets):
            disc = XM.discards_under(game, i, XM.candidate_key(seed, salt, gidx, episode, i, d))
            for w in range(worlds):
                h = PM.copy_of(ws[w])
                assert h.exchange(i, disc) == 0, "a candidate's exchange is legal"
                out.append((i * sets + d, w, h, XM.playout_key(seed, salt, gidx, episode, i, d, w, 0)))
    return out


def exchange_scores(games, seed, salt, seats, worlds, sets, W, net_seats, pick=NM.greedy):
    """games: [(lanes, episode, gidx, seat set or None)] -> scores [n, 6 * sets, worlds, 4] int64 of every playout (zeros
    for groups the contract does not have and for games that do not take part)."""
    out = np.zeros((len(games), XM.GROUPS * sets, worlds, 4), np.int64)
    where, hs, keys = [], [], []
    for g, (lanes, ep, gidx, s) in enumerate(games):
        for r, w, h, key in exchange_items(lanes, ep, seed, salt, gidx, seats if s is None else s, worlds, sets):
            where.append((g, r, w)); hs.append(h); keys.append(key)
    for (g, r, w), sc in zip(where, NM.play_out(hs, keys, W, net_seats, pick)):
        out[g, r, w] = sc
    return out


def first_best(column):
    """The first row at the maximum."""
    return int(np.argmax(column))


def exchange_choice(lanes, seed, salt, gidx, episode, seats, sums, sets, best=first_best):
    """(choice_out, discards_out [3]) of one game given its sums [6 * sets, 4]: tests/playout_exchange_model.choice_of
    with the rule for the best candidate as an argument."""
    game = O.Game.from_lanes(lanes)
    if not XM.takes_part(game, seats):
        return XM.choice_of(lanes, seed, salt, gidx, episode, seats, sums, sets)
    ncand = (6 // XM.group_size(game)) * sets
    i, d = divmod(best(np.asarray(sums)[:ncand, int(game.g.declarer)]), sets)
    return i, XM.padded(XM.discards_under(game, i, XM.candidate_key(seed, salt, gidx, episode, i, d)))


def playout_exchange(games, seed, salt, seats, worlds, sets, W, net_seats, pick=NM.greedy, best=first_best):
    """(sum [n, 6 * sets, 4] int64, choice [n] int8, discards [n, 3] uint8): the whole statement."""
    sums = exchange_scores(games, seed, salt, seats, worlds, sets, W, net_seats, pick).sum(axis=2)
    rows = [exchange_choice(lanes, seed, salt, gidx, ep, seats if s is None else s, sums[g], sets, best)
            for g, (lanes, ep, gidx, s) in enumerate(games)]
    return sums, np.array([r[0] for r in rows], np.int8), np.array([r[1] for r in rows], np.uint8).reshape(len(games), 3)


# ---- the bids
def bid_game(world, v, r, pkey):
    """Row r on `world` with v as the declarer (Klop: seat 0) at its first card: the Bot's exchange under pkey where the
    contract has one (tests/playout_bids_model.one_playout's set-up)."""
    code, king = BM.row_option(r)
    g = O.Game(world, code, 0 if code == S.KLOP else v, king)
    if int(g.g.phase) == 1:
        gs = S.GROUP_SIZE[code]
        group = 0
        for j in range(gs):
            group |= 1 << int(g.g.talon[j])
        assert g.exchange(0, S.bot_discards(pkey, int(g.g.hand[v]) | group, gs)) == 0
    return g


def bid_items(perm, episode, seed, salt, gidx, seats, worlds, contracts):
    """The live items of one deal: [(viewer v, row r, world w, the Game at its first card, its playout key)]."""
    if not BM.valid_perm(perm):
        return []
    out = []
    for v in range(4):
        if not (seats >> v) & 1:
            continue
        for w in range(worlds):
            world = BM.world_of(perm, v, BM.world_key(seed, salt, gidx, episode, v, w))
            for r in range(BM.OPTIONS):
                if BM.played(r, contracts):
                    key = BM.playout_key(seed, salt, gidx, episode, v, r, w, 0)
                    out.append((v, r, w, bid_game(world, v, r, key), key))
    return out


def viewer(v, game):
    """The seat whose score a bid playout contributes: the viewer's."""
    return v


def bid_scores(deals, seed, salt, seats, worlds, contracts, W, net_seats, pick=NM.greedy, scorer=viewer):
    """deals: [(perm [54], episode, gidx, seat set or None)] -> scores [n, 4, ROWS, worlds] int64: the scorer's final score
    of every playout (zeros for seats outside the set, rows outside `contracts`, row 19 and an invalid deal)."""
    out = np.zeros((len(deals), 4, BM.ROWS, worlds), np.int64)
    where, hs, keys = [], [], []
    for g, (perm, ep, gidx, s) in enumerate(deals):
        for v, r, w, h, key in bid_items(perm, ep, seed, salt, gidx, seats if s is None else s, worlds, contracts):
            where.append((g, v, r, w, scorer(v, h))); hs.append(h); keys.append(key)
    for (g, v, r, w, seat), sc in zip(where, NM.play_out(hs, keys, W, net_seats, pick)):
        out[g, v, r, w] = sc[seat]
    return out


def playout_bids(deals, seed, salt, seats, worlds, contracts, W, net_seats, pick=NM.greedy, scorer=viewer):
    """sum [n, 4, ROWS] int64: the whole statement."""
    return bid_scores(deals, seed, salt, seats, worlds, contracts, W, net_seats, pick, scorer).sum(axis=3)
