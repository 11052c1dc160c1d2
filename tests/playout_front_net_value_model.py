"""TEST INFRASTRUCTURE — the statements of tarok_playout_exchange_net_value and tarok_playout_bids_net_value
(include/tarok_env.h) on the CPU oracle.

tests/playout_front_net_model.py with the stop of tests/playout_net_value_model.py: every item — an exchange candidate or a
bid option in a world, a Game at 0 cards played — carries its VIEWER (the declarer for the exchange; the seat v whose row it
is for the bids, in the Klop row and in a pass item too) and a counter of the viewer's decisions left.  At the depth-th
position with the viewer to move the item stops without playing a card, and its result is V in the viewer's column and 0 in
the other three, where V is formed from output 54 of tests/policy_exact_ref.reference (float64) on
tests/observe_model.feature_words of the stop position by the header's float32 steps (NumPy float32, np.rint).  An item
starts at 0 cards, so the viewer has 12 decisions ahead: depth 13 never stops (tests/playout_net_model.play_out), depth
12 stops every item at the viewer's forced last card.  The pass item (pass_value) is tests/playout_pass_model.py's: three
Bots bid under the key of row 19 at sample 0 with the viewer silent, and the game they arrive at is set up on the viewer's
world with the Bot's exchange.  Nothing comes from the code under test.

`rule` names the statement ("spec") or one of the mutants the tests must tell apart from it:
  "late"      the value is read one viewer decision late;
  "declarer"  the viewer of a pass item taken as the item's declarer;
  "all"       V written into every column;
  "never12"   depth 12 never stops (the card launch's range);
  "nopass"    the pass row left 0.
"""
import numpy as np

import playout_bids_model as BM
import playout_front_net_model as FM
import playout_net_model as NM
import playout_net_value_model as VM
import playout_pass_model as PSM
from oracle import oracle as O

MAX_DEPTH = 13
PASS_ROW = PSM.PASS_ROW
RULES = ("spec", "late", "declarer", "all", "never12", "nopass")
points = VM.points


def play_out(games, keys, viewers, W, net_seats, depth, value_scale, pick=NM.greedy, rule="spec"):
    """Plays every oracle Game of `games` (at 0 cards played) in lock-step until it ends or stops: (results: four ints per
    item, info: per item dict(stopped, V, v, rounds, viewer, scores, at) as tests/playout_net_value_model.play_out's)."""
    assert rule in RULES and 1 <= depth <= MAX_DEPTH
    d = depth + (1 if rule == "late" or (rule == "never12" and depth == 12) else 0)
    if d >= MAX_DEPTH:                                # the viewer has 12 decisions: the counter never reaches 0
        res = [[int(x) for x in sc] for sc in NM.play_out(games, keys, W, net_seats, pick)]
        return res, [dict(stopped=False, V=None, v=None, rounds=None, at=None, viewer=v, scores=r) for v, r in zip(viewers, res)]
    return VM.play_out(games, keys, viewers, W, net_seats, d, value_scale, pick, "all" if rule == "all" else "spec")


def result_at(d, value_scale, rule="spec"):
    """An item's four results re-formed at another value_scale: the playouts do not depend on it."""
    if not d["stopped"]:
        return d["scores"]
    V = points(d["v"], value_scale)
    return [V] * 4 if rule == "all" else [V if s == d["viewer"] else 0 for s in range(4)]


# ---- the exchange
def exchange_info(games, seed, salt, seats, worlds, sets, W, net_seats, depth, pick=NM.greedy, rule="spec"):
    """games: [(lanes, episode, gidx, seat set or None)] -> [((g, r, w), play_out's dict)] of every live item."""
    where, hs, keys, viewers = [], [], [], []
    for g, (lanes, ep, gidx, s) in enumerate(games):
        declarer = int(O.Game.from_lanes(lanes).g.declarer)
        for r, w, h, key in FM.exchange_items(lanes, ep, seed, salt, gidx, seats if s is None else s, worlds, sets):
            where.append((g, r, w)); hs.append(h); keys.append(key); viewers.append(declarer)
    _, info = play_out(hs, keys, viewers, W, net_seats, depth, 1.0, pick, rule)
    return list(zip(where, info))


def exchange_outputs(games, seed, salt, seats, worlds, sets, info, value_scale, rule="spec"):
    """(sum [n, 6 * sets, 4] int64, choice [n] int8, discards [n, 3] uint8) of a model run at `value_scale`; the choice
    is tests/playout_front_net_model.exchange_choice on the summed results: the first row at the declarer's maximum."""
    sums = np.zeros((len(games), 6 * sets, 4), np.int64)
    for (g, r, w), d in info:
        sums[g, r] += result_at(d, value_scale, rule)
    rows = [FM.exchange_choice(lanes, seed, salt, gidx, ep, seats if s is None else s, sums[g], sets)
            for g, (lanes, ep, gidx, s) in enumerate(games)]
    return sums, np.array([r[0] for r in rows], np.int8), np.array([r[1] for r in rows], np.uint8).reshape(len(games), 3)


def playout_exchange(games, seed, salt, seats, worlds, sets, W, net_seats, depth, value_scale, pick=NM.greedy, rule="spec"):
    """(sums, choice, discards, info): the whole statement."""
    info = exchange_info(games, seed, salt, seats, worlds, sets, W, net_seats, depth, pick, rule)
    return exchange_outputs(games, seed, salt, seats, worlds, sets, info, value_scale, rule) + (info,)


# ---- the bids
def pass_item(perm, episode, seed, salt, gidx, v, w):
    """(the Game of viewer v's pass playout in world w at its first card, its key, (contract, declarer))."""
    world = BM.world_of(perm, v, BM.world_key(seed, salt, gidx, episode, v, w))
    key = PSM.pass_key(seed, salt, gidx, episode, v, w, 0)
    contract, declarer, king = PSM.pass_round(key, v)
    return BM.game_of(world, contract, declarer, king, key), key, (contract, declarer)


def bid_items(perm, episode, seed, salt, gidx, seats, worlds, contracts, pass_value, rule="spec"):
    """The live items of one deal: [(viewer v, row r, world w, the Game at its first card, its key, the item's viewer,
    (contract, declarer) of a pass item or None)]."""
    out = [(v, r, w, h, key, v, None) for v, r, w, h, key in FM.bid_items(perm, episode, seed, salt, gidx, seats, worlds, contracts)]
    if pass_value and rule != "nopass" and BM.valid_perm(perm):
        for v in range(4):
            if (seats >> v) & 1:
                for w in range(worlds):
                    h, key, what = pass_item(perm, episode, seed, salt, gidx, v, w)
                    out.append((v, PASS_ROW, w, h, key, what[1] if rule == "declarer" else v, what))
    return out


def bid_info(deals, seed, salt, seats, worlds, contracts, W, net_seats, depth, pass_value, pick=NM.greedy, rule="spec"):
    """deals: [(perm [54], episode, gidx, seat set or None)] -> [((g, v, r, w), play_out's dict with `item`: (contract,
    declarer) of a pass item, else None)] of every live item."""
    where, hs, keys, viewers, what = [], [], [], [], []
    for g, (perm, ep, gidx, s) in enumerate(deals):
        for v, r, w, h, key, viewer, item in bid_items(perm, ep, seed, salt, gidx, seats if s is None else s, worlds, contracts, pass_value, rule):
            where.append((g, v, r, w)); hs.append(h); keys.append(key); viewers.append(viewer); what.append(item)
    _, info = play_out(hs, keys, viewers, W, net_seats, depth, 1.0, pick, rule)
    return [(at, dict(d, item=item)) for at, d, item in zip(where, info, what)]


def bid_sums(n, info, value_scale, rule="spec"):
    """sum [n, 4, ROWS] int64 of a model run at `value_scale`: seat v's column of the results of v's items."""
    sums = np.zeros((n, 4, BM.ROWS), np.int64)
    for (g, v, r, w), d in info:
        sums[g, v, r] += result_at(d, value_scale, rule)[v]
    return sums


def playout_bids(deals, seed, salt, seats, worlds, contracts, W, net_seats, depth, value_scale, pass_value, pick=NM.greedy, rule="spec"):
    """(sum [n, 4, ROWS] int64, info): the whole statement."""
    info = bid_info(deals, seed, salt, seats, worlds, contracts, W, net_seats, depth, pass_value, pick, rule)
    return bid_sums(len(deals), info, value_scale, rule), info


def seen(info, value_scale):
    """What a launch's items show, for the guards against vacuous comparisons: a set of tags."""
    tags = set()
    Vs = {points(d["v"], value_scale) for _, d in info if d["stopped"]} - {0}
    if len(Vs) >= 2 and min(Vs) < 0 < max(Vs):
        tags.add("signs")
    for at, d in info:
        item = d.get("item")
        if item is not None:
            if item[1] != at[1]:
                tags.add("pass_other")                # a pass item whose declarer is not the viewer
            if item[0] == 0:
                tags.add("pass_klop")                 # a pass item that ends in Klop
    return tags
