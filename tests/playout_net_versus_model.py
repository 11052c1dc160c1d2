"""TEST INFRASTRUCTURE — the statement of tarok_playout_cards_net_versus (include/tarok_env.h) on the CPU oracle.

tests/playout_net_value_model.play_out with TWO weight sets, chosen per position from (viewer, mover, own_rel, opp_rel): the
relative seat of the mover is r = (mover - viewer) & 3; r in own_rel plays network A's greedy card, r in opp_rel network
B's, any other seat the Bot's card under the item's key.  With depth > 0 an item stops at its viewer's depth-th decision
and takes output 54 of the viewer's OWN network there — B if bit 0 of opp_rel is set, else A — through the header's float32
steps (playout_net_value_model.points); depth = 0 plays to the last card.  The worlds, the keys, the items, the feature
words and the forward are the existing models', imported; nothing comes from the code under test.

`rule` names the statement ("spec") or one of the mutants the tests must tell apart from it:
  "absolute"  the role sets read as ABSOLUTE seats (bit s for seat s) instead of seats relative to the viewer;
  "swapped"   networks A and B swapped;
  "other"     the stop value taken from the network that is NOT the viewer's.
"""
import numpy as np

import playout_model as PM
import playout_net_model as NM
import playout_net_value_model as VM
from oracle import oracle as O

RANKS = PM.RANKS
RULES = ("spec", "absolute", "swapped", "other")
BOT, A, B = 0, 1, 2


def role(viewer, mover, own_rel, opp_rel, rule="spec"):
    """0: the Bot, 1: network A, 2: network B plays `mover` in an item whose viewer is `viewer`."""
    assert 0 <= own_rel <= 15 and 0 <= opp_rel <= 15 and not own_rel & opp_rel
    r = mover if rule == "absolute" else (mover - viewer) & 3
    return A if (own_rel >> r) & 1 else B if (opp_rel >> r) & 1 else BOT


def viewer_net(opp_rel):
    """The network whose value head speaks for the viewer: B where the viewer (relative seat 0) plays B, else A."""
    return B if opp_rel & 1 else A


def play_out(games, keys, viewers, WA, WB, own_rel, opp_rel, depth, value_scale, rule="spec"):
    """Plays every oracle Game of `games` (after its candidate card) in lock-step until it ends or stops.  Returns
    (results: four ints per item, info: playout_net_value_model.play_out's dicts, plus `both`: the item met positions of
    network A and of network B)."""
    assert rule in RULES and 0 <= depth <= VM.MAX_DEPTH
    nets = {A: WB, B: WA} if rule == "swapped" else {A: WA, B: WB}
    vnet = viewer_net(opp_rel)
    if rule == "other":
        vnet = A + B - vnet
    m = len(games)
    left = [depth] * m
    res = [None] * m
    info = [dict(stopped=False, V=None, v=None, rounds=0, at=None, met=set()) for _ in range(m)]
    live = []
    for i, h in enumerate(games):
        if h.done:
            res[i] = [int(x) for x in h.scores]
        else:
            live.append(i)
    while live:
        stop, roles = set(), {}
        for i in live:
            info[i]["rounds"] += 1
            mover = games[i].seat()
            roles[i] = role(viewers[i], mover, own_rel, opp_rel, rule)
            if depth and mover == viewers[i]:
                left[i] -= 1
                if left[i] == 0:
                    stop.add(i)
        out = {}
        for net in (A, B):                            # one forward per network over the rows that need it
            rows = [i for i in live if (vnet if i in stop else roles[i]) == net]
            if rows:
                out.update(zip(rows, VM.forward([games[i] for i in rows], nets[net])))
        nxt = []
        for i in live:
            h = games[i]
            if i in stop:
                V = VM.points(float(out[i][54]), value_scale)
                info[i].update(stopped=True, v=float(out[i][54]), V=V, at=PM.copy_of(h))
                res[i] = [V if s == viewers[i] else 0 for s in range(4)]
                continue
            q = int(h.g.trick_no) * 4 + int(h.g.n_in_trick)
            if roles[i] == BOT:
                c = O.policy_action(keys[i], q, h.legal())
            else:
                info[i]["met"].add(roles[i])
                c = NM.greedy(out[i][:54], h.legal())
            r = h.step(c)
            assert r >= 0, "the card is legal"
            if r != 0:
                res[i] = [int(x) for x in h.scores]
            else:
                nxt.append(i)
        live = nxt
    for i in range(m):
        info[i].update(viewer=viewers[i], scores=res[i], both=info[i].pop("met") == {A, B})
    return res, info


def playout_scores(kind, games, seed, salt, seats, worlds, WA, WB, own_rel, opp_rel, depth, value_scale, words=None, rule="spec"):
    """games: [(lanes, episode, gidx, seat set or None)], words: one per game (kinds voids / hidden) -> (scores
    [n, 12, worlds, 4] int64, info: [((g, j, w), play_out's dict)])."""
    out = np.zeros((len(games), RANKS, worlds, 4), np.int64)
    where, hs, keys, viewers = [], [], [], []
    for g, (lanes, ep, gidx, s) in enumerate(games):
        viewer = O.Game.from_lanes(lanes).seat()
        for j, w, h, key in VM.items_of(kind, lanes, ep, seed, salt, gidx, seats if s is None else s, worlds, None if words is None else words[g]):
            where.append((g, j, w)); hs.append(h); keys.append(key); viewers.append(viewer)
    res, info = play_out(hs, keys, viewers, WA, WB, own_rel, opp_rel, depth, value_scale, rule)
    for (g, j, w), sc in zip(where, res):
        out[g, j, w] = sc
    return out, list(zip(where, info))


def playout_cards(kind, games, seed, salt, seats, worlds, WA, WB, own_rel, opp_rel, depth, value_scale, words=None, rule="spec"):
    """(sum [n, 12, 4] int64, cards [n] uint8, info): the whole statement; the card rule is tarok_playout_cards'."""
    scores, info = playout_scores(kind, games, seed, salt, seats, worlds, WA, WB, own_rel, opp_rel, depth, value_scale, words, rule)
    sums = scores.sum(axis=2)
    acts = np.array([PM.card_of(lanes, seed, gidx, ep, seats if s is None else s, sums[g])
                     for g, (lanes, ep, gidx, s) in enumerate(games)], np.uint8)
    return sums, acts, info
