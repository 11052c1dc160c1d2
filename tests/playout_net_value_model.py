"""TEST INFRASTRUCTURE — the statement of tarok_playout_cards_net_value (include/tarok_env.h) on the CPU oracle.

tests/playout_net_model.play_out with the stop: every item carries its VIEWER (the seat to move in the env's position, the
seat that played the candidate) and a counter of the viewer's decisions left.  At the depth-th position with the viewer
to move the item stops without playing a card, and its result is V in the viewer's column and 0 in the other three, where
V is formed from output 54 of tests/test_gpu_policy_exact.reference on playout_net_model.feature_words of the stop
position by the header's float32 steps (NumPy float32, np.rint).  An item whose game ends first keeps its true scores.
The worlds are the three existing world models', imported; nothing comes from the code under test.

`rule` names the statement ("spec") or one of the mutants the tests must tell apart from it:
  "late"   the value is read one viewer decision late (the counter starts at depth + 1);
  "after"  the value of the position AFTER the viewer's card at the stop (the game's true scores if that card ends it);
  "away"   round half away from zero instead of half to even;
  "all"    V written into every column.
"""
import numpy as np

import playout_model as PM
import playout_net_model as NM
import playout_net_worlds_model as WM
from oracle import oracle as O

RANKS = PM.RANKS
MAX_DEPTH = 12
KINDS = ("det", "voids", "hidden")                # TAROK_NET_WORLDS_DET / _VOIDS / _HIDDEN = 0 / 1 / 2
RULES = ("spec", "late", "after", "away", "all")
F32 = np.float32


def points(v, value_scale, half_even=True):
    """The header's float32 steps: t = v * value_scale; NaN -> 0; clamp to [-32767, 32767]; rint (ties to even)."""
    with np.errstate(over="ignore", invalid="ignore"):
        t = F32(F32(v) * F32(value_scale))
    if np.isnan(t):
        t = F32(0)
    t = F32(min(max(t, F32(-32767)), F32(32767)))
    if half_even:
        return int(np.rint(t))
    return int(np.sign(t) * np.floor(np.abs(np.float64(t)) + 0.5))


def forward(games, W):
    """[m, 64] float64 outputs (card logits 0..53, value 54) on the feature words of every Game's own position."""
    import torch
    from policy_exact_ref import reference
    return reference(torch.from_numpy(NM.expand([NM.feature_words(h) for h in games])), W)["out"].numpy()


def play_out(games, keys, viewers, W, net_seats, depth, value_scale, pick=NM.greedy, rule="spec"):
    """Plays every oracle Game of `games` (after its candidate card) in lock-step until it ends or stops.  Returns
    (results: four ints per item, info: per item dict(stopped, V, v, rounds, viewer, scores: the result, at: a copy of the
    stop position or None));
    rounds counts the card rounds the item was live in, the stop round included."""
    assert rule in RULES and 1 <= depth <= MAX_DEPTH
    m = len(games)
    left = [depth + (1 if rule == "late" else 0)] * m
    res = [None] * m
    info = [dict(stopped=False, V=None, v=None, rounds=0, at=None) for _ in range(m)]
    live = []
    for i, h in enumerate(games):
        if h.done:
            res[i] = [int(x) for x in h.scores]
        else:
            live.append(i)
    while live:
        stop = set()
        for i in live:
            info[i]["rounds"] += 1
            if games[i].seat() == viewers[i]:
                left[i] -= 1
                if left[i] == 0:
                    stop.add(i)
        rows = [i for i in live if i in stop or (net_seats >> games[i].seat()) & 1]
        out = dict(zip(rows, forward([games[i] for i in rows], W))) if rows else {}
        after = []                                    # rule "after": the stopping rows play the viewer's card first
        nxt = []
        for i in live:
            h = games[i]
            if i in stop and rule != "after":
                info[i].update(stopped=True, v=float(out[i][54]), at=PM.copy_of(h))
                continue
            q = int(h.g.trick_no) * 4 + int(h.g.n_in_trick)
            c = pick(out[i][:54], h.legal()) if (net_seats >> h.seat()) & 1 else O.policy_action(keys[i], q, h.legal())
            r = h.step(c)
            assert r >= 0, "the card is legal"
            if r != 0:
                res[i] = [int(x) for x in h.scores]
            elif i in stop:
                after.append(i)
            else:
                nxt.append(i)
        if after:
            for i, o in zip(after, forward([games[i] for i in after], W)):
                info[i].update(stopped=True, v=float(o[54]), at=PM.copy_of(games[i]))
        for i in live:
            if info[i]["stopped"] and res[i] is None:
                V = points(info[i]["v"], value_scale, half_even=rule != "away")
                info[i]["V"] = V
                res[i] = [V] * 4 if rule == "all" else [V if s == viewers[i] else 0 for s in range(4)]
        live = nxt
    for i in range(m):
        info[i].update(viewer=viewers[i], scores=res[i])
    return res, info


def items_of(kind, lanes, episode, seed, salt, gidx, seats, worlds, word):
    if kind == "det":
        return NM.items_of(lanes, episode, seed, salt, gidx, seats, worlds)
    return WM.items_of(kind, lanes, episode, seed, salt, gidx, seats, worlds, word)


def playout_scores(kind, games, seed, salt, seats, worlds, W, net_seats, depth, value_scale, words=None, pick=NM.greedy, rule="spec"):
    """games: [(lanes, episode, gidx, seat set or None)], words: one per game (kinds voids / hidden) -> (scores
    [n, 12, worlds, 4] int64, info: [((g, j, w), play_out's dict)])."""
    out = np.zeros((len(games), RANKS, worlds, 4), np.int64)
    where, hs, keys, viewers = [], [], [], []
    for g, (lanes, ep, gidx, s) in enumerate(games):
        viewer = O.Game.from_lanes(lanes).seat()
        for j, w, h, key in items_of(kind, lanes, ep, seed, salt, gidx, seats if s is None else s, worlds, None if words is None else words[g]):
            where.append((g, j, w)); hs.append(h); keys.append(key); viewers.append(viewer)
    res, info = play_out(hs, keys, viewers, W, net_seats, depth, value_scale, pick, rule)
    for (g, j, w), sc in zip(where, res):
        out[g, j, w] = sc
    return out, list(zip(where, info))


def playout_cards(kind, games, seed, salt, seats, worlds, W, net_seats, depth, value_scale, words=None, pick=NM.greedy, rule="spec"):
    """(sum [n, 12, 4] int64, cards [n] uint8, info): the whole statement; the card rule is tarok_playout_cards'."""
    scores, info = playout_scores(kind, games, seed, salt, seats, worlds, W, net_seats, depth, value_scale, words, pick, rule)
    sums = scores.sum(axis=2)
    acts = np.array([PM.card_of(lanes, seed, gidx, ep, seats if s is None else s, sums[g])
                     for g, (lanes, ep, gidx, s) in enumerate(games)], np.uint8)
    return sums, acts, info


def seen(info, value_scale):
    """What a launch's items show, for the guards against vacuous comparisons: a set of tags."""
    tags = set()
    stopped = [d for _, d in info if d["stopped"]]
    if stopped and len(stopped) < len(info):
        tags.add("mixed")                             # stopped and finished items in one launch
    Vs = {d["V"] for d in stopped}
    if any(V > 0 for V in Vs) and any(V < 0 for V in Vs) and len(Vs) >= 3:
        tags.add("signs")
    for d in stopped:
        if points(d["v"], value_scale) != points(d["v"], value_scale, half_even=False):
            tags.add("tie")
        if abs(d["V"]) == 32767:
            tags.add("clamped")
    return tags
