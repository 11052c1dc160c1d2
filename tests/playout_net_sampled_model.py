"""TEST INFRASTRUCTURE — the statement of tarok_playout_cards_net_sampled (include/tarok_env.h) on the CPU oracle.

tests/playout_net_versus_model.play_out with, per position, the card of tests/play_mode_model.play_mode under the ROLE'S
play mode and the ITEM'S key: a seat of role A at q cards played plays play_mode(A's 54 logits, legal, q, item key,
temperature_a, epsilon_a)["card"] — the tempered inverse-CDF draw on draw 192 + q (the arg-max at temperature 0), or the
Bot's card where the coin 256 + q says explore —, role B the same with B's logits and B's mode, any other seat the Bot's
card.  There is one item per (game, rank j, world w, sample k); the samples of a world start from the same dealt position
and item k's key is playout_det_model.playout_key(..., card, w, k): the Bot launches' pkey with the sample number in its
ten low bits.  The value stop is the versus model's.  The worlds, the keys, the feature words, the forward and the sampler
are the existing models', imported; nothing comes from the code under test.

Every item carries `margin`: the smallest play_mode margin of any TEMPERED draw along its playout that decided a card (inf
if there was none): a float32 sampler may answer differently from this float64 one only where a draw lies that close to an
edge of the CDF, so a comparison leaves out what depends on an item whose margin is under its bound.

`rule` names the statement ("spec") or one of the mutants the tests must tell apart from it:
  "counter"   the tempered draw taken on counter 128 + q (the Bot's) instead of 192 + q;
  "played"    `played` off by one: q + 1 in the draws' counters;
  "bmode"     network B's mode used for network A;
  "nosample"  the sample bits dropped from the key: every sample of a world plays sample 0's key.
"""
import numpy as np

import play_mode_model as MM
import playout_det_model as DM
import playout_model as PM
import playout_net_value_model as VM
import playout_net_versus_model as XM
from oracle import oracle as O

RANKS = PM.RANKS
RULES = ("spec", "counter", "played", "bmode", "nosample")
BOT, A, B = XM.BOT, XM.A, XM.B


def mode_cards(logits, masks, played, keys, mode, rule="spec"):
    """play_mode_model.play_mode on float32 logits under mode = (temperature, epsilon) -> (cards, margins): the margin counts
    only where the tempered draw decided the card (not at temperature 0, not for an exploring row)."""
    played = [q + 1 for q in played] if rule == "played" else played
    keep = MM.DRAW_SAMPLE
    try:
        if rule == "counter":
            MM.DRAW_SAMPLE = MM.DRAW_BOT
        out = MM.play_mode(np.asarray(logits, np.float64).astype(np.float32), masks, played, keys, mode[0], mode[1])
    finally:
        MM.DRAW_SAMPLE = keep
    return out["card"], np.where(out["explored"], np.inf, out["margin"])


def play_out(games, keys, viewers, WA, WB, own_rel, opp_rel, depth, value_scale, mode_a, mode_b, rule="spec"):
    """Plays every oracle Game of `games` (after its candidate card) in lock-step until it ends or stops.  Returns (results:
    four ints per item, info: per item dict(stopped, V, v, viewer, scores, margin, draws: the tempered draws it made))."""
    assert rule in RULES and 0 <= depth <= VM.MAX_DEPTH
    nets = {A: WA, B: WB}
    modes = {A: mode_b if rule == "bmode" else mode_a, B: mode_b}
    vnet = XM.viewer_net(opp_rel)
    m = len(games)
    left = [depth] * m
    res = [None] * m
    info = [dict(stopped=False, V=None, v=None, margin=np.inf, draws=0) for _ in range(m)]
    live = [i for i, h in enumerate(games) if not h.done]
    for i, h in enumerate(games):
        if h.done:
            res[i] = [int(x) for x in h.scores]
    while live:
        stop, roles = set(), {}
        for i in live:
            mover = games[i].seat()
            roles[i] = XM.role(viewers[i], mover, own_rel, opp_rel)
            if depth and mover == viewers[i]:
                left[i] -= 1
                if left[i] == 0:
                    stop.add(i)
        cards, value = {}, {}
        for net in (A, B):                            # one forward per network over the rows that need it
            rows = [i for i in live if (vnet if i in stop else roles[i]) == net]
            if not rows:
                continue
            out = VM.forward([games[i] for i in rows], nets[net])
            value.update((i, float(o[54])) for i, o in zip(rows, out) if i in stop)
            play = [(i, o) for i, o in zip(rows, out) if i not in stop]
            if play:
                hs = [games[i] for i, _ in play]
                qs = [int(h.g.trick_no) * 4 + int(h.g.n_in_trick) for h in hs]
                cs, ms = mode_cards([o[:54] for _, o in play], [h.legal() for h in hs], qs, [keys[i] for i, _ in play], modes[net], rule)
                for (i, _), c, mg in zip(play, cs, ms):
                    cards[i] = int(c)
                    if mg < np.inf:
                        info[i]["draws"] += 1
                        info[i]["margin"] = min(info[i]["margin"], float(mg))
        nxt = []
        for i in live:
            h = games[i]
            if i in stop:
                V = VM.points(value[i], value_scale)
                info[i].update(stopped=True, v=value[i], V=V)
                res[i] = [V if s == viewers[i] else 0 for s in range(4)]
                continue
            q = int(h.g.trick_no) * 4 + int(h.g.n_in_trick)
            c = O.policy_action(keys[i], q, h.legal()) if roles[i] == BOT else cards[i]
            r = h.step(c)
            assert r >= 0, "the card is legal"
            if r != 0:
                res[i] = [int(x) for x in h.scores]
            else:
                nxt.append(i)
        live = nxt
    for i in range(m):
        info[i].update(viewer=viewers[i], scores=res[i])
    return res, info


def items_of(kind, lanes, episode, seed, salt, gidx, seats, worlds, samples, word, rule="spec"):
    """[(rank j, world w, sample k, the world's Game with the candidate applied — a copy per sample —, the item's key)]."""
    game = O.Game.from_lanes(lanes)
    out = []
    if not PM.takes_part(game, seats):
        return out
    _, _, legal, played = PM.position(game)
    cards = PM.cards_of(legal)
    for j, w, h, key0 in VM.items_of(kind, lanes, episode, seed, salt, gidx, seats, worlds, word):
        assert key0 == DM.playout_key(seed, salt, gidx, episode, played, cards[j], w, 0)
        for k in range(samples):
            key = key0 if rule == "nosample" else DM.playout_key(seed, salt, gidx, episode, played, cards[j], w, k)
            out.append((j, w, k, PM.copy_of(h), key))
    return out


def playout_scores(kind, games, seed, salt, seats, worlds, samples, WA, WB, own_rel, opp_rel, depth, value_scale, mode_a, mode_b,
                   words=None, rule="spec"):
    """games: [(lanes, episode, gidx, seat set or None)], words: one per game (kinds voids / hidden) -> (scores
    [n, 12, worlds, samples, 4] int64, margin [n, 12, worlds, samples] (inf where no item or no tempered draw), info)."""
    out = np.zeros((len(games), RANKS, worlds, samples, 4), np.int64)
    margin = np.full((len(games), RANKS, worlds, samples), np.inf)
    where, hs, keys, viewers = [], [], [], []
    for g, (lanes, ep, gidx, s) in enumerate(games):
        viewer = O.Game.from_lanes(lanes).seat()
        for j, w, k, h, key in items_of(kind, lanes, ep, seed, salt, gidx, seats if s is None else s, worlds, samples,
                                        None if words is None else words[g], rule):
            where.append((g, j, w, k)); hs.append(h); keys.append(key); viewers.append(viewer)
    res, info = play_out(hs, keys, viewers, WA, WB, own_rel, opp_rel, depth, value_scale, mode_a, mode_b, rule)
    for at, sc, d in zip(where, res, info):
        out[at] = sc
        margin[at] = d["margin"]
    return out, margin, list(zip(where, info))


def playout_cards(kind, games, seed, salt, seats, worlds, samples, WA, WB, own_rel, opp_rel, depth, value_scale, mode_a, mode_b,
                  words=None, rule="spec"):
    """(sum [n, 12, 4] int64, cards [n] uint8, row_margin [n, 12]: the smallest margin of the row's items, info): the whole
    statement; the card rule is tarok_playout_cards'."""
    scores, margin, info = playout_scores(kind, games, seed, salt, seats, worlds, samples, WA, WB, own_rel, opp_rel, depth, value_scale,
                                          mode_a, mode_b, words, rule)
    sums = scores.sum(axis=(2, 3))
    acts = np.array([PM.card_of(lanes, seed, gidx, ep, seats if s is None else s, sums[g])
                     for g, (lanes, ep, gidx, s) in enumerate(games)], np.uint8)
    return sums, acts, margin.min(axis=(2, 3)), info


def rows_with_a_choice(games, seats=15):
    """[n, 12] bool: the rows (game, rank) that exist — a legal card of a game that takes part — and whose playouts have a
    card left to choose: the game is not in its last trick, where every seat holds one card."""
    out = np.zeros((len(games), RANKS), bool)
    for g, (lanes, ep, gidx, s) in enumerate(games):
        game = O.Game.from_lanes(lanes)
        if PM.takes_part(game, seats if s is None else s):
            _, _, legal, played = PM.position(game)
            out[g, :len(PM.cards_of(legal))] = played < 44     # after 44 cards every seat holds one card: all forced
    return out
