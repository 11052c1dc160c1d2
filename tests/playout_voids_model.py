"""TEST INFRASTRUCTURE — the float-free statement of tarok_shown_voids and tarok_playout_cards_voids (include/tarok_env.h)
on the CPU oracle.

Void-aware determinized playouts: the worlds of tests/playout_det_model.py, drawn uniformly among the re-deals that also
give no seat a card of a class the play has shown it void in.  Everything here is the oracle's (oracle/tarok_spec.py:
rng32, pick; oracle/oracle.py: Game, to_trick_winner), math.comb and integer arithmetic; nothing comes from the code under
test.  The helpers are shaped like playout_det_model.py's, with the void word as one more argument.
"""
import ctypes as C
import math

import numpy as np

import playout_det_model as DM
import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

RANKS = PM.RANKS
NO_CARD = PM.NO_CARD
M64 = (1 << 64) - 1
BERAC, ODPRTI_BERAC = 7, 9
DRAW_AB = 64                  # draws 64 and 65 of the world key: the pair (a, b)
DRAW_SPLIT = 128              # draw 128 + i: card i of the pool between o1 and o2


def card_class(c):
    return min(int(c) >> 3, 4)


def class_cards(bits):
    """The cards of the classes whose bits are set in a 5-bit void field."""
    m = 0
    for k in range(5):
        if (bits >> k) & 1:
            m |= S.SUIT[k]
    return m


def first_leader(contract, declarer):
    return int(declarer) if int(contract) in (BERAC, ODPRTI_BERAC) else 0


def shown_voids(cards, first_leader):
    """The void word of a game from the cards played so far, in order, and the seat that led the first trick."""
    word, lead = 0, int(first_leader)
    for t in range(0, len(cards), 4):
        trick = [int(c) for c in cards[t:t + 4]]
        led = card_class(trick[0])
        for j in range(1, len(trick)):
            seat, k = (lead + j) & 3, card_class(trick[j])
            if k != led:
                word |= 1 << (5 * seat + led)
                if k != 4 and led != 4:
                    word |= 1 << (5 * seat + 4)
        if len(trick) == 4:
            lead = (lead + O.lib().to_trick_winner(O.u8arr(trick))) & 3
    return word


def voids_of_lanes(lanes, hist_column):
    """The void word of one game from its canonical lanes and its column of the history [48]: 0 unless in play."""
    game = O.Game.from_lanes(lanes)
    in_play, _, _, played = PM.position(game)
    if not in_play:
        return 0
    return shown_voids([int(x) for x in hist_column[:played]], first_leader(game.g.contract, game.g.declarer))


def allowed_of(pool, others, voids):
    """allowed[i] = the cards of the pool the i-th other seat may hold under the void word."""
    return [int(pool) & ~class_cards((int(voids) >> (5 * o)) & 31) for o in others]


def groups_of(pool, allowed):
    a0, a1, a2 = allowed
    return dict(F=[a0 & ~(a1 | a2), a1 & ~(a0 | a2), a2 & ~(a0 | a1)], G01=a0 & a1 & ~a2, G02=a0 & a2 & ~a1, G12=a1 & a2 & ~a0,
                Q=a0 & a1 & a2, E=int(pool) & ~(a0 | a1 | a2))


def count_voids(pool, caps, allowed):
    """(Total, {(a, b): T(a, b)} in drawing order, the group dict, [r0, r1, r2]); Total is None when the position falls
    back before the count (a card without an allowed seat, or a negative r_i)."""
    gr = groups_of(pool, allowed)
    r = [int(caps[i]) - S.popcount(gr["F"][i]) for i in range(3)]
    if gr["E"] or min(r) < 0:
        return None, {}, gr, r
    n01, n02, n12, q = (S.popcount(gr[k]) for k in ("G01", "G02", "G12", "Q"))
    weights = {}
    for a in range(n01 + 1):
        for b in range(n02 + 1):
            s0, r1p, r2p = r[0] - a - b, r[1] - (n01 - a), r[2] - (n02 - b)
            if 0 <= s0 <= q and r1p >= 0 and r2p >= 0 and r1p <= n12 + q - s0:
                weights[(a, b)] = math.comb(n01, a) * math.comb(n02, b) * math.comb(q, s0) * math.comb(n12 + q - s0, r1p)
            else:
                weights[(a, b)] = 0
    return sum(weights.values()), weights, gr, r


def deal_voids(pool, caps, allowed, wkey):
    """The three masks of the constrained re-deal, or None where the definition falls back to the plain walk (an empty
    allowed set, a negative r_i, no consistent deal).  The all-zero void word is the caller's case (world_of)."""
    total, weights, gr, r = count_voids(pool, caps, allowed)
    if not total:
        return None
    big = (S.rng32(wkey, DRAW_AB) << 32) | S.rng32(wkey, DRAW_AB + 1)
    u = (big * total) >> 64
    run, pair = 0, None
    for ab, t in weights.items():                             # insertion order: a outer, b inner, both ascending
        run += t
        if run > u:
            pair = ab
            break
    a, b = pair
    n01, n02, q = S.popcount(gr["G01"]), S.popcount(gr["G02"]), S.popcount(gr["Q"])
    c01, c02 = [a, n01 - a], [b, n02 - b]
    k0, kq = r[0] - a - b, q
    k1, k2 = r[1] - (n01 - a), r[2] - (n02 - b)
    masks = list(gr["F"])
    for i, c in enumerate(PM.cards_of(pool)):
        bit = 1 << c
        if bit & gr["G01"]:
            t = 0 if S.pick(S.rng32(wkey, i), c01[0] + c01[1]) < c01[0] else 1
            c01[t] -= 1
            masks[t] |= bit
        elif bit & gr["G02"]:
            t = 0 if S.pick(S.rng32(wkey, i), c02[0] + c02[1]) < c02[0] else 1
            c02[t] -= 1
            masks[2 * t] |= bit
        elif bit & (gr["Q"] | gr["G12"]):
            if bit & gr["Q"]:
                mine = S.pick(S.rng32(wkey, i), kq) < k0
                kq -= 1
                if mine:
                    k0 -= 1
                    masks[0] |= bit
                    continue
            if S.pick(S.rng32(wkey, DRAW_SPLIT + i), k1 + k2) < k1:
                k1 -= 1
                masks[1] |= bit
            else:
                k2 -= 1
                masks[2] |= bit
    assert c01 == [0, 0] and c02 == [0, 0] and (k0, kq, k1, k2) == (0, 0, 0, 0)
    return masks


def world_of(game, wkey, voids):
    """A copy of `game` (in play) as world wkey of the seat to move sees it under the void word."""
    seat = game.seat()
    oth = DM.others_of(seat)
    if not any((int(voids) >> (5 * o)) & 31 for o in oth):
        return DM.world_of(game, wkey)
    g0 = game.g
    pool = 0
    for o in oth:
        pool |= int(g0.hand[o])
    masks = deal_voids(pool, [S.popcount(int(g0.hand[o])) for o in oth], allowed_of(pool, oth, voids), wkey)
    if masks is None:
        return DM.world_of(game, wkey)
    h = PM.copy_of(game)
    g = h.g
    for o, m in zip(oth, masks):
        g.hand[o] = m
    if g.king >= 0:
        kb = 1 << (8 * int(g.king) + 7)
        if pool & kb:
            (holder,) = [o for o in oth if int(g.hand[o]) & kb]
            g.team = (1 << int(g.declarer)) | (1 << holder)
    return h


def playout_scores(lanes, episode, seed, salt, gidx, seats, worlds, samples, voids):
    """scores [12, worlds, samples, 4] int64 of every playout, as playout_det_model.playout_scores, under the void word."""
    assert 1 <= worlds <= DM.MAX_WORLDS and 1 <= samples <= DM.MAX_SAMPLES and 0 <= seats <= 15
    game = O.Game.from_lanes(lanes)
    out = np.zeros((RANKS, worlds, samples, 4), np.int64)
    if not PM.takes_part(game, seats):
        return out
    _, _, legal, played = PM.position(game)
    for w in range(worlds):
        world = world_of(game, DM.world_key(seed, salt, gidx, episode, played, w), voids)
        assert world.legal() == legal and world.seat() == game.seat()
        for j, c in enumerate(PM.cards_of(legal)):
            for k in range(samples):
                out[j, w, k] = PM.one_playout(world, c, DM.playout_key(seed, salt, gidx, episode, played, c, w, k), played)
    return out


sums_of = DM.sums_of


def playout_cards(lanes, episode, seed, salt, gidx, seats, worlds, samples, voids):
    """(sum [12][4] int64, the card) — the whole statement for one game; the card rule is tarok_playout_cards'."""
    sums = sums_of(playout_scores(lanes, episode, seed, salt, gidx, seats, worlds, samples, voids), worlds, samples)
    return sums, PM.card_of(lanes, seed, gidx, episode, seats, sums)


def replay_pass(seed, mix, gidx, episode, seats, worlds, samples, salt=0):
    """One game of one pass of evaluate_playout_vs_bot(worlds=..., voids=True) on the oracle: the void word is rebuilt from
    the cards played so far at every move.  Returns (actions [48] — 255 once the game is over —, final scores [4])."""
    g = O.Game.synth(seed, gidx, episode, mix)
    lead = first_leader(g.g.contract, g.g.declarer)
    actions = [NO_CARD] * 48
    cards = []
    for t in range(48):
        if g.done:
            break
        _, card = playout_cards(g.lanes(), episode, seed, salt, gidx, seats, worlds, samples, shown_voids(cards, lead))
        actions[t] = card
        cards.append(card)
        assert g.step(card) >= 0
    assert g.done
    return actions, g.scores


def bot_game(seed, gidx, episode, mix, cards):
    """(the synthetic game after `cards` Bot cards or at its end, the cards played, the first leader): what the tests play."""
    g = O.Game.synth(seed, gidx, episode, mix)
    lead = first_leader(g.g.contract, g.g.declarer)
    key = O.game_key(seed, gidx, episode)
    played = []
    for q in range(cards):
        if g.done:
            break
        c = O.policy_action(key, q, g.legal())
        played.append(c)
        g.step(c)
    return g, played, lead


def true_voids(game):
    """The largest sound void word of a position: every (seat, class) of which the seat's hand holds no card."""
    word = 0
    for s in range(4):
        for k in range(5):
            if not int(game.g.hand[s]) & S.SUIT[k]:
                word |= 1 << (5 * s + k)
    return word
