"""TEST INFRASTRUCTURE — the float-free statement of tarok_played_cards and tarok_playout_cards_hidden
(include/tarok_env.h) on the CPU oracle.

Determinized playouts whose worlds also re-deal what only other seats have seen: in a Klop the face-down talon cards
nobody has been given yet, in Tri .. Solo_ena the declarer's discards when another seat is to move.  The oracle's struct
keeps hands, piles and talon apart, so a world is a few writes on a copy of the game: `hand[o]`, `talon[slot]`,
`pile[declarer]` and `team`.  Everything here is the oracle's (oracle/tarok_spec.py: rng32, pick, DISCARDABLE, GROUP_SIZE;
oracle/oracle.py: Game) and integer arithmetic; nothing comes from the code under test.  The helpers are shaped like
playout_det_model.py's, with the word of played cards as one more argument.
"""
import numpy as np

import playout_det_model as DM
import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

RANKS = PM.RANKS
NO_CARD = PM.NO_CARD
KLOP = 0
EXCHANGE_CONTRACTS = (1, 2, 3, 4, 5, 6)          # Tri, Dve, Ena, Solo_tri, Solo_dve, Solo_ena
DRAW_DISCARD = 256                               # draw 256 + i: card i of the discardable pool
DRAW_SLOT = 320                                  # draw 320 + j: the slot of the j-th new talon card


def mask_of(cards):
    m = 0
    for c in cards:
        m |= 1 << int(c)
    return m


def played_of_lanes(lanes, hist_column):
    """The word of one game from its canonical lanes and its column of the history [48]: the first `played` entries
    of a game in play or finished, nothing of a game that waits."""
    g = O.Game.from_lanes(lanes).g
    if g.phase < PM.PHASE_PLAY:
        return 0
    return mask_of(hist_column[:int(g.trick_no) * 4 + int(g.n_in_trick)])


def deal_four(pool, caps, wkey):
    """The ascending walk with four running capacities (o0, o1, o2, the talon): card i on draw i of wkey."""
    caps = list(caps)
    masks = [0, 0, 0, 0]
    for i, c in enumerate(PM.cards_of(pool)):
        r = S.pick(S.rng32(wkey, i), sum(caps))
        t, run = 0, caps[0]
        while r >= run:
            t += 1
            run += caps[t]
        masks[t] |= 1 << c
        caps[t] -= 1
    assert caps == [0, 0, 0, 0]
    return masks


def hidden_discards(game, viewer, played):
    """The declarer's discards where they are hidden from `viewer` and re-dealt, else 0."""
    g = game.g
    if int(g.contract) not in EXCHANGE_CONTRACTS or g.phase != PM.PHASE_PLAY or int(g.declarer) == viewer:
        return 0
    d = int(g.pile[int(g.declarer)]) & ~int(played)
    if S.popcount(d) != S.GROUP_SIZE[int(g.contract)] or d & ~S.DISCARDABLE:
        return 0                                            # (the reference's "too few discardable cards": they stay seen)
    return d


def pick_discards(pool, n, wkey):
    """A uniform n-subset of the discardable cards of `pool`, sequentially: card i of their ascending walk is taken when
    pick(rng32(wkey, 256 + i), cards left) is below the number still needed."""
    cards = PM.cards_of(pool & S.DISCARDABLE)
    out, need = 0, n
    for i, c in enumerate(cards):
        if S.pick(S.rng32(wkey, DRAW_DISCARD + i), len(cards) - i) < need:
            out |= 1 << c
            need -= 1
    assert need == 0
    return out


def set_team(g, oth, pool):
    if g.king >= 0:
        kb = 1 << (8 * int(g.king) + 7)
        if pool & kb:
            (holder,) = [o for o in oth if int(g.hand[o]) & kb]
            g.team = (1 << int(g.declarer)) | (1 << holder)


def world_for(game, wkey, played, viewer=None):
    """A copy of `game` as world wkey of `viewer` (default: the seat to move) sees it, given the word of played cards."""
    viewer = game.seat() if viewer is None else int(viewer)
    oth = DM.others_of(viewer)
    h = PM.copy_of(game)
    g = h.g
    hands = [int(g.hand[o]) for o in oth]
    caps = [S.popcount(x) for x in hands]
    pool = hands[0] | hands[1] | hands[2]
    tl = int(g.talon_left)
    if int(g.contract) == KLOP and tl > 0:
        masks = deal_four(pool | mask_of(g.talon[i] for i in range(tl)), caps + [tl], wkey)
        for o, m in zip(oth, masks):
            g.hand[o] = m
        free = list(range(tl))
        for j, c in enumerate(PM.cards_of(masks[3])):
            g.talon[free.pop(S.pick(S.rng32(wkey, DRAW_SLOT + j), len(free)))] = c
        assert not free
        return h
    disc = hidden_discards(game, viewer, played)
    new = pick_discards(pool | disc, S.popcount(disc), wkey) if disc else 0
    masks = DM.deal_pool((pool | disc) & ~new, caps, wkey)
    for o, m in zip(oth, masks):
        g.hand[o] = m
    d = int(g.declarer)
    g.pile[d] = (int(g.pile[d]) & ~disc) | new
    set_team(g, oth, pool)
    return h


def playout_scores(lanes, episode, seed, salt, gidx, seats, worlds, samples, played):
    """scores [12, worlds, samples, 4] int64 of every playout, as playout_det_model.playout_scores, given the word."""
    assert 1 <= worlds <= DM.MAX_WORLDS and 1 <= samples <= DM.MAX_SAMPLES and 0 <= seats <= 15
    game = O.Game.from_lanes(lanes)
    out = np.zeros((RANKS, worlds, samples, 4), np.int64)
    if not PM.takes_part(game, seats):
        return out
    _, _, legal, n = PM.position(game)
    for w in range(worlds):
        world = world_for(game, DM.world_key(seed, salt, gidx, episode, n, w), played)
        assert world.legal() == legal and world.seat() == game.seat()
        for j, c in enumerate(PM.cards_of(legal)):
            for k in range(samples):
                out[j, w, k] = PM.one_playout(world, c, DM.playout_key(seed, salt, gidx, episode, n, c, w, k), n)
    return out


sums_of = DM.sums_of


def playout_cards(lanes, episode, seed, salt, gidx, seats, worlds, samples, played):
    """(sum [12][4] int64, the card) — the whole statement for one game; the card rule is tarok_playout_cards'."""
    sums = sums_of(playout_scores(lanes, episode, seed, salt, gidx, seats, worlds, samples, played), worlds, samples)
    return sums, PM.card_of(lanes, seed, gidx, episode, seats, sums)


def replay_pass(seed, mix, gidx, episode, seats, worlds, samples, salt=0, exchange=None):
    """One game of one pass of evaluate_playout_vs_bot(worlds=..., hidden=True) on the oracle: the word is rebuilt from
    the cards played so far at every move.  exchange=D: the game starts deferred and the model of
    tests/playout_exchange_model.py makes the exchange first.  Returns (actions [48] — 255 once the game is over —,
    final scores [4])."""
    if exchange is None:
        g = O.Game.synth(seed, gidx, episode, mix)
    else:
        import playout_exchange_model as XM
        g = XM.deferred_game(seed, gidx, episode, mix)
        _, choice, disc = XM.playout_exchange(g.lanes(), episode, seed, salt, gidx, seats, worlds, samples, exchange)
        if XM.waiting(g):
            assert g.exchange(choice, disc[:XM.group_size(g)]) == 0
    actions = [NO_CARD] * 48
    played = 0
    for t in range(48):
        if g.done:
            break
        _, card = playout_cards(g.lanes(), episode, seed, salt, gidx, seats, worlds, samples, played)
        actions[t] = card
        played |= 1 << card
        assert g.step(card) >= 0
    assert g.done
    return actions, g.scores


def bot_game(seed, gidx, episode, mix, cards):
    """(the synthetic game after `cards` Bot cards or at its end, the word of the cards played)."""
    g = O.Game.synth(seed, gidx, episode, mix)
    key = O.game_key(seed, gidx, episode)
    played = 0
    for q in range(cards):
        if g.done:
            break
        c = O.policy_action(key, q, g.legal())
        played |= 1 << c
        g.step(c)
    return g, played
