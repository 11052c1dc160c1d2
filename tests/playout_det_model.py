"""TEST INFRASTRUCTURE — the float-free statement of tarok_playout_cards_det (include/tarok_env.h) on the CPU oracle.

Determinized Monte-Carlo playouts: world w re-deals the cards the seat to move cannot see (the hands of the three other
seats) among those seats, sizes kept, and the playouts of tests/playout_model.py run on the re-dealt copy.  The oracle's
struct keeps hands, piles and talon apart, so a world is two writes on a copy of the game: `hand[o]` and `team`.
Everything here is the oracle's (oracle/tarok_spec.py: rng32, pick, game_key; oracle/oracle.py: Game) and integer
arithmetic; nothing comes from the code under test.

World w and sample k depend on neither `worlds` nor `samples`: `playout_scores` returns every single playout, and the sums
of a smaller launch are sums over a corner of the same array (`sums_of`).
"""
import numpy as np

import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

RANKS = PM.RANKS
MAX_WORLDS = 64
MAX_SAMPLES = PM.MAX_SAMPLES
NO_CARD = PM.NO_CARD
M64 = (1 << 64) - 1


def world_key(seed, salt, gidx, episode, played, w):
    """wkey = game_key(seed ^ salt, gidx, W), W = 7 << 61 | ep << 28 | played << 22 | w."""
    e = (7 << 61) | ((int(episode) & 0xFFFFFFFF) << 28) | (int(played) << 22) | int(w)
    return S.game_key((int(seed) ^ int(salt)) & M64, int(gidx), e)


def playout_key(seed, salt, gidx, episode, played, card, w, k):
    """pkey = game_key(seed ^ salt, gidx, D), D = 3 << 62 | ep << 28 | played << 22 | card << 16 | w << 10 | k."""
    e = (3 << 62) | ((int(episode) & 0xFFFFFFFF) << 28) | (int(played) << 22) | (int(card) << 16) | (int(w) << 10) | int(k)
    return S.game_key((int(seed) ^ int(salt)) & M64, int(gidx), e)


def others_of(seat):
    return [o for o in range(4) if o != seat]


def deal_pool(pool, caps, wkey):
    """The walk: the cards of `pool` in ascending number, card i on draw i of wkey, to the first of the three seats whose
    running interval holds r = pick(rng32(wkey, i), cap0 + cap1 + cap2).  Returns the three masks."""
    caps = list(caps)
    masks = [0, 0, 0]
    for i, c in enumerate(PM.cards_of(pool)):
        r = S.pick(S.rng32(wkey, i), caps[0] + caps[1] + caps[2])
        t = 0 if r < caps[0] else (1 if r < caps[0] + caps[1] else 2)
        masks[t] |= 1 << c
        caps[t] -= 1
    assert caps == [0, 0, 0]
    return masks


def world_of(game, wkey):
    """A copy of `game` (in play) as world wkey of the seat to move sees it: the other hands re-dealt, the team set."""
    h = PM.copy_of(game)
    g = h.g
    seat = game.seat()
    oth = others_of(seat)
    pool = 0
    for o in oth:
        pool |= int(g.hand[o])
    masks = deal_pool(pool, [bin(int(g.hand[o])).count("1") for o in oth], wkey)
    for o, m in zip(oth, masks):
        g.hand[o] = m
    if g.king >= 0:                                        # a contract with a called king (Tri, Dve, Ena)
        kb = 1 << (8 * int(g.king) + 7)
        if pool & kb:                                      # nobody at the mover's seat knows who holds it
            (holder,) = [o for o in oth if int(g.hand[o]) & kb]
            g.team = (1 << int(g.declarer)) | (1 << holder)
    return h


def playout_scores(lanes, episode, seed, salt, gidx, seats, worlds, samples):
    """scores [12, worlds, samples, 4] int64 of every playout (zeros beyond the legal cards and for a game that does not
    take part) from canonical lanes (tarok_get_state's, one game)."""
    assert 1 <= worlds <= MAX_WORLDS and 1 <= samples <= MAX_SAMPLES and 0 <= seats <= 15
    game = O.Game.from_lanes(lanes)
    out = np.zeros((RANKS, worlds, samples, 4), np.int64)
    if not PM.takes_part(game, seats):
        return out
    _, _, legal, played = PM.position(game)
    for w in range(worlds):
        world = world_of(game, world_key(seed, salt, gidx, episode, played, w))
        assert world.legal() == legal and world.seat() == game.seat()
        for j, c in enumerate(PM.cards_of(legal)):
            for k in range(samples):
                out[j, w, k] = PM.one_playout(world, c, playout_key(seed, salt, gidx, episode, played, c, w, k), played)
    return out


def sums_of(scores, worlds, samples):
    """sum_out [12, 4] of a launch at (worlds, samples) <= the model run's."""
    return scores[:, :worlds, :samples].sum(axis=(1, 2))


def playout_cards(lanes, episode, seed, salt, gidx, seats, worlds, samples):
    """(sum [12][4] int64, the card) — the whole statement for one game; the card rule is tarok_playout_cards'."""
    sums = sums_of(playout_scores(lanes, episode, seed, salt, gidx, seats, worlds, samples), worlds, samples)
    return sums, PM.card_of(lanes, seed, gidx, episode, seats, sums)


def replay_pass(seed, mix, gidx, episode, seats, worlds, samples, salt=0):
    """One game of one pass of evaluate_playout_vs_bot(worlds=...) on the oracle: the synthetic game (seed, gidx, episode)
    of `mix` played to its end with the model's card at every move (the determinized player on `seats`, the Bot
    elsewhere).  Returns (actions [48] — 255 once the game is over —, final scores [4])."""
    g = O.Game.synth(seed, gidx, episode, mix)
    actions = [NO_CARD] * 48
    for t in range(48):
        if g.done:
            break
        _, card = playout_cards(g.lanes(), episode, seed, salt, gidx, seats, worlds, samples)
        actions[t] = card
        assert g.step(card) >= 0
    assert g.done
    return actions, g.scores
