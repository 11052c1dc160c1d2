"""TEST INFRASTRUCTURE — the float-free statement of tarok_playout_exchange (include/tarok_env.h) on the CPU oracle.

The declarer's one decision before the first card — which talon group to pick up, which cards to lay down — valued by
determinized playouts.  Candidate (i, d): group i with the Bot sampler's discards under a key of its own; world w: the
three hands the DECLARER cannot see re-dealt (tests/playout_det_model.deal_pool, the viewer given explicitly: world_for);
playout (i, d, w, k): the candidate's exchange applied to the world, then all 48 cards by the Bot.  Everything here is the
oracle's (oracle/tarok_spec.py: game_key, bot_discards, deal, sample_setup; oracle/oracle.py: Game, Game.exchange) and
integer arithmetic; nothing comes from the code under test.

Candidate d, world w and sample k depend on none of the launch's sizes: `playout_scores` returns every single playout and
a smaller launch sums a corner of the same array (`sums_of`).
"""
import numpy as np

import playout_det_model as DM
import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

GROUPS = 6
MAX_SETS = 8
MAX_WORLDS = DM.MAX_WORLDS
MAX_SAMPLES = PM.MAX_SAMPLES
PHASE_EXCHANGE = 1
NO_CHOICE, PAD = -1, 255
FIELD_63 = 63                # the cards-played field of the world and playout keys: never a card count
M64 = (1 << 64) - 1


def candidate_key(seed, salt, gidx, episode, i, d):
    """ckey = game_key(seed ^ salt, gidx, 5 << 61 | ep << 28 | i << 6 | d)."""
    e = (5 << 61) | ((int(episode) & 0xFFFFFFFF) << 28) | (int(i) << 6) | int(d)
    return S.game_key((int(seed) ^ int(salt)) & M64, int(gidx), e)


def world_key(seed, salt, gidx, episode, w):
    """wkey = game_key(seed ^ salt, gidx, 7 << 61 | ep << 28 | 63 << 22 | w)."""
    e = (7 << 61) | ((int(episode) & 0xFFFFFFFF) << 28) | (FIELD_63 << 22) | int(w)
    return S.game_key((int(seed) ^ int(salt)) & M64, int(gidx), e)


def playout_key(seed, salt, gidx, episode, i, d, w, k):
    """pkey = game_key(seed ^ salt, gidx, 3 << 62 | ep << 28 | 63 << 22 | (8 i + d) << 16 | w << 10 | k)."""
    e = (3 << 62) | ((int(episode) & 0xFFFFFFFF) << 28) | (FIELD_63 << 22) | ((8 * int(i) + int(d)) << 16) | (int(w) << 10) | int(k)
    return S.game_key((int(seed) ^ int(salt)) & M64, int(gidx), e)


def waiting(game):
    return int(game.g.phase) == PHASE_EXCHANGE


def group_size(game):
    return S.GROUP_SIZE[int(game.g.contract)]


def group_mask(game, i):
    gs = group_size(game)
    m = 0
    for j in range(gs):
        m |= 1 << int(game.g.talon[i * gs + j])
    return m


def discards_under(game, i, key):
    """The Bot sampler's discards for group i under `key`: draws 68 + j on the discardable cards of hand | group."""
    g = game.g
    return S.bot_discards(key, int(g.hand[int(g.declarer)]) | group_mask(game, i), group_size(game))


def padded(discards):
    return list(discards) + [PAD] * (3 - len(discards))


def world_for(game, viewer, wkey):
    """A copy of `game` as world wkey of seat `viewer` sees it: the three other hands re-dealt by §8.4's walk, the team
    of a called king that lies among them set to the declarer and the seat that received it."""
    h = PM.copy_of(game)
    g = h.g
    oth = DM.others_of(viewer)
    pool = 0
    for o in oth:
        pool |= int(g.hand[o])
    masks = DM.deal_pool(pool, [bin(int(g.hand[o])).count("1") for o in oth], wkey)
    for o, m in zip(oth, masks):
        g.hand[o] = m
    if g.king >= 0:
        kb = 1 << (8 * int(g.king) + 7)
        if pool & kb:
            (holder,) = [o for o in oth if int(g.hand[o]) & kb]
            g.team = (1 << int(g.declarer)) | (1 << holder)
    return h


def takes_part(game, seats):
    return waiting(game) and bool((int(seats) >> int(game.g.declarer)) & 1)


def one_playout(world, i, discards, pkey):
    """The candidate's exchange on a copy of `world`, then every card by the Bot under pkey (draw 128 + q)."""
    h = PM.copy_of(world)
    assert h.exchange(i, discards) == 0, "a candidate's exchange is legal"
    return PM.one_playout(h, O.policy_action(pkey, 0, h.legal()), pkey, 0)


def playout_scores(lanes, episode, seed, salt, gidx, seats, worlds, samples, sets):
    """scores [6, sets, worlds, samples, 4] int64 of every playout (zeros for groups the contract does not have and for
    a game that does not take part) from canonical lanes (tarok_get_state's, one game)."""
    assert 1 <= worlds <= MAX_WORLDS and 1 <= samples <= MAX_SAMPLES and 1 <= sets <= MAX_SETS and 0 <= seats <= 15
    game = O.Game.from_lanes(lanes)
    out = np.zeros((GROUPS, sets, worlds, samples, 4), np.int64)
    if not takes_part(game, seats):
        return out
    declarer = int(game.g.declarer)
    ws = [world_for(game, declarer, world_key(seed, salt, gidx, episode, w)) for w in range(worlds)]
    for i in range(6 // group_size(game)):
        for d in range(sets):
            disc = discards_under(game, i, candidate_key(seed, salt, gidx, episode, i, d))
            for w in range(worlds):
                for k in range(samples):
                    out[i, d, w, k] = one_playout(ws[w], i, disc, playout_key(seed, salt, gidx, episode, i, d, w, k))
    return out


def sums_of(scores, worlds, samples, sets):
    """sum_out [6 * sets, 4] (row i * sets + d) of a launch at (worlds, samples, sets) <= the model run's."""
    return scores[:, :sets, :worlds, :samples].sum(axis=(2, 3)).reshape(GROUPS * sets, 4)


def choice_of(lanes, seed, salt, gidx, episode, seats, sums, sets):
    """(choice_out, discards_out [3]) of one game given its sums [6 * sets, 4]: the first candidate at the maximum of
    the declarer's sums where the game takes part; the Bot's exchange under the GAME's key where it waits with the
    declarer outside the set; -1 and 255s otherwise."""
    game = O.Game.from_lanes(lanes)
    if not waiting(game):
        return NO_CHOICE, [PAD] * 3
    if not takes_part(game, seats):
        return 0, padded(discards_under(game, 0, S.game_key(seed, gidx, episode)))
    declarer = int(game.g.declarer)
    best = 0
    for r in range(1, (6 // group_size(game)) * sets):
        if sums[r][declarer] > sums[best][declarer]:
            best = r
    i, d = divmod(best, sets)
    return i, padded(discards_under(game, i, candidate_key(seed, salt, gidx, episode, i, d)))


def playout_exchange(lanes, episode, seed, salt, gidx, seats, worlds, samples, sets):
    """(sum [6 * sets][4], choice, discards [3]) — the whole statement for one game."""
    sums = sums_of(playout_scores(lanes, episode, seed, salt, gidx, seats, worlds, samples, sets), worlds, samples, sets)
    return (sums,) + choice_of(lanes, seed, salt, gidx, episode, seats, sums, sets)


def deferred_game(seed, gidx, episode, mix):
    """The synthetic game (seed, gidx, episode) of `mix` as reset(defer_exchange=True) leaves it."""
    key = S.game_key(seed, gidx, episode)
    contract, declarer, king = S.sample_setup(key, mix)
    return O.Game(S.deal(key), contract, declarer, king)


def replay_pass(seed, mix, gidx, episode, seats, worlds, samples, sets, salt=0, cards=False):
    """One game of one pass on the oracle: the deferred game, the model's exchange (the playout player on `seats`, the
    Bot's own exchange elsewhere), then the cards.  cards=False is evaluate_exchange_vs_bot: the Bot plays every card.
    cards=True is evaluate_playout_vs_bot(samples, worlds=worlds, exchange=sets): the determinized player of
    tests/playout_det_model.py plays the cards of `seats` at the same (worlds, samples) and salt.
    Returns (choice, discards [3], actions [48] — 255 once the game is over —, final scores [4])."""
    g = deferred_game(seed, gidx, episode, mix)
    _, choice, disc = playout_exchange(g.lanes(), episode, seed, salt, gidx, seats, worlds, samples, sets)
    if waiting(g):
        assert g.exchange(choice, disc[:group_size(g)]) == 0
    key = S.game_key(seed, gidx, episode)
    actions = [PAD] * 48
    for t in range(48):
        if g.done:
            break
        if cards:
            _, card = DM.playout_cards(g.lanes(), episode, seed, salt, gidx, seats, worlds, samples)
        else:
            card = O.policy_action(key, t, g.legal())
        actions[t] = card
        assert g.step(card) >= 0
    assert g.done
    return choice, disc, actions, g.scores
