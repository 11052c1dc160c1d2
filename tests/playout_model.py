"""TEST INFRASTRUCTURE — the float-free statement of tarok_playout_cards (include/tarok_env.h) on the CPU oracle, per game.

Open-hand Monte-Carlo playouts: every legal card of the seat to move is played and the game finished `samples` times by
the Bot, on the TRUE hidden hands; the final scores are summed.  Everything here is the oracle's (oracle/oracle.py:
game_key, policy_action, Game.step / legal / scores) and integer arithmetic; nothing comes from the code under test.

Sample k of a card does not depend on `samples`, so `playout_scores` returns the scores of every single playout and the
sums for any smaller `samples` are prefix sums of the same array (`sums_of`): one model run serves several launches.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O

RANKS = 12
MAX_SAMPLES = 1024
NO_CARD = 255
PHASE_PLAY = 2
DRAW_POLICY = 128            # O.policy_action(key, q, legal) is the uniform legal card of draw 128 + q


def cards_of(mask):
    return [c for c in range(54) if (int(mask) >> c) & 1]


def position(game):
    """(in play, seat to move, legal mask, cards played) of an oracle Game."""
    g = game.g
    if g.phase != PHASE_PLAY:
        return False, 0, 0, 0
    return True, game.seat(), game.legal(), int(g.trick_no) * 4 + int(g.n_in_trick)


def playout_key(seed, salt, gidx, episode, played, card, k):
    """pkey = game_key(seed ^ salt, gidx, E), E = 1 << 63 | ep << 28 | played << 22 | card << 16 | k."""
    e = (1 << 63) | ((int(episode) & 0xFFFFFFFF) << 28) | (int(played) << 22) | (int(card) << 16) | int(k)
    return O.game_key((int(seed) ^ int(salt)) & ((1 << 64) - 1), gidx, e)


def copy_of(game):
    h = O.Game()
    C.memmove(C.byref(h.g), C.byref(game.g), C.sizeof(O.ToGame))
    return h


def one_playout(game, card, key, played):
    """The four final scores of `game` after `card` and the Bot's cards to the end (the game is not changed)."""
    h = copy_of(game)
    r = h.step(card)
    assert r >= 0, "the candidate card is legal"
    q = played + 1
    while r == 0:
        r = h.step(O.policy_action(key, q, h.legal()))
        assert r >= 0
        q += 1
    return h.scores


def takes_part(game, seats):
    in_play, seat, _, _ = position(game)
    return in_play and bool((int(seats) >> seat) & 1)


def playout_scores(lanes, episode, seed, salt, gidx, seats, samples):
    """scores [12, samples, 4] int64 of every playout (zeros beyond the legal cards and for a game that does not take
    part) from canonical lanes (tarok_get_state's, one game)."""
    assert 1 <= samples <= MAX_SAMPLES and 0 <= seats <= 15
    game = O.Game.from_lanes(lanes)
    out = np.zeros((RANKS, samples, 4), np.int64)
    if not takes_part(game, seats):
        return out
    _, _, legal, played = position(game)
    for j, c in enumerate(cards_of(legal)):
        for k in range(samples):
            out[j, k] = one_playout(game, c, playout_key(seed, salt, gidx, episode, played, c, k), played)
    return out


def sums_of(scores, samples):
    """sum_out [12, 4] for `samples` <= the model run's: the first `samples` playouts of every card."""
    return scores[:, :samples].sum(axis=1)


def card_of(lanes, seed, gidx, episode, seats, sums):
    """action_out of one game, given its sums [12, 4]: the lowest-ranked legal card at the maximum of the mover's sums
    where the game takes part, the Bot's card (policy_action under the GAME's key, draw 128 + played) where it is in play
    with the mover outside the set, 255 otherwise."""
    game = O.Game.from_lanes(lanes)
    in_play, seat, legal, played = position(game)
    if not in_play:
        return NO_CARD
    if not (int(seats) >> seat) & 1:
        return O.policy_action(O.game_key(seed, gidx, episode), played, legal)
    cards = cards_of(legal)
    best = 0
    for j in range(1, len(cards)):
        if sums[j][seat] > sums[best][seat]:
            best = j
    return cards[best]


def playout_cards(lanes, episode, seed, salt, gidx, seats, samples):
    """(sum [12][4] int64, the card) — the whole statement for one game."""
    sums = sums_of(playout_scores(lanes, episode, seed, salt, gidx, seats, samples), samples)
    return sums, card_of(lanes, seed, gidx, episode, seats, sums)


def playout_values_loop(sums, words, samples):
    """tarok_amd.env.playout_values as a loop: [N, 54] float32."""
    n = len(words)
    out = np.full((n, 54), -np.inf, np.float32)
    for i in range(n):
        w = int(words[i]) & ((1 << 64) - 1)
        seat = (w >> 54) & 3
        for j, c in enumerate(cards_of(w & ((1 << 54) - 1))):
            out[i, c] = np.float32(np.float32(int(sums[i][j][seat])) / np.float32(samples))
    return out


def replay_pass(seed, mix, gidx, episode, seats, samples, salt=0):
    """One game of one pass of evaluate_playout_vs_bot on the oracle: the synthetic game (seed, gidx, episode) of `mix`
    played to its end with the model's card at every move (the playout player on `seats`, the Bot elsewhere).
    Returns (actions [48] — 255 once the game is over —, final scores [4])."""
    g = O.Game.synth(seed, gidx, episode, mix)
    actions = [NO_CARD] * 48
    for t in range(48):
        if g.done:
            break
        _, card = playout_cards(g.lanes(), episode, seed, salt, gidx, seats, samples)
        actions[t] = card
        assert g.step(card) >= 0
    assert g.done
    return actions, g.scores
