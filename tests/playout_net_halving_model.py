"""TEST INFRASTRUCTURE — the statement of tarok_playout_cards_net_halving (include/tarok_env.h) over the rows of the existing
net launch.

World w and the item key of a net playout depend on no launch size, so a rank that has played the worlds below the
cumulative end e has, as its row, the existing net launch's row at worlds = e.  Given those rows at every cumulative end —
from tarok_playout_cards_net / _voids / _hidden / _value on the GPU, or from tests/playout_net_model.py,
playout_net_worlds_model.py or playout_net_value_model.py on the CPU — the rounds are walked here with the survivor rule of
tests/playout_halving_model.py.  Integer arithmetic; nothing comes from the code under test.
"""
import numpy as np

import playout_halving_model as HM

RANKS = HM.RANKS
ALIVE_BOUNDS = (12, 6, 3, 2)                        # a_0 = 12, a_{r+1} = ceil(a_r / 2): the most ranks alive in round r


def walk(rows, nlegal, mover, round_worlds):
    """One game that takes part.  rows: per round r the existing launch's [12, 4] sums at worlds = e_r (the cumulative end).
    Returns (sum [12,4] int64, count [12] int64, the ranks alive after the last round played, flags) — flags: `tie` (a cut
    fell between two equal mover's sums), `early` (the game was down to one card before the last round)."""
    ends = HM.ends_of(round_worlds)
    assert len(rows) == len(ends)
    sums, count = np.zeros((RANKS, 4), np.int64), np.zeros(RANKS, np.int64)
    alive, flags = list(range(nlegal)), dict(tie=False, early=False)
    for r, e in enumerate(ends):
        if r > 0 and len(alive) == 1:
            flags["early"] = True
            break
        for j in alive:
            sums[j], count[j] = np.asarray(rows[r][j], np.int64), e
        if r + 1 < len(ends):
            kept = HM.survivors(sums[:, mover], alive)
            out = [j for j in alive if j not in kept]
            if out and min(int(sums[j, mover]) for j in kept) == max(int(sums[j, mover]) for j in out):
                flags["tie"] = True
            alive = kept
    return sums, count, alive, flags


def card_rank(sums, alive, mover):
    """The launch's rank among the ranks alive: the lowest at the maximum of the mover's sum."""
    return min(alive, key=lambda j: (-int(sums[j, mover]), j))


def launch(rows, legal_words, takes_part, round_worlds, last_actions):
    """A whole batch.  rows: per round [n, 12, 4] sums of the existing launch at the cumulative ends; legal_words [n] u64:
    the observation words (legal mask in bits 0..53, the mover in bits 54..55); takes_part [n] bool; last_actions [n] u8:
    the existing launch's cards (the Bot's card or 255 where a game does not take part).
    Returns (sum [n,12,4] int64, count [n,12] int64, action [n] u8, flags per game)."""
    n = len(legal_words)
    sums, count = np.zeros((n, RANKS, 4), np.int64), np.zeros((n, RANKS), np.int64)
    action, flags = np.array(last_actions, np.uint8).copy(), [None] * n
    for g in range(n):
        if not takes_part[g]:
            continue
        word = int(legal_words[g])
        cards = [c for c in range(54) if (word >> c) & 1]
        mover = (word >> 54) & 3
        sums[g], count[g], alive, flags[g] = walk([r[g] for r in rows], len(cards), mover, round_worlds)
        action[g] = cards[card_rank(sums[g], alive, mover)]
    return sums, count, action, flags


def item_fraction(nlegal, round_worlds):
    """The items a game of nlegal cards plays under the schedule, over the uniform launch's nlegal * W (no early exit but
    the one-card rule; the ranks alive follow ceil(k / 2))."""
    k, items = nlegal, 0
    for r, w in enumerate(round_worlds):
        if r > 0 and k == 1:
            break
        items += k * int(w)
        k = max(1, (k + 1) // 2)
    return items / float(nlegal * sum(int(w) for w in round_worlds))
