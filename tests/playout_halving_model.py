"""TEST INFRASTRUCTURE — the statement of tarok_playout_cards_halving and tarok_playout_targets_counts (include/tarok_env.h)
on the CPU oracle.

Sequential halving over the worlds of tests/playout_det_model.py / playout_voids_model.py / playout_hidden_model.py: the
single playouts are those models' `playout_scores` arrays [12, W, S, 4] (world w and sample k depend on no launch size), the
rounds and the survivor rule are written here from the definition, with a plain sort.  Integer arithmetic; nothing comes
from the code under test.  The counts-target statement is float64 numpy with a bound derived from the number formats.
"""
import numpy as np

import distill_model as DI
import playout_model as PM

RANKS = PM.RANKS
KINDS = ("det", "voids", "hidden")
MAX_ROUNDS = 4


def survivors(values, alive):
    """The ranks of `alive` that stay after a round that is not the last: the max(1, ceil(k / 2)) with the highest value,
    ties to the lower rank — a sort by (value descending, rank ascending)."""
    alive = sorted(alive)
    keep = max(1, (len(alive) + 1) // 2) if alive else 0
    order = sorted(alive, key=lambda j: (-int(values[j]), j))
    return sorted(order[:keep])


def ends_of(round_worlds):
    assert 1 <= len(round_worlds) <= MAX_ROUNDS and all(int(w) >= 1 for w in round_worlds)
    return np.cumsum([int(w) for w in round_worlds]).tolist()


def halve(scores, nlegal, mover, round_worlds, samples, rule=survivors):
    """(sum [12,4] int64, count [12] int64, the ranks alive after the last round played) from a model's single playouts
    scores [12, >= W, >= samples, 4] for a game that takes part with nlegal legal cards."""
    sums, count = np.zeros((RANKS, 4), np.int64), np.zeros(RANKS, np.int64)
    alive, e0 = list(range(nlegal)), 0
    ends = ends_of(round_worlds)
    for r, e1 in enumerate(ends):
        if r > 0 and len(alive) == 1:                       # a game with one card alive plays no further round
            break
        for j in alive:
            sums[j] += scores[j, e0:e1, :samples].sum(axis=(0, 1))
            count[j] = e1 * samples
        if r + 1 < len(ends):
            alive = rule(sums[:, mover], alive)
        e0 = e1
    return sums, count, alive


def model_scores(kind, lanes, episode, seed, salt, gidx, seats, worlds, samples, word=None):
    """The kind's single playouts [12, worlds, samples, 4]."""
    if kind == "det":
        import playout_det_model as M
        return M.playout_scores(lanes, episode, seed, salt, gidx, seats, worlds, samples)
    if kind == "voids":
        import playout_voids_model as M
    else:
        import playout_hidden_model as M
    return M.playout_scores(lanes, episode, seed, salt, gidx, seats, worlds, samples, int(word))


def playout_cards_halving(kind, lanes, episode, seed, salt, gidx, seats, round_worlds, samples, word=None, scores=None):
    """(sum [12,4], count [12], the card) — the whole statement for one game.  scores: the kind's single playouts at
    (>= W, >= samples), where the caller has them already."""
    from oracle import oracle as O
    game = O.Game.from_lanes(lanes)
    sums, count = np.zeros((RANKS, 4), np.int64), np.zeros(RANKS, np.int64)
    if not PM.takes_part(game, seats):
        return sums, count, PM.card_of(lanes, seed, gidx, episode, seats, sums)
    _, mover, legal, _ = PM.position(game)
    cards = PM.cards_of(legal)
    if scores is None:
        scores = model_scores(kind, lanes, episode, seed, salt, gidx, seats, sum(int(w) for w in round_worlds), samples, word)
    sums, count, alive = halve(scores, len(cards), mover, round_worlds, samples)
    best = min(alive, key=lambda j: (-int(sums[j, mover]), j))
    return sums, count, cards[best]


def replay_pass(seed, mix, gidx, episode, seats, round_worlds, samples, salt=0):
    """One game of one pass of evaluate_playout_vs_bot(halving=...) on the oracle (the det kind): (actions [48], scores)."""
    from oracle import oracle as O
    g = O.Game.synth(seed, gidx, episode, mix)
    actions = [PM.NO_CARD] * 48
    for t in range(48):
        if g.done:
            break
        _, _, card = playout_cards_halving("det", g.lanes(), episode, seed, salt, gidx, seats, round_worlds, samples)
        actions[t] = card
        assert g.step(card) >= 0
    assert g.done
    return actions, g.scores


# ---- tarok_playout_targets_counts
def targets_counts_reference(sums, counts, words, tau, sets):
    """(q [N,64] float64, has [N], card [N] — the tau = 0 card, 255 without a teacher or without a counted rank, M [N] —
    the largest |mean| among the counted ranks) from the definition: m_j = sum / count on the ranks j < nl with count > 0."""
    sums, counts = np.asarray(sums).astype(np.int64), np.asarray(counts).astype(np.int64)
    n = sums.shape[0]
    words = [int(w) & ((1 << 64) - 1) for w in np.asarray(words).reshape(-1).tolist()]
    sets = np.broadcast_to(np.asarray(sets), (n,))
    q, has, card, big = np.zeros((n, 64), np.float64), np.zeros(n, bool), np.full(n, 255, np.int64), np.zeros(n, np.float64)
    for g in range(n):
        legal, s = words[g] & ((1 << 54) - 1), (words[g] >> 54) & 3
        if legal == 0 or not (int(sets[g]) >> s) & 1:
            continue
        has[g] = True
        cards = DI.cards_of(legal)[:RANKS]
        on = [j for j in range(len(cards)) if counts[g, j] > 0]
        if not on:
            continue
        m = {j: float(sums[g, j, s]) / float(counts[g, j]) for j in on}
        big[g] = max(abs(v) for v in m.values())
        cmax = max(int(counts[g, j]) for j in on)
        top = [j for j in on if counts[g, j] == cmax]
        best = min(top, key=lambda j: (-int(sums[g, j, s]), j))       # equal counts: the sums order the means exactly
        card[g] = cards[best]
        if tau == 0:
            q[g, cards[best]] = 1.0
        else:
            mx = max(m.values())
            e = {j: np.exp((m[j] - mx) / float(tau)) for j in on}
            tot = sum(e.values())
            for j in on:
                q[g, cards[j]] = e[j] / tot
    return q, has, card, big


def targets_counts_bound(q, big, tau):
    """|kernel - q| per element, DERIVED.  The store and the float32 softmax are tests/distill_model.py's target_bound:
    q (2^-8 + 2^-14) + 2^-120.  What is new is the argument: m_j = fl(fl(sum) / fl(count)) carries at most two roundings of
    the sum's conversion and the division (the count, <= 2^16, converts exactly): |dm| <= 2^-23 |m| (1 + 2^-24) < 2^-22 M
    with M = max |m|; the difference of two such means adds their errors and one rounding of its own, the division by tau one
    more: |dz| <= (2 * 2^-22 M + 2^-23 * 2 M) / tau + 2^-24 |z| <= 2^-20 M / tau + 2^-24 |z|, and |z| < 104 for an
    exponential that does not underflow (2^-24 * 104 < 2^-17, already inside target_bound's 2^-14).  An error dz in every
    argument changes a softmax entry by at most a factor exp(2 dz): relative 2 dz (1 + dz) < 4 * 2^-20 M / tau.  tau = 0 is
    exact (integers): the bound is the store's."""
    q = np.asarray(q, np.float64)
    extra = 0.0 if tau == 0 else 4.0 * 2.0 ** -20 * np.asarray(big, np.float64)[:, None] / float(tau)
    return np.where(q > 0, q * (2.0 ** -8 + 2.0 ** -14 + extra) + 2.0 ** -120, 0.0)
