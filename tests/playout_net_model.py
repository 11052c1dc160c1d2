"""TEST INFRASTRUCTURE — the statement of tarok_playout_cards_net (include/tarok_env.h) on the CPU oracle.

tarok_playout_cards_det at one playout per (legal card, world), with the cards after the candidate played by a policy
network on the seats of `net_seats` and by the Bot on the others.  The worlds and the keys are tests/playout_det_model.py's;
the network's card is the lowest-numbered legal card at the maximum of the logits, and the logits are the float64 forward
with the kernels' two bf16 stores written in (tests/test_gpu_policy_exact.reference) on the feature words of the playout's
own position, stated on the oracle's Game by tests/observe_model.py.  With the exactly summable weight sets of that test the float64
logits ARE the kernel's float32 logits, so the comparison with the GPU is of integers.

All playouts of a call run in lock-step, one forward per card round over the rows that need one; `pick` is the card rule
(the mutants of tests/test_playout_net_cpu.py replace it).  Nothing comes from the code under test.
"""
import numpy as np

import playout_det_model as DM
import playout_model as PM
from observe_model import expand, feature_words  # noqa: F401  (the one statement of the feature words)
from oracle import oracle as O

RANKS = PM.RANKS
DECK = (1 << 54) - 1


def logits_of(words, W):
    """The 54 card logits of every row, float64 with the two bf16 stores."""
    import torch
    from policy_exact_ref import reference
    return reference(torch.from_numpy(expand(words)), W)["out"][:, :54].numpy()


def greedy(logits, legal):
    """The lowest-numbered legal card at the maximum of the logits."""
    cards = PM.cards_of(legal)
    top = max(logits[c] for c in cards)
    return min(c for c in cards if logits[c] == top)


def play_out(games, keys, W, net_seats, pick=greedy):
    """Plays every oracle Game of `games` (after its candidate card) to its end in lock-step: the seats of net_seats play
    pick(logits, legal), the others the Bot's card under the game's key at q cards played.  Returns the final scores."""
    live = [i for i, h in enumerate(games) if not h.done]
    while live:
        net = [i for i in live if (net_seats >> games[i].seat()) & 1]
        cards = {}
        if net:
            lg = logits_of([feature_words(games[i]) for i in net], W)
            for r, i in enumerate(net):
                cards[i] = pick(lg[r], games[i].legal())
        nxt = []
        for i in live:
            h = games[i]
            q = int(h.g.trick_no) * 4 + int(h.g.n_in_trick)
            c = cards[i] if i in cards else O.policy_action(keys[i], q, h.legal())
            r = h.step(c)
            assert r >= 0, "the card is legal"
            if r == 0:
                nxt.append(i)
        live = nxt
    return [h.scores for h in games]


def items_of(lanes, episode, seed, salt, gidx, seats, worlds):
    """The live items of one game: [(rank j, world w, the world's Game with the candidate applied, its playout key)]."""
    game = O.Game.from_lanes(lanes)
    if not PM.takes_part(game, seats):
        return []
    _, _, legal, played = PM.position(game)
    out = []
    for w in range(worlds):
        world = DM.world_of(game, DM.world_key(seed, salt, gidx, episode, played, w))
        assert world.legal() == legal and world.seat() == game.seat()
        for j, c in enumerate(PM.cards_of(legal)):
            h = PM.copy_of(world)
            assert h.step(c) >= 0
            out.append((j, w, h, DM.playout_key(seed, salt, gidx, episode, played, c, w, 0)))
    return out


def playout_scores(games, seed, salt, seats, worlds, W, net_seats, pick=greedy):
    """games: [(lanes, episode, gidx, seat set)] -> scores [n, 12, worlds, 4] int64 of every playout (zeros beyond the
    legal cards and for games that do not take part)."""
    out = np.zeros((len(games), RANKS, worlds, 4), np.int64)
    where, hs, keys = [], [], []
    for g, (lanes, ep, gidx, s) in enumerate(games):
        for j, w, h, key in items_of(lanes, ep, seed, salt, gidx, seats if s is None else s, worlds):
            where.append((g, j, w)); hs.append(h); keys.append(key)
    for (g, j, w), sc in zip(where, play_out(hs, keys, W, net_seats, pick)):
        out[g, j, w] = sc
    return out


def playout_cards(games, seed, salt, seats, worlds, W, net_seats, pick=greedy):
    """(sum [n, 12, 4] int64, cards [n] uint8): the whole statement; the card rule is tarok_playout_cards'."""
    sums = playout_scores(games, seed, salt, seats, worlds, W, net_seats, pick).sum(axis=2)
    acts = np.array([PM.card_of(lanes, seed, gidx, ep, seats if s is None else s, sums[g])
                     for g, (lanes, ep, gidx, s) in enumerate(games)], np.uint8)
    return sums, acts
