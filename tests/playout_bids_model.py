"""TEST INFRASTRUCTURE — the float-free statement of tarok_playout_bids and tarok_bid_round (include/tarok_env.h) on the
CPU oracle.

The bid valued by determinized playouts: viewer v holds twelve cards and has seen nothing else, so a world re-deals the
other 42 (three hands and the talon, one ascending walk with four capacities, then the talon's slot order); every option
— Klop, Tri / Dve / Ena with each king, the Solos, Berac, Solo_brez, Odprti_berac — is set up on the world with v as the
declarer and played to the end by the Bot.  Then the bidding round: Igra.licitacija's control flow with the playout
bidder's answer rule on some seats and the Bot's draw on the others.  Everything here is the oracle's
(oracle/tarok_spec.py: game_key, rng32, pick, deal, bot_discards, GROUP_SIZE; oracle/oracle.py: Game, policy_action) and
integer arithmetic; nothing comes from the code under test.

World w and sample k depend on none of the launch's sizes: `playout_scores` returns every single playout and a smaller
launch sums a corner of the same array (`sums_of`).
"""
import numpy as np

import playout_det_model as DM
import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

ROWS = 20                    # rows per viewer, the last one padding
OPTIONS = 19
DEFAULT_CONTRACTS, ALL_CONTRACTS = 0x00F, 0x3FF
MAX_WORLDS = DM.MAX_WORLDS
MAX_SAMPLES = PM.MAX_SAMPLES
DRAW_SLOT = 320              # draw 320 + j: the slot of the j-th talon card
NAPREJ = -10
PAD = 255
M64 = (1 << 64) - 1
KING_CONTRACTS = (S.TRI, S.DVE, S.ENA)


def row_option(r):
    """(contract code, called suit or -1) of row r < 19."""
    if r == 0:
        return S.KLOP, -1
    if r <= 12:
        return 1 + (r - 1) // 4, (r - 1) % 4
    return r - 9, -1


def rows_of(code):
    return [r for r in range(OPTIONS) if row_option(r)[0] == code]


def played(r, contracts):
    return bool((int(contracts) >> row_option(r)[0]) & 1)


def world_key(seed, salt, gidx, episode, v, w):
    """wkey = game_key(seed ^ salt, gidx, 2 << 61 | ep << 28 | v << 6 | w)."""
    e = (2 << 61) | ((int(episode) & 0xFFFFFFFF) << 28) | (int(v) << 6) | int(w)
    return S.game_key((int(seed) ^ int(salt)) & M64, int(gidx), e)


def playout_key(seed, salt, gidx, episode, v, r, w, k):
    """pkey = game_key(seed ^ salt, gidx, 3 << 61 | ep << 28 | v << 26 | r << 21 | w << 15 | k)."""
    e = (3 << 61) | ((int(episode) & 0xFFFFFFFF) << 28) | (int(v) << 26) | (int(r) << 21) | (int(w) << 15) | int(k)
    return S.game_key((int(seed) ^ int(salt)) & M64, int(gidx), e)


def valid_perm(perm):
    return len(perm) == 54 and sorted(int(c) for c in perm) == list(range(54))


def walk(pool, caps, wkey):
    """The ascending walk over the cards of `pool` (a list) with running capacities `caps` (the last one the talon's):
    card i draws pick(rng32(wkey, i), capacities left) and goes to the part whose interval holds the draw; the talon's
    cards, ascending, then take the pick(rng32(wkey, 320 + j), free slots left)-th free slot.  Returns (the parts before
    the talon as sorted lists, the talon as a list by slot)."""
    caps = list(caps)
    parts = [[] for _ in caps]
    for i, c in enumerate(sorted(pool)):
        r = S.pick(S.rng32(wkey, i), sum(caps))
        t = 0
        while r >= caps[t]:
            r -= caps[t]
            t += 1
        parts[t].append(c)
        caps[t] -= 1
    assert not any(caps)
    free = list(range(len(parts[-1])))
    talon = [None] * len(free)
    for j, c in enumerate(parts[-1]):
        talon[free.pop(S.pick(S.rng32(wkey, DRAW_SLOT + j), len(free)))] = c
    return parts[:-1], talon


def world_of(perm, v, wkey):
    """The deal `perm` as world wkey of seat v sees it: v's twelve cards stay, the other 42 are re-dealt."""
    perm = [int(c) for c in perm]
    own = perm[12 * v:12 * v + 12]
    pool = [c for c in range(54) if c not in own]
    hands, talon = walk(pool, [12, 12, 12, 6], wkey)
    out = []
    for s in range(4):
        out += own if s == v else hands.pop(0)
    return out + talon


def one_playout(world, v, r, pkey):
    """Row r on `world` with v as the declarer (Klop: seat 0): the Bot's exchange under pkey where the contract has one,
    then every card by the Bot under pkey (draw 128 + q).  Returns the VIEWER's final score."""
    code, king = row_option(r)
    g = O.Game(world, code, 0 if code == S.KLOP else v, king)
    if int(g.g.phase) == 1:
        gs = S.GROUP_SIZE[code]
        group = 0
        for j in range(gs):
            group |= 1 << int(g.g.talon[j])
        assert g.exchange(0, S.bot_discards(pkey, int(g.g.hand[v]) | group, gs)) == 0
    q = 0
    while not g.done:
        assert g.step(O.policy_action(pkey, q, g.legal())) >= 0
        q += 1
    return g.scores[v]


def playout_scores(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts):
    """scores [4, ROWS, worlds, samples] int64 of every playout (the viewer's score; zeros for seats outside the set, rows
    outside `contracts`, row 19 and an invalid deal)."""
    assert 1 <= worlds <= MAX_WORLDS and 1 <= samples <= MAX_SAMPLES and 1 <= contracts <= ALL_CONTRACTS and 0 <= seats <= 15
    out = np.zeros((4, ROWS, worlds, samples), np.int64)
    if not valid_perm(perm):
        return out
    for v in range(4):
        if not (seats >> v) & 1:
            continue
        for w in range(worlds):
            world = world_of(perm, v, world_key(seed, salt, gidx, episode, v, w))
            for r in range(OPTIONS):
                if played(r, contracts):
                    for k in range(samples):
                        out[v, r, w, k] = one_playout(world, v, r, playout_key(seed, salt, gidx, episode, v, r, w, k))
    return out


def sums_of(scores, worlds, samples):
    """sum_out [4, ROWS] of a launch at (worlds, samples) <= the model run's."""
    return scores[:, :, :worlds, :samples].sum(axis=(2, 3))


def playout_bids(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts):
    return sums_of(playout_scores(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts), worlds, samples)


def answer(S_row, min_igra, obvezno, prednost, playouts, threshold, contracts):
    """The playout bidder's licitiram(min_igra, obvezno, prednost) from its sums."""
    cands = [r for r in range(OPTIONS)
             if played(r, contracts) and 10 * row_option(r)[0] >= 10
             and (10 * row_option(r)[0] >= min_igra if prednost else 10 * row_option(r)[0] > min_igra)]
    best = None
    for r in cands:
        if best is None or int(S_row[r]) > int(S_row[best]):
            best = r
    ok = best is not None and int(S_row[best]) > int(threshold) * int(playouts)
    if obvezno is None:
        return 10 * row_option(best)[0] if ok else NAPREJ
    stand = max(int(S_row[r]) for r in rows_of(obvezno // 10))
    return 10 * row_option(best)[0] if ok and int(S_row[best]) > stand else obvezno


def bid_round(key, sums, playouts, threshold, contracts, seats):
    """(contract code, declarer, king suit — 0 without a called king) of one game: the round of Igra.py:75-114, cut
    after 8 re-bidding rounds; the n-th call draws 72 + n where the Bot answers."""
    calls = [0]

    def ask(seat, min_igra, obvezno, prednost):
        n = calls[0]
        calls[0] += 1
        if (seats >> seat) & 1:
            return answer(sums[seat], min_igra, obvezno, prednost, playouts, threshold, contracts)
        wish = S.bot_wish(S.rng32(key, S.DRAW_BID + n))
        if wish >= min_igra if prednost else wish > min_igra:
            return wish
        return NAPREJ if obvezno is None else obvezno

    still, top = [], 10
    for seat in (1, 2, 3):
        b = ask(seat, top, None, False)
        if b != NAPREJ:
            still.append(seat)
        top = max(top, b)
    if top == 10:
        holder, top = 0, ask(0, NAPREJ, 0, False)
    else:
        b = ask(0, top, None, True)
        if b != NAPREJ:
            still.append(0)
        top = max(top, b)
        holder = min(still)
        rounds = 0
        while len(still) != 1 and rounds < S.BID_ROUND_CAP:
            rounds += 1
            nxt = []
            for seat in (1, 2, 3, 0):
                if seat in still:
                    b = ask(seat, top, top if seat == holder else None, False)
                    if b != NAPREJ:
                        nxt.append(seat)
                        holder, top = seat, b
            still = nxt
    contract = top // 10
    declarer = 0 if contract == S.KLOP else holder
    king = 0
    if contract in KING_CONTRACTS:
        if (seats >> declarer) & 1:
            rows = rows_of(contract)
            king = max(range(4), key=lambda k: (int(sums[declarer][rows[k]]), -k))
        else:
            king = S.pick(S.rng32(key, S.DRAW_KING), 4)
    return contract, declarer, king


def bidding(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts, threshold=0):
    """(sums [4, ROWS], contract, declarer, king) of one game: both launches."""
    sums = playout_bids(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts)
    return (sums,) + bid_round(S.game_key(seed, gidx, episode), sums, worlds * samples, threshold, contracts, seats)


def game_of(perm, contract, declarer, king, key):
    """The game reset(deals, contract, declarer, king_suit) leaves: set up, the Bot's exchange under the game's key."""
    g = O.Game(perm, contract, declarer, king if contract in KING_CONTRACTS else -1)
    if int(g.g.phase) == 1:
        gs = S.GROUP_SIZE[contract]
        group = 0
        for j in range(gs):
            group |= 1 << int(g.g.talon[j])
        assert g.exchange(0, S.bot_discards(key, int(g.g.hand[declarer]) | group, gs)) == 0
    return g


def replay_pass(seed, gidx, episode, seats, worlds, samples, contracts=DEFAULT_CONTRACTS, threshold=0, salt=0, cards=None):
    """One game of one pass of evaluate_bidding_vs_bot on the oracle: the device's own deal, the model's bidding round
    (the playout bidder on `seats`), the Bot's exchange, then the cards.  cards=None: the Bot plays every card;
    cards=(W, S): the determinized player of tests/playout_det_model.py plays the cards of `seats`
    (evaluate_playout_vs_bot(S, worlds=W, bidding=(worlds, samples))).
    Returns (contract, declarer, king, actions [48] — 255 once the game is over —, final scores [4])."""
    key = S.game_key(seed, gidx, episode)
    perm = S.deal(key)
    _, contract, declarer, king = bidding(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts, threshold)
    g = game_of(perm, contract, declarer, king, key)
    actions = [PAD] * 48
    for t in range(48):
        if g.done:
            break
        if cards is None:
            card = O.policy_action(key, t, g.legal())
        else:
            _, card = DM.playout_cards(g.lanes(), episode, seed, salt, gidx, seats, cards[0], cards[1])
        actions[t] = card
        assert g.step(card) >= 0
    assert g.done
    return contract, declarer, king, actions, g.scores
