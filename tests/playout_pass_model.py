"""TEST INFRASTRUCTURE — the float-free statement of tarok_playout_bids_pass and tarok_bid_round_pass (include/tarok_env.h)
on the CPU oracle.

The value of a pass: what viewer v expects to score when ANOTHER seat declares.  On each world of tarok_playout_bids (the
same world key: tests/playout_bids_model.py's world_of, imported) a TAROK_MIX_BOT game is played under the playout key
of row 19: three Bots bid, v gives its least answer on every call — Naprej, or the forced bid where it has one — the
contract, declarer and king they arrive at are set up on the world's hands, the Bot exchanges and plays every card, and
v's score is row 19.  Then the bidding round with that row as the bar: thr(v) = S(19) + margin * playouts.

Everything here is the oracle's (oracle/tarok_spec.py: game_key, rng32, pick, bot_wish, bot_discards; oracle/oracle.py:
Game, policy_action), the walk and the keys of tests/playout_bids_model.py, and integer arithmetic; the round and the
answer rule are written out here once more.  Nothing comes from the code under test.
"""
import numpy as np

import playout_bids_model as BM
from oracle import oracle as O
from oracle import tarok_spec as S

PASS_ROW = 19
ROWS = BM.ROWS
NAPREJ = BM.NAPREJ


def pass_key(seed, salt, gidx, episode, v, w, k):
    """tarok_playout_bids' pkey with r = 19."""
    return BM.playout_key(seed, salt, gidx, episode, v, PASS_ROW, w, k)


def run_round(ask):
    """Igra.licitacija's control flow (Igra.py:75-114), cut after 8 re-bidding rounds, with the answers behind
    ask(seat, min_igra, obvezno, prednost).  Returns (final bid, holder)."""
    still, top = [], 10
    for seat in (1, 2, 3):
        b = ask(seat, top, None, False)
        if b != NAPREJ:
            still.append(seat)
        top = max(top, b)
    if top == 10:
        return ask(0, NAPREJ, 0, False), 0
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
    return top, holder


def bot_answer(key, n, min_igra, obvezno, prednost):
    """The Bot's n-th answer of a round under `key`: draw 72 + n behind the player-side filter."""
    wish = S.bot_wish(S.rng32(key, S.DRAW_BID + n))
    if wish >= min_igra if prednost else wish > min_igra:
        return wish
    return NAPREJ if obvezno is None else obvezno


def pass_round(pkey, v):
    """(contract, declarer, king — 0 without one) of a pass playout: three Bots under pkey, seat v silent."""
    calls = [0]

    def ask(seat, min_igra, obvezno, prednost):
        n = calls[0]
        calls[0] += 1
        if seat == v:
            return NAPREJ if obvezno is None else obvezno
        return bot_answer(pkey, n, min_igra, obvezno, prednost)

    top, holder = run_round(ask)
    contract = top // 10
    declarer = 0 if contract == S.KLOP else holder
    king = S.pick(S.rng32(pkey, S.DRAW_KING), 4) if contract in BM.KING_CONTRACTS else 0
    return contract, declarer, king


def one_pass_playout(world, v, pkey):
    """The viewer's final score of the pass playout under pkey on `world`."""
    contract, declarer, king = pass_round(pkey, v)
    g = BM.game_of(world, contract, declarer, king, pkey)
    q = 0
    while not g.done:
        assert g.step(O.policy_action(pkey, q, g.legal())) >= 0
        q += 1
    return g.scores[v]


def pass_scores(perm, episode, seed, salt, gidx, seats, worlds, samples):
    """scores [4, worlds, samples] int64 of every pass playout (zeros for seats outside the set and an invalid deal)."""
    assert 1 <= worlds <= BM.MAX_WORLDS and 1 <= samples <= BM.MAX_SAMPLES and 0 <= seats <= 15
    out = np.zeros((4, worlds, samples), np.int64)
    if not BM.valid_perm(perm):
        return out
    for v in range(4):
        if not (seats >> v) & 1:
            continue
        for w in range(worlds):
            world = BM.world_of(perm, v, BM.world_key(seed, salt, gidx, episode, v, w))
            for k in range(samples):
                out[v, w, k] = one_pass_playout(world, v, pass_key(seed, salt, gidx, episode, v, w, k))
    return out


def playout_scores(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts):
    """[4, ROWS, worlds, samples]: tests/playout_bids_model.py's playouts of rows 0..18 with the pass playouts in row 19;
    BM.sums_of sums a corner of it."""
    out = BM.playout_scores(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts)
    out[:, PASS_ROW] = pass_scores(perm, episode, seed, salt, gidx, seats, worlds, samples)
    return out


def pass_sums(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts):
    """sum_out [4, ROWS] of tarok_playout_bids_pass for one game."""
    return BM.sums_of(playout_scores(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts), worlds, samples)


def bar(S_row, playouts, margin):
    return int(S_row[PASS_ROW]) + int(margin) * int(playouts)


def answer(S_row, min_igra, obvezno, prednost, playouts, margin, contracts):
    """The pass-aware licitiram(min_igra, obvezno, prednost) of a seat from its twenty sums."""
    best = None
    for r in range(1, BM.OPTIONS):
        b = 10 * BM.row_option(r)[0]
        if BM.played(r, contracts) and (b >= min_igra if prednost else b > min_igra):
            if best is None or int(S_row[r]) > int(S_row[best]):
                best = r
    ok = best is not None and int(S_row[best]) > bar(S_row, playouts, margin)
    if obvezno is not None:
        ok = ok and int(S_row[best]) > max(int(S_row[r]) for r in BM.rows_of(obvezno // 10))
    return 10 * BM.row_option(best)[0] if ok else (NAPREJ if obvezno is None else obvezno)


def bid_round(key, sums, playouts, margin, contracts, seats):
    """(contract, declarer, king) of tarok_bid_round_pass for one game."""
    calls = [0]

    def ask(seat, min_igra, obvezno, prednost):
        n = calls[0]
        calls[0] += 1
        if (seats >> seat) & 1:
            return answer(sums[seat], min_igra, obvezno, prednost, playouts, margin, contracts)
        return bot_answer(key, n, min_igra, obvezno, prednost)

    top, holder = run_round(ask)
    contract = top // 10
    declarer = 0 if contract == S.KLOP else holder
    king = 0
    if contract in BM.KING_CONTRACTS:
        if (seats >> declarer) & 1:
            rows = BM.rows_of(contract)
            king = max(range(4), key=lambda k: (int(sums[declarer][rows[k]]), -k))
        else:
            king = S.pick(S.rng32(key, S.DRAW_KING), 4)
    return contract, declarer, king


def replay_pass(seed, gidx, episode, seats, worlds, samples, contracts=BM.DEFAULT_CONTRACTS, margin=0, salt=0):
    """One game of one pass of evaluate_bidding_vs_bot(pass_value=True) on the oracle: the device's own deal, the
    pass-aware round on the model's twenty sums, the Bot's exchange and the Bot's cards.
    Returns (contract, declarer, king, actions [48] — 255 once the game is over —, final scores [4])."""
    key = S.game_key(seed, gidx, episode)
    perm = S.deal(key)
    sums = pass_sums(perm, episode, seed, salt, gidx, seats, worlds, samples, contracts)
    contract, declarer, king = bid_round(key, sums, worlds * samples, margin, contracts, seats)
    g = BM.game_of(perm, contract, declarer, king, key)
    actions = [BM.PAD] * 48
    for t in range(48):
        if g.done:
            break
        actions[t] = O.policy_action(key, t, g.legal())
        assert g.step(actions[t]) >= 0
    assert g.done
    return contract, declarer, king, actions, g.scores
