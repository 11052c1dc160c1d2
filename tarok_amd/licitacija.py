"""Host-side bidding round — the control flow of `Igra.licitacija` (Igra.py:75-114).

`licitacija()` is the host form: one call per game with any `licitiram` callback; the GPU env
takes its outcome (declarer seat, contract) as `tarok_reset` inputs.  The device runs the same
round for every game at once in `tarok_bid_round` (`TarokVecEnv.bid_round`), with the Bot's
answers or with the playout bidder's, whose rule `playout_answer` states here as a pure host
function on `tarok_playout_bids`' sums.

Bids are the reference's `int(Tip_igre)` values (Tip_igre.py:4-15) so that the `>` / `>=`
comparisons of the player-side filter (Igralec.py:58-74) mean the same thing.
"""

NAPREJ, KLOP, TRI, DVE, ENA = -10, 0, 10, 20, 30
SOLO_TRI, SOLO_DVE, SOLO_ENA, BERAC, SOLO_BREZ, ODPRTI_BERAC = 40, 50, 60, 70, 80, 90
ALL_BIDS = (NAPREJ, KLOP, TRI, DVE, ENA, SOLO_TRI, SOLO_DVE, SOLO_ENA, BERAC, SOLO_BREZ, ODPRTI_BERAC)


def base_filter(zelim, min_igra, obvezno=None, prednost=False):
    """What `Igralec.licitiram` (Igralec.py:58-74) lets through: the wish if it beats
    (`prednost`: at least matches) the standing bid, else the forced bid, else Naprej."""
    ok = zelim >= min_igra if prednost else zelim > min_igra
    if ok:
        return zelim
    return NAPREJ if obvezno is None else obvezno


def licitacija(licitiram, max_rounds=64):
    """Run one bidding round.

    `licitiram(seat, min_igra, obvezno, prednost) -> int` is asked exactly as the
    reference asks `igralci[seat].licitiram(min_igra, id, obvezno, prednost)`, in the same
    order.  Returns `(declarer_seat, contract_value)`.

    Order of play (Igra.py:81-114): seats 1,2,3 bid over a floor of Tri; if nobody did,
    seat 0 must play at least Klop; otherwise seat 0 may match the top bid (priority), and
    the bidders keep going — seat 0 asked last, the current holder allowed to stand on its
    bid — until one is left.
    """
    still_in = set()
    top = TRI
    for seat in (1, 2, 3):
        b = licitiram(seat, top, None, False)
        if b != NAPREJ:
            still_in.add(seat)
        top = max(top, b)
    if top == TRI:
        return 0, licitiram(0, NAPREJ, KLOP, False)
    b = licitiram(0, top, None, True)
    if b != NAPREJ:
        still_in.add(0)
    top = max(top, b)
    holder = min(still_in)
    rounds = 0
    while len(still_in) != 1:
        if not still_in or rounds >= max_rounds:
            # the reference spins forever here; a player that drops a bid it holds breaks the protocol
            raise RuntimeError("licitacija: no bidder left / bidding does not terminate")
        rounds += 1
        order = sorted(still_in)
        if order[0] == 0:
            order = order[1:] + [0]
        nxt = set()
        for seat in order:
            b = licitiram(seat, top, top if seat == holder else None, False)
            if b != NAPREJ:
                nxt.add(seat)
                holder = seat
                top = b
        still_in = nxt
    return holder, top


BID_OPTIONS = 19                                 # rows of a viewer in tarok_playout_bids' sums (row 19 is padding)
BID_PASS_ROW = 19                                # ... or, from tarok_playout_bids_pass, the summed score of passing


def row_bid(row):
    """int(Tip_igre) of row 0..18 of tarok_playout_bids' sums: Klop; Tri, Dve, Ena x four kings; the six others."""
    return 0 if row == 0 else (10 * (1 + (row - 1) // 4) if row <= 12 else 10 * (row - 9))


def playout_answer(S_row, min_igra, obvezno, prednost, playouts, threshold=0, contracts=0x00F, pass_value=False):
    """The answer of a playout bidder to licitiram(min_igra, obvezno, prednost), as tarok_bid_round gives it, from the
    seat's row of tarok_playout_bids' sums (S_row[r], r < 19; any integer sequence).
    Candidates: the rows of the contracts in `contracts` (bit int(Tip_igre) / 10) from Tri up that beat min_igra (at least
    match it with prednost); best = the largest sum, the lowest row on ties.  Without obvezno: the best row's bid if its
    sum exceeds threshold * playouts, else Naprej.  With obvezno = o: the best row's bid if its sum also exceeds the
    largest sum among the rows of o itself, else o.
    pass_value=True (tarok_bid_round_pass): the bar is S_row[19] + threshold * playouts, the seat's own value of a pass
    plus a margin of `threshold` points per game; nothing else changes.
    As the callback of licitacija():  lambda seat, m, o, p: playout_answer(S[seat], m, o, p, playouts)."""
    best = None
    for r in range(1, BID_OPTIONS):
        b = row_bid(r)
        if not (int(contracts) >> (b // 10)) & 1:
            continue
        if not (b >= min_igra if prednost else b > min_igra):
            continue
        if best is None or int(S_row[r]) > int(S_row[best]):
            best = r
    bar = (int(S_row[BID_PASS_ROW]) if pass_value else 0) + int(threshold) * int(playouts)
    bid = best is not None and int(S_row[best]) > bar
    if obvezno is None:
        return row_bid(best) if bid else NAPREJ
    stand = max(int(S_row[r]) for r in range(BID_OPTIONS) if row_bid(r) == obvezno)
    return row_bid(best) if bid and int(S_row[best]) > stand else obvezno
