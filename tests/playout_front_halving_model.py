"""TEST INFRASTRUCTURE — the statement of tarok_playout_exchange_net_halving / tarok_playout_bids_net_halving
(include/tarok_env.h) in plain Python.

The single playouts are the existing launches': world w depends on no launch size, so a row that has played the worlds
0 .. e - 1 holds the uniform launch's row at worlds = e.  The walk below therefore takes `rows_at(e)` — the uniform launch's
(or a model's) sums at worlds = e — and applies the rounds and the survivor rule from the definition, with a plain sort.
Integer arithmetic; nothing comes from the code under test.  Also the header's bounds and scratch formulas, restated."""
import numpy as np

MAX_ROUNDS, MAX_WORLDS = 4, 64
PASS_ROW, BID_ROWS = 19, 20


def keep_of(k):
    return max(1, (k + 1) // 2)


def survivors(values, alive):
    """The arms of `alive` that stay: the max(1, ceil(k / 2)) with the highest value, ties to the lower index."""
    order = sorted(alive, key=lambda j: (-int(values[j]), j))
    return sorted(order[:keep_of(len(alive))]) if alive else []


def ends_of(round_worlds):
    assert 1 <= len(round_worlds) <= MAX_ROUNDS and all(int(w) >= 1 for w in round_worlds) and sum(round_worlds) <= MAX_WORLDS
    return np.cumsum([int(w) for w in round_worlds]).tolist()


def walk(arms, column_at, round_worlds, rule=survivors):
    """arms: the indices that start alive; column_at(e)[j]: arm j's compared sum over the worlds 0 .. e - 1.
    -> (count {arm: the end of the last round it played}, the arms alive at the end, the end of the last round played (0: none),
    cuts [(alive before, values, alive after)] of every cut made)."""
    alive, count, cuts, played = sorted(arms), {}, [], 0
    ends = ends_of(round_worlds)
    for r, e1 in enumerate(ends):
        if not alive or (r > 0 and len(alive) == 1):        # one arm alive: no further round
            break
        played = e1
        for j in alive:
            count[j] = e1
        if r + 1 < len(ends):
            values = column_at(e1)
            after = rule(values, alive)
            cuts.append((list(alive), [int(values[j]) for j in alive], after))
            alive = after
    return count, alive, played, cuts


def value_of(total, worlds, count):
    """The nearest integer to total * worlds / count, halves away from zero; 0 where count is 0 — in Python integers."""
    total, worlds, count = int(total), int(worlds), int(count)
    if count == 0:
        return 0
    num = total * worlds
    q = (2 * abs(num) + count) // (2 * count)
    return -q if num < 0 else q


def exchange_game(arms, declarer, sums_at, round_worlds, rows):
    """One game that takes part.  arms: its candidates' rows; sums_at(e): [rows, 4] the uniform launch's sums at worlds = e.
    -> (sum [rows, 4] int64, count [rows] int64, the best row among the alive, the cuts, the alive)."""
    count, alive, _, cuts = walk(arms, lambda e: np.asarray(sums_at(e))[:, declarer], round_worlds)
    out, cnt = np.zeros((rows, 4), np.int64), np.zeros(rows, np.int64)
    for j, e in count.items():
        out[j], cnt[j] = np.asarray(sums_at(e))[j], e
    best = min(alive, key=lambda j: (-int(out[j, declarer]), j))
    return out, cnt, best, cuts, alive


def bid_unit(rows_mask, pass_value, sums_at, round_worlds):
    """One (game, viewer) that takes part.  rows_mask: the 19-bit word of its rows; sums_at(e): [20] the uniform launch's row
    sums of this viewer at worlds = e.  -> (sum [20], count [20], value [20], the cuts, the alive)."""
    arms = [r for r in range(PASS_ROW) if (rows_mask >> r) & 1]
    count, alive, played, cuts = walk(arms, lambda e: np.asarray(sums_at(e)), round_worlds)
    if pass_value and played:
        count[PASS_ROW] = played                               # the bar: every round its unit plays
    W = sum(int(w) for w in round_worlds)
    out, cnt, val = np.zeros(BID_ROWS, np.int64), np.zeros(BID_ROWS, np.int64), np.zeros(BID_ROWS, np.int64)
    for j, e in count.items():
        out[j], cnt[j] = int(np.asarray(sums_at(e))[j]), e
        val[j] = value_of(out[j], W, e)
    return out, cnt, val, cuts, alive


def tie_at_a_cut(cuts):
    """A cut where the last arm kept and the first arm dropped hold the same value."""
    for before, values, after in cuts:
        v = dict(zip(before, values))
        out = [j for j in before if j not in after]
        if out and min(v[j] for j in after) == max(v[j] for j in out):
            return True
    return False


# ---- the header's bounds and scratch formulas
def popc(x):
    return bin(int(x)).count("1")


def bid_row_mask(contracts):
    m = contracts & 1
    for c in (1, 2, 3):
        if contracts & (1 << c):
            m |= 0xF << (1 + 4 * (c - 1))
    return m | (((contracts >> 4) & 0x3F) << 13)


def alive_bound(arms, r):
    for _ in range(r):
        arms = (arms + 1) // 2
    return arms


def exchange_bounds(n, round_worlds, sets):
    return [n * alive_bound(6 * sets, r) * int(w) for r, w in enumerate(round_worlds)]


def bid_bounds(n, round_worlds, contracts, seats, per_game, pass_value):
    u, rows = (4 if per_game else popc(seats & 15)), popc(bid_row_mask(contracts))
    return [n * u * (alive_bound(rows, r) + int(bool(pass_value))) * int(w) for r, w in enumerate(round_worlds)]


def _bytes(bounds, extra, units):
    if max(bounds) >= 1 << 31:
        return -1
    return (48 * max(bounds) + extra + 12 * units + 4 * ((units + 255) // 256) + 4 + 15) // 16 * 16


def exchange_scratch(n, round_worlds, sets):
    return _bytes(exchange_bounds(n, round_worlds, sets), 20 * 6 * n * sets, 6 * n)


def bid_scratch(n, round_worlds, contracts=0x00F, seats=15, per_game=False, pass_value=False):
    return _bytes(bid_bounds(n, round_worlds, contracts, seats, per_game, pass_value), 8 * 80 * n + 40 * n, 4 * n)
