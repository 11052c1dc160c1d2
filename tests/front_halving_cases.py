"""TEST INFRASTRUCTURE — what the GPU tests of tarok_playout_exchange_net_halving / tarok_playout_bids_net_halving share: the
guarded launches of the two entries over a guarded scratch of exactly the header's size, and the expectation built from
tarok_playout_*_net_list launches at the cumulative ends, walked by tests/playout_front_halving_model.py.  Importing it needs
no GPU."""
import ctypes

import numpy as np

import front_list_cases as F
import playout_front_halving_model as M

X_NAMES = ("sum", "count", "choice", "discards")
B_NAMES = ("sum", "count", "value")


def schedule_args(schedule):
    schedule = [int(w) for w in schedule]
    return len(schedule), (ctypes.c_int * len(schedule))(*schedule)


def exchange_halving(env, kw, schedule, sets, net_seats, depth, scale=70.0, salt=3, seats=15, per_game=None, want=X_NAMES, scratch_out=None,
                     size=None):
    """One tarok_playout_exchange_net_halving into guarded outputs: (sum, count, choice, discards), None where not asked."""
    import gpu_harness as H
    from guarded import Guarded
    n, rows = env.n, 6 * sets
    outs = [Guarded("sum_out", 1, n, np.int32, inner=(rows, 4), device="cuda") if "sum" in want else None,
            Guarded("count_out", 1, n, np.int32, inner=(rows,), device="cuda") if "count" in want else None,
            Guarded("choice_out", 1, n, np.int8, device="cuda") if "choice" in want else None,
            Guarded("discards_out", 1, n, np.uint8, inner=(3,), device="cuda") if "discards" in want else None]
    rounds, arr = schedule_args(schedule)
    size = M.exchange_scratch(n, schedule, sets) if size is None else size
    H._launch(env, "tarok_playout_exchange_net_halving",
              [rounds, arr, int(sets), int(salt), int(seats), H.dev_u8(per_game), int(net_seats), F.abi_depth(depth), float(scale)] + list(kw), outs,
              ("tarok_playout_exchange_net_halving_scratch_bytes", (rounds, arr, int(sets)), size), True,
              ("halving", tuple(schedule), sets, net_seats, seats, depth), scratch_out)
    read = (H.read_words, H.read_words, H.read_bytes, H.read_bytes)
    return tuple(None if o is None else f(o) for f, o in zip(read, outs))


def bids_halving(env, kw, episode, schedule, net_seats, depth, pass_value, scale=70.0, contracts=F.DEFAULT, deals=None, salt=3, seats=15,
                 per_game=None, want=B_NAMES, scratch_out=None, size=None):
    """One tarok_playout_bids_net_halving into guarded outputs: (sum, count, value) [n, 4, 20] i32, None where not asked."""
    import gpu_harness as H
    from guarded import Guarded
    n = env.n
    outs = [Guarded(name + "_out", 1, n, np.int32, inner=(4, 20), device="cuda") if name in want else None for name in B_NAMES]
    rounds, arr = schedule_args(schedule)
    size = M.bid_scratch(n, schedule, contracts, seats, per_game is not None, pass_value) if size is None else size
    H._launch(env, "tarok_playout_bids_net_halving",
              [int(episode), H.dev_u8(deals), rounds, arr, int(contracts), int(salt), int(seats), H.dev_u8(per_game), int(net_seats),
               F.abi_depth(depth), float(scale), int(pass_value)] + list(kw), outs,
              ("tarok_playout_bids_net_halving_scratch_bytes",
               (rounds, arr, int(contracts), int(seats), int(per_game is not None), int(pass_value)), size), True,
              ("halving", tuple(schedule), contracts, net_seats, seats, depth, pass_value), scratch_out)
    return tuple(None if o is None else H.read_words(o) for o in outs)


class Tally:
    """What the inputs of the schedule tests contained, summed over their cases."""

    def __init__(self):
        self.ties = self.early = self.differs = self.units = 0

    def __repr__(self):
        return "units %d: a tie at a cut %d, left early %d, best differs from the uniform launch %d" % (self.units, self.ties, self.early, self.differs)


def expect_exchange(env, kw, schedule, sets, net_seats, depth, tally, **kw_launch):
    """(sum, count, choice, discards) of the halving launch from list launches at the cumulative ends."""
    from oracle import oracle as O
    n, rows, W = env.n, 6 * sets, sum(schedule)
    at = {}

    def uniform(e):
        if e not in at:
            scr = []
            at[e] = F.exchange_list(env, kw, e, sets, net_seats, depth, scratch_out=scr, **kw_launch) + (scr[0],)
        return at[e]
    full = uniform(W)
    on, _, _ = F.list_words(full[3], F.exchange_bound(n, W, sets), 6 * n)
    cands = env.exchange_candidates(sets, salt=kw_launch.get("salt", 3)).cpu().numpy().reshape(n, rows, 3)
    lanes = env.state()
    sums, count = np.zeros((n, rows, 4), np.int32), np.zeros((n, rows), np.int32)
    choice, discards = full[1].copy(), full[2].copy()
    for g in range(n):
        arms = [i * sets + d for i in range(6) for d in range(sets) if (int(on[g * 6 + i]) >> d) & 1]
        if not arms:
            continue
        declarer = int(O.Game.from_lanes(lanes[:, g]).g.declarer)
        s, c, best, cuts, alive = M.exchange_game(arms, declarer, lambda e: uniform(e)[0][g].astype(np.int64), schedule, rows)
        sums[g], count[g], choice[g], discards[g] = s, c, best // sets, cands[g, best]
        tally.units += 1
        tally.ties += int(M.tie_at_a_cut(cuts))
        tally.early += int(c.max() < W)
        tally.differs += int(best != int(np.argmax(full[0][g][:len(arms), declarer])))
    return sums, count, choice, discards


def expect_bids(env, kw, episode, schedule, net_seats, depth, pass_value, tally, contracts=F.DEFAULT, **kw_launch):
    """(sum, count, value) of the halving launch from list launches at the cumulative ends."""
    n, W = env.n, sum(schedule)
    at = {}

    def uniform(e):
        if e not in at:
            scr = []
            at[e] = (F.bids_list(env, kw, episode, e, net_seats, depth, pass_value, contracts=contracts, scratch_out=scr, **kw_launch), scr[0])
        return at[e]
    full = uniform(W)
    bound = F.bid_bound(n, W, contracts, kw_launch.get("seats", 15), kw_launch.get("per_game") is not None, pass_value)
    on, _, _ = F.list_words(full[1], bound, 4 * n, 40 * n)
    out = [np.zeros((n, 4, 20), np.int32) for _ in range(3)]
    rows = M.bid_row_mask(contracts)
    for u in range(4 * n):
        if not int(on[u]):
            continue
        g, v = divmod(u, 4)
        s, c, val, cuts, alive = M.bid_unit(rows, pass_value, lambda e: uniform(e)[0][g, v].astype(np.int64), schedule)
        out[0][g, v], out[1][g, v], out[2][g, v] = s, c, val
        arms = [r for r in range(19) if (rows >> r) & 1]
        best = min(alive, key=lambda j: (-int(s[j]), j))
        tally.units += 1
        tally.ties += int(M.tie_at_a_cut(cuts))
        tally.early += int(c[:19].max() < W)
        tally.differs += int(best != min(arms, key=lambda j: (-int(full[0][g, v, j]), j)))
    return tuple(out)
