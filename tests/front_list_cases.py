"""TEST INFRASTRUCTURE — what the tests of tarok_playout_exchange_net_list / tarok_playout_bids_net_list share: the Python
restatement of the header's bounds and scratch formulas (CPU tests), and for the GPU tests the guarded launches of the list
entries and of the dense launches they must equal, the reading of a list launch's scratch, and the comparison of a compacted
list with the dense grid.  Importing it needs no GPU."""
import numpy as np

LIVE = 0x8000800080008000
SENTINEL_U64 = 0xA5A5A5A5A5A5A5A5
DEFAULT, ALL = 0x00F, 0x3FF
FRONT_MAX_DEPTH = 13


# ---- the header's formulas
def bid_row_mask(contracts):
    m = contracts & 1
    for c in (1, 2, 3):
        if contracts & (1 << c):
            m |= 0xF << (1 + 4 * (c - 1))
    return m | (((contracts >> 4) & 0x3F) << 13)


def bid_rows(contracts, pass_value):
    return bid_row_mask(contracts) | ((1 << 19) if pass_value else 0)


def popc(x):
    return bin(int(x)).count("1")


def exchange_bound(n, worlds, sets):
    return n * 6 * sets * worlds


def bid_bound(n, worlds, contracts, seats, per_game, pass_value):
    return n * (4 if per_game else popc(seats & 15)) * popc(bid_rows(contracts, pass_value)) * worlds


def scratch_bytes(bound, units, extra=0):
    """48 x bound + extra + 8 x units + 4 x ceil(units / 256) + 4, rounded up to 16; -1 for a bound that reaches 2^31."""
    if bound >= 1 << 31:
        return -1
    return (48 * bound + extra + 8 * units + 4 * ((units + 255) // 256) + 4 + 15) // 16 * 16


def exchange_scratch(n, worlds, sets):
    return scratch_bytes(exchange_bound(n, worlds, sets), 6 * n)


def bid_scratch(n, worlds, contracts=DEFAULT, seats=15, per_game=False, pass_value=False):
    return scratch_bytes(bid_bound(n, worlds, contracts, seats, per_game, pass_value), 4 * n, 40 * n)


# ---- the GPU launches (gpu_harness is imported where it is used)
def abi_depth(depth):
    return 0 if depth is None else int(depth)


def to_the_end(depth):
    return depth is None or int(depth) in (0, FRONT_MAX_DEPTH)


def exchange_list(env, kw, worlds, sets, net_seats, depth, scale=70.0, salt=3, seats=15, per_game=None, want=("sum", "choice", "discards"),
                  scratch_out=None, size=None):
    """One tarok_playout_exchange_net_list into guarded outputs over a guarded scratch of exactly the header's size."""
    import gpu_harness as H
    size = exchange_scratch(env.n, worlds, sets) if size is None else size
    return H.launch_exchange(env, "tarok_playout_exchange_net_list",
                             [int(worlds), int(sets), int(salt), int(seats), H.dev_u8(per_game), int(net_seats), abi_depth(depth), float(scale)] + list(kw),
                             sets, want, scratch=("tarok_playout_exchange_net_list_scratch", (int(worlds), int(sets)), size), check_env_untouched=True,
                             tag=("list", worlds, sets, net_seats, seats, depth), scratch_out=scratch_out)


def exchange_dense(env, kw, worlds, sets, net_seats, depth, scale=70.0, salt=3, seats=15, per_game=None, want=("sum", "choice", "discards"),
                   scratch_out=None):
    """The existing launch the list launch must equal: tarok_playout_exchange_net to the end, else _value at the depth."""
    import gpu_harness as H
    value = [] if to_the_end(depth) else [int(depth), float(scale)]
    return H.launch_exchange(env, "tarok_playout_exchange_net" + ("_value" if value else ""),
                             [int(worlds), int(sets), int(salt), int(seats), H.dev_u8(per_game), int(net_seats)] + value + list(kw), sets, want,
                             scratch=("tarok_playout_exchange_net_scratch", (int(worlds), int(sets)), env.n * 6 * sets * worlds * 48),
                             check_env_untouched=True, tag=("dense", worlds, sets, net_seats, seats, depth), scratch_out=scratch_out)


def bids_list(env, kw, episode, worlds, net_seats, depth, pass_value, scale=70.0, contracts=DEFAULT, deals=None, salt=3, seats=15, per_game=None,
              scratch_out=None, size=None):
    """One tarok_playout_bids_net_list into a guarded sum_out [n, 4, 20] i32 over a guarded scratch of exactly the header's size."""
    import gpu_harness as H
    from guarded import Guarded
    g_sum = Guarded("sum_out", 1, env.n, np.int32, inner=(4, 20), device="cuda")
    size = bid_scratch(env.n, worlds, contracts, seats, per_game is not None, pass_value) if size is None else size
    H._launch(env, "tarok_playout_bids_net_list",
              [int(episode), H.dev_u8(deals), int(worlds), int(contracts), int(salt), int(seats), H.dev_u8(per_game), int(net_seats), abi_depth(depth),
               float(scale), int(pass_value)] + list(kw), [g_sum],
              ("tarok_playout_bids_net_list_scratch", (int(worlds), int(contracts), int(seats), int(per_game is not None), int(pass_value)), size),
              True, ("list", worlds, contracts, net_seats, seats, depth, pass_value), scratch_out)
    return H.read_words(g_sum)


def bids_dense(env, kw, episode, worlds, net_seats, depth, pass_value, scale=70.0, contracts=DEFAULT, deals=None, salt=3, seats=15,
               per_game=None, scratch_out=None):
    """The existing launch the list launch must equal: tarok_playout_bids_net to the end without the pass, else _value (at 13
    where the list launch runs to the end)."""
    import gpu_harness as H
    from guarded import Guarded
    if to_the_end(depth) and not pass_value:
        return H.launch_bids_net(env, kw, worlds, net_seats, contracts, deals, salt, seats, per_game, episode, scratch_out)
    g_sum = Guarded("sum_out", 1, env.n, np.int32, inner=(4, 20), device="cuda")
    H._launch(env, "tarok_playout_bids_net_value",
              [int(episode), H.dev_u8(deals), int(worlds), int(contracts), int(salt), int(seats), H.dev_u8(per_game), int(net_seats),
               FRONT_MAX_DEPTH if to_the_end(depth) else int(depth), float(scale), int(pass_value)] + list(kw), [g_sum],
              ("tarok_playout_bids_net_scratch", (int(worlds),), env.n * 80 * worlds * 48 + env.n * 40), True,
              ("dense", worlds, contracts, net_seats, seats, depth, pass_value), scratch_out)
    return H.read_words(g_sum)


def list_words(scratch, bound, units, extra=0):
    """(on [units], base [units], total) of a list launch's scratch bytes."""
    at = 48 * bound + extra
    on = scratch[at:at + 4 * units].view(np.uint32)
    base = scratch[at + 4 * units:at + 8 * units].view(np.uint32)
    at += 8 * units + 4 * ((units + 255) // 256)
    return on, base, int(scratch[at:at + 4].view(np.uint32)[0])


def assert_list_is_the_dense_grid_compacted(list_scr, dense_scr, bound, dense_items, units, extra=0):
    """The dense launch's scratch lay between guard bands, so a slot that held no item still has the sentinel for a key.  The
    list's total is the number of dense slots that held one; the compact keys and result words are the dense ones in
    ascending slot order; nothing at or above the total was written in any of the four item arrays.  -> the total."""
    import gpu_harness as H
    dkey, _, dres = H.item_arrays(dense_scr[:dense_items * 48], dense_items)
    live = dkey != np.uint64(SENTINEL_U64)
    assert (dres[~live] == 0).all(), "a dense slot without an item has a result"
    on, base, total = list_words(list_scr, bound, units, extra)
    assert total == int(live.sum()), ("the total word", total, int(live.sum()))
    assert total <= bound
    lkey, _, lres = H.item_arrays(list_scr[:bound * 48], bound)
    assert (lkey[:total] == dkey[live]).all(), "an item's key"
    assert (lres[:total] == dres[live]).all(), "an item's result word"
    for name, lo, width in (("i01", 0, 16), ("i23", 16 * bound, 16), ("ikey", 32 * bound, 8), ("ires", 40 * bound, 8)):
        rest = list_scr[lo + total * width:lo + bound * width]
        assert (rest == 0xA5).all(), ("written at or above the total", name)
    counts = np.array([popc(o) for o in on], np.int64)
    return total, on, base, counts
