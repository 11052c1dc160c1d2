"""CPU: the definition of tarok_playout_bids / tarok_bid_round as tests/playout_bids_model.py states it, the host answer
rule (tarok_amd.licitacija.playout_answer) and the argument checks of both C calls.  No GPU involved."""
import collections
import ctypes as C
import math
import os

import pytest

import playout_bids_model as BM
import playout_det_model as DM
import playout_exchange_model as XM
import playout_model as PM
from oracle import tarok_spec as S
from tarok_amd import licitacija as LI


def test_rows():
    assert [BM.row_option(r)[0] for r in range(19)] == [0] + [1] * 4 + [2] * 4 + [3] * 4 + [4, 5, 6, 7, 8, 9]
    assert [BM.row_option(r)[1] for r in range(1, 13)] == [0, 1, 2, 3] * 3
    assert [LI.row_bid(r) for r in range(19)] == [10 * BM.row_option(r)[0] for r in range(19)]
    from tarok_amd import karte as K
    assert [K.bid_row_option(r) for r in range(19)] == [BM.row_option(r) for r in range(19)]


def test_a_world_keeps_the_viewers_hand_the_sizes_and_the_deck():
    for gidx in range(40):
        perm = S.deal(S.game_key(1, gidx, 0))
        for v in range(4):
            world = BM.world_of(perm, v, BM.world_key(1, 0, gidx, 0, v, gidx % 5))
            assert sorted(world) == list(range(54))
            assert sorted(world[12 * v:12 * v + 12]) == sorted(perm[12 * v:12 * v + 12])
            assert world != perm


def test_the_walk_is_uniform_on_a_small_pool():
    """Hands 1 / 1 / 1 and a talon of 2 from five cards: 5! / 1 = 120 ordered arrangements (the talon's slot order counts),
    24,000 world keys, each arrangement within 5 sigma of 200."""
    seen = collections.Counter()
    trials = 24000
    for t in range(trials):
        hands, talon = BM.walk([3, 9, 20, 33, 51], [1, 1, 1, 2], BM.world_key(7, 0, t, 1, 2, t % 64))
        seen[(hands[0][0], hands[1][0], hands[2][0], talon[0], talon[1])] += 1
    assert len(seen) == 120
    p = 1 / 120
    sigma = math.sqrt(trials * p * (1 - p))
    assert all(abs(c - trials * p) < 5 * sigma for c in seen.values()), (min(seen.values()), max(seen.values()))


def test_talon_slot_order():
    """The j-th talon card, ascending, takes the pick(rng32(wkey, 320 + j), free slots left)-th free slot."""
    for t in range(200):
        wkey = BM.world_key(3, 1, t, 0, 1, 0)
        _, talon = BM.walk(list(range(10, 20)), [2, 1, 1, 6], wkey)
        cards = sorted(talon)
        free, exp = list(range(6)), [None] * 6
        for j, c in enumerate(cards):
            exp[free.pop(S.pick(S.rng32(wkey, 320 + j), len(free)))] = c
        assert talon == exp
    assert any(BM.walk(list(range(10, 20)), [2, 1, 1, 6], BM.world_key(3, 1, t, 0, 1, 0))[1] !=
               sorted(BM.walk(list(range(10, 20)), [2, 1, 1, 6], BM.world_key(3, 1, t, 0, 1, 0))[1]) for t in range(5))


def test_the_partner_follows_the_worlds_hands():
    """A called king in the viewer's hand or in the world's talon: the viewer plays alone; else with its holder."""
    from oracle import oracle as O
    alone = together = 0
    for gidx in range(60):
        perm = S.deal(S.game_key(2, gidx, 0))
        v = gidx & 3
        world = BM.world_of(perm, v, BM.world_key(2, 0, gidx, 0, v, 0))
        for king in range(4):
            g = O.Game(world, S.TRI, v, king)
            kc = 8 * king + 7
            holder = world.index(kc) // 12
            if holder == v or holder == 4:
                assert int(g.g.team) == 1 << v
                alone += 1
            else:
                assert int(g.g.team) == (1 << v) | (1 << holder)
                together += 1
    assert alone > 20 and together > 100


def test_prefix_property_in_worlds_and_samples():
    perm = S.deal(S.game_key(5, 9, 2))
    big = BM.playout_scores(perm, 2, 5, 1, 9, 0b0101, 3, 2, 0x083)
    for w, s in ((1, 1), (2, 1), (3, 2), (1, 2)):
        small = BM.playout_scores(perm, 2, 5, 1, 9, 0b0101, w, s, 0x083)
        assert (small == big[:, :, :w, :s]).all()
        assert (BM.sums_of(big, w, s) == small.sum(axis=(2, 3))).all()
    assert not big[1].any() and not big[3].any() and big[0].any() and big[2].any()
    played = [r for r in range(20) if r < 19 and BM.played(r, 0x083)]
    assert played == [0, 1, 2, 3, 4, 16] and not big[:, [r for r in range(20) if r not in played]].any()
    assert not BM.playout_scores(perm[:53] + [perm[0]], 2, 5, 1, 9, 15, 1, 1, 1).any()


def test_key_separation_from_every_stream_of_the_key_table():
    """Tags 010 and 011 in the top three bits of the episode word: no other stream of INTEGRATION.md section 2 has them —
    the game's own key (episode < 2^32: 000), tarok_playout_cards (1 << 63: 100 .. with ep < 2^32 never 01x), the
    candidates (101), the determinized playouts (3 << 62: 11x) and worlds (111)."""
    ep, gidx, seed, salt = 7, 11, 5, 0
    ours = {BM.world_key(seed, salt, gidx, ep, v, w) for v in range(4) for w in range(4)}
    ours |= {BM.playout_key(seed, salt, gidx, ep, v, r, w, k) for v in range(4) for r in range(19) for w in range(2) for k in range(2)}
    assert len(ours) == 16 + 4 * 19 * 4
    others = {S.game_key(seed, gidx, e) for e in range(64)}
    others |= {PM.playout_key(seed, salt, gidx, ep, n, c, k) for n in (0, 5) for c in range(54) for k in range(2)}
    others |= {DM.world_key(seed, salt, gidx, ep, n, w) for n in (0, 5) for w in range(4)}
    others |= {DM.playout_key(seed, salt, gidx, ep, n, c, w, k) for n in (0, 5) for c in range(54) for w in range(2) for k in range(2)}
    others |= {XM.world_key(seed, salt, gidx, ep, w) for w in range(4)}
    others |= {XM.candidate_key(seed, salt, gidx, ep, i, d) for i in range(6) for d in range(8)}
    others |= {XM.playout_key(seed, salt, gidx, ep, i, d, w, k) for i in range(6) for d in range(8) for w in range(2) for k in range(2)}
    assert not ours & others
    top = lambda v, r, w, k: ((3 << 61) | (ep << 28) | (v << 26) | (r << 21) | (w << 15) | k) >> 61
    assert top(3, 18, 63, 1023) == 3 and ((2 << 61) | (0xFFFFFFFF << 28) | (3 << 6) | 63) >> 61 == 2
    # the fields of a playout key do not overlap: k < 2^10 <= 2^15, w < 2^6, r < 2^5, v < 2^2, below the episode's bit 28
    assert (1023 < 1 << 15) and (63 << 15 < 1 << 21) and (18 << 21 < 1 << 26) and (3 << 26 < 1 << 28)


def random_sums(key, lo=-20, span=41):
    return [[S.rng32(key, 200 + 20 * v + r) % span + lo if r < 19 else 0 for r in range(20)] for v in range(4)]


def test_the_models_loop_is_licitacija_with_playout_answer():
    checked = 0
    for i in range(3000):
        key = S.game_key(8, i, 1)
        sums = random_sums(key)
        contracts = (BM.DEFAULT_CONTRACTS, BM.ALL_CONTRACTS, 0x2AB)[i % 3]
        threshold = (0, -7, 5)[(i // 3) % 3]
        calls = []

        def ask(seat, m, o, p):
            calls.append(seat)
            return LI.playout_answer(sums[seat], m, o, p, 1, threshold, contracts)
        try:
            declarer, top = LI.licitacija(ask, max_rounds=8)
        except RuntimeError:
            continue
        c, d, k = BM.bid_round(key, sums, 1, threshold, contracts, 15)
        assert (c, d) == (top // 10, declarer if top else 0), i
        if c in (1, 2, 3):
            rows = BM.rows_of(c)
            assert sums[d][rows[k]] == max(sums[d][r] for r in rows) and all(sums[d][rows[j]] < sums[d][rows[k]] for j in range(k))
        else:
            assert k == 0
        checked += 1
    assert checked > 2500


def test_the_empty_seat_set_is_the_bots_round_on_10000_keys():
    for i in range(10000):
        key = S.game_key(12, i, 3)
        declarer, contract = S.bot_bidding(key)
        c, d, k = S.sample_setup(key, S.MIX_BOT)
        assert (c, d) == (contract, declarer)
        assert BM.bid_round(key, None, 1, 0, BM.DEFAULT_CONTRACTS, 0) == (c, d, max(k, 0)), i


@pytest.mark.parametrize("answer", [lambda *a: BM.answer(*a), lambda *a: LI.playout_answer(*a)])
def test_the_answer_rules_edges(answer):
    row = [0] * 20
    A = lambda S_, m, o, p, playouts=1, thr=0, contracts=BM.ALL_CONTRACTS: answer(S_, m, o, p, playouts, thr, contracts)
    # no candidate: nothing beats Odprti_berac; nothing in the mask beats Ena
    assert A([9] * 20, 90, None, False) == -10 and A([9] * 20, 90, 90, False) == 90
    assert A([9] * 20, 30, None, False, contracts=BM.DEFAULT_CONTRACTS) == -10
    # a tie goes to the lowest row: Tri with suit 0 before Dve
    row = [0] * 20
    row[1] = row[5] = row[13] = 4
    assert A(row, 0, None, False) == 10 and A(row, 10, None, False) == 20 and A(row, 20, None, False) == 40
    # the threshold is strict and scales with the playouts
    assert A(row, 0, None, False, playouts=2, thr=2) == -10 and A(row, 0, None, False, playouts=1, thr=3) == 10
    row[16], row[17], row[18] = -3, -9, -9
    assert A(row, 60, None, False) == -10 and A(row, 60, None, False, thr=-4) == 70
    # priority: matching the standing bid is allowed
    assert A(row, 40, None, True) == 40 and A(row, 40, None, False) == -10
    # the holder stands unless a higher bid is worth strictly more than standing
    row = [0] * 20
    row[2], row[6] = 5, 5
    assert A(row, 10, 10, False) == 10
    row[6] = 6
    assert A(row, 10, 10, False) == 20 and A(row, 10, 10, False, thr=6) == 10
    # the forced Klop: Klop's own sum is the bar, and Klop is never a candidate
    row = [-9] * 20
    row[0], row[9] = -2, -1
    assert A(row, -10, 0, False) == 0 and A(row, -10, 0, False, thr=-5) == 30
    row[0] = 3
    assert A(row, -10, 0, False, thr=-5) == 0
    assert A([50] + [0] * 19, -10, None, False, thr=-1, contracts=1) == -10


def test_argument_checks_without_a_gpu():
    """TAROK_EINVAL before any HIP call: a NULL env never reaches the device, and no env exists without one."""
    from tarok_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import tarok_amd
        tarok_amd.build()
    L = C.CDLL(_native.LIB_PATH)
    vp, i32, u32, u64 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64
    L.tarok_playout_bids.restype = i32
    L.tarok_playout_bids.argtypes = [vp, u32, vp, i32, i32, i32, u64, i32, vp, vp, vp]
    L.tarok_bid_round.restype = i32
    L.tarok_bid_round.argtypes = [vp, u32, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    out = (C.c_int32 * 80)()
    o8 = (C.c_int8 * 4)()
    assert L.tarok_playout_bids(None, 0, None, 1, 1, 15, 0, 15, None, out, None) == -1
    assert L.tarok_bid_round(None, 0, out, 1, 0, 15, 15, None, o8, o8, o8, None) == -1
    # the other checks come before the env is touched: a fake, never dereferenced handle shows them
    fake = (C.c_char * 4096)()
    h = C.cast(fake, vp)
    for worlds, samples, contracts, seats in ((0, 1, 15, 15), (65, 1, 15, 15), (1, 0, 15, 15), (1, 1025, 15, 15), (1, 1, 0, 15),
                                              (1, 1, 0x400, 15), (1, 1, 15, -1), (1, 1, 15, 16)):
        assert L.tarok_playout_bids(h, 0, None, worlds, samples, contracts, 0, seats, None, out, None) == -1
    assert L.tarok_playout_bids(h, 0, None, 1, 1, 15, 0, 15, None, None, None) == 0          # sum_out NULL: nothing is launched
    for sums, playouts, contracts, seats, outs in ((out, 0, 15, 15, (o8, o8, o8)), (out, 1, 0, 15, (o8, o8, o8)),
                                                   (out, 1, 0x400, 15, (o8, o8, o8)), (out, 1, 15, 16, (o8, o8, o8)),
                                                   (out, 1, 15, -1, (o8, o8, o8)), (None, 1, 15, 1, (o8, o8, o8)),
                                                   (out, 1, 15, 0, (None, None, None))):
        assert L.tarok_bid_round(h, 0, sums, playouts, 0, contracts, seats, None, outs[0], outs[1], outs[2], None) == -1
    assert L.tarok_bid_round(h, 0, None, 1, 0, 15, 0, o8, o8, o8, o8, None) == -1             # a seat array without sums
