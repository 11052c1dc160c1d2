"""CPU-side checks of the void-aware determinized playouts (tarok_shown_voids, tarok_playout_cards_voids): the model of
tests/playout_voids_model.py — the soundness of the void rule on every contract, the counting against brute force, the
uniformity of the constrained re-deal, what a world keeps, the fallbacks, the team rule, the prefix property — and the
argument validation of the two entry points, which make no HIP call and so run without a GPU."""
import ctypes
import inspect
import itertools

import numpy as np
import pytest

import playout_det_model as DM
import playout_model as PM
import playout_voids_model as VM
from oracle import oracle as O
from oracle import tarok_spec as S

SEED = 23
SALT = 6
OTHERS = [1, 2, 3]                       # the hand-made positions: seat 0 moves


def popcount(m):
    return bin(int(m)).count("1")


def word(*pairs):
    """A void word from (seat, class) pairs."""
    w = 0
    for s, k in pairs:
        w |= 1 << (5 * s + k)
    return w


@pytest.mark.parametrize("mix", [S.MIX_ALL, S.MIX_BOT] + [S.MIX_FIXED + c for c in range(10)])
def test_the_void_rule_is_sound_on_every_contract(mix):
    """200 Bot games per mix: after every card, no seat holds a card of a class its bits mark void — and the bits do
    fill up: by the end of a game most seats have shown something."""
    shown = games = 0
    for gidx in range(200):
        g = O.Game.synth(SEED, gidx, 0, mix)
        lead = VM.first_leader(g.g.contract, g.g.declarer)
        key = O.game_key(SEED, gidx, 0)
        cards, w = [], 0
        for q in range(48):
            if g.done:
                break
            c = O.policy_action(key, q, g.legal())
            cards.append(c)
            g.step(c)
            w = VM.shown_voids(cards, lead)
            assert w < 1 << 20
            for s in range(4):
                assert not int(g.g.hand[s]) & VM.class_cards((w >> (5 * s)) & 31), (mix, gidx, q, s, hex(w))
        games += 1
        shown += popcount(w)
    assert games == 200 and shown > 200


def brute(pool, caps, allowed):
    """Every assignment of the pool's cards to the three seats that keeps the sizes and the allowed sets:
    {(mask0, mask1, mask2)}, and the counts by (a, b) = (cards of G01 on o0, cards of G02 on o0)."""
    cards = PM.cards_of(pool)
    gr = VM.groups_of(pool, allowed)
    deals, by_ab = set(), {}
    for assign in itertools.product(range(3), repeat=len(cards)):
        if any(not (allowed[t] >> c) & 1 for c, t in zip(cards, assign)):
            continue
        masks = [0, 0, 0]
        for c, t in zip(cards, assign):
            masks[t] |= 1 << c
        if [popcount(m) for m in masks] != list(caps):
            continue
        deals.add(tuple(masks))
        ab = (popcount(masks[0] & gr["G01"]), popcount(masks[0] & gr["G02"]))
        by_ab[ab] = by_ab.get(ab, 0) + 1
    return deals, by_ab


def cards_mask(*cards):
    return sum(1 << c for c in cards)


# hand-made pools for seat 0 to move: (pool, caps of seats 1 / 2 / 3, void word, what it is there for)
EVERY_GROUP = (cards_mask(0, 1, 8, 9, 16, 17, 24, 32, 33), (4, 3, 2),
               word((3, 0), (2, 1), (1, 2), (2, 3), (3, 3)))            # G01 = clubs, G02, G12, a forced card, Q = taroks
POSITIONS = [
    EVERY_GROUP,
    (cards_mask(0, 1, 8, 9, 32, 40), (2, 2, 2), word((3, 0), (2, 1))),                     # G01 and G02 at once, no G12
    (cards_mask(0, 8, 16, 17, 32, 33, 34), (3, 2, 2), word((1, 2), (2, 2), (2, 0))),       # two forced cards to seat 3
    (cards_mask(2, 3, 4, 10, 33, 35, 50, 53), (3, 3, 2), word((1, 4), (3, 0), (3, 1))),    # seat 1 takes no tarok
    (cards_mask(0, 1, 2, 8, 16, 32), (3, 2, 1), word((2, 0), (3, 0), (1, 1))),             # clubs forced: fill seat 1
    (cards_mask(5, 6, 12, 20, 36, 37, 38, 39, 52), (4, 3, 2), word((0, 0), (0, 4))),       # the mover's own bits: ignored
]


@pytest.mark.parametrize("pos", range(len(POSITIONS)))
def test_the_count_equals_brute_force(pos):
    pool, caps, w = POSITIONS[pos]
    assert popcount(pool) == sum(caps) and 6 <= popcount(pool) <= 9
    allowed = VM.allowed_of(pool, OTHERS, w)
    total, weights, gr, r = VM.count_voids(pool, caps, allowed)
    deals, by_ab = brute(pool, caps, allowed)
    assert total == len(deals) > 0
    assert {ab: t for ab, t in weights.items() if t} == by_ab
    if pos == 0:
        assert all(gr[k] for k in ("G01", "G02", "G12", "Q")) and gr["F"][0] and not gr["E"]
    if pos == 1:
        assert gr["G01"] and gr["G02"] and not gr["G12"]
    if pos == 5:
        assert gr["Q"] == pool                                             # nothing constrains: every card is free


def test_an_empty_allowed_set_a_negative_rest_and_an_empty_count_fall_back():
    pool, caps = cards_mask(0, 1, 8, 24, 32, 33), (2, 2, 2)
    nobody = word((1, 3), (2, 3), (3, 3))                                  # card 24 may go nowhere
    total, _, gr, _ = VM.count_voids(pool, caps, VM.allowed_of(pool, OTHERS, nobody))
    assert total is None and gr["E"] == 1 << 24
    crowded = word((2, 0), (3, 0), (2, 1), (3, 1))                         # three cards forced on seat 1, which holds two
    total, _, _, r = VM.count_voids(pool, caps, VM.allowed_of(pool, OTHERS, crowded))
    assert total is None and r[0] == -1
    pool, caps = cards_mask(0, 1, 8, 9), (0, 1, 3)
    stuck = word((3, 0), (1, 1), (2, 1))                                   # two clubs for seats 1 and 2, which hold one card
    total, weights, _, r = VM.count_voids(pool, caps, VM.allowed_of(pool, OTHERS, stuck))
    assert total == 0 and min(r) >= 0 and not brute(pool, caps, VM.allowed_of(pool, OTHERS, stuck))[0]
    for pool, caps, w in ((cards_mask(0, 1, 8, 24, 32, 33), (2, 2, 2), nobody), (cards_mask(0, 1, 8, 24, 32, 33), (2, 2, 2), crowded),
                          (cards_mask(0, 1, 8, 9), (0, 1, 3), stuck)):
        assert VM.deal_voids(pool, caps, VM.allowed_of(pool, OTHERS, w), 12345) is None


@pytest.mark.parametrize("pos", [0, 1, 3])
def test_the_constrained_deal_is_uniform(pos):
    """1,000 x (the number of valid deals) world keys: every valid deal within 5 sigma of 1,000 (sigma^2 = N p (1 - p),
    p = 1 / deals), no other deal at all.  Deterministic: it ran once and stays."""
    pool, caps, w = POSITIONS[pos]
    allowed = VM.allowed_of(pool, OTHERS, w)
    deals, _ = brute(pool, caps, allowed)
    d = len(deals)
    assert 4 <= d <= 60
    n = 1000 * d
    counts = dict.fromkeys(deals, 0)
    for i in range(n):
        masks = VM.deal_voids(pool, caps, allowed, DM.world_key(SEED, SALT, i // 64, pos, 20, i % 64))
        counts[tuple(masks)] += 1                                          # (KeyError: an invalid deal)
    sigma = (n * (1 / d) * (1 - 1 / d)) ** 0.5
    assert all(abs(c - 1000) <= 5 * sigma for c in counts.values()), counts


def hands(game):
    return [int(game.g.hand[s]) for s in range(4)]


@pytest.mark.parametrize("cards", [5, 13, 22, 34, 46])
def test_a_world_keeps_everything_the_mover_can_see_and_the_voids(cards):
    contracts, differ, constrained = set(), 0, 0
    for gidx in range(100):
        g, played, lead = VM.bot_game(SEED, gidx, 1, S.MIX_ALL, cards)
        if g.done:
            continue
        contracts.add(int(g.g.contract))
        seat = g.seat()
        before = g.lanes()
        for w_ in (VM.shown_voids(played, lead), VM.true_voids(g)):
            for w in range(3):
                wkey = DM.world_key(SEED, SALT, gidx, 1, len(played), w)
                x = VM.world_of(g, wkey, w_)
                assert (g.lanes() == before).all()                               # the game itself is not touched
                h0, h1 = hands(g), hands(x)
                assert [popcount(m) for m in h1] == [popcount(m) for m in h0]    # the hand sizes
                pool0 = pool1 = 0
                for o in DM.others_of(seat):
                    pool0 |= h0[o]
                    pool1 |= h1[o]
                    assert not h1[o] & VM.class_cards((w_ >> (5 * o)) & 31)      # the voids hold
                assert pool1 == pool0                                            # the union of the other hands
                assert all(h1[a] & h1[b] == 0 for a, b in itertools.combinations(range(4), 2))
                assert h1[seat] == h0[seat]                                      # the mover's hand,
                la, lb = g.lanes(), x.lanes()
                assert (la[4:9] == lb[4:9]).all()                                # the piles and the talon ids,
                team_field = np.uint64(15 << 42)
                assert (la[9] & ~team_field) == (lb[9] & ~team_field)            # and all of the rest but the team
                assert x.legal() == g.legal() and x.seat() == seat
                differ += h1 != h0
                constrained += h1 != hands(DM.world_of(g, wkey))
    assert len(contracts) >= (8 if cards < 22 else 4)
    if cards < 46:
        assert differ > 100 and constrained > 100


def test_the_fallbacks_are_the_determinized_worlds():
    """No void of another seat (the mover's own bits do not count), or a word the hands contradict: playout_det_model's
    world, hands and team."""
    same = 0
    for gidx in range(40):
        g, played, lead = VM.bot_game(SEED, gidx, 0, S.MIX_NAVADNA3, 9)
        seat = g.seat()
        oth = DM.others_of(seat)
        full = word(*[(oth[0], k) for k in range(5)])                     # o0 may hold nothing: its cards go nowhere else
        nobody = word(*[(o, k) for o in oth for k in range(5)])
        for w_ in (0, word((seat, 0), (seat, 4)), 31 << (5 * seat), nobody, full | word((oth[1], 4), (oth[2], 4))):
            for w in range(2):
                wkey = DM.world_key(SEED, SALT, gidx, 0, 9, w)
                x, y = VM.world_of(g, wkey, w_), DM.world_of(g, wkey)
                assert hands(x) == hands(y) and int(x.g.team) == int(y.g.team)
                same += 1
    assert same == 400


def test_the_team_follows_the_king_forced_or_drawn():
    """Tri / Dve / Ena with the called king unseen: the world's team is the declarer and whoever received the king — by a
    forced card (only one seat may hold its suit) and by a draw."""
    forced = drawn = changed = 0
    for cards in (6, 17, 30):
        for gidx in range(150):
            g, played, lead = VM.bot_game(SEED, gidx, 0, S.MIX_NAVADNA3, cards)
            if g.done:
                continue
            seat = g.seat()
            oth = DM.others_of(seat)
            kb = 1 << (8 * int(g.g.king) + 7)
            if not any(int(g.g.hand[o]) & kb for o in oth):
                continue
            w_ = VM.true_voids(g)
            may = [o for o in oth if not (w_ >> (5 * o + int(g.g.king))) & 1]
            for w in range(2):
                x = VM.world_of(g, DM.world_key(SEED, SALT, gidx, 0, len(played), w), w_)
                (holder,) = [o for o in oth if int(x.g.hand[o]) & kb]
                assert holder in may
                assert int(x.g.team) == (1 << int(g.g.declarer)) | (1 << holder)
                forced += len(may) == 1
                drawn += len(may) > 1
                changed += int(x.g.team) != int(g.g.team)
    assert forced >= 20 and drawn >= 20 and changed >= 10, (forced, drawn, changed)


def test_worlds_and_samples_are_prefixes():
    g, played, lead = VM.bot_game(SEED, 7, 1, S.MIX_ALL, 22)
    w_ = VM.shown_voids(played, lead)
    assert w_ and not g.done
    lanes = g.lanes()
    sc = VM.playout_scores(lanes, 1, SEED, 9, 7, 15, 4, 3, w_)
    assert sc.shape == (12, 4, 3, 4)
    for worlds, samples in ((1, 1), (2, 3), (4, 2), (4, 3)):
        sums, _ = VM.playout_cards(lanes, 1, SEED, 9, 7, 15, worlds, samples, w_)
        assert (sums == VM.sums_of(sc, worlds, samples)).all()
        assert (sums == sc[:, :worlds, :samples].reshape(12, -1, 4).sum(axis=1)).all()
    assert (VM.playout_scores(lanes, 1, SEED, 9, 7, 15, 4, 3, 0) == DM.playout_scores(lanes, 1, SEED, 9, 7, 15, 4, 3)).all()


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- before the dlopen: one HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_abi_list_and_python_surface_have_the_void_aware_playouts():
    from tarok_amd import _native, karte as K
    from tarok_amd import evaluate as EV
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.selfplay import SelfPlay
    assert "tarok_shown_voids" in _native.SYMBOLS and "tarok_playout_cards_voids" in _native.SYMBOLS
    assert K.VOID_SEAT_BITS == 5 and K.VOID_TAROK == 4
    sig = inspect.signature(TarokVecEnv.playout_cards_voids).parameters
    assert list(sig)[1:] == ["worlds", "samples", "salt", "seats", "seats_per_game", "voids", "sum_out", "action_out"]
    assert sig["salt"].default == 0 and sig["seats"].default == 15 and sig["voids"].default is None
    assert list(inspect.signature(TarokVecEnv.shown_voids).parameters) == ["self", "out"]
    assert inspect.signature(EV.evaluate_playout_vs_bot).parameters["voids"].default is False
    assert inspect.signature(SelfPlay.evaluate).parameters["playout_voids"].default is False


def test_the_entry_points_validate_before_any_hip_call(L):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create, and no
    history either) is enough."""
    z = ctypes.c_void_p(0)
    stand_in = ctypes.create_string_buffer(1 << 16)
    env = ctypes.cast(stand_in, ctypes.c_void_p)
    out = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    f = L.tarok_shown_voids
    assert f(None, out, z) == -1
    assert f(env, z, z) == -1
    assert f(env, out, z) == -1                                # an env without TAROK_HISTORY
    f = L.tarok_playout_cards_voids
    assert f(None, 4, 4, 0, 15, z, out, out, out, z) == -1
    assert f(env, 4, 4, 0, 15, z, z, out, out, z) == -1        # voids is required
    assert f(env, 0, 4, 0, 15, z, out, out, out, z) == -1
    assert f(env, 65, 4, 0, 15, z, out, out, out, z) == -1
    assert f(env, -2, 4, 0, 15, z, out, out, out, z) == -1
    assert f(env, 4, 0, 0, 15, z, out, out, out, z) == -1
    assert f(env, 4, 1025, 0, 15, z, out, out, out, z) == -1
    assert f(env, 4, 4, 0, 16, z, out, out, out, z) == -1
    assert f(env, 4, 4, 0, -1, z, out, out, out, z) == -1
    assert f(env, 4, 4, 0, 15, z, out, z, z, z) == -1
