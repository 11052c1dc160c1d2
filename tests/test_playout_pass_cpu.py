"""CPU: the definition of tarok_playout_bids_pass / tarok_bid_round_pass as tests/playout_pass_model.py states it, the host
answer rule with its pass switch (tarok_amd.licitacija.playout_answer) and the learner's loss with the pass row.  No GPU
involved."""
import numpy as np
import pytest

import bid_head_model as HM
import playout_bids_model as BM
import playout_det_model as DM
import playout_exchange_model as XM
import playout_model as PM
import playout_pass_model as PS
from oracle import tarok_spec as S
from tarok_amd import licitacija as LI

KEYS = 3000


def scripted_round(pkey, v):
    """Igra.licitacija's control flow as the host state machine walks it, the Bot's dice of `pkey` on three seats and a
    scripted player on v that gives its least answer; None where the round does not end within the device's 8 rounds."""
    n = [0]

    def ask(seat, m, o, p):
        i = n[0]
        n[0] += 1
        if seat == v:
            return LI.NAPREJ if o is None else o
        return LI.base_filter(S.bot_wish(S.rng32(pkey, S.DRAW_BID + i)), m, o, p)
    try:
        declarer, top = LI.licitacija(ask, max_rounds=8)
    except RuntimeError:
        return None
    return top // 10, (declarer if top else 0)


@pytest.mark.parametrize("v", [0, 1, 2, 3])
def test_who_declares_in_a_pass_playout_and_the_round_is_licitacija_with_v_muted(v):
    checked, klops, declarers = 0, 0, set()
    for i in range(KEYS):
        pkey = PS.pass_key(9, 1, i, 2, v, i % 64, i % 7)
        c, d, k = PS.pass_round(pkey, v)
        # the first answers of the Bots among seats 1, 2, 3 (call n = seat - 1; v's own call counts): a wish has to beat
        # the floor of Tri and every bid before it
        running = 10
        for seat in (1, 2, 3):
            if seat != v:
                running = max(running, S.bot_wish(S.rng32(pkey, S.DRAW_BID + seat - 1)))
        bots_passed = running == 10
        if v == 0:
            assert (d == 0) == (c == S.KLOP) == bots_passed, (i, c, d)
        else:
            assert d != v and (c != S.KLOP or d == 0) and (c != S.KLOP or bots_passed), (i, c, d)
        assert k == (S.pick(S.rng32(pkey, S.DRAW_KING), 4) if c in (1, 2, 3) else 0)
        klops += c == S.KLOP
        declarers.add(d)
        want = scripted_round(pkey, v)
        if want is not None:
            assert (c, d) == want, (i, (c, d), want)
            checked += 1
    assert checked > 0.9 * KEYS and klops > 0 and declarers == {0, 1, 2, 3} - ({v} if v else set())


def test_seat_zero_muted_declares_exactly_when_three_bots_pass():
    """With v = 0 silent, seat 0 is left the forced Klop when the three Bots pass: a Bot's wish beats the floor of Tri with
    probability 1/3 (Dve or Ena), so about 8/27 of the keys."""
    n = sum(PS.pass_round(PS.pass_key(4, 0, i, 0, 0, 0, 0), 0)[:2] == (S.KLOP, 0) for i in range(KEYS))
    assert abs(n - KEYS * 8 / 27) < 5 * (KEYS * (8 / 27) * (19 / 27)) ** 0.5, n
    # a viewer on another seat: the three Bots that pass are two Bots and v itself, and seat 0, a Bot, may bid on
    c = [PS.pass_round(PS.pass_key(4, 0, i, 0, 2, 0, 0), 2) for i in range(KEYS)]
    assert all(d != 2 for _, d, _ in c) and any(ct == S.KLOP for ct, _, _ in c) and any(ct in (1, 2, 3) and d == 0 for ct, d, _ in c)


def test_prefix_property_in_worlds_and_samples():
    perm = S.deal(S.game_key(5, 9, 2))
    big = PS.playout_scores(perm, 2, 5, 1, 9, 0b0101, 3, 2, 0x003)
    for w, s in ((1, 1), (2, 1), (3, 2), (1, 2)):
        small = PS.playout_scores(perm, 2, 5, 1, 9, 0b0101, w, s, 0x003)
        assert (small == big[:, :, :w, :s]).all()
        assert (PS.pass_sums(perm, 2, 5, 1, 9, 0b0101, w, s, 0x003) == big[:, :, :w, :s].sum(axis=(2, 3))).all()
    # (a seat that neither declares nor is called scores nothing: a viewer's pass row may well be all zero)
    assert big[[0, 2], 19].any() and not big[1].any() and not big[3].any()
    # rows 0..18 are the playout bidder's own, and the pass row does not depend on the mask
    assert (big[:, :19] == BM.playout_scores(perm, 2, 5, 1, 9, 0b0101, 3, 2, 0x003)[:, :19]).all()
    assert (PS.playout_scores(perm, 2, 5, 1, 9, 0b0101, 3, 2, 0x200)[:, 19] == big[:, 19]).all()
    assert not PS.playout_scores(perm[:53] + [perm[0]], 2, 5, 1, 9, 15, 1, 1, 1).any()


def test_key_separation_of_row_19():
    ep, gidx, seed, salt = 7, 11, 5, 0
    ours = {PS.pass_key(seed, salt, gidx, ep, v, w, k) for v in range(4) for w in range(4) for k in range(4)}
    assert len(ours) == 64
    others = {BM.playout_key(seed, salt, gidx, ep, v, r, w, k) for v in range(4) for r in range(19) for w in range(4) for k in range(4)}
    others |= {BM.world_key(seed, salt, gidx, ep, v, w) for v in range(4) for w in range(64)}
    others |= {S.game_key(seed, gidx, e) for e in range(64)}
    others |= {PM.playout_key(seed, salt, gidx, ep, n, c, k) for n in (0, 5) for c in range(54) for k in range(2)}
    others |= {DM.world_key(seed, salt, gidx, ep, n, w) for n in (0, 5) for w in range(4)}
    others |= {DM.playout_key(seed, salt, gidx, ep, n, c, w, k) for n in (0, 5) for c in range(54) for w in range(2) for k in range(2)}
    others |= {XM.world_key(seed, salt, gidx, ep, w) for w in range(4)}
    others |= {XM.candidate_key(seed, salt, gidx, ep, i, d) for i in range(6) for d in range(8)}
    others |= {XM.playout_key(seed, salt, gidx, ep, i, d, w, k) for i in range(6) for d in range(8) for w in range(2) for k in range(2)}
    assert not ours & others
    # r = 19 fits the row field (bits 21..25) below v's bits 26, 27 and above the largest w
    assert 19 < 32 and (19 << 21) < (1 << 26) and (63 << 15) < (1 << 21) and 1023 < (1 << 15)


def random_sums(key, lo=-20, span=41):
    return [[S.rng32(key, 200 + 20 * v + r) % span + lo if r < 19 else 0 for r in range(20)] for v in range(4)]


def test_with_row_19_zero_it_is_the_playout_bidders_round_at_threshold_margin():
    differs = 0
    for i in range(KEYS):
        key = S.game_key(8, i, 1)
        sums = random_sums(key)
        contracts = (BM.DEFAULT_CONTRACTS, BM.ALL_CONTRACTS, 0x2AB)[i % 3]
        margin = (-30, 0, 40)[(i // 3) % 3]
        playouts = 1 + i % 2
        seats = (15, 1 << (i & 3), 0b0110)[(i // 9) % 3]
        assert PS.bid_round(key, sums, playouts, margin, contracts, seats) == BM.bid_round(key, sums, playouts, margin, contracts, seats), i
        for v in range(4):
            for m, o, p in ((10, None, False), (20, None, True), (10, 10, False), (-10, 0, False), (30, 30, False)):
                a = PS.answer(sums[v], m, o, p, playouts, margin, contracts)
                assert a == BM.answer(sums[v], m, o, p, playouts, margin, contracts)
                assert a == LI.playout_answer(sums[v], m, o, p, playouts, margin, contracts, pass_value=True)
                assert a == LI.playout_answer(sums[v], m, o, p, playouts, margin, contracts)
        # ... and a pass row that is not zero moves the bar by exactly that much
        for v in range(4):
            sums[v][19] = S.rng32(key, 300 + v) % 31 - 15
        differs += PS.bid_round(key, sums, playouts, margin, contracts, seats) != BM.bid_round(key, sums, playouts, margin, contracts, seats)
        for v in range(4):
            for m, o, p in ((10, None, False), (-10, 0, False)):
                a = PS.answer(sums[v], m, o, p, playouts, margin, contracts)
                assert a == LI.playout_answer(sums[v], m, o, p, playouts, margin, contracts, pass_value=True)
                shifted = list(sums[v])
                shifted[19] = 0
                assert a == BM.answer([s - sums[v][19] for s in shifted], m, o, p, playouts, margin, contracts)
    assert differs > 50


@pytest.mark.parametrize("answer", [lambda *a: PS.answer(*a), lambda *a: LI.playout_answer(*a, pass_value=True)])
def test_hand_made_rows(answer):
    A = lambda S_, m, o, p, playouts=1, margin=0, contracts=BM.ALL_CONTRACTS: answer(S_, m, o, p, playouts, margin, contracts)
    # a bid that clears 0 but not the pass
    row = [0] * 20
    row[1], row[19] = 4, 6
    assert A(row, 0, None, False) == -10 and BM.answer(row, 0, None, False, 1, 0, BM.ALL_CONTRACTS) == 10
    row[19] = 3
    assert A(row, 0, None, False) == 10 and A(row, 0, None, False, margin=1) == -10        # (strict: 4 > 3 + 1 fails)
    # a negative bid that clears a more negative pass
    row = [-50] * 20
    row[5], row[19] = -4, -9
    assert A(row, 10, None, False) == 20 and BM.answer(row, 10, None, False, 1, 0, BM.ALL_CONTRACTS) == -10
    assert A(row, 10, None, False, playouts=2, margin=3) == -10 and A(row, 10, None, False, playouts=2, margin=2) == 20
    # the holder standing: the bid has to beat both the pass and standing
    row = [0] * 20
    row[2], row[6], row[19] = 5, 9, 7
    assert A(row, 10, 10, False) == 20
    row[19] = 9
    assert A(row, 10, 10, False) == 10                                                   # over standing, not over the pass
    row[19], row[2] = 0, 9
    assert A(row, 10, 10, False) == 10                                                   # over the pass, not over standing
    # the forced Klop: Klop's own sum and the pass are both bars; the answer is Klop, never Naprej
    row = [-9] * 20
    row[0], row[9], row[19] = -2, -1, -5
    assert A(row, -10, 0, False) == 30
    row[19] = -1
    assert A(row, -10, 0, False) == 0
    row[0], row[19] = 3, -20
    assert A(row, -10, 0, False) == 0
    # the pass row is never a candidate, whatever it holds
    assert A([-5] * 19 + [1000], 0, None, False, margin=-2000) == 10
    assert A([0] * 19 + [-1000], 90, None, False) == -10


def test_the_round_on_hand_made_sums():
    """Seat 3 alone in the set, the three Bots wishing Naprej: with a Dve worth 4 (Tri is the floor, no bid for seats 1, 2,
    3) the seat declares it against a pass worth 3, and passes against one worth 4, which leaves seat 0 the forced Klop."""
    key = next(S.game_key(21, i, 0) for i in range(1000)
               if all(S.bot_wish(S.rng32(S.game_key(21, i, 0), S.DRAW_BID + n)) == -10 for n in (0, 1, 3)))
    sums = [[0] * 20 for _ in range(4)]
    sums[3][6] = 4
    sums[3][19] = 3
    assert PS.bid_round(key, sums, 1, 0, BM.DEFAULT_CONTRACTS, 8) == (2, 3, 1)
    sums[3][19] = 4
    assert PS.bid_round(key, sums, 1, 0, BM.DEFAULT_CONTRACTS, 8) == (0, 0, 0)
    assert PS.bid_round(key, sums, 1, -1, BM.DEFAULT_CONTRACTS, 8) == (2, 3, 1)
    assert BM.bid_round(key, sums, 1, 0, BM.DEFAULT_CONTRACTS, 8) == (2, 3, 1)


def numpy_loss(out, sums, playouts, reward_scale, contracts, pass_value):
    rows = [r for r in range(19) if BM.played(r, contracts)] + ([19] if pass_value else [])
    d = np.asarray(out, np.float64)[:, rows] - np.asarray(sums, np.float64)[:, rows] / playouts * reward_scale
    a = np.abs(d)
    return float(np.where(a <= 1, 0.5 * d * d, a - 0.5).mean())


@pytest.mark.parametrize("contracts", [BM.DEFAULT_CONTRACTS, BM.ALL_CONTRACTS, 0x001])
def test_the_learners_loss_with_and_without_the_pass_row(contracts):
    import torch
    from tarok_amd import bidding as B
    rng = np.random.default_rng(7)
    words = np.array([HM.game_words(rng.permutation(54).tolist()) for _ in range(64)], np.uint64)
    fw = torch.from_numpy(words.view(np.int64))
    sums = torch.from_numpy(rng.integers(-1200, 1200, size=(64, 4, BM.ROWS)).astype(np.int32))
    flat = sums.reshape(256, BM.ROWS)
    plain, passing = B.BidLearner(None, contracts=contracts, seed=3), B.BidLearner(None, contracts=contracts, seed=3, pass_value=True)
    with torch.no_grad():
        out = passing.outputs(fw)
        assert (plain.outputs(fw) == out).all()
    for lr, pv in ((plain, False), (passing, True)):
        want = numpy_loss(out.numpy(), flat.numpy(), 16, 1.0 / 70.0, contracts, pv)
        got = float(lr.loss(fw, sums, 16).detach())
        assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (pv, got, want)
        assert abs(want - HM.huber_loss(out.numpy(), flat.numpy(), 16, 1.0 / 70.0, contracts)) > 1e-6 or not pv
        o = out.clone().requires_grad_(True)
        B.bid_loss(o, flat, 16, 1.0 / 70.0, contracts, pass_value=pv).backward()
        used = np.array([BM.played(r, contracts) for r in range(19)] + [pv] + [False] * 44)
        g = o.grad.numpy()
        assert (g[:, ~used] == 0).all() and (g[:, used] != 0).mean() > 0.99
        other = flat.clone()
        other[:, 19] += 999
        assert (float(lr.loss(fw, other, 16).detach()) == got) == (not pv)
    # without the switch the loss is the one the learner had: the same number as the head model's statement
    assert abs(float(plain.loss(fw, sums, 16).detach()) - HM.huber_loss(out.numpy(), flat.numpy(), 16, 1.0 / 70.0, contracts)) < 1e-5
    first = float(passing.loss(fw, sums, 16).detach())
    for _ in range(20):
        passing.step(fw, sums, 16)
    assert float(passing.loss(fw, sums, 16).detach()) < first
