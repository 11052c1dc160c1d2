"""CPU: the exchange head's definition (tests/exchange_head_model.py) on hand-made games, the learner's targets and loss
(tarok_amd/exchange.py) against the numpy statement, and the argument checks of both C calls.  No GPU involved."""
import ctypes as C
import os

import numpy as np
import pytest

import exchange_head_model as EM
from oracle import oracle as O
from oracle import tarok_spec as S

XM = EM.XM
INF, NAN = float("inf"), float("nan")
HIGH_TAROKS = list(range(39, 54))                    # not discardable, like the kings and the pagat


def deal_with(hand, declarer, talon):
    """A deal row in which `declarer` holds `hand` (12 cards) and the talon is `talon` (6 cards, in order)."""
    rest = [c for c in range(54) if c not in hand and c not in talon]
    perm = []
    for v in range(4):
        perm += list(hand) if v == declarer else [rest.pop() for _ in range(12)]
    return perm + list(talon)


def bits(w, lo, hi):
    return [b for b in range(lo, hi) if (w >> b) & 1]


@pytest.mark.parametrize("contract", range(1, 7))
def test_every_contract_declarer_and_group(contract):
    gs = S.GROUP_SIZE[contract]
    for declarer in range(4):
        hand = list(range(3 * declarer, 3 * declarer + 9)) + [32, 40, 53]
        talon = [60 - 9 - j for j in range(6)]       # 51 .. 46
        king = (declarer + 1) % 4
        game = O.Game(deal_with(hand, declarer, talon), contract, declarer, king if contract <= 3 else -1)
        assert XM.waiting(game)
        words = EM.game_words(game)
        for i in range(8):
            w = words[i]
            if i >= 6 // gs:
                assert w == [0, 0, 0, 0]
                continue
            group = talon[i * gs:(i + 1) * gs]
            assert bits(w[0], 0, 54) == sorted(hand + group) and bits(w[0], 54, 58) == [54 + declarer]
            assert bits(w[0], 58, 61) == [61 - gs] and bits(w[0], 61, 64) == ([61] if contract >= 4 else [])
            assert bits(w[1], 0, 54) == sorted(set(talon) - set(group)) and bits(w[1], 58, 64) == [58 + i]
            assert bits(w[1], 54, 58) == ([54 + king] if contract <= 3 else [])
            assert bits(w[2], 0, 54) == sorted(group)
            taroks = sum(1 for c in hand + group if c >= 32)
            assert bits(w[3], 0, 16) == list(range(taroks))
            for k in range(4):
                assert bits(w[3], 16 + 8 * k, 24 + 8 * k) == [16 + 8 * k + j for j in range(sum(1 for c in hand if c // 8 == k))]
            assert bits(w[3], 52, 55) == [52, 54] and bits(w[3], 55, 64) == []
        assert EM.game_words(game, part=False) == [[0] * 4] * 8


def test_where_the_called_king_lies():
    king = 2
    kc = 8 * king + 7
    plain = [0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 33, 34]
    for where, hand, talon in (("hand", plain[:11] + [kc], [40, 41, 42, 43, 44, 45]),
                               ("group 1", plain, [40, 41, kc, 43, 44, 45]),
                               ("another hand", plain, [40, 41, 42, 43, 44, 45])):
        game = O.Game(deal_with(hand, 1, talon), 2, 1, king)             # Dve: groups of two
        flags = [(w[2] >> 54) & 7 for w in EM.game_words(game)[:3]]
        assert flags == {"hand": [2, 2, 2], "group 1": [4, 1, 4], "another hand": [0, 0, 0]}[where], where
        assert all((w[3] >> (48 + king)) & 1 == (where == "hand" or (where == "group 1" and i == 1))
                   for i, w in enumerate(EM.game_words(game)[:3]))
    solo = O.Game(deal_with(plain[:11] + [kc], 1, [40, 41, 42, 43, 44, 45]), 5, 1, -1)
    assert all((w[2] >> 54) == 0 and (w[1] >> 54) & 15 == 0 for w in EM.game_words(solo)[:3])


def test_the_whole_hand_stands_in_when_too_few_cards_are_discardable():
    hand, talon = HIGH_TAROKS[:12], [7, 15, 23, 31, 32, 0]               # the kings, the pagat and one discardable card
    game = O.Game(deal_with(hand, 0, talon), 1, 0, 0)                     # Tri: group 0 = three kings, group 1 = king, pagat, 0
    key = S.game_key(1, 2, 3)
    rows = np.zeros((8, 64))
    rows[0, 54], rows[0, [7, 15, 23]], rows[0, 50] = 1.0, (5.0, 6.0, 4.0), 4.5
    assert EM.candidate_mask(EM.mask_of(hand + talon[:3]), 3) == EM.mask_of(hand + talon[:3])
    assert EM.decide(game, 15, key, rows) == (0, [15, 7, 50])            # non-discardable cards, by score
    rows[1, 54], rows[1, 31], rows[1, 0] = 2.0, 9.0, -1.0
    assert EM.decide(game, 15, key, rows) == (1, [31, 32, 39])           # one discardable card is fewer than three: all of P_1, ties by card
    game = O.Game(deal_with(hand, 0, talon), 3, 0, 0)                     # Ena: six groups of one
    rows = np.zeros((8, 64))
    rows[5, 54] = 1.0
    assert EM.decide(game, 15, key, rows) == (5, [0, 255, 255])          # card 0 alone is discardable, and enough
    rows[4, 54] = 1.0
    assert EM.decide(game, 15, key, rows) == (4, [32, 255, 255])         # the fallback's ties go to the lowest card


def test_ties_nan_and_infinities():
    assert EM.clean(NAN) == -INF and EM.clean(-INF) == -INF and EM.clean(INF) == INF and EM.clean(-0.0) == 0.0
    rows = np.zeros((6, 64))
    assert EM.choice_of(rows, 6) == 0
    rows[:, 54] = [1, 3, 3, 2, 3, 9]
    assert EM.choice_of(rows, 6) == 5 and EM.choice_of(rows, 3) == 1 and EM.choice_of(rows, 2) == 1      # (rows beyond ngroups do not count)
    rows[:, 54] = [NAN, -INF, NAN, -INF, NAN, NAN]
    assert EM.choice_of(rows, 6) == 0                                     # NaN is -inf: a tie at the bottom
    rows[:, 54] = [NAN, -5, INF, INF, NAN, NAN]
    assert EM.choice_of(rows, 6) == 2 and EM.choice_of(rows, 2) == 1
    row = np.zeros(64)
    cand = EM.mask_of([3, 5, 9, 20, 41])
    assert EM.select(row, cand, 3) == [3, 5, 9]
    row[[3, 5, 9, 20, 41]] = [NAN, 2, 2, -INF, INF]
    assert EM.select(row, cand, 3) == [41, 5, 9] and EM.select(row, cand, 1) == [41]
    row[[5, 9, 41]] = NAN
    assert EM.select(row, cand, 3) == [3, 5, 9]                           # all -inf: by card number
    row[2] = 100.0
    assert EM.select(row, cand, 2) == [3, 5]                              # a card outside the candidates never goes


def test_the_three_output_cases():
    hand, talon = list(range(12)), [40, 41, 42, 43, 44, 45]
    key = S.game_key(5, 6, 7)
    rows = np.zeros((8, 64))
    rows[1, 54] = 1.0
    game = O.Game(deal_with(hand, 2, talon), 4, 2, -1)
    assert EM.decide(game, 4, key, rows) == (1, [0, 1, 2])
    bot = XM.padded(S.bot_discards(key, EM.mask_of(hand + talon[:3]), 3))
    assert EM.decide(game, 11, key, rows) == (0, bot) and len(set(bot)) == 3
    klop = O.Game(deal_with(hand, 0, talon), 0, 0, -1)
    assert EM.decide(klop, 15, key, rows) == (-1, [255, 255, 255])
    done = O.Game(deal_with(hand, 2, talon), 4, 2, -1)
    assert done.exchange(0, [0, 1, 2]) == 0 and EM.decide(done, 15, key, rows) == (-1, [255, 255, 255])


@pytest.fixture(scope="module")
def batch():
    """64 synthetic games waiting (or not) for the exchange: feature words, made-up sums and the model's candidates."""
    import torch
    n, sets, seed, episode = 64, 4, 7, 2
    games = [XM.deferred_game(seed, g, episode, S.MIX_ALL) for g in range(n)]
    words = np.array([EM.game_words(g, XM.takes_part(g, 15)) for g in games], np.uint64)
    cands = np.array([EM.candidates(g.lanes(), episode, seed, 0, i, 15, sets) for i, g in enumerate(games)], np.uint8)
    rng = np.random.default_rng(3)
    sums = rng.integers(-16 * 150, 16 * 150, (n, 6 * sets, 4)).astype(np.int32)
    assert 10 < (words[:, 0, 0] != 0).sum() < n
    return torch.from_numpy(words.view(np.int64)), torch.from_numpy(sums), torch.from_numpy(cands), 16


def test_the_learners_targets_and_loss_equal_the_numpy_statement(batch):
    import torch
    from tarok_amd import exchange as X
    fw, sums, cands, playouts = batch
    lr = X.ExchangeLearner(None, seed=3)
    want = EM.targets(fw.numpy().view(np.uint64), sums.numpy(), cands.numpy(), playouts, 1.0 / 70.0)
    got = X.exchange_targets(fw, sums, cands, playouts, 1.0 / 70.0)
    assert (got[0].numpy() == want[0]).all() and (got[3].numpy() == want[3]).all()
    assert np.abs(got[1].numpy() - want[1]).max() < 1e-5 and np.abs(got[2].numpy() - want[2]).max() < 1e-5
    live, known = want[0], want[3]
    assert known.sum() > live.sum() and (known.sum(axis=2)[live] >= 1).all() and not known[~live].any()
    with torch.no_grad():
        out = lr.outputs(fw)
    assert tuple(out.shape) == (64, 6, 64)
    x = EM.expand(fw.numpy().view(np.uint64)[:, :6].reshape(-1, 4))
    assert (X.TarokVecEnv.expand_feature_words(fw[:, :6].reshape(-1, 4), torch.float64).numpy() == x).all()
    loss = float(lr.loss(fw, sums, cands, playouts).detach())
    ref = EM.loss(out.numpy(), *want)
    assert abs(loss - ref) <= 1e-5 * max(1.0, abs(ref)), (loss, ref)
    d = out.numpy()[..., 54][live] - want[1][live]
    assert (np.abs(d) > 1).any() and (np.abs(d) < 1).any()              # both branches of the Huber loss
    # no gradient into an unknown entry: not through the outputs ...
    o = out.clone().requires_grad_(True)
    X.exchange_loss(o, *got).backward()
    g = o.grad.numpy()
    assert (g[..., 55:] == 0).all() and (g[..., 54][~live] == 0).all() and (g[..., :54][~known] == 0).all()
    assert (g[..., 54][live] != 0).all() and (g[..., :54][known] != 0).mean() > 0.99
    # ... and not through the targets: other sums in the rows the contract does not have, the same loss
    other = sums.clone().view(64, 6, 4, 4)
    other[~torch.from_numpy(live)] += 999
    assert float(lr.loss(fw, other.view(64, 24, 4), cands, playouts).detach()) == loss
    # a batch without a waiting game has no loss and no NaN
    none = torch.zeros_like(fw)
    assert float(lr.loss(none, sums, cands, playouts).detach()) == 0.0


def test_twenty_adam_steps_lower_the_loss_of_a_fixed_batch(batch):
    from tarok_amd import exchange as X
    lr = X.ExchangeLearner(None, seed=1, lr=1e-3)
    first = float(lr.loss(*batch).detach())
    seen = [lr.step(*batch) for _ in range(20)]
    last = float(lr.loss(*batch).detach())
    assert seen[0] == pytest.approx(first) and last < first, (first, last)
    a, b = X.ExchangeLearner(None, seed=5), X.ExchangeLearner(None, seed=5)      # the initial weights follow the seed
    assert all((p == q).all() for p, q in zip(a.net.parameters(), b.net.parameters()))
    w = a.weights()
    assert [tuple(t.shape) for t in w] == [(256, 256), (256,), (256, 256), (256,), (64, 256), (64,)]
    X.TarokVecEnv.check_mlp_weights(w)
    with pytest.raises(ValueError):
        X.ExchangeLearner(None, reward_scale=0.0)


def test_argument_checks_without_a_gpu():
    """TAROK_EINVAL before any HIP call: a NULL env never reaches the device, and the other checks come before the env
    is touched — a fake, never dereferenced handle shows them.  All outputs NULL: TAROK_OK, nothing launched."""
    from tarok_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import tarok_amd
        tarok_amd.build()
    L = C.CDLL(_native.LIB_PATH)
    vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
    L.tarok_exchange_values.restype = i32
    L.tarok_exchange_values.argtypes = [vp] + [vp] * 6 + [i32] + [vp] * 6
    L.tarok_exchange_candidates.restype = i32
    L.tarok_exchange_candidates.argtypes = [vp, i32, u64, i32, vp, vp, vp]
    fake = (C.c_char * 4096)()
    h, w = C.cast(fake, vp), C.cast(fake, vp)
    out = (C.c_int8 * 64)()
    call = lambda env=h, ws=(w,) * 6, seats=15, outs=(None, out, None, None): L.tarok_exchange_values(env, *ws, seats, None, *outs, None)
    assert call(env=None) == -1
    for k in range(6):
        assert call(ws=tuple(None if j == k else w for j in range(6))) == -1
    for seats in (-1, 16):
        assert call(seats=seats) == -1
    assert call(outs=(None, None, None, None)) == 0
    cand = lambda env=h, sets=4, seats=15, o=out: L.tarok_exchange_candidates(env, sets, 0, seats, None, o, None)
    assert cand(env=None) == -1
    for sets in (0, -1, 9):
        assert cand(sets=sets) == -1
    for seats in (-1, 16):
        assert cand(seats=seats) == -1
    assert cand(o=None) == 0
