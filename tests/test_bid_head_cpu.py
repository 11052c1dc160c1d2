"""CPU: the definition of the bidding head as tests/bid_head_model.py states it — the feature words on hand-made hands,
the zeros rule against the playout teacher's model, the scaling — and the learner's loss and update
(tarok_amd.bidding.BidLearner on CPU tensors) and the argument checks of tarok_bid_values.  No GPU involved."""
import ctypes as C
import os

import numpy as np
import pytest

import bid_head_model as HM
import playout_bids_model as BM
from tarok_amd import karte as K

TAROKS = list(range(32, 54))
SUIT = lambda k: list(range(8 * k, 8 * k + 8))


def bits(word, lo, n):
    return (word >> lo) & ((1 << n) - 1)


def test_hand_made_hands():
    # no taroks: 8 + 4 suit cards, kings of suits 0 only
    w = HM.feature_words(SUIT(0) + SUIT(1)[:4], 2)
    assert w[0] == sum(1 << c for c in SUIT(0) + SUIT(1)[:4]) | (1 << 56)
    assert bits(w[1], 0, 16) == 0
    assert [bits(w[1], 16 + 8 * k, 8) for k in range(4)] == [0xFF, 0x0F, 0, 0]
    assert bits(w[1], 48, 4) == 0b0001 and bits(w[1], 52, 3) == 0
    # twelve taroks without the trula's ends: 2..13
    w = HM.feature_words(TAROKS[1:13], 0)
    assert bits(w[1], 0, 16) == 0xFFF and bits(w[1], 16, 32) == 0 and bits(w[1], 48, 7) == 0
    # a void suit (suit 2), one card of suit 3, three taroks
    w = HM.feature_words(SUIT(0)[:5] + SUIT(1)[:3] + [24] + TAROKS[3:6], 1)
    assert [bits(w[1], 16 + 8 * k, 8) for k in range(4)] == [0x1F, 0x07, 0, 0x01] and bits(w[1], 0, 12) == 0b111
    # all four kings and the trula
    w = HM.feature_words(HM.KINGS + [K.PAGAT, K.MOND, K.SKIS] + TAROKS[5:10], 3)
    assert bits(w[1], 48, 4) == 0b1111 and bits(w[1], 52, 3) == 0b111 and bits(w[1], 0, 12) == 0xFF
    assert [bits(w[1], 16 + 8 * k, 8) for k in range(4)] == [1, 1, 1, 1]
    for i, c in enumerate((K.PAGAT, K.MOND, K.SKIS)):                   # each of the trula alone
        assert bits(HM.feature_words([c], 0)[1], 52, 3) == 1 << i
    assert HM.KINGS == [7, 15, 23, 31] and (K.PAGAT, K.MOND, K.SKIS) == (32, 52, 53)


def test_each_seat_reserved_words_and_the_layout():
    rng = np.random.default_rng(1)
    for t in range(400):
        perm = rng.permutation(54).tolist()
        for v, w in enumerate(HM.game_words(perm)):
            assert bits(w[0], 54, 10) == 1 << v and bits(w[0], 0, 54) == sum(1 << c for c in perm[12 * v:12 * v + 12])
            assert w[2] == 0 and w[3] == 0
            assert all(w[j] & ~HM.LAYOUT[j] == 0 for j in range(4))
            # thermometers: contiguous from bit 0, and the lengths add up to twelve
            lens = [bin(bits(w[1], 0, 12)).count("1")] + [bin(bits(w[1], 16 + 8 * k, 8)).count("1") for k in range(4)]
            assert sum(lens) == 12
            for f, ln in zip([bits(w[1], 0, 12)] + [bits(w[1], 16 + 8 * k, 8) for k in range(4)], lens):
                assert f == (1 << ln) - 1
    x = HM.expand(np.array(HM.game_words(list(range(54))), np.uint64))
    assert x.shape == (4, 256) and x[:, 128:].sum() == 0 and x[1, 12:24].all() and x[1, 55] == 1 and x[1, 54] == 0
    assert HM.game_words([0] * 54) == [[1 << (54 + v), 0, 0, 0] for v in range(4)]      # an invalid row: the empty hand


def test_the_zeros_rule_is_the_teachers():
    """keep() against what tests/playout_bids_model.py leaves zero, on masks and seat sets: a model run with one world
    and one sample whose playouts are replaced by the constant 1 marks exactly the entries that carry a value."""
    perm = list(range(54))
    real = BM.one_playout
    BM.one_playout = lambda *a: 1
    try:
        for contracts in (BM.DEFAULT_CONTRACTS, BM.ALL_CONTRACTS, 1, 1 << 2, 1 << 7, 1 << 9, 0x155):
            for seats in (0, 1, 6, 8, 15):
                want = BM.playout_bids(perm, 0, 0, 0, 0, seats, 1, 1, contracts) != 0
                assert (HM.keep(seats, contracts) == want).all(), (contracts, seats)
        assert not BM.playout_bids([0] * 54, 0, 0, 0, 0, 15, 1, 1, BM.ALL_CONTRACTS).any() and not HM.keep(15, BM.ALL_CONTRACTS, False).any()
    finally:
        BM.one_playout = real
    assert not HM.keep(15, BM.ALL_CONTRACTS)[:, 19].any() and HM.keep(15, BM.ALL_CONTRACTS)[:, :19].all()


def test_the_scaling_the_clamp_and_the_nan_rule():
    y = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.25, 3.0e-41], np.float32)
    assert HM.values(y, 1.0).tolist() == [0, 2, 2, 0, -2, 2 ** 30, -2 ** 30, 2 ** 30, -2 ** 30, -2 ** 30, 0, 0]
    assert HM.values(np.float32(0.1), 1120.0) == int(np.rint(np.float32(0.1) * np.float32(1120.0)))
    assert HM.values(np.float32(1.0), 2.0 ** 20) == 2 ** 20 and HM.values(np.float32(1025.0), 2.0 ** 20) == 2 ** 30


# ---- the learner on CPU tensors
@pytest.fixture(scope="module")
def batch():
    import torch
    rng = np.random.default_rng(7)
    words = np.array([HM.game_words(rng.permutation(54).tolist()) for _ in range(64)], np.uint64)        # [64, 4, 4]
    sums = rng.integers(-1200, 1200, size=(64, 4, BM.ROWS)).astype(np.int32)
    sums[:, :, 19] = 0
    return torch.from_numpy(words.view(np.int64)), torch.from_numpy(sums)


@pytest.mark.parametrize("contracts", [BM.DEFAULT_CONTRACTS, BM.ALL_CONTRACTS, 0x204])
def test_the_loss_is_the_numpy_statement(batch, contracts):
    import torch
    from tarok_amd import bidding as B
    fw, sums = batch
    lr = B.BidLearner(None, contracts=contracts, seed=3)
    with torch.no_grad():
        out = lr.outputs(fw)
    assert tuple(out.shape) == (256, 64)
    x = HM.expand(fw.numpy().view(np.uint64).reshape(256, 4))
    assert (B.TarokVecEnv.expand_feature_words(fw.reshape(-1, 4), torch.float64).numpy() == x).all()
    want = HM.huber_loss(out.numpy(), sums.numpy().reshape(256, BM.ROWS), 16, 1.0 / 70.0, contracts)
    got = float(lr.loss(fw, sums, 16).detach())
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)
    # both branches of the Huber loss are met, and a masked row has no gradient: not through the outputs ...
    d = out.numpy()[:, :19] - sums.numpy().reshape(256, BM.ROWS)[:, :19] / 16 / 70.0
    assert (np.abs(d) > 1).any() and (np.abs(d) < 1).any()
    o = out.clone().requires_grad_(True)
    B.bid_loss(o, sums.reshape(256, BM.ROWS), 16, 1.0 / 70.0, contracts).backward()
    played = np.array([BM.played(r, contracts) for r in range(19)] + [False] * 45)
    g = o.grad.numpy()
    assert (g[:, ~played] == 0).all() and (g[:, played] != 0).mean() > 0.99
    # ... and not through the targets: other sums in the masked rows, the same loss
    other = sums.clone().reshape(256, BM.ROWS)
    other[:, ~torch.from_numpy(played[:20])] += 999
    assert float(lr.loss(fw, other, 16).detach()) == got


def test_twenty_adam_steps_lower_the_loss_of_a_fixed_batch(batch):
    from tarok_amd import bidding as B
    fw, sums = batch
    lr = B.BidLearner(None, seed=1, lr=1e-3)
    first = float(lr.loss(fw, sums, 16).detach())
    seen = [lr.step(fw, sums, 16) for _ in range(20)]
    last = float(lr.loss(fw, sums, 16).detach())
    assert seen[0] == pytest.approx(first) and last < first, (first, last)
    a, b = B.BidLearner(None, seed=5), B.BidLearner(None, seed=5)         # the initial weights follow the seed
    assert all((p == q).all() for p, q in zip(a.net.parameters(), b.net.parameters()))
    w = a.weights()
    assert [tuple(t.shape) for t in w] == [(256, 256), (256,), (256, 256), (256,), (64, 256), (64,)]
    B.TarokVecEnv.check_mlp_weights(w)
    with pytest.raises(ValueError):
        B.BidLearner(None, playouts_equiv=2 ** 15)                       # 2^15 * 70 exceeds the kernel's scale
    with pytest.raises(ValueError):
        B.BidLearner(None, contracts=0)


def test_argument_checks_without_a_gpu():
    """TAROK_EINVAL before any HIP call: a NULL env never reaches the device, and the other checks come before the env
    is touched — a fake, never dereferenced handle shows them."""
    from tarok_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import tarok_amd
        tarok_amd.build()
    L = C.CDLL(_native.LIB_PATH)
    vp, i32, u32, f32 = C.c_void_p, C.c_int, C.c_uint32, C.c_float
    L.tarok_bid_values.restype = i32
    L.tarok_bid_values.argtypes = [vp, u32, vp] + [vp] * 6 + [f32, i32, i32] + [vp] * 5
    fake = (C.c_char * 4096)()
    h, w = C.cast(fake, vp), C.cast(fake, vp)
    out = (C.c_int32 * 80)()
    call = lambda env=h, ws=(w,) * 6, scale=1.0, contracts=15, seats=15, outs=(out, None, None): L.tarok_bid_values(
        env, 0, None, *ws, scale, contracts, seats, None, *outs, None)
    assert call(env=None) == -1
    for k in range(6):
        assert call(ws=tuple(None if j == k else w for j in range(6))) == -1
    for scale in (0.0, -1.0, float("nan"), float("inf"), float("-inf"), 2.0 ** 20 + 1):
        assert call(scale=scale) == -1
    for contracts in (0, -1, 0x400):
        assert call(contracts=contracts) == -1
    for seats in (-1, 16):
        assert call(seats=seats) == -1
    assert call(outs=(None, None, None)) == -1
