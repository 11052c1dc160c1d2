"""TEST INFRASTRUCTURE — the statement of tarok_bid_values (include/tarok_env.h) and of the bidding head's loss, on the
CPU oracle's deal, numpy and float64 torch.  Nothing here comes from the code under test: the card numbers are the
vocabulary's (tarok_amd/karte.py), the rows are tests/playout_bids_model.py's, the deal is oracle/tarok_spec.py's.

  feature_words(cards, seat)   the 256 input bits of a bidder as four 64-bit words
  forward(x, W, stores)        the 256-256-256-64 network in float64; stores=True writes in the kernel's two bf16
                               activation stores (round-to-nearest-even), as tests/test_gpu_policy_exact.py's reference
  keep(seats, contracts, ok)   which of a game's [4, 20] entries are not tarok_playout_bids' zeros
  values(y, scale)             the float32 scaling, the clamp, the NaN rule and rintf
  forward_bound(x, W)          how far a float32-accumulating, bf16-storing forward may be from forward(stores=False)
  huber_loss(out, sums, ...)   the learner's loss
"""
import numpy as np

import playout_bids_model as BM
from oracle import tarok_spec as S
from tarok_amd import karte as K

ROWS, OPTIONS = BM.ROWS, BM.OPTIONS
CLAMP = 2.0 ** 30
U32, U16 = 2.0 ** -24, 2.0 ** -8          # unit roundoffs of float32 and bf16 (8 significant bits)
KINGS = [K.card_id(s, 8) for s in range(4)]


def feature_words(cards, seat):
    """cards: the card ids of a hand (any iterable; at most twelve taroks count).  Returns four Python ints."""
    cards = sorted(set(int(c) for c in cards))
    assert all(0 <= c < 54 for c in cards) and 0 <= seat < 4
    w0 = sum(1 << c for c in cards) | (1 << (54 + seat))
    taroks = sum(1 for c in cards if c >= 32)
    w1 = 0
    for j in range(12):
        if taroks > j:
            w1 |= 1 << j
    for k in range(4):
        held = sum(1 for c in cards if c // 8 == k)
        for j in range(8):
            if held > j:
                w1 |= 1 << (16 + 8 * k + j)
        if KINGS[k] in cards:
            w1 |= 1 << (48 + k)
    for i, c in enumerate((K.PAGAT, K.MOND, K.SKIS)):
        if c in cards:
            w1 |= 1 << (52 + i)
    return [w0, w1, 0, 0]


LAYOUT = [(1 << 58) - 1, ((1 << 12) - 1) | (((1 << 39) - 1) << 16), 0, 0]     # every bit the layout can set


def hands_of(perm):
    """The four hands of a deal row (54 card ids: 4 x 12, then the talon), or None for a row tarok_reset would flag."""
    if not BM.valid_perm(perm):
        return None
    return [[int(c) for c in perm[12 * v:12 * v + 12]] for v in range(4)]


def game_words(perm):
    """[4][4] feature words of a deal row; an invalid row: the words of the empty hand (the seat bit alone)."""
    hands = hands_of(perm)
    return [feature_words(hands[v] if hands else [], v) for v in range(4)]


def own_deal(seed, gidx, episode):
    return S.deal(S.game_key(seed, gidx, episode))


def expand(words):
    """uint64 [..., 4] -> float64 0/1 [..., 256]: feature f = bit f % 64 of word f / 64."""
    w = np.asarray(words, np.uint64)
    bits = (w[..., :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(w.shape[:-1] + (256,)).astype(np.float64)


def forward(x, W, stores=True):
    """x [n, 256] float64 numpy, W = (W1, b1, W2, b2, W3, b3) float64 torch tensors ([out, in] weights).  Returns y [n, 64]
    float64 numpy and the hidden layers (h1, h2) as stored."""
    import torch
    W1, b1, W2, b2, W3, b3 = W
    bf = (lambda t: t.to(torch.bfloat16).double()) if stores else (lambda t: t)
    x = torch.from_numpy(np.ascontiguousarray(x, np.float64))
    h1 = bf(torch.relu(x @ W1.T + b1))
    h2 = bf(torch.relu(h1 @ W2.T + b2))
    return (h2 @ W3.T + b3).numpy(), (h1.numpy(), h2.numpy())


def forward_bound(x, W):
    """A bound on |kernel output - forward(x, W, stores=False)| per entry [n, 64], for bf16-exact weights, 0/1 inputs and a
    kernel that (a) forms every product exactly (bf16 x bf16 fits float32), (b) sums a layer's 256 products and the bias
    in float32 in SOME order and grouping — every such sum s of terms t_i obeys |fl(s) - s| <= g sum |t_i| with
    g = 257 u32 / (1 - 257 u32), and the factor 2 below leaves room for the matrix unit's internal alignment of a group
    of products — and (c) stores h1 and h2 as bf16, relative error u16 = 2^-8.  ReLU does not stretch an error.
      e1 = a1 (1 + u16) + u16 h1,                a1 = 2 g (|x| |W1|^T + |b1|)
      e2 = (|W2| e1 + a2) (1 + u16) + u16 h2,    a2 = 2 g (|W2| (h1 + e1) + |b2|)
      e3 = |W3| e2 + a3,                         a3 = 2 g (|W3| (h2 + e2) + |b3|)
    with h1, h2 the unrounded float64 layers."""
    import torch
    W1, b1, W2, b2, W3, b3 = [t.abs() for t in W]
    _, (h1, h2) = forward(x, W, stores=False)
    h1, h2 = torch.from_numpy(h1), torch.from_numpy(h2)
    x = torch.from_numpy(np.ascontiguousarray(x, np.float64)).abs()
    g = 2 * 257 * U32 / (1 - 257 * U32)
    a1 = g * (x @ W1.T + b1)
    e1 = a1 * (1 + U16) + U16 * h1
    a2 = g * ((h1 + e1) @ W2.T + b2)
    e2 = (e1 @ W2.T + a2) * (1 + U16) + U16 * h2
    a3 = g * ((h2 + e2) @ W3.T + b3)
    return (e2 @ W3.T + a3).numpy()


def keep(seats, contracts, valid=True):
    """[4, ROWS] bool: the entries that carry a value; the others are zero."""
    m = np.zeros((4, ROWS), bool)
    if valid:
        for v in range(4):
            if (int(seats) >> v) & 1:
                for r in range(OPTIONS):
                    m[v, r] = BM.played(r, contracts)
    return m


def values(y, scale):
    """(int32) rintf(fminf(fmaxf(y * scale, -2^30), 2^30)) with the product in float32; a NaN becomes -2^30."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(y, np.float32) * np.float32(scale)
    p = np.where(np.isnan(p), np.float32(-CLAMP), p)
    return np.rint(np.clip(p, np.float32(-CLAMP), np.float32(CLAMP))).astype(np.int64).astype(np.int32)


def bid_values(perms, W, scale, contracts, seats_of):
    """The launch on deal rows `perms`: (value [n, 4, ROWS] int32, raw [n, 4, ROWS] float32, words [n, 4, 4] uint64) with
    the network in float64 and both bf16 stores written in — the kernel's numbers to the bit whenever W's sums are exact
    in float32 in any order."""
    n = len(perms)
    words = np.array([game_words(p) for p in perms], np.uint64)
    y, _ = forward(expand(words.reshape(n * 4, 4)), W, stores=True)
    y = y.reshape(n, 4, 64)[:, :, :ROWS]
    m = np.stack([keep(seats_of[g], contracts, BM.valid_perm(perms[g])) for g in range(n)])
    raw = np.where(m, y.astype(np.float32), np.float32(0))
    return np.where(m, values(y.astype(np.float32), scale), 0).astype(np.int32), raw, words


def huber_loss(out, sums, playouts, reward_scale, contracts):
    """out [M, >= 19] float, sums [M, ROWS] int: mean over the entries (m, r), r a row of `contracts`, of
    h(out - sums / playouts * reward_scale), h(d) = d^2 / 2 for |d| <= 1, |d| - 1/2 beyond."""
    rows = [r for r in range(OPTIONS) if BM.played(r, contracts)]
    d = np.asarray(out, np.float64)[:, rows] - np.asarray(sums, np.float64)[:, rows] / playouts * reward_scale
    a = np.abs(d)
    return float(np.where(a <= 1, 0.5 * d * d, a - 0.5).mean())


def replay_pass(seed, gidx, episode, seats, W, scale, playouts_equiv, contracts=BM.DEFAULT_CONTRACTS, threshold=0):
    """One game of one pass of evaluate_bidnet_vs_bot on the oracle: the device's own deal, the head's values on `seats`,
    the model's bidding round on them, the Bot's exchange, then every card by the Bot.
    Returns (values [4, ROWS], contract, declarer, king, actions [48] — 255 once the game is over —, final scores [4])."""
    from oracle import oracle as O
    key = S.game_key(seed, gidx, episode)
    perm = S.deal(key)
    vals = bid_values([perm], W, scale, contracts, [seats])[0][0]
    contract, declarer, king = BM.bid_round(key, vals, playouts_equiv, threshold, contracts, seats)
    g = BM.game_of(perm, contract, declarer, king, key)
    actions = [BM.PAD] * 48
    for t in range(48):
        if g.done:
            break
        actions[t] = O.policy_action(key, t, g.legal())
        assert g.step(actions[t]) >= 0
    assert g.done
    return vals, contract, declarer, king, actions, g.scores
