"""TEST INFRASTRUCTURE — the statement of tarok_exchange_values and tarok_exchange_candidates (include/tarok_env.h) and of
the exchange head's targets and loss, on the CPU oracle's game, numpy and float64 torch.  Nothing here comes from the code
under test: the card numbers are the vocabulary's (tarok_amd/karte.py), the game is oracle/oracle.py's, the Bot's discards
and the discardable cards oracle/tarok_spec.py's, the candidate keys tests/playout_exchange_model.py's.

  row_words(game, i, part)       the 256 input bits of row i as four 64-bit words (zeros where the row is not live)
  forward(x, W, stores)          the 256-256-256-64 network in float64 with the kernel's two bf16 stores written in
  forward_bound(x, W)            how far a float32-accumulating, bf16-storing forward may be from forward(stores=False)
  clean, choice_of, select       the NaN rule, the group and the discards from rows of 64 outputs
  decide(game, seats, key, y)    the three output cases for one game
  exchange_values(...)           the launch on canonical lanes
  candidates(...)                tarok_exchange_candidates for one game
  targets, loss                  the learner's two targets and its Huber loss
  replay_pass                    one game of one pass of evaluate_exchangenet_vs_bot
"""
import numpy as np

import playout_exchange_model as XM
from oracle import oracle as O
from oracle import tarok_spec as S
from tarok_amd import karte as K

ROWS, GROUPS, VALUE = 8, 6, 54
NO_CHOICE, PAD = XM.NO_CHOICE, XM.PAD
U32, U16 = 2.0 ** -24, 2.0 ** -8          # unit roundoffs of float32 and bf16 (8 significant bits)
KINGS = [K.card_id(s, 8) for s in range(4)]
TRI, ENA, SOLO_TRI, SOLO_ENA = 1, 3, 4, 6


def mask_of(cards):
    m = 0
    for c in cards:
        m |= 1 << int(c)
    return m


def cards_of(mask):
    return [c for c in range(54) if (int(mask) >> c) & 1]


def shape_word(cards):
    """Thermometers of a card set: bit j < 16 iff more than j taroks, bit 16 + 8k + j iff more than j cards of suit k,
    bit 48 + k the king of suit k, bits 52, 53, 54 pagat, mond, skis."""
    cards = set(int(c) for c in cards)
    taroks = sum(1 for c in cards if c >= 32)
    w = 0
    for j in range(16):
        if taroks > j:
            w |= 1 << j
    for k in range(4):
        held = sum(1 for c in cards if c // 8 == k)
        for j in range(8):
            if held > j:
                w |= 1 << (16 + 8 * k + j)
        if KINGS[k] in cards:
            w |= 1 << (48 + k)
    for i, c in enumerate((K.PAGAT, K.MOND, K.SKIS)):
        if c in cards:
            w |= 1 << (52 + i)
    return w


def ngroups_of(game):
    return 6 // XM.group_size(game)


def row_words(game, i, part=True):
    """The four feature words of row i of `game` (an oracle Game waiting for the exchange); zeros if the game does not
    take part (`part`) or the contract has no group i."""
    if not part or not XM.waiting(game) or i >= ngroups_of(game):
        return [0, 0, 0, 0]
    g = game.g
    gs, d, contract = XM.group_size(game), int(g.declarer), int(g.contract)
    assert TRI <= contract <= SOLO_ENA
    H = int(g.hand[d])
    T = mask_of(g.talon[j] for j in range(6))
    Ti = XM.group_mask(game, i)
    P, R = H | Ti, T & ~Ti
    w0 = P | (1 << (54 + d)) | (1 << (58 + 3 - gs)) | ((1 << 61) if contract >= SOLO_TRI else 0)
    w1 = R | (1 << (58 + i))
    w2 = Ti
    if contract <= ENA:
        k = int(g.king)
        assert 0 <= k < 4
        kb = 1 << KINGS[k]
        w1 |= 1 << (54 + k)
        w2 |= ((1 << 54) if Ti & kb else 0) | ((1 << 55) if H & kb else 0) | ((1 << 56) if R & kb else 0)
    return [w0, w1, w2, shape_word(cards_of(P))]


def game_words(game, part=True):
    return [row_words(game, i, part) for i in range(ROWS)]


def expand(words):
    """uint64 [..., 4] -> float64 0/1 [..., 256]: feature f = bit f % 64 of word f / 64."""
    w = np.asarray(words, np.uint64)
    bits = (w[..., :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(w.shape[:-1] + (256,)).astype(np.float64)


def forward(x, W, stores=True):
    """x [n, 256] float64 numpy, W = (W1, b1, W2, b2, W3, b3) float64 torch tensors ([out, in] weights).  Returns y [n, 64]
    float64 numpy and the hidden layers (h1, h2) as stored: with stores=True each hidden layer is rounded to bf16
    (nearest even) after bias and ReLU, as the kernel stores it."""
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


def clean(y):
    """fmaxf(y, -inf): a NaN becomes -inf."""
    y = float(y)
    return float("-inf") if y != y else y


def choice_of(rows, ngroups):
    """The i < ngroups with the largest clean(rows[i][54]), the lowest i on ties."""
    best = 0
    for i in range(1, ngroups):
        if clean(rows[i][VALUE]) > clean(rows[best][VALUE]):
            best = i
    return best


def select(row, cand, gs):
    """gs times: the card of mask `cand` with the largest clean(row[c]), the lowest card on ties, removed once taken."""
    cand, out = int(cand), []
    for _ in range(gs):
        best = None
        for c in cards_of(cand):
            if best is None or clean(row[c]) > clean(row[best]):
                best = c
        out.append(best)
        cand &= ~(1 << best)
    return out


def candidate_mask(pickup, gs):
    """The Bot's own rule: the discardable cards of what the declarer holds, all of it if those are fewer than gs."""
    cand = int(pickup) & S.DISCARDABLE
    return cand if bin(cand).count("1") >= gs else int(pickup)


def decide(game, seats, key, rows):
    """(choice, discards [3]) of one game: rows [8][64] are the network's outputs of its rows; key the game's own key."""
    if not XM.waiting(game):
        return NO_CHOICE, [PAD] * 3
    if not XM.takes_part(game, seats):
        return 0, XM.padded(XM.discards_under(game, 0, key))
    gs = XM.group_size(game)
    i = choice_of(rows, ngroups_of(game))
    pickup = int(game.g.hand[int(game.g.declarer)]) | XM.group_mask(game, i)
    return i, XM.padded(select(rows[i], candidate_mask(pickup, gs), gs))


def exchange_values(lanes, W, seed, gidx0, episode, seats_of, stores=True):
    """The launch on canonical lanes [n][10]: (raw [n, 8, 64] float32, choice [n] int8, discards [n, 3] uint8, words
    [n, 8, 4] uint64) with the network in float64 and both bf16 stores written in — the kernel's numbers to the bit
    whenever W's sums are exact in float32 in any order."""
    n = len(lanes)
    games = [O.Game.from_lanes(l) for l in lanes]
    words = np.array([game_words(g, XM.takes_part(g, seats_of[j])) for j, g in enumerate(games)], np.uint64)
    y, _ = forward(expand(words.reshape(n * ROWS, 4)), W, stores=stores)
    live = (words[:, :, 0] != 0)
    with np.errstate(over="ignore", invalid="ignore"):
        raw = np.where(live[:, :, None], y.reshape(n, ROWS, 64).astype(np.float32), np.float32(0))
    choice, disc = decisions(games, raw, seed, gidx0, episode, seats_of)
    return raw, choice, disc, words


def decisions(games, raw, seed, gidx0, episode, seats_of):
    """choice [n] int8 and discards [n, 3] uint8 of oracle games given the rows' outputs raw [n, 8, 64]."""
    n = len(games)
    choice, disc = np.zeros(n, np.int8), np.zeros((n, 3), np.uint8)
    for j, g in enumerate(games):
        choice[j], disc[j] = decide(g, seats_of[j], S.game_key(seed, gidx0 + j, episode), raw[j])
    return choice, disc


def candidates(lanes, episode, seed, salt, gidx, seats, sets):
    """cand_out [6 * sets][3] of one game: row i * sets + d the discards of candidate (i, d) under the teacher's ckey."""
    game = O.Game.from_lanes(lanes)
    out = [[PAD] * 3 for _ in range(GROUPS * sets)]
    if XM.takes_part(game, seats):
        for i in range(ngroups_of(game)):
            for d in range(sets):
                out[i * sets + d] = XM.padded(XM.discards_under(game, i, XM.candidate_key(seed, salt, gidx, episode, i, d)))
    return out


def targets(words, sums, cands, playouts, reward_scale):
    """The learner's targets from words [n, 8, 4], sums [n, 6 D, 4], cands [n, 6 D, 3]: (live [n, 6] bool, value [n, 6],
    score [n, 6, 54], known [n, 6, 54] bool) in float64, by loops."""
    n = len(words)
    sets = np.asarray(sums).shape[1] // GROUPS
    live = np.zeros((n, GROUPS), bool)
    value = np.zeros((n, GROUPS))
    score = np.zeros((n, GROUPS, 54))
    known = np.zeros((n, GROUPS, 54), bool)
    for g in range(n):
        for i in range(GROUPS):
            w0 = int(words[g][i][0])
            if not w0:
                continue
            live[g, i] = True
            (declarer,) = [v for v in range(4) if (w0 >> (54 + v)) & 1]
            scaled = [float(sums[g][i * sets + d][declarer]) / playouts * reward_scale for d in range(sets)]
            value[g, i] = sum(scaled) / sets
            for c in range(54):
                with_c = [scaled[d] for d in range(sets) if c in [int(x) for x in cands[g][i * sets + d]]]
                if with_c:
                    known[g, i, c] = True
                    score[g, i, c] = sum(with_c) / len(with_c) - value[g, i]
    return live, value, score, known


def huber(d):
    a = np.abs(d)
    return np.where(a <= 1, 0.5 * d * d, a - 0.5)


def loss(out, live, value, score, known):
    """out [n, 6, 64]: mean Huber (delta 1) of output 54 over the live rows plus that of outputs c < 54 over the known
    entries; a term without entries is 0."""
    out = np.asarray(out, np.float64)
    lv = float(huber(out[..., VALUE][live] - value[live]).mean()) if live.any() else 0.0
    ls = float(huber(out[..., :54][known] - score[known]).mean()) if known.any() else 0.0
    return lv + ls


def replay_pass(seed, mix, gidx, episode, seats, W):
    """One game of one pass of evaluate_exchangenet_vs_bot on the oracle: the deferred game, the head's exchange for a
    declarer in `seats` (the Bot's own elsewhere), then every card by the Bot.
    Returns (choice, discards [3], actions [48] — 255 once the game is over —, final scores [4])."""
    g = XM.deferred_game(seed, gidx, episode, mix)
    _, choice, disc, _ = exchange_values([g.lanes()], W, seed, gidx, episode, [seats])
    choice, disc = int(choice[0]), [int(x) for x in disc[0]]
    if XM.waiting(g):
        assert g.exchange(choice, disc[:XM.group_size(g)]) == 0
    key = S.game_key(seed, gidx, episode)
    actions = [PAD] * 48
    for t in range(48):
        if g.done:
            break
        actions[t] = O.policy_action(key, t, g.legal())
        assert g.step(actions[t]) >= 0
    assert g.done
    return choice, disc, actions, g.scores
