"""TEST INFRASTRUCTURE — the playout teacher's target rows (tarok_playout_targets) and the distillation term of the fused
learner (tarok_learn_chain_distill) as float64 numpy statements written from the definitions in include/tarok_env.h, and
the bounds a float32 evaluation with a bf16 output has to meet.  Nothing here comes from the kernels; no bound is fitted to
what a kernel returns.

Target row of a game with a teacher (legal != 0 and the seat to move in the game's seat set), nl = min(popcount(legal), 12):
    z_j = (sum[j][s] - max_k sum[k][s]) / (playouts tau),  q = softmax(z) at the j-th lowest legal card, 0 elsewhere;
    tau = 0: 1 at the card of the smallest rank at the maximum.  A game without a teacher: 64 zeros.
Distillation term of a sample with target row q (columns of illegal cards and 54..63 dropped), weight w:
    S = sum_c q_c,  ce = -sum_c q_c log p_c,  d ce / d logit_c = S p_c - q_c on the legal cards.
"""
import numpy as np

RANKS = 12


def cards_of(mask):
    return [c for c in range(54) if (int(mask) >> c) & 1]


def targets_reference(sums, words, playouts, tau, sets):
    """sums [N,12,4] int, words [N] observation words (any integer dtype), sets [N] (or one) 4-bit seat sets.
    Returns (q [N,64] float64, has [N] bool, card [N]: the one-hot card at tau = 0 / the playout launch's card, 255
    without a teacher)."""
    sums = np.asarray(sums).astype(np.int64)
    n = sums.shape[0]
    words = [int(w) & ((1 << 64) - 1) for w in np.asarray(words).reshape(-1).tolist()]
    sets = np.broadcast_to(np.asarray(sets), (n,))
    q = np.zeros((n, 64), np.float64)
    has = np.zeros(n, bool)
    card = np.full(n, 255, np.int64)
    for g in range(n):
        legal, s = words[g] & ((1 << 54) - 1), (words[g] >> 54) & 3
        if legal == 0 or not (int(sets[g]) >> s) & 1:
            continue
        has[g] = True
        cards = cards_of(legal)[:RANKS]
        v = sums[g, :len(cards), s]
        best = int(np.argmax(v))                        # (the first maximum)
        card[g] = cards[best]
        if tau == 0:
            q[g, cards[best]] = 1.0
        else:
            e = np.exp((v - v.max()).astype(np.float64) / (float(playouts) * float(tau)))
            q[g, cards] = e / e.sum()
    return q, has, card


def target_bound(q):
    """|kernel - q| per element for one bf16 rounding of a float32 softmax: 2^-8 q is the store (round to nearest even, 8
    significant bits).  The float32 part: sum - max is an exact integer, its conversion and the division round once each
    (2^-23 |z| in all); an exponential that does not underflow has |z| < 104, so its argument is off by less than 2^-16 and
    its value, with expf's own ulp or two, by less than 2^-15 relative; the sum of at most twelve such terms and the final
    division keep that: 2^-14 with a margin of 2.  The floor 2^-120 covers values at the edge of underflow (flushed or
    denormal: both are 0 within it).  Exactly 0 where q is 0 by definition."""
    q = np.asarray(q, np.float64)
    return np.where(q > 0, q * (2.0 ** -8 + 2.0 ** -14) + 2.0 ** -120, 0.0)


def distill_reference(ref, q):
    """Extends a loss_model.loss_reference dict (a copy) with S [n], ce [n] and d_distill [n,64] (per unit weight, per unit
    coefficient) for target rows q [n,64]: columns of illegal cards and 54..63 are not looked at (NaN allowed there)."""
    q = np.asarray(q, np.float64)
    legal, has = ref["legal"], ref["has"]
    assert q.shape == (ref["n"], 64)
    qs = np.where(legal & has[:, None], q[:, :54], 0.0)
    assert np.isfinite(qs).all()
    S = qs.sum(1)
    ce = -(qs * ref["logp_all"]).sum(1)
    d = np.zeros((ref["n"], 64))
    d[:, :54] = np.where(legal & has[:, None], S[:, None] * ref["p"] - qs, 0.0)
    out = dict(ref)
    out.update(q=qs, S=S, ce=ce, d_distill=d)
    return out


def distill_gradient(dref, coef):
    """d (pi + vf value - ent H + coef ce) / d out per unit weight, [n,64]."""
    import loss_model as L
    return L.loss_gradient(dref) + coef * dref["d_distill"]


def distill_bound(dref, part, scale, coef):
    """loss_model.loss_bound of the whole gradient `part` plus the floor of the new term on the legal columns:
    2^-15 scale_i |coef| S_i.  S p - q inherits p's 2^-17 relative error (loss_bound's derivation: __expf) on S p <= S; S
    itself is a float32 sum of at most 54 bf16 numbers (54 x 2^-24 relative) and the product, the difference and the
    add into the row round at 2^-23 (S + q): together below 2^-16 S, taken with a margin of 2.  The store's 2^-8 |want|
    is loss_bound's, on the whole gradient."""
    import loss_model as L
    scale = np.asarray(scale, np.float64)
    b = L.loss_bound(dref, part, scale)
    extra = 2.0 ** -15 * scale * abs(coef) * dref["S"]
    b[:, :54] += np.where(dref["legal"] & dref["has"][:, None], extra[:, None], 0.0)
    return b


def distill_means(dref):
    """{weighted mean of ce, weighted mean of S} and the divisor max(sum w, 1)."""
    w = dref["w"]
    wsum = max(float(w.sum()), 1.0)
    return np.array([(w * dref["ce"]).sum() / wsum, (w * dref["S"]).sum() / wsum]), wsum


def distill_means_bound(dref):
    """ce: log p is off by about 2^-18 absolute (loss_model.terms_bound), so a sample's ce by 2^-18 S, and its float32 sum
    of at most 54 products by 54 x 2^-24 sum q |log p| < 2^-18 |ce|... taken as 2^-17 (S + |ce|) per sample; the block sums
    (a butterfly and four waves in float32, the blocks in double) add 10 x 2^-24 relative.  S: exact products, the same
    sums: 2^-17 S is generous.  Floor 2^-23 as in terms_bound."""
    w = dref["w"]
    wsum = max(float(w.sum()), 1.0)
    return np.array([2.0 ** -17 * (w * (dref["S"] + np.abs(dref["ce"]))).sum() / wsum + 2.0 ** -23,
                     2.0 ** -17 * (w * dref["S"]).sum() / wsum + 2.0 ** -23])


# ---- target rows for hand-made samples (tests/loss_model.build_cases)
def bf16_round(x):
    """float64 array -> the nearest bf16 (ties to even) as float64, through torch's conversion."""
    import torch
    return torch.from_numpy(np.asarray(x, np.float64)).to(torch.float32).to(torch.bfloat16).double().numpy()


def target_rows(legal, kind, seed=0):
    """[n,64] float64 rows that are bf16 numbers: 'onehot' (the (i mod count)-th legal card of sample i: every legal card in
    turn over the set), 'uniform' (bf16(1 / count) on the legal cards), 'random' (a bf16-rounded softmax of random scores),
    'zero'."""
    legal = np.asarray(legal, bool)
    n = legal.shape[0]
    q = np.zeros((n, 64))
    rnd = np.random.RandomState(seed)
    for i in range(n):
        cards = np.flatnonzero(legal[i])
        if len(cards) == 0 or kind == "zero":
            continue
        if kind == "onehot":
            q[i, cards[i % len(cards)]] = 1.0
        elif kind == "uniform":
            q[i, cards] = 1.0 / len(cards)
        else:
            x = rnd.randn(len(cards)) * 2.0
            e = np.exp(x - x.max())
            q[i, cards] = e / e.sum()
    return bf16_round(q)


def target_rows_random(legal, seed=0):
    """target_rows(legal, 'random', seed) for sets of 10^5 rows and more, without the loop over the rows: the same draws (one
    RandomState stream consumed row by row over the legal cards in ascending order, which is the row-major order of the
    matrix) and the same softmax, over the whole matrix at once.  tests/test_distill_cpu.py holds the two equal."""
    legal = np.asarray(legal, bool)
    x = np.full(legal.shape, -np.inf)
    x[legal] = np.random.RandomState(seed).randn(int(legal.sum())) * 2.0
    has = legal.any(1)
    e = np.where(legal, np.exp(x - np.where(has, x.max(1), 0.0)[:, None]), 0.0)
    q = np.zeros((legal.shape[0], 64))
    q[:, :54] = e / np.where(has, e.sum(1), 1.0)[:, None]
    return bf16_round(q)


def with_nans(q, legal):
    """The rows with NaN in every column the term must not look at: illegal cards and 54..63."""
    out = np.array(q, np.float64)
    out[:, :54] = np.where(np.asarray(legal, bool), out[:, :54], np.nan)
    out[:, 54:] = np.nan
    return out
