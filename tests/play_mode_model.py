"""TEST INFRASTRUCTURE — the play mode of the policy launches (include/tarok_env.h, tarok_set_play_mode) stated in numpy
float64: which card a game plays under (temperature, epsilon) and with what log-probability.

The three draws are oracle/tarok_spec.py's: the inverse-CDF draw 192 + cards played, the exploration coin 256 + cards
played, and the Bot's card (draw 128 + cards played: pick among the legal cards, kth_bit).  Nothing of the code under
test is used.  No GPU in here.
"""
import numpy as np

from oracle import tarok_spec as S
from policy_exact_ref import U, legal_matrix

DRAW_BOT, DRAW_SAMPLE, DRAW_EXPLORE = S.DRAW_POLICY, 192, 256


def keys_of(seed, first_game, episodes):
    return [S.game_key(seed, first_game + i, int(ep)) for i, ep in enumerate(episodes)]


def threshold(epsilon):
    return int(np.floor(float(epsilon) * 2.0 ** 24))


def bot_cards(masks, played, keys):
    return np.array([S.kth_bit(int(m), S.pick(S.rng32(k, DRAW_BOT + int(p)), bin(int(m)).count("1")))
                     for m, p, k in zip(masks, played, keys)], np.int64)


def play_mode(logits, masks, played, keys, temperature, epsilon):
    """logits [n, >= 54] float32 values (the numbers the sampler reads), masks [n] legal cards (none empty), played [n]
    cards played so far, keys [n] the games' draw keys.  Returns a dict of [n] arrays:
      card      the card the mode plays           logp     log((1 - e) p_T(card) + e / k), e = thr / 2^24
      explored  the coin sent the game to the Bot's card     bot   that card (computed for every row)
      plain     the card without exploration (the inverse-CDF draw, or the arg-max at temperature 0)
      margin    distance of the draw from the nearest CDF edge between two legal cards, relative to the sum (inf at
                temperature 0 and for a single legal card): a float32 sampler may answer differently only below its
                rounding margin
      tol       the bound on |logp - this| for a float32 kernel (derived in tests/test_gpu_play_mode.py)"""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32
    masks = np.asarray(masks, np.uint64)
    n = len(masks)
    rows = np.arange(n)
    legal = legal_matrix(masks)
    assert legal.any(1).all()
    k = legal.sum(1)
    l = np.where(legal, logits[:, :54].astype(np.float64), -np.inf)
    mx = l.max(1, keepdims=True)
    last = 53 - np.argmax(legal[:, ::-1], 1)
    if temperature == 0:
        plain = np.argmax(legal & (l == mx), 1)                            # the lowest-numbered legal card at the maximum
        p = np.zeros((n, 54)); p[rows, plain] = 1.0
        margin = np.full(n, np.inf)
        t = np.zeros((n, 54))
    else:
        inv_t = float(np.float32(1.0) / np.float32(temperature))           # the float32 the host passes to the kernel
        t = np.where(legal, (l - mx) * inv_t, 0.0)
        e = np.where(legal, np.exp(t), 0.0)
        cdf = np.cumsum(e, 1)
        tot = cdf[:, -1:]
        r = np.array([S.rng32(key, DRAW_SAMPLE + int(q)) for key, q in zip(keys, played)], np.uint64)
        u = ((r >> np.uint64(8)).astype(np.float64) + 0.5) / 2.0 ** 24
        take = legal & (cdf > u[:, None] * tot)
        plain = np.where(take.any(1), np.argmax(take, 1), last)
        inner = legal & (np.arange(54)[None, :] != last[:, None])
        margin = np.where(inner, np.abs(cdf / tot - u[:, None]), np.inf).min(1)
        p = e / tot
    thr = threshold(epsilon)
    eps = thr / 2.0 ** 24
    bot = bot_cards(masks, played, keys)
    explored = np.zeros(n, bool)
    if thr > 0:
        coin = np.array([S.rng32(key, DRAW_EXPLORE + int(q)) >> 8 for key, q in zip(keys, played)], np.int64)
        explored = coin < thr
    card = np.where(explored, bot, plain)
    with np.errstate(divide="ignore"):
        logp = np.log((1.0 - eps) * p[rows, card] + eps / k)
    absd = np.abs(t)
    tol = U * (18 + 4 * (absd[rows, card] + (p * absd).sum(1)) + 4 * np.abs(logp)) + 1e-9
    return dict(card=card, logp=logp, explored=explored, bot=bot, plain=plain, margin=margin, tol=tol, k=k, legal=legal)
