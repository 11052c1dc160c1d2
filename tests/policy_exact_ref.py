"""TEST INFRASTRUCTURE — the exact probes of the policy forward and its sampler: the exactly summable weight sets R and P, the
float64 reference forward, the conditions under which it is exact, the sampler's reference and small word helpers.
tests/test_gpu_policy_exact.py checks the kernels against these; other test modules take the weight sets and the
references from here.  No GPU is needed to import or to run anything but kernel_weights."""
import numpy as np


U = 2.0 ** -24                      # unit roundoff of float32 (half an ulp, relative)
NS = (1, 128, 129, 333)             # k_policy_mlp: 128 games per workgroup; 333 = two full groups and a ragged one of 77
LEADS = (0, 1, 2, 3, 5, 14, 31, 46)  # random lock-steps played before each position (trick positions 0-3, first to last trick)
SEED = 29
# (s, a, c) of the sets P: W1[o][(o + s) % 256] = 1, W2[o][(a o + c) % 256] = 1
P_PARAMS = ((0, 1, 0), (32, 3, 32), (64, 5, 7), (96, 7, 64), (128, 9, 96), (160, 11, 128), (192, 13, 160), (224, 15, 224),
            (13, 255, 5))


# ---- weight sets (float64 tensors of exactly representable values, on the CPU) and the exact reference
def weights_r(seed=1):
    """Set R: W1 in {-3..3}, b1 in {-2..6}, W2 in {-4..4}, b2 in {-8..8} (+ 0.5 on every second unit), W3 in {-4..4} 2^-13,
    b3 in {-8..8} / 8: all exact in bf16 (the biases are float32 anyway)."""
    import torch
    g = torch.Generator(); g.manual_seed(seed)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).double()
    half = 0.5 * (torch.arange(256) % 2).double()
    return [ri(-3, 3, 256, 256), ri(-2, 6, 256), ri(-4, 4, 256, 256), ri(-8, 8, 256) + half,
            ri(-4, 4, 64, 256) * 2.0 ** -13, ri(-8, 8, 64) / 8]


def weights_p(s, a, c, seed=2):
    """A set P: permutation matrices in layers 1 and 2 (H1[o] = x[(o + s) % 256], H2[o] = H1[(a o + c) % 256], a odd), no
    hidden biases, W3 in {-3..3} / 8, b3 in {-4..4} / 8."""
    import torch
    assert a % 2 == 1, "not true: a % 2 == 1"
    g = torch.Generator(); g.manual_seed(seed + 1000 * s + a)
    o = torch.arange(256)
    W1, W2 = torch.zeros(256, 256, dtype=torch.float64), torch.zeros(256, 256, dtype=torch.float64)
    W1[o, (o + s) % 256] = 1
    W2[o, (a * o + c) % 256] = 1
    zero = torch.zeros(256, dtype=torch.float64)
    return [W1, zero, W2, zero.clone(), torch.randint(-3, 4, (64, 256), generator=g).double() / 8,
            torch.randint(-4, 5, (64,), generator=g).double() / 8]


def fragment_slots(W):
    """{(feature tile, k-step, half)} of the fragment order ([out / 32][16 k-steps][2 halves][32 rows][8]) that hold a
    non-zero of W."""
    o, k = np.nonzero(W.numpy())
    return set(zip((o >> 5).tolist(), (k >> 4).tolist(), ((k >> 3) & 1).tolist()))


def reference(x, W):
    """float64 forward of features x [n, 256] with the kernels' two bf16 stores written in: dict of z1, h1, z2, h2, out
    ([n, 64]: card logits 0..53, value 54)."""
    import torch
    W1, b1, W2, b2, W3, b3 = W
    bf = lambda t: t.to(torch.bfloat16).double()
    z1 = x @ W1.T + b1
    h1 = bf(torch.relu(z1))
    z2 = h1 @ W2.T + b2
    h2 = bf(torch.relu(z2))
    return dict(x=x, z1=z1, h1=h1, z2=z2, h2=h2, out=h2 @ W3.T + b3)


def _quantum(t):
    """The largest power of two, at most 1, that every entry of t is a multiple of."""
    q = 1.0
    for _ in range(60):
        if bool(((t / q) == (t / q).round()).all()):
            return q
        q /= 2
    raise AssertionError("no power-of-two quantum")


def exactness(r, W):
    """The conditions under which float32 accumulation of reference r is exact in any order: per layer, the sum of the
    magnitudes (bias included) in units of the layer's quantum — it has to stay below 2^24.  Returns the three maxima."""
    W1, b1, W2, b2, W3, b3 = W
    out = []
    for x, Wl, b in ((r["x"], W1, b1), (r["h1"], W2, b2), (r["h2"], W3, b3)):
        q = min(_quantum(x) * _quantum(Wl), _quantum(b))                  # (powers of two: the smaller divides the other)
        out.append(float(((x.abs() @ Wl.abs().T + b.abs()) / q).max()))
    return out


def h2_rounding(r):
    """(share of H2 entries the bf16 store changes, share that are exact ties between two bf16 neighbours)."""
    import torch
    v = torch.relu(r["z2"])
    assert torch.equal(v.float().double(), v), "not true: torch.equal(v.float().double(), v)"  # exact in float32: its low 16 bits say what the store does
    low = v.float().numpy().view(np.uint32) & 0xFFFF
    return float((r["h2"] != v).double().mean()), float((low == 0x8000).mean())


def check_conditions_r(r, W, rounded_min=0.05, ties_min=0.01):
    import torch
    assert max(exactness(r, W)) < 2 ** 24, "not true: max(exactness(r, W)) < 2 ** 24"
    assert torch.equal(r["h1"], torch.relu(r["z1"])), "not true: torch.equal(r[\"h1\"], torch.relu(r[\"z1\"]))"  # |z1| < 256: H1 is stored exactly
    rounded, ties = h2_rounding(r)
    assert rounded >= rounded_min and ties >= ties_min, (rounded, ties)
    assert torch.equal(r["out"].float().double(), r["out"]), "not true: torch.equal(r[\"out\"].float().double(), r[\"out\"])"  # every logit is a float32
    return rounded, ties


def check_conditions_p(r, W):
    import torch
    assert max(exactness(r, W)) < 2 ** 24, "not true: max(exactness(r, W)) < 2 ** 24"
    for k in ("h1", "h2"):
        assert bool(((r[k] == 0) | (r[k] == 1)).all()), "not true: bool(((r[k] == 0) | (r[k] == 1)).all())"
    out = r["out"]
    assert torch.equal(out.to(torch.bfloat16).double(), out) and float(out.abs().max()) < 32, "set P: a logit is not a bf16 value below 32"
    assert torch.equal(out * 8, (out * 8).round()), "not true: torch.equal(out * 8, (out * 8).round())"


def synthetic_features(rows=4096, seed=3):
    """0/1 rows with the real features' sparsity: 8 to 55 ones each."""
    import torch
    g = torch.Generator(); g.manual_seed(seed)
    count = torch.randint(8, 56, (rows, 1), generator=g)
    rank = torch.rand(rows, 256, generator=g).argsort(1).argsort(1)
    return (rank < count).double()


# ---- the float64 statement of the sampler
def legal_matrix(masks):
    return ((np.asarray(masks, np.uint64)[:, None] >> np.arange(54, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def draws(S, seed, first_game, episodes, played):
    """r = rng32(game_key(seed, game, episode), 192 + cards played) of every game."""
    return np.array([S.rng32(S.game_key(seed, first_game + i, int(ep)), 192 + int(p)) for i, (ep, p) in enumerate(zip(episodes, played))],
                    np.uint64)


def sampler_reference(logits, masks, r):
    """Masked inverse-CDF draw in float64 for games WITH a legal card: u = ((r >> 8) + 0.5) / 2^24, the card is the
    first legal c whose CDF exceeds u sum (the last legal card if none does).  Returns dict: card, logp_all [n, 54],
    near (u within 1e-5 of a CDF boundary between two legal cards, relative to the sum: the only games a float32 sampler
    may answer differently) and tol_of(cards), the bound on |logp - float64| derived in test_sampler_against_float64."""
    legal = legal_matrix(masks)
    assert legal.any(1).all(), "not true: legal.any(1).all()"
    l = np.where(legal, np.asarray(logits, np.float64)[:, :54], -np.inf)
    d = l - l.max(1, keepdims=True)
    e = np.where(legal, np.exp(d), 0.0)
    cdf = np.cumsum(e, 1)
    tot = cdf[:, -1:]
    u = ((np.asarray(r, np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) / 2.0 ** 24
    last = 53 - np.argmax(legal[:, ::-1], 1)
    take = legal & (cdf > u[:, None] * tot)
    card = np.where(take.any(1), np.argmax(take, 1), last)
    inner = legal & (np.arange(54)[None, :] != last[:, None])
    near = (inner & (np.abs(cdf / tot - u[:, None]) < 1e-5)).any(1)
    p = e / tot
    logp_all = np.where(legal, d - np.log(tot), -np.inf)
    absd = np.where(legal, np.abs(d), 0.0)
    mean_d = (p * absd).sum(1)

    def tol_of(cards):
        rows = np.arange(len(cards))
        return U * (16 + 3 * (absd[rows, cards] + mean_d) + 4 * np.abs(logp_all[rows, cards])) + 1e-9
    return dict(card=card, logp_all=logp_all, near=near, legal=legal, tol_of=tol_of)


def kernel_weights(T, W, w3_row_to_54=None):
    """Float64 weight set -> what tarok_policy_mlp takes (bf16 fragment order, float32 biases), on the device."""
    import torch
    W1, b1, W2, b2, W3, b3 = W
    if w3_row_to_54 is not None:
        W3 = W3.clone()
        W3[54] = W3[w3_row_to_54]
    order = T.TarokVecEnv.mfma_weight_order
    for t in (W1, W2, W3):
        assert torch.equal(t.to(torch.bfloat16).double(), t), "not true: torch.equal(t.to(torch.bfloat16).double(), t)"
    return [order(W1.cuda()), b1.float().cuda(), order(W2.cuda()), b2.float().cuda(), order(W3.cuda()), b3.float().cuda()]


def _u64(t):
    return t.detach().cpu().numpy().view(np.uint64)


def _played(words):
    return ((words >> np.uint64(56)) & np.uint64(63)).astype(np.int64)


def _zero_net(T, b3):
    """Weights with which every game's logits are b3 (all matrices zero): the sampler of policy_body on hand-built logits."""
    import torch
    z = torch.zeros(256, 256, dtype=torch.float64)
    return kernel_weights(T, [z, torch.zeros(256, dtype=torch.float64), z, torch.zeros(256, dtype=torch.float64),
                              torch.zeros(64, 256, dtype=torch.float64), b3.double()])


def _word(cards, played):
    m = 0
    for c in cards:
        m |= 1 << c
    return m | (played << 56)
