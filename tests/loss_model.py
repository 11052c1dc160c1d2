"""TEST INFRASTRUCTURE — the loss phase of the fused learner (k_learn_chain in tarok_amd/csrc/tarok_learner.inc) and of
tarok_ppo_loss (k_ppo_loss in tarok_amd/csrc/tarok_env.hip) as a float64 numpy statement written out by hand, the
per-element bounds a bf16 output of a float32 evaluation has to meet, and hand-made samples that reach every path of the
loss.  tests/test_loss_model_cpu.py holds the statement against float64 autograd, a float32 restatement against the bounds
and eight mutants of that restatement against the comparator; tests/test_gpu_loss_exact.py holds the kernels.

The loss of one sample with a legal card, played card a, over the legal cards:
    z_c = logit_c - max,  p = softmax(z),  log p_c = z_c - log(sum exp z),  H = -sum p log p
    ratio = exp(log p_a - logp_old),  pi = -min(ratio A, clamp(ratio, 1 - clip, 1 + clip) A),  value = (out_54 - ret)^2
    loss = sum_i w_i (pi_i + vf value_i - ent H_i) / wsum
and its gradient with respect to the 64 outputs, in three additive parts PER UNIT WEIGHT:
    d_policy_c  = g (delta_ca - p_c),  g = d pi / d log p_a = -A ratio where the unclipped branch is active, else 0
    d_entropy_c = d H / d logit_c = -p_c (log p_c + H)
    d_value_54  = 2 (out_54 - ret)
    d loss / d out = scale_i (d_policy + vf d_value - ent d_entropy),  scale_i = w_i (chain) or w_i / wsum (tarok_ppo_loss)
A sample without a legal card has weight 0 and every part 0, as in the kernels.
"""
import numpy as np

MODES = {                      # name: (clip, vf, ent)
    "policy": (0.2, 0.0, 0.0),
    "entropy": (0.2, 0.0, 1.0),
    "value": (0.2, 1.0, 0.0),
    "mixed": (0.2, 0.5, 0.01),
}
Z_MAX = 64.0                   # the bounds are claimed for |logit - row max over the legal cards| <= 64 only


def legal_matrix(masks):
    return ((np.asarray(masks, np.uint64)[:, None] >> np.arange(54, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def loss_reference(logits, legal, act, logp_old, A, ret, w, clip, vf, ent):
    """logits [n,64] f64 (54 = the value), legal [n,54] bool, act [n] int (>= 54 is clamped to 53, as the kernels do: only
    on rows of weight 0), logp_old, A, ret, w [n].  Returns a dict of per-sample pi, v (= (value - ret)^2), H, p [n,54],
    logp_all [n,54] (0 where illegal), ratio, g, value, and d_policy, d_entropy, d_value [n,64]."""
    logits = np.asarray(logits, np.float64)
    legal = np.asarray(legal, bool)
    n = logits.shape[0]
    assert logits.shape == (n, 64) and legal.shape == (n, 54)
    act = np.asarray(act).astype(np.int64)
    act = np.where(act < 54, act, 53)
    logp_old, A, ret, w = (np.asarray(t, np.float64) for t in (logp_old, A, ret, w))
    rows = np.arange(n)
    has = legal.any(1)
    w = np.where(has, w, 0.0)
    assert (w[~legal[rows, act]] == 0).all(), "a weighted sample plays an illegal card"
    l = np.where(legal, logits[:, :54], -np.inf)
    mx = np.where(has, l.max(1, initial=-np.inf), 0.0)
    z = np.where(legal, logits[:, :54] - mx[:, None], 0.0)
    assert np.abs(z).max(initial=0.0) <= Z_MAX, "logits outside the range the bounds are claimed for"
    e = np.where(legal, np.exp(z), 0.0)
    s = np.where(has, e.sum(1), 1.0)
    p = e / s[:, None]
    logp_all = np.where(legal, z - np.log(s)[:, None], 0.0)
    H = -(p * logp_all).sum(1)
    played = legal[rows, act]
    la = np.where(played, logp_all[rows, act], -np.inf)
    with np.errstate(over="ignore"):
        ratio = np.where(has, np.exp(la - logp_old), 0.0)
    s1, s2 = ratio * A, np.clip(ratio, 1.0 - clip, 1.0 + clip) * A
    first, inside = s1 <= s2, (ratio > 1.0 - clip) & (ratio < 1.0 + clip)
    g = np.where(has & (first | inside), -A * ratio, 0.0)
    pi = np.where(has, -np.minimum(s1, s2), 0.0)
    value = logits[:, 54]
    dv = np.where(has, value - ret, 0.0)
    delta = np.zeros((n, 54)); delta[rows, act] = 1.0
    d_policy, d_entropy, d_value = np.zeros((n, 64)), np.zeros((n, 64)), np.zeros((n, 64))
    d_policy[:, :54] = np.where(legal, g[:, None] * (delta - p), 0.0)
    d_entropy[:, :54] = np.where(legal, -p * (logp_all + H[:, None]), 0.0)
    d_value[:, 54] = 2.0 * dv
    return dict(n=n, legal=legal, has=has, act=act, w=w, A=A, ret=ret, clip=clip, vf=vf, ent=ent, pi=pi, v=dv * dv, H=H, p=p,
                logp_all=logp_all, logp=np.where(played, la, 0.0), ratio=ratio, g=g, value=np.where(has, value, 0.0),
                d_policy=d_policy, d_entropy=d_entropy, d_value=d_value)


def loss_gradient(ref):
    """d (pi + vf value - ent H) / d out per unit weight, [n,64], with the coefficients the reference was made with."""
    return ref["d_policy"] + ref["vf"] * ref["d_value"] - ref["ent"] * ref["d_entropy"]


def loss_means(ref, wsum=None):
    """The three weighted means {pi, value, H} and the weight sum (at least 1).  wsum: the divisor, where it is not the sum
    of the weights that count (tarok_ppo_loss divides by the sum of the weights it is GIVEN, a row without a card included)."""
    w = ref["w"]
    wsum = max(float(w.sum()), 1.0) if wsum is None else float(wsum)
    return np.array([(w * ref[k]).sum() / wsum for k in ("pi", "v", "H")]), wsum


def loss_bound(ref, part, scale):
    """Per-element bound [n,64] on |kernel - scale_i part| of a bf16 output computed in float32; part [n,64] per unit
    weight (loss_gradient(ref), or one of its parts in an isolated mode), scale [n].
      columns 0..53, legal:  2^-8 |want| + 2^-15 scale_i (|g_i| + ent)
          2^-8 is the unit roundoff of a round-to-nearest bf16 store (8 significant bits: neighbours 2^-7 apart in
          [1, 2), so half a step is 2^-8 relative just above a power of two) — the store may use this term up; what is
          left for the arithmetic is the floor.  The floor is the float32 evaluation: __expf(z) = exp2(z log2 e) is off
          by about |z| 2^-23 relative, at most 2^-17 for |z| <= 64, so p, and with it g (delta - p), by 2^-17 |g|; log p
          and H inherit about 2^-18 absolute, so ent p (log p + H) moves by about 2^-17 ent; the floor carries a margin
          of 4 over that.
      column 54:  2^-8 |want| + 2^-20 scale_i vf (|value| + |ret|)
          value - ret rounds once (2^-24 (|value| + |ret|)), the factor 2 vf doubles it, the two products add 2^-23
          relative: 2^-22 and a margin of 4.
      columns 55..63 and illegal cards: 0 — the output must compare equal to zero."""
    scale = np.asarray(scale, np.float64)
    want = scale[:, None] * part
    b = np.zeros_like(want)
    floor = 2.0 ** -15 * scale * (np.abs(ref["g"]) + ref["ent"])
    b[:, :54] = np.where(ref["legal"], 2.0 ** -8 * np.abs(want[:, :54]) + floor[:, None], 0.0)
    b[:, 54] = 2.0 ** -8 * np.abs(want[:, 54]) + 2.0 ** -20 * scale * ref["vf"] * (np.abs(ref["value"]) + np.abs(ref["ret"]))
    b[~ref["has"]] = 0.0
    return b


def gemm_reference(inp, W, mask):
    """(inp @ W) . mask in float64: a backward GEMM of the chain with its ReLU mask (inp [n,K], W [K,N], mask [n,N])."""
    return (np.asarray(inp, np.float64) @ np.asarray(W, np.float64)) * np.asarray(mask, bool)


def gemm_bound(inp, W, K, mask=None):
    """Bound on |kernel - gemm_reference| for a bf16 output of a float32-accumulated product whose bf16 input is the
    kernel's own: 2^-8 |want| (the store, as above) + K 2^-23 (|inp| @ |W|) — one float32 ulp per accumulated term, not
    half of one: the MFMA's order and internal rounding of its additions are not specified.  0 where the mask is 0."""
    inp, W = np.asarray(inp, np.float64), np.asarray(W, np.float64)
    assert inp.shape[1] == K == W.shape[0]
    b = 2.0 ** -8 * np.abs(inp @ W) + K * 2.0 ** -23 * (np.abs(inp) @ np.abs(W))
    return b if mask is None else b * np.asarray(mask, bool)


def terms_bound(ref, wsum=None):
    """Bound on |kernel - float64| of the three weighted means: 2^-18 sum w_i |term_i| / wsum + 2^-8 2^-15.
    Each sample's term carries the 2^-18 of log p (relative for pi through the ratio, absolute for H, which is O(1) or
    exact) and 2^-22 for the square; the float32 sum of at most 333 terms — six levels of a wave's butterfly, then at most
    four waves in order, the blocks in double — adds 10 x 2^-24 relative to sum |term|: together below 2^-18.  The floor
    2^-23 covers sums that cancel to (almost) nothing."""
    w = ref["w"]
    wsum = max(float(w.sum()), 1.0) if wsum is None else float(wsum)
    return np.array([2.0 ** -18 * (w * np.abs(ref[k])).sum() / wsum + 2.0 ** -8 * 2.0 ** -15 for k in ("pi", "v", "H")])


def violations(got, want, bound, what, limit=3):
    """Compare element by element.  Returns (largest error / bound over the elements with a non-zero bound — elements with
    bound 0 must compare equal and count as infinite when they do not —, list of messages for the first `limit` elements
    outside their bound, each naming `what`, sample, column, the two values and the bound)."""
    got, want, bound = (np.asarray(t, np.float64) for t in (got, want, bound))
    assert got.shape == want.shape == bound.shape
    err = np.abs(got - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isnan(got), np.inf, ratio)
    bad = np.argwhere(ratio > 1.0)
    msgs = ["%s: sample %d column %d: kernel %r, reference %r, bound %.3g" % (what, i, j, got[i, j], want[i, j], bound[i, j])
            for i, j in bad[:limit]]
    if len(bad) > limit:
        msgs.append("%s: %d elements outside their bound in all" % (what, len(bad)))
    return float(ratio.max(initial=0.0)), msgs


# ---- hand-made samples
KINDS = ("none", "one", "low", "high", "lead", "full", "some")
QUADRANTS = ("above+", "above-", "below+", "below-", "inside+", "inside-")     # ratio against 1 +- clip, sign of A
STATS = {"mixed": (0.125, 1.5), "policy": (0.125, 1.5), "entropy": (0.0, 1.5), "value": (0.0, 1.5)}   # (mean, 1 / std)


def _mask_of(cards):
    m = 0
    for c in cards:
        m |= 1 << int(c)
    return m


def build_cases(n, seed, mode="mixed"):
    """Hand-made samples [n] whatever the logits turn out to be: legal masks (uint64 and [n,54] bool), card bytes, known
    bits, old values rec.z, returns rec.y, stats {mean, 1 / std, ., .}, and the chosen log ratio of every sample; once the
    logits are known, finish_cases sets logp_old from it.  check_cases states what the set guarantees.

    Every number of the advantage is exact in float32: rec.z = k / 64, mean = 1 / 8, rec.y = rec.z + mean + u with u a
    signed multiple of 2^-10 in [1/16, 2], 1 / std = 1.5 — so (rec.y - rec.z - mean) (1 / std) = 1.5 u without a rounding,
    in the kernel and here.  In the entropy-only and value-only modes rec.y = rec.z and mean = 0: A is exactly 0."""
    assert n >= 257 and mode in MODES
    rnd = np.random.RandomState(seed)
    known = np.arange(n) % 5 != 4
    kidx = rnd.permutation(np.flatnonzero(known))
    kind = np.empty(n, dtype=object)
    quota = [("one", 20), ("none", 5), ("low", n // 16), ("high", n // 16), ("lead", n // 8), ("full", n // 16)]
    at = 0
    for name, k in quota:
        kind[kidx[at:at + k]] = name
        at += k
    kind[kidx[at:]] = "some"
    others = np.flatnonzero(~known)
    kind[others] = rnd.choice(KINDS, len(others))
    kind[others[:2]] = "none"                                   # (rows without a card and without the known bit too)
    card = np.zeros(n, np.int64)
    quadrant = np.zeros(n, np.int64)
    masks = np.zeros(n, np.uint64)
    free = 0                                                    # running number of the known samples whose card is ours to choose
    low_cards = [c for c in range(54) if c % 8 < 4]
    high_cards = [c for c in range(54) if c % 8 >= 4]
    for j, i in enumerate(list(kidx) + list(others)):
        k = kind[i]
        quadrant[i] = j % 6
        if k == "none":
            cards, card[i] = [], rnd.randint(54)
        elif k in ("low", "high"):
            pool = low_cards if k == "low" else high_cards
            cards = rnd.choice(pool, rnd.randint(1, 13), replace=False).tolist()
            card[i] = cards[rnd.randint(len(cards))]
        else:
            if known[i]:
                card[i] = free % 54                              # every card 0..53 in turn, its three plays in three quadrants
                quadrant[i] = (free // 54 + free) % 6            # in a row (at most one of them a clipped one)
                free += 1
            else:
                card[i] = rnd.randint(54)
            rest = [c for c in range(54) if c != card[i]]
            extra = {"one": 0, "lead": 11, "full": 53, "some": rnd.randint(1, 12)}[k]
            cards = [int(card[i])] + rnd.choice(rest, extra, replace=False).tolist()
        masks[i] = np.uint64(_mask_of(cards))
    byte = card.astype(np.uint8)
    byte[np.flatnonzero(~known)[::5]] = 255                     # the `act < 54` clamp, on rows that carry no weight
    # the chosen log ratio: outside the clip range by 0.05 .. 0.5 in the logarithm, or inside it by at least 0.02
    clip = MODES[mode][0]
    up, dn = np.log(1.0 + clip), np.log(1.0 - clip)
    t = rnd.rand(n)
    log_ratio = np.where(quadrant < 2, up + 0.05 + 0.45 * t, np.where(quadrant < 4, dn - 0.05 - 0.45 * t, dn + 0.02 + (up - dn - 0.04) * t))
    sign = np.where(quadrant % 2 == 0, 1.0, -1.0)
    u = sign * rnd.randint(64, 2049, n) * 2.0 ** -10
    z = rnd.randint(-128, 129, n) / 64.0
    mean, inv_std = STATS[mode]
    if mode in ("entropy", "value"):
        u = np.zeros(n)
    y = z + mean + u
    for t_ in (y, z, u):
        assert (t_.astype(np.float32).astype(np.float64) == t_).all()
    return dict(n=n, mode=mode, masks=masks, legal=legal_matrix(masks), card=byte, known=known, kind=kind, quadrant=quadrant,
                log_ratio=log_ratio, ret=y, val=z, A=u * inv_std, stats=np.array([mean, inv_std, 0.8, 0.0], np.float32))


def finish_cases(cases, logits):
    """With the logits known: logp_old (float32) = the float64 log-probability of the played card minus the chosen log
    ratio, and the reference of the case set in its mode.  Returns (logp_old, ref)."""
    clip, vf, ent = MODES[cases["mode"]]
    w = cases["known"].astype(np.float64)
    args = (cases["legal"], cases["card"], np.zeros(cases["n"]), cases["A"], cases["ret"], w, clip, vf, ent)
    first = loss_reference(logits, *args)
    logp_old = (first["logp"] - cases["log_ratio"]).astype(np.float32)
    ref = loss_reference(logits, args[0], args[1], logp_old.astype(np.float64), *args[3:])
    return logp_old, ref


def records(cases, logp_old):
    """rec [n,4] float32 of the fused learner: {logp_old, return, old value, bits: card | known << 8}."""
    rec = np.zeros((cases["n"], 4), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = logp_old, cases["ret"], cases["val"]
    rec[:, 3] = (cases["card"].astype(np.uint32) | (cases["known"].astype(np.uint32) << 8)).view(np.float32)
    return rec


def check_cases(cases, ref):
    """The conditions the case set is built for, as hard assertions (they keep a test from hiding a failure)."""
    n, known, kind, legal = cases["n"], cases["known"], cases["kind"], cases["legal"]
    count = legal.sum(1)
    live = known & (count > 0)
    act = ref["act"]
    assert (ref["w"] == live).all() and legal[np.flatnonzero(live), act[live]].all()
    # every card is the played card of at least 3 known samples, at least 2 of them with a gradient (not clipped)
    plays = np.bincount(act[live], minlength=54)
    moving = np.bincount(act[live & (ref["g"] != 0)], minlength=54) if cases["mode"] in ("mixed", "policy") else plays
    assert plays.min() >= 3 and moving.min() >= 2, (plays.min(), moving.min())
    # legal sets
    assert (known & (count == 1)).sum() >= 16
    low = (np.arange(54) % 8 < 4)
    assert (live & ~legal[:, ~low].any(1)).sum() >= n // 16 and (live & ~legal[:, low].any(1)).sum() >= n // 16
    assert (known & (kind == "lead") & (count == 12)).sum() >= n // 8
    assert (known & (count == 54)).sum() >= n // 16 and (cases["masks"][count == 54] == np.uint64((1 << 54) - 1)).all()
    assert (count == 0).sum() >= 4 and (known & (count == 0)).sum() >= 2 and (~known & (count == 0)).sum() >= 2
    # known bits and the card byte
    assert 0.15 <= (~known).mean() <= 0.25
    assert ((cases["card"] == 255) & ~known).sum() >= 3 and not ((cases["card"] >= 54) & known).any()
    # the advantage and the clip quadrants
    clip = ref["clip"]
    mean, inv_std = float(cases["stats"][0]), float(cases["stats"][1])
    if cases["mode"] in ("mixed", "policy"):
        assert mean != 0 and inv_std != 1
        A, ratio = ref["A"], ref["ratio"]
        assert (np.abs(A[live]) > 1e-3).all()
        assert (np.abs(ratio[live] - (1 + clip)) > 1e-3).all() and (np.abs(ratio[live] - (1 - clip)) > 1e-3).all()
        for hi, pos in ((1, 1), (1, 0), (0, 1), (0, 0)):
            q = live & ((ratio > 1 + clip) if hi else (ratio < 1 - clip)) & ((A > 0) if pos else (A < 0))
            assert q.sum() >= n / 16, (hi, pos, q.sum())
        inside = live & (ratio > 1 - clip) & (ratio < 1 + clip)
        assert (inside & (A > 0)).sum() >= n / 16 and (inside & (A < 0)).sum() >= n / 16
        assert (ref["g"][live & (ratio > 1 + clip) & (A > 0)] == 0).all() and (ref["g"][live & (ratio < 1 - clip) & (A < 0)] == 0).all()
        assert (ref["g"][live & ~((ratio > 1 + clip) & (A > 0)) & ~((ratio < 1 - clip) & (A < 0))] != 0).all()
    else:
        assert mean == 0 and (ref["A"] == 0).all()
        assert (cases["ret"].astype(np.float32).view(np.uint32) == cases["val"].astype(np.float32).view(np.uint32)).all()


# ---- feature rows that carry the cases' legal masks
def features_with_masks(x, legal):
    """0/1 feature rows x [n,256] with the legal cards written into bits 0..53 of feature word 1 (features 64..117)."""
    x = np.array(x, np.float64)
    x[:, 64:118] = np.asarray(legal, np.float64)
    return x


def pack_feature_words(x):
    """[n,256] 0/1 -> [n,4] int64 feature words (feature f = bit f % 64 of word f // 64): the inverse of
    TarokVecEnv.expand_feature_words."""
    bits = np.asarray(x).astype(np.uint64).reshape(-1, 4, 64)
    return (bits << np.arange(64, dtype=np.uint64)).sum(2, dtype=np.uint64).view(np.int64)
