"""Exact probes of the MFMA policy forward (policy_body in tarok_env.hip: tarok_policy_mlp, tarok_policy_step), of its
two-lane sampler, of the stand-alone sampler (tarok_sample_policy) and of the fused learner's forward (tarok_learn_chain's
H1 / H2) — the root of the chain of bit-for-bit tests the rollout's outputs hang on.

Why the references are exact.  The forward sums products of bf16 values in float32.  With weights that are small
integers times a power of two and 0/1 features, every product and every partial sum of a layer is an integer multiple
of one quantum and stays below 2^24 quanta, so EVERY order of additions gives the same exactly representable float32
value.  The only roundings left are the float32 -> bf16 stores of H1 and H2, round-to-nearest-even, which
`tensor.to(torch.bfloat16)` reproduces.  A float64 evaluation with those two casts written in is then the kernel's
result to the bit, not an approximation of it (test_learn_dw_is_exact_on_integer_inputs rests on the same fact).

  weight set R ("rounding"): random integer weights whose second layer reaches |z2| ~ 2000, so that a good share of
      the H2 entries are rounded by the bf16 store and many of them are exact ties (round-to-nearest-EVEN decides);
  weight sets P ("paths"): W1 and W2 permutation matrices — every hidden unit copies one input — whose single non-zero
      per row visits every k-step, half and feature tile of the MFMA fragment order; the logits are multiples of 1/8
      below 32, exact in bf16, so the stand-alone sampler can be fed the very same numbers.

The constructors, the reference and their conditions are plain functions; test_weight_sets_meet_their_conditions checks
them on synthetic features anywhere.  The GPU tests are marked `gpu`:
    python -m pytest tests/test_gpu_policy_exact.py -m gpu -q
"""
import numpy as np
import pytest

from policy_exact_ref import (LEADS, NS, P_PARAMS, SEED, U, _played, _u64, _word, _zero_net, check_conditions_p, check_conditions_r, draws,
                              fragment_slots, kernel_weights, legal_matrix, reference, sampler_reference, synthetic_features, weights_p,
                              weights_r)
from gpu_harness import T  # noqa: F401  (the module fixture)


def test_weight_sets_meet_their_conditions():
    """On synthetic 0/1 features of the real sparsity: set R keeps every layer's sums below 2^24 quanta, stores H1
    exactly, rounds at least 5 % of H2 (at least 1 % exact ties) and gives float32 logits; the sets P give 0/1 hidden
    layers and logits that are multiples of 1/8 below 32 (bf16 values); the permutations of all sets P together put a
    non-zero into every (feature tile, k-step, half) slot of both hidden layers' fragment order; and the reference's
    bf16 cast is round-to-nearest-even on the ties."""
    import torch
    x = synthetic_features()
    assert 8 <= int(x.sum(1).min()) and int(x.sum(1).max()) <= 55
    W = weights_r()
    for t, lo, hi, scale in zip(W, (-3, -2, -4, -8, -4, -8), (3, 6, 4, 8.5, 4, 8), (1, 1, 1, 1, 2.0 ** 13, 8)):
        assert lo <= float((t * scale).min()) and float((t * scale).max()) <= hi
        assert torch.equal(t.float().double(), t)
    for t in (W[0], W[2], W[4]):
        assert torch.equal(t.to(torch.bfloat16).double(), t)
    r = reference(x, W)
    rounded, ties = check_conditions_r(r, W)
    assert float(r["z1"].abs().max()) < 256 and float(r["z2"].abs().max()) > 1000
    # round-to-nearest-even, stated once by hand: 257 lies halfway between the bf16 neighbours 256 and 258 -> 256 (even
    # mantissa); 259 between 258 and 260 -> 260; 129.5 between 129 and 130 -> 130
    assert torch.tensor([257.0, 259.0, 129.5]).to(torch.bfloat16).tolist() == [256.0, 260.0, 130.0]
    slots1, slots2 = set(), set()
    for s, a, c in P_PARAMS:
        Wp = weights_p(s, a, c)
        assert bool((Wp[0].sum(0) == 1).all()) and bool((Wp[0].sum(1) == 1).all())
        assert bool((Wp[2].sum(0) == 1).all()) and bool((Wp[2].sum(1) == 1).all())
        check_conditions_p(reference(x, Wp), Wp)
        slots1 |= fragment_slots(Wp[0]); slots2 |= fragment_slots(Wp[2])
    every = {(t, k, h) for t in range(8) for k in range(16) for h in range(2)}
    assert slots1 == every and slots2 == every
    assert fragment_slots(weights_p(0, 1, 0)[4]) == {(t, k, h) for t in range(2) for k in range(16) for h in range(2)}


def compare_with_sampler_reference(ref, action, logp, what):
    """Cards equal wherever the draw is not within 1e-5 of a boundary; every card legal; every logp within the derived
    bound of the float64 log-probability of the card the kernel reports.  Returns (games left out, games, max error)."""
    action = np.asarray(action).astype(np.int64)
    rows = np.arange(len(action))
    assert (action < 54).all() and ref["legal"][rows, action].all(), what
    keep = ~ref["near"]
    wrong = np.nonzero(keep & (action != ref["card"]))[0]
    assert wrong.size == 0, "%s: %d cards differ from the float64 draw, first at game %d: %d vs %d" % (
        what, wrong.size, wrong[0], action[wrong[0]], ref["card"][wrong[0]])
    err = np.abs(np.asarray(logp, np.float64) - ref["logp_all"][rows, action])
    tol = ref["tol_of"](action)
    assert tol.max() < 1e-4
    bad = np.nonzero(err > tol)[0]
    assert bad.size == 0, "%s: logp of game %d off by %.3g (bound %.3g)" % (what, bad[0], err[bad[0]], tol[bad[0]])
    return int((~keep).sum()), len(action), float(err.max())


# ---- GPU
@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


def _launch(env, kw, words):
    import torch
    fw = torch.zeros((env.n, 4), dtype=torch.int64, device="cuda")
    a, lp, v = env.policy_mlp(kw, words, feature_words_out=fw)
    return dict(action=a.cpu().numpy(), logp=lp.cpu(), value=v.cpu(), fw=fw)


@pytest.fixture(scope="module")
def runs(T, S):
    """Every tarok_policy_mlp launch the tests below judge, made once: for each n of NS an env of mixed contracts walked
    through LEADS random lock-steps with auto-reset; at each position one launch per weight set (R and every P), on set
    P also tarok_sample_policy on the reference's logits, and at n = 333 two positions with every W3 row in turn copied
    into row 54.  Each entry carries the float64 reference of its launch (from the launch's own feature words, which
    test_fused_policy_mlp_kernel_vs_torch pins to tarok_observe)."""
    import torch
    K = T.karte
    WR = weights_r()
    WP = [weights_p(*p) for p in P_PARAMS]
    out = []
    for n in NS:
        env = T.TarokVecEnv(n, seed=SEED, mix=K.MIX_ALL)
        kr = kernel_weights(T, WR)
        kp = [kernel_weights(T, w) for w in WP]
        obs = env.reset()
        done = 0
        for lead in LEADS:
            while done < lead:
                obs, _, _ = env.step(env.policy_random(obs), auto_reset=True)
                done += 1
            words = obs.words.clone()
            episodes, _ = env.counters()
            pos = dict(n=n, lead=lead, words=_u64(words), episodes=episodes)
            got = _launch(env, kr, words)
            x = T.TarokVecEnv.expand_feature_words(got["fw"], torch.float64).cpu()
            pos["x"], pos["fw"] = x, got["fw"].cpu()
            pos["R"] = dict(got=got, ref=reference(x, WR))
            pos["P"] = []
            for w, k in zip(WP, kp):
                got = _launch(env, k, words)
                assert torch.equal(got["fw"].cpu(), pos["fw"])
                ref = reference(x, w)
                pad = torch.zeros((n, 64), dtype=torch.bfloat16, device="cuda")
                pad[:, :54] = ref["out"][:, :54].to(torch.bfloat16).cuda()
                a2, lp2 = env.sample_policy(pad, words)
                pos["P"].append(dict(got=got, ref=ref, alone=dict(action=a2.cpu().numpy(), logp=lp2.cpu())))
            pos["row54"] = []
            if n == 333 and lead in (3, 31):
                for name, w, ref in (("R", WR, pos["R"]["ref"]), ("P", WP[2], pos["P"][2]["ref"])):
                    for row in range(54):
                        v = env.policy_mlp(kernel_weights(T, w, w3_row_to_54=row), words)[2].cpu()
                        pos["row54"].append((name, row, v, (ref["h2"] @ w[4][row] + w[5][54])))
            out.append(pos)
        env.close()
    return out, WR, WP


@pytest.mark.gpu
def test_positions_and_references_meet_the_conditions(T, runs):
    """Before any kernel output is looked at: the positions cover trick positions 0-3, the first and the last trick
    and every n of NS; on the real features set R keeps float32 exact, rounds at least 5 % of H2 with at least 1 %
    ties (per n, over its positions) and gives float32 logits; every set P gives 0/1 hidden layers and bf16 logits."""
    import torch
    K = T.karte
    out, WR, WP = runs
    assert sorted({p["n"] for p in out}) == sorted(NS)
    played = np.concatenate([_played(p["words"]) for p in out])
    assert set(range(4)) <= set((played % 4).tolist()) and played.min() == 0 and played.max() >= 44
    for n in NS:
        mine = [p for p in out if p["n"] == n]
        cat = {k: torch.cat([p["R"]["ref"][k] for p in mine]) for k in ("x", "z1", "h1", "z2", "h2", "out")}
        check_conditions_r(cat, WR)
        for j, w in enumerate(WP):
            check_conditions_p({k: torch.cat([p["P"][j]["ref"][k] for p in mine]) for k in cat}, w)
    for p in out:                                                            # feature word 1 = the legal cards of the observation word
        assert (_u64(p["fw"])[:, 1] & np.uint64(K.OBS_MASK) == p["words"] & np.uint64(K.OBS_MASK)).all()


@pytest.mark.gpu
def test_value_out_is_bit_exact(runs):
    """value_out == column 54 of the exact reference, as float32 bits, for set R and every set P at every n and
    position — and with each W3 row 0..53 in turn copied into row 54 (bias b3[54] kept), so that the path of output 54
    through the head is exact for every k-pattern the head carries.  A weight fragment from the wrong k-step, half or
    feature tile, a bias quad shifted, an H store that truncates: each moves some value by at least one quantum."""
    import torch
    out, WR, WP = runs
    checked = 0
    for p in out:
        for name, e in [("R", p["R"])] + [("P%d" % j, e) for j, e in enumerate(p["P"])]:
            want = e["ref"]["out"][:, 54]
            assert torch.equal(want.float().double(), want)
            got = e["got"]["value"]
            if not torch.equal(got, want.float()):
                bad = (got != want.float()).nonzero().flatten()
                pytest.fail("set %s, n = %d, %d lock-steps in: %d values differ, first at game %d: %r vs %r"
                            % (name, p["n"], p["lead"], bad.numel(), bad[0], got[bad[0]].item(), want[bad[0]].item()))
            checked += 1
        for name, row, got, want in p["row54"]:
            assert torch.equal(want.float().double(), want)
            assert torch.equal(got, want.float()), "set %s, W3 row %d in row 54, %d lock-steps in" % (name, row, p["lead"])
            checked += 1
    assert checked == len(NS) * len(LEADS) * (1 + len(P_PARAMS)) + 2 * 2 * 54


@pytest.mark.gpu
def test_policy_mlp_equals_sample_policy_on_exact_logits(runs):
    """On the sets P the logits are bf16 values, so tarok_sample_policy can be fed exactly what tarok_policy_mlp's head
    produced (the reference's logits, zero-padded to 64 columns).  Both kernels then run the same float32 statement in
    the same order — maximum, exps, the sum over cards 0..26 and then 27..53 continuing from it, the running CDF from the
    same start, the fall-through — so `action` and the BITS of `logp` are identical for every game.  A wrong logit (a
    card's column read from the wrong place), a swapped lane pair or another draw index breaks it."""
    import torch
    out, _, _ = runs
    games = 0
    for p in out:
        for j, e in enumerate(p["P"]):
            what = "set P%d, n = %d, %d lock-steps in" % (j, p["n"], p["lead"])
            assert (e["got"]["action"] == e["alone"]["action"]).all(), what
            assert torch.equal(e["got"]["logp"].view(torch.int32), e["alone"]["logp"].view(torch.int32)), what
            games += p["n"]
    assert games == sum(NS) * len(LEADS) * len(P_PARAMS)


def _hand_built(T, S, n, seed):
    """Hand-built sampler inputs for an env of n games at episode 0: random bf16 logits (sd 2, +30 on a third of the
    illegal cards: a leaked mask bit would dominate), legal sets of 1..12 cards anywhere in 0..53, cards played 0..47."""
    import torch
    rnd = np.random.RandomState(seed)
    logits = torch.from_numpy(rnd.randn(n, 64) * 2).to(torch.bfloat16)
    masks = np.zeros(n, np.uint64)
    for i in range(n):
        for c in rnd.choice(54, rnd.randint(1, 13), replace=False):
            masks[i] |= np.uint64(1) << np.uint64(c)
    legal = np.zeros((n, 64), bool); legal[:, :54] = legal_matrix(masks)
    bump = torch.from_numpy(~legal & (rnd.rand(n, 64) < 0.33))
    logits[bump] = 30.0
    played = rnd.randint(0, 48, n).astype(np.uint64)
    words = masks | (rnd.randint(0, 4, n).astype(np.uint64) << np.uint64(54)) | (played << np.uint64(56))
    return logits, masks, played, words


@pytest.mark.gpu
def test_sampler_against_float64(T, S, runs):
    """The card has ONE right answer: u = ((r >> 8) + 0.5) / 2^24 with r = rng32(game_key(seed, game, episode), 192 +
    cards played) — oracle/tarok_spec.py's functions, the episode from env.counters() — and the card is the first legal
    c whose float64 CDF of exp(l_c - max) exceeds u sum.  Judged: tarok_sample_policy on hand-built logits (333 games)
    and tarok_policy_mlp on set R (every n and position).  A game is left out of the card comparison only if u lies
    within 1e-5 of a boundary between two legal cards (relative to the sum); at most 0.2 % of the games may be (a
    condition: about 12 boundaries x 2e-5 = 0.03 % are expected); every other card must match.

    The bound on |logp - float64|, u = 2^-24 (half a float32 ulp), to first order:
      d_c = l_c - max: one subtraction, u |d_c|;  t_c = log2(e) d_c: the constant and the product, 2 u |t_c|;
      e_c = v_exp_f32(t_c): 1 ulp = 2 u (the ISA manuals state "1ULP accuracy" for v_exp_f32 and v_log_f32), and
          the 3 u |t_c| carried in reach e_c as 3 u |d_c| (ln 2 log2 e = 1): e_c is off by at most (2 + 3 |d_c|) u;
      sum: at most 12 legal cards (a hand) -> at most 12 additions of non-negative terms (the zeros of illegal cards add
          exactly): 12 u, plus the terms' own errors weighted by their share, (2 + 3 sum_c p_c |d_c|) u;
      q = e_a / sum: one correctly rounded division, u;
      logf(q): the kernels' __logf compiles to the full logf — v_log_f32 (1 ulp = 2 u of log2 q) times ln 2 as a
          two-word constant with an fma for the product's low part and one final rounding, 2 u more — at most
          4 u |logp|, and q's relative error arrives unchanged:
      |logp - float64| <= u (16 + 3 (|d_a| + sum_c p_c |d_c|) + 4 |logp|)  [+ 1e-9: second order and the reference's own].
    For a card 10 below the maximum drawn at p = e^-10: 6e-8 x (16 + 30 + 3 + 40) = 5e-6; typical games: 1.3e-6.  The
    largest bound of any game here is asserted to be below 1e-4 (the old tests allow 2e-3 and 0.08); the test prints
    the largest error it saw (run with -s)."""
    import torch
    K = T.karte
    out, WR, _ = runs
    left_out = games = 0
    worst = 0.0
    # tarok_sample_policy on hand-built rows
    n = 333
    env = T.TarokVecEnv(n, seed=SEED + 1, mix=K.MIX_ALL, game_offset=1000)
    env.reset()
    episodes, _ = env.counters()
    assert (episodes == 0).all()
    logits, masks, played, words = _hand_built(T, S, n, seed=5)
    a, lp = env.sample_policy(logits.cuda().contiguous(), torch.from_numpy(words.view(np.int64)).cuda())
    ref = sampler_reference(logits.double().numpy(), masks, draws(S, SEED + 1, 1000, episodes, played))
    k, m, w = compare_with_sampler_reference(ref, a.cpu().numpy(), lp.cpu().numpy(), "tarok_sample_policy")
    left_out += k; games += m; worst = max(worst, w)
    worst_alone = w
    env.close()
    # tarok_policy_mlp on set R
    for p in out:
        live = (p["words"] & np.uint64(K.OBS_MASK)) != 0
        assert live.all()                                                    # (auto-reset: every slot has a card to play)
        ref = sampler_reference(p["R"]["ref"]["out"].numpy(), p["words"] & np.uint64(K.OBS_MASK),
                                draws(S, SEED, 0, p["episodes"], _played(p["words"])))
        got = p["R"]["got"]
        k, m, w = compare_with_sampler_reference(ref, got["action"], got["logp"].numpy(),
                                                 "tarok_policy_mlp, set R, n = %d, %d lock-steps in" % (p["n"], p["lead"]))
        left_out += k; games += m; worst = max(worst, w)
    print("sampler vs float64: %d games, %d left out, max |logp - float64| = %.3g (tarok_sample_policy alone: %.3g)"
          % (games, left_out, worst, worst_alone))
    assert games == 333 + sum(NS) * len(LEADS)
    assert left_out <= 0.002 * games, (left_out, games)
    assert worst < 1e-4


def _both_samplers(T, env, logits_row, words):
    """[(name, action, logp)] of tarok_sample_policy and of tarok_policy_mlp's sampler (zero matrices, b3 = the logits)
    on the same logits row for every game and the same hand-built observation words."""
    import torch
    w = torch.from_numpy(np.asarray(words, np.uint64).view(np.int64)).cuda()
    row = logits_row.to(torch.bfloat16)
    a, lp = env.sample_policy(row.repeat(env.n, 1).cuda().contiguous(), w)
    a2, lp2, val = env.policy_mlp(_zero_net(T, row.float()), w)
    assert (val.cpu() == row[54].float()).all()
    return [("tarok_sample_policy", a.cpu().numpy(), lp.cpu().numpy()), ("tarok_policy_mlp", a2.cpu().numpy(), lp2.cpu().numpy())]


@pytest.mark.gpu
def test_sampler_edges(T, S):
    """The edges of both samplers (tarok_sample_policy; policy_body's two-lane one through tarok_policy_mlp with zero
    matrices and b3 = the logits), a handful of rows per launch:
      one legal card -> that card, logp == 0.0 exactly; no legal card -> 255 and 0.0;
      all legal logits equal -> every exp is exactly 1, the sum an exact integer k, so with u restated in numpy float32 by
        the kernel's three operations the card is the floor(u)-th legal one for EVERY game (no game left out), and logp is
        within one rounding of the division plus one ulp of the logarithm of -log(k) — for cards played 0..47 and legal
        sets only in cards 0..26, only in 27..53 and in both (the lane-pair split of policy_body);
      a legal card 100 below the maximum (its exp underflows) is never drawn;
      a draw at the very top of the CDF ((r >> 8) = 2^24 - 1, where the float32 u equals the sum and no card's CDF exceeds
        it: found by a search over game indices on the CPU and re-checked here) -> the last legal card, from either half."""
    import torch
    K = T.karte
    rnd = np.random.RandomState(11)
    n = 144
    env = T.TarokVecEnv(n, seed=SEED + 2, mix=K.MIX_ALL, game_offset=7)
    env.reset()
    episodes, _ = env.counters()
    assert (episodes == 0).all()
    # ---- one card / no card
    row = torch.from_numpy(rnd.randn(64) * 3)
    words = [_word([i % 54] if i % 5 else [], i % 48) for i in range(n)]
    for name, a, lp in _both_samplers(T, env, row, words):
        for i in range(n):
            assert (int(a[i]), float(lp[i])) == ((i % 54, 0.0) if i % 5 else (255, 0.0)), (name, i)
    # ---- all legal logits equal
    row = torch.full((64,), 1.25, dtype=torch.float64)
    sets, words = [], []
    for i in range(n):
        played, kind = i % 48, i // 48                                       # kind 0: cards 0..26, 1: 27..53, 2: both halves
        if kind == 2:
            cards = sorted(rnd.choice(27, rnd.randint(1, 7), replace=False).tolist() + (27 + rnd.choice(27, rnd.randint(1, 7), replace=False)).tolist())
        else:
            cards = sorted((27 * kind + rnd.choice(27, rnd.randint(2, 13), replace=False)).tolist())
        sets.append(cards); words.append(_word(cards, played))
    r = draws(S, SEED + 2, 7, episodes, [i % 48 for i in range(n)])
    for name, a, lp in _both_samplers(T, env, row, words):
        for i, cards in enumerate(sets):
            k = len(cards)
            u = (np.float32(int(r[i]) >> 8) + np.float32(0.5)) * np.float32(1.0 / 16777216.0) * np.float32(k)
            assert u.dtype == np.float32
            assert int(a[i]) == cards[min(int(np.floor(u)), k - 1)], (name, i, cards, float(u))
            assert abs(float(lp[i]) + np.log(k)) <= U + np.spacing(np.float32(np.log(k))), (name, i, k, float(lp[i]))
    # ---- a legal card 100 below the maximum is never drawn (and the rest of the draw is the float64 one)
    row = torch.from_numpy(rnd.randn(64)).clamp(max=1.5).to(torch.bfloat16).double()
    low = [4, 26, 27, 40]
    row[[1, 50]] = 2.0                                                       # the maximum of every legal set below
    row[low] = 2.0 - 100.0
    assert torch.equal(row.to(torch.bfloat16).double(), row)
    sets, words = [], []
    for i in range(n):
        others = [c for c in rnd.choice(54, rnd.randint(2, 9), replace=False).tolist() if c not in low]
        cards = sorted(set(others + [50 if i % 2 else 1]) | {low[i % 4]})    # (never the last legal card together with a top draw: below)
        sets.append(cards); words.append(_word(cards, i % 48))
    masks = np.array([w & K.OBS_MASK for w in words], np.uint64)
    ref = sampler_reference(row.numpy()[None, :].repeat(n, 0), masks, r)
    assert (int(r.max()) >> 8) < 2 ** 24 - 1
    for name, a, lp in _both_samplers(T, env, row, words):
        assert not any(int(a[i]) in low for i in range(n)), name
        compare_with_sampler_reference(ref, a, lp, name + ", a card 100 below the maximum")
    env.close()
    # ---- the top of the CDF
    for game, played in TOP_DRAWS:
        assert S.rng32(S.game_key(TOP_SEED, game, 0), 192 + played) >> 8 == 2 ** 24 - 1
        env = T.TarokVecEnv(4, seed=TOP_SEED, mix=K.MIX_ALL, game_offset=game - 1)       # the game is row 1
        env.reset()
        assert (env.counters()[0] == 0).all()
        row = torch.from_numpy(rnd.randn(64)).to(torch.bfloat16).double()
        for cards in ([3, 10, 20], [5, 30, 50], [0, 26], [27, 53], [2, 9, 12, 26, 27], [8]):
            words = [_word(cards, played)] * 4
            rr = draws(S, TOP_SEED, game - 1, [0] * 4, [played] * 4)
            ref = sampler_reference(row.numpy()[None, :].repeat(4, 0), np.array([w & K.OBS_MASK for w in words], np.uint64), rr)
            assert ref["card"][1] == cards[-1]
            for name, a, lp in _both_samplers(T, env, row, words):
                assert int(a[1]) == cards[-1], (name, game, cards, int(a[1]))
                compare_with_sampler_reference(ref, a, lp, name + ", top of the CDF")
        env.close()


TOP_SEED = 41
TOP_DRAWS = ((92280, 16), (196923, 30))   # (game index, cards played) with rng32(game_key(41, game, 0), 192 + played) >> 8 == 2^24 - 1


SENTINEL_BF16 = 0x7FC1                    # (as in test_gpu_learner.py: a NaN payload no kernel writes)


@pytest.mark.gpu
@pytest.mark.parametrize("B,indexed", [(33, True), (33, False), (333, True), (333, False)])
def test_learner_forward_equals_the_reference(T, runs, B, indexed):
    """tarok_learn_chain's H1 and H2 (bf16 [B, 256], the only place the hidden layers are visible) EQUAL the exact
    reference's on set R and on a set P, loaded through learn_adam(..., apply=False), on feature words of the real
    positions above — gathered through an index or row by row, the padding rows keeping their sentinel.  (The float64
    autograd tests of tests/test_gpu_learner.py allow 0.02 (1 + max) here.)"""
    import torch
    K = T.karte
    out, WR, WP = runs
    mine = [p for p in out if p["n"] == 333]
    words = torch.cat([p["fw"] for p in mine]).cuda().contiguous()
    masks = torch.from_numpy(np.concatenate([p["words"] for p in mine]).view(np.int64)).cuda() & K.OBS_MASK
    M = words.shape[0]
    g = torch.Generator(device="cuda"); g.manual_seed(B)
    idx = torch.randperm(M, device="cuda", generator=g)[:B].contiguous() if indexed else torch.arange(B, device="cuda")
    x = torch.cat([p["x"] for p in mine])[idx.cpu()]
    act = (((masks.unsqueeze(-1) >> torch.arange(54, device="cuda")) & 1) > 0).float().argmax(1)    # the lowest legal card
    rec = torch.zeros((M, 4), device="cuda")
    rec[:, 1] = torch.randn(M, device="cuda", generator=g)
    rec[:, 3] = (act.to(torch.int32) | 256).view(torch.float32)
    stats = torch.tensor([0.1, 0.9, 0.8, 0.0], device="cuda")
    env = T.TarokVecEnv(256, seed=1)
    for name, W in (("R", WR), ("P", WP[3])):
        ref = reference(x, W)
        flat = torch.cat([t.reshape(-1) for t in W]).float().cuda().contiguous()
        assert flat.numel() == K.MLP_PARAMS
        bf = lambda k: torch.empty(k, dtype=torch.bfloat16, device="cuda")
        wf = dict(w1=bf(65536), w2=bf(65536), w3=bf(16384), w3t=bf(16384), w2t=bf(65536))
        env.learn_adam(flat, None, None, None, None, wf, apply=False)
        bias = (flat[K.MLP_B1:K.MLP_B1 + 256], flat[K.MLP_B2:K.MLP_B2 + 256], flat[K.MLP_B3:K.MLP_B3 + 64])
        act_t = lambda k: torch.zeros((B + K.LEARN_PAD, k), dtype=torch.bfloat16, device="cuda")
        H1, H2, dH2, dH1, dOut = act_t(256), act_t(256), act_t(256), act_t(256), act_t(64)
        for t_ in (H1, H2):
            t_[B:].view(torch.int16).fill_(SENTINEL_BF16)
        Xw = torch.zeros((B + K.LEARN_PAD, 4), dtype=torch.int64, device="cuda")
        scratch = torch.empty(((B + 95) // 96, 4), device="cuda")
        terms = torch.empty(4, device="cuda")
        env.learn_chain(B, words, idx if indexed else None, rec, stats, 0.2, 0.5, 0.01, wf, bias, Xw, H1, H2, dOut, dH2, dH1, scratch, terms)
        assert torch.equal(Xw[:B], words[idx])
        for got, want, hn in ((H1, ref["h1"], "H1"), (H2, ref["h2"], "H2")):
            assert (got[B:].view(torch.int16) == SENTINEL_BF16).all().item(), hn
            got = got[:B].double().cpu()
            if not torch.equal(got, want):
                bad = (got != want).nonzero()
                pytest.fail("set %s: %d entries of %s differ, first at sample %d unit %d: %r vs %r"
                            % (name, bad.shape[0], hn, bad[0, 0], bad[0, 1], got[tuple(bad[0])].item(), want[tuple(bad[0])].item()))
        assert torch.isfinite(terms[:3]).all().item()
    env.close()


@pytest.mark.gpu
def test_policy_step_equals_policy_mlp_on_set_r(T):
    """tarok_policy_step (policy_body<2>: two 128-game tiles per workgroup) on set R at n = 333 + 256 (two workgroups of
    256 games and a ragged one of 77): value_out, logp_out and action_out have the bits of a tarok_policy_mlp launch on
    the same observation words, at three positions.  (The existing equivalence test uses torch-initialised weights only.)"""
    import torch
    K = T.karte
    n = 333 + 256
    env = T.TarokVecEnv(n, seed=SEED + 3, mix=K.MIX_ALL)
    kr = kernel_weights(T, weights_r())
    obs = env.reset()
    for _ in range(6):
        obs, _, _ = env.step(env.policy_random(obs), auto_reset=True)
    words = [obs.words.clone(), torch.zeros(n, dtype=torch.int64, device="cuda")]
    for t in range(3):
        fw1 = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        a1, lp1, v1 = env.policy_mlp(kr, words[t & 1], feature_words_out=fw1)
        a2 = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
        lp2, v2 = torch.full((n,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
        fw2 = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        env.policy_step(kr, words[t & 1], words[(t + 1) & 1], a2, lp2, v2, feature_words_out=fw2)
        assert torch.equal(a1, a2) and torch.equal(fw1, fw2), t
        assert torch.equal(lp1.view(torch.int32), lp2.view(torch.int32)) and torch.equal(v1.view(torch.int32), v2.view(torch.int32)), t
        assert (a1 < 54).all().item() and lp1.min().item() < 0
    env.close()
