"""GPU: the play mode of the policy launches (tarok_set_play_mode) — greedy, tempered and epsilon-greedy play — against
the float64 model of tests/play_mode_model.py, and the default mode (1, 0) against an env that was never touched.

n = 300 games: two partial 128-game tiles of tarok_policy_mlp, and a second, partial 256-game workgroup of the step
launches.  Positions come from a handful of step_random lock-steps with auto-reset (legal sets of 1 to 12 cards).  On the
integer weight set R of tests/policy_exact_ref.py the logits are known exactly (float32 values, ties among them),
so the arg-max has one right answer per row.

    python -m pytest tests/test_gpu_play_mode.py -m gpu -q
"""
import numpy as np
import pytest

import play_mode_model as PM
from policy_exact_ref import U, _played, _u64, _word, _zero_net, kernel_weights, reference, weights_r
from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

N, SEED = 300, 61
LEADS = (0, 1, 2, 3, 5, 14)
NEAR = 1e-5            # the float32 rounding margin of a tempered draw, derived in test_temperature's docstring
MASK54 = np.uint64((1 << 54) - 1)
MODES = ((0.0, 0.0), (0.5, 0.0), (2.0, 0.0), (0.0, 1.0), (0.0, 0.25), (1.0, 0.25))      # (temperature, epsilon) of the fixture's launches


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def set_mode(env, t, e):
    env.set_play_mode(t, e)
    assert env.play_mode == (np.float32(t), np.float32(e))


@pytest.fixture(scope="module")
def positions(T):
    """Six positions of an env of 300 mixed-contract games; at each the observation words, the draw keys and — from the
    (1, 0) launch's own feature words — the exact logits of set R, with that launch's value bits; then, under every mode
    of MODES, one tarok_policy_mlp launch on set R and one tarok_sample_policy launch on the same logits as bf16 (the
    network reads the env's state: its launches are made while the env stands at the position).  Computed once."""
    import torch
    K = T.karte
    WR = weights_r()
    kr = kernel_weights(T, WR)
    env = T.TarokVecEnv(N, seed=SEED, mix=K.MIX_ALL)
    out, done = [], 0
    obs = env.reset()
    for lead in LEADS:
        while done < lead:
            obs, _, _ = env.step_random(auto_reset=True)
            done += 1
        words = env.legal_actions().words.clone()
        episodes, _ = env.counters()
        fw = torch.zeros((N, 4), dtype=torch.int64, device="cuda")
        _, _, v = env.policy_mlp(kr, words, feature_words_out=fw)
        x = T.TarokVecEnv.expand_feature_words(fw, torch.float64).cpu()
        ref = reference(x, WR)["out"]
        assert torch.equal(ref.float().double(), ref)
        w = _u64(words)
        assert ((w & MASK54) != 0).all()
        logits = ref.float().numpy()
        lb = bf16_pad(logits)
        got = {}
        for mode in MODES:
            set_mode(env, *mode)
            a, lp, v1 = env.policy_mlp(kr, words)
            a2, lp2 = env.sample_policy(lb, words)
            got[mode] = dict(a=a.cpu(), lp=lp.cpu(), v=bits(v1), a2=a2.cpu(), lp2=lp2.cpu())
        set_mode(env, 1.0, 0.0)
        out.append(dict(words=words, masks=w & MASK54, played=_played(w), keys=PM.keys_of(SEED, 0, episodes),
                        logits=logits, logits_bf16=lb.float().cpu().numpy(), value=bits(v), got=got))
    ks = np.concatenate([PM.play_mode(p["logits"], p["masks"], p["played"], p["keys"], 0.0, 0.0)["k"] for p in out])
    assert ks.min() == 1 and ks.max() == 12
    yield env, kr, out
    env.close()


def bf16_pad(logits):
    import torch
    pad = torch.zeros((logits.shape[0], 64), dtype=torch.bfloat16, device="cuda")
    pad[:, :54] = torch.from_numpy(logits[:, :54]).to(torch.bfloat16).cuda()
    return pad


def hand_built(n, seed):
    """Random bf16 logits (sd 2), legal sets of 1..12 cards anywhere, cards played 0..47, for games 0..n-1 at episode 0."""
    import torch
    rnd = np.random.RandomState(seed)
    logits = torch.from_numpy(rnd.randn(n, 64) * 2).to(torch.bfloat16)
    masks = np.zeros(n, np.uint64)
    for i in range(n):
        for c in rnd.choice(54, rnd.randint(1, 13), replace=False):
            masks[i] |= np.uint64(1) << np.uint64(c)
    played = rnd.randint(0, 48, n).astype(np.uint64)
    words = masks | (rnd.randint(0, 4, n).astype(np.uint64) << np.uint64(54)) | (played << np.uint64(56))
    return logits, masks, played.astype(np.int64), words


def dev_words(words):
    import torch
    return torch.from_numpy(np.asarray(words, np.uint64).view(np.int64)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
def test_default_mode_is_untouched(T):
    """Twin envs: one never touched, one after set_play_mode(0, 0.3) and back to (1, 0).  tarok_policy_mlp and eight
    tarok_policy_step launches write equal bits in every row of every output.  (Where the library has no play mode the
    twins are two plain envs: the test passes on both sides of the change.)"""
    import torch
    K = T.karte
    kr = kernel_weights(T, weights_r())
    res = []
    for touched in (False, True):
        env = T.TarokVecEnv(N, seed=SEED + 1, mix=K.MIX_ALL)
        if touched and hasattr(env, "set_play_mode"):
            set_mode(env, 0.0, 0.3)
            set_mode(env, 1.0, 0.0)
        obs = env.reset()
        for _ in range(3):
            obs, _, _ = env.step_random(auto_reset=True)
        z = lambda dt, *s: torch.full(s, 77, dtype=dt, device="cuda")
        words = [obs.words.clone(), z(torch.int64, N)]
        fw0 = z(torch.int64, N, 4)
        got = [t.clone() for t in env.policy_mlp(kr, words[0], feature_words_out=fw0)] + [fw0]
        act, logp, val = z(torch.uint8, 8, N), z(torch.float32, 8, N), z(torch.float32, 8, N)
        fw, rew, dn = z(torch.int64, 8, N, 4), z(torch.int16, 8, N, 4), z(torch.uint8, 8, N)
        for t in range(8):
            env.policy_step(kr, words[t & 1], words[(t + 1) & 1], act[t], logp[t], val[t], feature_words_out=fw[t],
                            reward_out=rew[t], done_out=dn[t])
        res.append([g.cpu() for g in got] + [act.cpu(), logp.cpu().view(torch.int32), val.cpu().view(torch.int32), fw.cpu(), rew.cpu(),
                                              dn.cpu(), words[0].cpu(), words[1].cpu(), torch.from_numpy(env.state().view(np.int64))])
        env.close()
    for a, b in zip(*res):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.float32 else a, b.view(torch.uint8) if b.dtype == torch.float32 else b)
    assert (res[0][4] < 54).all()


EDGE_ROWS = (  # (legal cards, logits by card: the rest are -1)
    ([17], {}), ([], {}), ([2, 9, 26, 27, 40], {2: 1.5, 9: 1.5, 26: 1.5, 27: 1.5, 40: 1.5}), ([3, 26, 30], {26: 4.0}),
    ([3, 27, 30], {27: 4.0}), ([3, 26, 27, 50], {26: 4.0, 27: 4.0}), ([0, 53], {0: 2.0, 53: 2.0}), ([27, 53], {53: 0.5}),
    ([0, 26], {26: 0.5}), ([5, 26, 27], {27: 4.0, 26: 3.5}))


def test_greedy_is_exact(T, positions):
    """(0, 0) on set R: tarok_policy_mlp's card is the model's arg-max (the lowest-numbered legal card at the maximum of
    the exact float32 logits) on every row, logp is 0.0 bit for bit, and value_out has the bits of the (1, 0) launch;
    tarok_sample_policy on the same logits as bf16 agrees with the model on the bf16 values.  Then hand-built edge rows
    through both samplers: one legal card, none, all logits equal, the maximum on card 26, on card 27 (the lane-pair
    seam), equal maxima on 26 and 27 and across the far ends."""
    import torch
    env, kr, pos = positions
    ties = 0
    for p in pos:
        m = PM.play_mode(p["logits"], p["masks"], p["played"], p["keys"], 0.0, 0.0)
        g = p["got"][(0.0, 0.0)]
        assert (g["a"].numpy() == m["card"]).all()
        assert (bits(g["lp"]) == 0).all() and (g["v"] == p["value"]).all()
        mb = PM.play_mode(p["logits_bf16"], p["masks"], p["played"], p["keys"], 0.0, 0.0)
        assert (g["a2"].numpy() == mb["card"]).all() and (bits(g["lp2"]) == 0).all()
        top = np.where(mb["legal"], p["logits_bf16"][:, :54], -np.inf)
        ties += int(((top == top.max(1, keepdims=True)).sum(1) > 1).sum())
    assert ties > 0                                  # (as bf16 some maxima repeat; the float32 ones do in the edge rows below)
    # ---- edge rows (every game reads the same logits row: zero matrices, b3 = the row)
    small = T.TarokVecEnv(4, seed=SEED, mix=T.karte.MIX_ALL)
    set_mode(small, 0.0, 0.0)
    small.reset()
    for cards, vals in EDGE_ROWS:
        row = torch.full((64,), -1.0)
        for c, x in vals.items():
            row[c] = x
        words = dev_words([_word(cards, 9)] * 4)
        want = 255 if not cards else min(c for c in cards if row[c] == max(row[d] for d in cards))
        a, lp = small.sample_policy(row.to(torch.bfloat16).repeat(4, 1).cuda().contiguous(), words)
        a2, lp2, _ = small.policy_mlp(_zero_net(T, row), words)
        for name, aa, ll in (("tarok_sample_policy", a, lp), ("tarok_policy_mlp", a2, lp2)):
            assert (aa.cpu().numpy() == want).all() and (bits(ll) == 0).all(), (name, cards, vals, aa.cpu().tolist())
    small.close()


def check_tempered(m, action, logp, what):
    """Cards equal the model's wherever the draw is not within NEAR of a CDF edge; logp within the model's bound of the
    float64 log-probability of the card the kernel reports.  Returns (rows left out, worst logp error)."""
    action = action.cpu().numpy().astype(np.int64)
    keep = m["margin"] >= NEAR
    assert (action[keep] == m["card"][keep]).all(), what
    same = action == m["card"]                                          # (a row left out that drew the neighbour: no logp of the model's)
    err = np.abs(logp.cpu().numpy().astype(np.float64) - m["logp"])[same]
    print("%s: %d rows, %d left out, max |logp - float64| = %.3g (bound %.3g)" % (what, len(action), int((~keep).sum()), err.max(), m["tol"].max()))
    assert (err <= m["tol"][same]).all(), (what, float(err.max()))
    return int((~keep).sum()), float(err.max())


@pytest.mark.parametrize("temperature", [0.5, 2.0])
def test_temperature(T, positions, temperature):
    """(T, 0) for T = 0.5 and 2: the card is the model's inverse-CDF draw from p_T ~ exp((l - max) * inv_t), inv_t the
    float32 1 / T.  Inputs: set R through tarok_policy_mlp (exact logits), hand-built random bf16 logits through
    tarok_sample_policy (and the set R logits as bf16), and one random logits row through both samplers (zero matrices, b3 = the row).

    The margin.  A float32 sampler can answer differently from the float64 one only if u lies nearer a CDF edge than the
    rounding error of cdf_c / sum - u.  With u = 2^-24 and t_c = (l_c - max) * inv_t: the difference costs u |t_c|, the
    NEW multiply by inv_t u |t_c|, the constant and product of log2(e) 2 u |t_c|, v_exp_f32 1 ulp = 2 u: e_c is off by
    (2 + 4 |t_c|) u e_c <= (2 + 1.5) u (x e^-x <= 0.37) — the existing sampler's term with 4 in place of 3.  At most 12
    legal cards: 42 u from the terms, 12 u from each of the two running sums, 3 u from the three operations of u sum:
    below 70 u = 4.2e-6 relative to the sum, so NEAR = 1e-5, the margin of the existing test, stands.  Rows nearer than
    that are left out of the card comparison, at most 1 % of them; the model alone is asserted to leave out no more
    before any kernel output is looked at (about 12 edges x 2e-5 = 0.03 % are expected).

    logp.  The bound of tests/test_gpu_policy_exact.py with the same two terms: u (16 + 4 (|t_a| + sum_c p_c |t_c|) +
    4 |logp|), plus 2 u for the mode's mixture (one division e / k, one fused multiply-add; 1 - e is exact) although e is
    0 here: u (18 + 4 (...) + 4 |logp|) + 1e-9.  For a card at t = -10 drawn at p = e^-10: 6e-8 x (18 + 40 + 4 + 40) =
    6.1e-6; every bound here is asserted to be below 1e-4."""
    import torch
    env, kr, pos = positions
    logits_h, masks_h, played_h, words_h = hand_built(N, 7)
    keys0 = PM.keys_of(SEED, 0, np.zeros(N, np.int64))
    row = torch.from_numpy(np.random.RandomState(8).randn(64) * 2).to(torch.bfloat16).float()
    models = [PM.play_mode(p["logits"], p["masks"], p["played"], p["keys"], temperature, 0.0) for p in pos]
    models_b = [PM.play_mode(p["logits_bf16"], p["masks"], p["played"], p["keys"], temperature, 0.0) for p in pos]
    mh = PM.play_mode(logits_h.float().numpy(), masks_h, played_h, keys0, temperature, 0.0)
    mr = PM.play_mode(row.numpy()[None, :].repeat(N, 0), masks_h, played_h, keys0, temperature, 0.0)
    # the model alone: how many rows the margin leaves out, and the size of the bounds
    total = sum(len(m["card"]) for m in models + models_b) + 3 * N
    near = sum(int((m["margin"] < NEAR).sum()) for m in models + models_b) + int((mh["margin"] < NEAR).sum()) + 2 * int((mr["margin"] < NEAR).sum())
    assert near <= 0.01 * total, (near, total)
    assert max(float(m["tol"].max()) for m in models + models_b + [mh, mr]) < 1e-4
    left = 0
    for j, (p, m, mb) in enumerate(zip(pos, models, models_b)):
        g = p["got"][(temperature, 0.0)]
        assert (g["v"] == p["value"]).all()
        left += check_tempered(m, g["a"], g["lp"], "tarok_policy_mlp, set R, position %d, T = %g" % (j, temperature))[0]
        left += check_tempered(mb, g["a2"], g["lp2"], "tarok_sample_policy, set R as bf16, position %d, T = %g" % (j, temperature))[0]
    # hand-built rows: the env's keys are those of episode 0 only on a fresh env
    fresh = T.TarokVecEnv(N, seed=SEED, mix=T.karte.MIX_ALL)
    set_mode(fresh, temperature, 0.0)
    fresh.reset()
    assert (fresh.counters()[0] == 0).all()
    w = dev_words(words_h)
    a, lp = fresh.sample_policy(logits_h.cuda().contiguous(), w)
    left += check_tempered(mh, a, lp, "tarok_sample_policy, random logits, T = %g" % temperature)[0]
    a, lp = fresh.sample_policy(row.to(torch.bfloat16).repeat(N, 1).cuda().contiguous(), w)
    left += check_tempered(mr, a, lp, "tarok_sample_policy, one random row, T = %g" % temperature)[0]
    a, lp, _ = fresh.policy_mlp(_zero_net(T, row), w)
    left += check_tempered(mr, a, lp, "tarok_policy_mlp, one random row, T = %g" % temperature)[0]
    fresh.close()
    assert left == near


def test_epsilon_one_is_the_bot(T, positions):
    """(0, 1): every row's card is tarok_step_random's on a twin env at the same position (and the model's), and logp is
    log(1 / k) within one rounding of the division and one ulp of the logarithm."""
    K = T.karte
    env, kr, pos = positions
    twin = T.TarokVecEnv(N, seed=SEED, mix=K.MIX_ALL)
    twin.reset()
    at, cards = {}, {}
    for step in range(max(LEADS) + 1):                                   # the twin walks the same lock-steps: its card at each position
        at[step] = twin.legal_actions().words.clone()
        twin.step_random(auto_reset=True)
        cards[step] = twin.action.cpu().numpy().copy()
    twin.close()
    for lead, p in zip(LEADS, pos):
        assert (at[lead] == p["words"]).all().item()
        bot = cards[lead]
        m = PM.play_mode(p["logits"], p["masks"], p["played"], p["keys"], 0.0, 1.0)
        assert (m["card"] == bot).all() and m["explored"].all()
        g = p["got"][(0.0, 1.0)]
        for name, aa, ll in (("tarok_policy_mlp", g["a"], g["lp"]), ("tarok_sample_policy", g["a2"], g["lp2"])):
            assert (aa.numpy() == bot).all(), name
            want = -np.log(m["k"].astype(np.float64))
            assert (np.abs(ll.numpy() - want) <= U + np.spacing(np.abs(want).astype(np.float32))).all(), name
        assert (g["v"] == p["value"]).all()


@pytest.mark.parametrize("temperature", [0.0, 1.0])
def test_epsilon_quarter(T, positions, temperature):
    """(0, 0.25) and (1, 0.25): the coin is integer-exact, so the card is the model's on every row — the Bot's where the
    game explores, the arg-max or the draw elsewhere — and logp is the mixture's log((1 - e) p_T(card) + e / k) within the
    bound of test_temperature.  Both samplers."""
    env, kr, pos = positions
    explored = rows = 0
    for p in pos:
        m = PM.play_mode(p["logits"], p["masks"], p["played"], p["keys"], temperature, 0.25)
        mb = PM.play_mode(p["logits_bf16"], p["masks"], p["played"], p["keys"], temperature, 0.25)
        g = p["got"][(temperature, 0.25)]
        for name, mm, aa, ll in (("tarok_policy_mlp", m, g["a"], g["lp"]), ("tarok_sample_policy", mb, g["a2"], g["lp2"])):
            assert (aa.numpy() == mm["card"]).all(), (name, int((mm["margin"] < NEAR).sum()))
            err = np.abs(ll.numpy().astype(np.float64) - mm["logp"])
            print("%s, (%g, 0.25): max |logp - float64| = %.3g (bound %.3g)" % (name, temperature, err.max(), mm["tol"].max()))
            assert mm["tol"].max() < 1e-4 and (err <= mm["tol"]).all(), (name, float(err.max()))
        assert (g["v"] == p["value"]).all()
        explored += int(m["explored"].sum()); rows += len(m["card"])
        assert (m["explored"] == mb["explored"]).all()
    assert 0.18 * rows < explored < 0.32 * rows                      # (1800 rows: 0.25 +- 6 sigma)


def test_all_five_launches_agree(T):
    """Under (0, 0.25), for 8 lock-steps with auto-reset on four envs of the same seed: tarok_policy_step,
    tarok_policy_step_seats (seats = 15, and a per-game set) and tarok_policy_step_versus (a per-game set, two networks)
    write the card, logp and value of a tarok_policy_mlp launch with the mover's network on the same observation words,
    bit for bit (a Bot seat: the oracle's Bot card and logp 0); and the env half — next observation word, done, reward —
    follows from that card through tests/oracle_model.py for every slot."""
    import torch
    from oracle_model import SlotModel
    K = T.karte
    A = kernel_weights(T, weights_r(1))
    B = kernel_weights(T, weights_r(5))
    per_h = ((np.arange(N) * 7 + 3) % 16).astype(np.uint8)
    per = torch.from_numpy(per_h).cuda()
    kinds = (("step", {}), ("seats15", dict(seats=15)), ("seats_per_game", dict(seats_per_game=per)),
             ("versus", dict(seats_per_game=per, opponent=B)))
    seen = dict(net=0, bot=0, b=0, done=0, explored=0)
    for name, kw in kinds:
        env = T.TarokVecEnv(N, seed=SEED + 2, mix=K.MIX_ALL)
        set_mode(env, 0.0, 0.25)
        models = [SlotModel(SEED + 2, i, K.MIX_ALL) for i in range(N)]
        obs = env.reset()
        for _ in range(2):
            obs, _, _ = env.step_random(auto_reset=True)
            for m in models:
                m.card(None, True)
        z = lambda dt, *s: torch.full(s, 77, dtype=dt, device="cuda")
        words = [obs.words.clone(), z(torch.int64, N)]
        for t in range(8):
            w_in, w_out = words[t & 1], words[(t + 1) & 1]
            fa, fb = z(torch.int64, N, 4), z(torch.int64, N, 4)
            ea = [x.cpu().numpy() for x in env.policy_mlp(A, w_in, feature_words_out=fa)]
            eb = [x.cpu().numpy() for x in env.policy_mlp(B, w_in)]
            act, lp, val, fw = z(torch.uint8, N), z(torch.float32, N), z(torch.float32, N), z(torch.int64, N, 4)
            rew, dn = z(torch.int16, N, 4), z(torch.uint8, N)
            env.policy_step(A, w_in, w_out, act, lp, val, feature_words_out=fw, reward_out=rew, done_out=dn, **kw)
            act_h, lp_h, val_h, rew_h, dn_h, out_h = act.cpu().numpy(), bits(lp), bits(val), rew.cpu().numpy(), dn.cpu().numpy(), _u64(w_out)
            assert torch.equal(fw, fa), (name, t)
            w_h = _u64(w_in)
            pm = PM.play_mode(np.zeros((N, 64), np.float32), w_h & MASK54, _played(w_h), [m.key for m in models], 0.0, 0.25)
            for i, m in enumerate(models):
                assert m.legal() == int(w_h[i] & MASK54) != 0
                in_set = True if name in ("step", "seats15") else bool((int(per_h[i]) >> m.g.seat()) & 1)
                if in_set or name == "versus":
                    e = ea if in_set else eb
                    want = (int(e[0][i]), e[1][i:i + 1].view(np.uint32)[0], e[2][i:i + 1].view(np.uint32)[0])
                    row = m.card(want[0], True)
                    seen["net"] += 1; seen["b"] += not in_set; seen["explored"] += bool(pm["explored"][i])
                    if pm["explored"][i]:
                        assert want[0] == pm["bot"][i], (name, t, i)
                else:
                    row = m.card(None, True)
                    want = (row.action, 0, ea[2][i:i + 1].view(np.uint32)[0])
                    seen["bot"] += 1
                assert (int(act_h[i]), lp_h[i], val_h[i]) == want, (name, t, i)
                assert not row.rejected and int(out_h[i]) == row.obs and int(dn_h[i]) == row.done, (name, t, i)
                if row.done:
                    assert rew_h[i].tolist() == list(row.reward), (name, t, i)
                    seen["done"] += 1
        env.close()
    assert min(seen.values()) > 0, seen


EVAL = dict(n_games=256, episodes=1, seed=12)


def test_greedy_evaluation_replays_on_the_oracle(T):
    """evaluate_vs_bot(..., temperature=0) on 256 games x 1 episode, inspected: every pass's scores are the oracle replay
    of its recorded actions from its recorded start (the Bot's cards the oracle's own), pass 0's scores are those of a
    (1, 0) evaluation, and two calls return identical dicts.  evaluate_vs_policy of a network against itself returns
    advantage exactly 0.0 at (0, 0) and at (0, 0.25)."""
    from oracle_model import SlotModel
    from tarok_amd import evaluate as EV
    K = T.karte
    W = kernel_weights(T, weights_r())
    n = EVAL["n_games"]
    rec, rec1 = [], []
    scores = EV._play_passes_mode(W, n, 1, EVAL["seed"], K.MIX_BOT, 0, inspect=rec, temperature=0.0)
    scores1 = EV._play_passes_mode(W, n, 1, EVAL["seed"], K.MIX_BOT, 0, inspect=rec1)
    result = EV.evaluate_vs_bot(W, n, 1, seed=EVAL["seed"], temperature=0)
    assert result == EV.duplicate_advantage(scores) == EV.evaluate_vs_bot(W, n, 1, seed=EVAL["seed"], temperature=0)
    assert (scores[0] == scores1[0]).all() and (rec[0]["actions"] == rec1[0]["actions"]).all()
    assert any((a["actions"] != b["actions"]).any() for a, b in zip(rec[1:], rec1[1:]))      # greedy did play other cards
    network_cards = 0
    for r in rec:
        for i in range(n):
            m = SlotModel(EVAL["seed"], i, K.MIX_BOT, episode=0)
            assert (r["start"][:, i] == m.g.lanes()).all()
            for t in range(48):
                legal, a = m.legal(), int(r["actions"][t, i])
                if legal and (r["seats"] >> m.g.seat()) & 1:
                    assert a < 54 and (legal >> a) & 1
                    m.card(a)
                    network_cards += 1
                else:
                    assert m.card(None).action == a
            assert list(r["scores"][i]) == m.sum
    assert network_cards > 0
    for eps in (0.0, 0.25):
        assert EV.evaluate_vs_policy(W, W, n, 1, seed=EVAL["seed"], temperature=0, epsilon=eps)["advantage"] == 0.0
