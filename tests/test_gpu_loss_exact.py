"""The link between the exact forward (tests/test_gpu_policy_exact.py) and the exact weight gradients
(tests/test_gpu_learner_sizes.py), element by element: the loss phase of k_learn_chain, its two backward GEMMs with their
ReLU masks, and k_ppo_loss, the same loss on the torch path.

Stage-wise: every stage is compared per element with a float64 reference (tests/loss_model.py) that is fed the kernel's
own, already checked, output of the stage before —
    H1, H2      EQUAL the exact reference (weight sets R and P: the logits are exact float32 / bf16 numbers)
    dOut        within loss_bound of scale_i (d_policy + vf d_value - ent d_entropy) of those exact logits
    dH2, dH1    within gemm_bound of (the kernel's dOut @ W3) . (H2 > 0) and (the kernel's dH2 @ W2) . (H1 > 0)
— on hand-made samples (loss_model.build_cases: every card played, forced plays, one-nibble legal sets, rows without a
card, both sides of the clip range with both signs of the advantage, rows without the known bit).  The bounds come from
bf16 and float32 rounding (derived in loss_model.py, held against a float32 restatement in tests/test_loss_model_cpu.py);
none of them was fitted to what the kernels give.  Every test prints the largest error / bound it saw (run with -s).

    python -m pytest tests/test_gpu_loss_exact.py -m gpu -q
"""
import numpy as np
import pytest

import loss_model as L
from gpu_harness import T  # noqa: F401  (the module fixture)
from policy_exact_ref import synthetic_features
from learner_cases import CONFIGS, M, N2, SEED, SEED2, SETS, Learner, features, forward_of, subset_reference


@pytest.fixture(scope="module")
def chain_runs(T):
    """Every tarok_learn_chain launch the tests below judge, made once: weight sets R and two P x four modes x CONFIGS on
    the M = 333 hand-made samples, each with the float64 reference of its rows."""
    import torch
    x, masks = features(M, SEED)
    words_np = L.pack_feature_words(x)
    words = torch.from_numpy(words_np).cuda().contiguous()
    assert torch.equal(T.TarokVecEnv.expand_feature_words(words, torch.float64).cpu(), torch.from_numpy(x))
    assert ((words_np[:, 1].view(np.uint64) & np.uint64(T.karte.OBS_MASK)) == masks).all()
    rnd = np.random.RandomState(SEED)
    index = {B: rnd.permutation(M)[:B] for B, _ in CONFIGS}
    runs = []
    fwd = {}
    for name in SETS:
        W, r = forward_of(name, x)
        fwd[name] = (W, r)
        logits = r["out"].numpy()
        learner = Learner(T, W)
        for mode in L.MODES:
            cases = L.build_cases(M, SEED, mode)
            assert (cases["masks"] == masks).all()
            logp_old, ref = L.finish_cases(cases, logits)
            L.check_cases(cases, ref)
            rec = torch.from_numpy(L.records(cases, logp_old)).cuda().contiguous()
            stats = torch.from_numpy(cases["stats"]).cuda()
            for B, indexed in CONFIGS:
                rows = index[B] if indexed else np.arange(B)
                idx = torch.from_numpy(rows).cuda().contiguous() if indexed else None
                got = learner.chain(B, words, idx, rec, stats, mode)
                runs.append(dict(set=name, mode=mode, B=B, indexed=indexed, rows=rows, got=got, words=words_np[rows],
                                 ref=subset_reference(cases, logits, logp_old, rows),
                                 what="set %s, %s mode, B = %d, %s" % (name, mode, B, "through an index" if indexed else "index NULL")))
        learner.close()
    return runs, fwd


@pytest.mark.gpu
def test_chain_loss_term_by_term(chain_runs):
    """dOut[:B] of every launch against w (d_policy + vf d_value - ent d_entropy) under loss_bound — policy only, entropy only
    (ent = 1, A = 0), value only (vf = 1, A = 0) and mixed (0.2, 0.5, 0.01).  Beside it: H1 and H2 equal the exact reference,
    the gathered feature words are the rows asked for, the padding rows keep their sentinel, rows without the known bit or
    without a legal card are zero in dOut, dH2 and dH1, terms[0..2] lie within terms_bound (derived there) of the float64
    means and terms[3] == 1 / max(sum w, 1) as a float32."""
    runs, fwd = chain_runs
    worst = {m: 0.0 for m in L.MODES}
    worst_terms = 0.0
    fails = []
    for e in runs:
        got, ref, what = e["got"], e["ref"], e["what"]
        _, r = fwd[e["set"]]
        assert all(got["pads"].values()), (what, got["pads"])
        assert (got["Xw"] == e["words"]).all(), what
        for hn, key in (("H1", "h1"), ("H2", "h2")):
            want = r[key].numpy()[e["rows"]]
            assert np.array_equal(got[hn], want), "%s: %s differs from the exact reference in %d entries" % (what, hn, (got[hn] != want).sum())
        dead = ref["w"] == 0
        assert dead.sum() >= 4 or e["B"] < 96
        for k in ("dOut", "dH2", "dH1"):
            assert (got[k][dead] == 0).all(), "%s: %s of a row of weight 0 is not zero" % (what, k)
        part = L.loss_gradient(ref)
        ratio, msgs = L.violations(got["dOut"], ref["w"][:, None] * part, L.loss_bound(ref, part, ref["w"]), "chain loss (dOut), " + what)
        worst[e["mode"]] = max(worst[e["mode"]], ratio)
        fails += msgs
        means, wsum = L.loss_means(ref)
        tb = L.terms_bound(ref)
        terr = np.abs(got["terms"][:3].astype(np.float64) - means)
        worst_terms = max(worst_terms, float((terr / tb).max()))
        for k in range(3):
            if terr[k] > tb[k]:
                fails.append("chain loss (terms[%d]), %s: kernel %r, reference %r, bound %.3g" % (k, what, got["terms"][k], means[k], tb[k]))
        assert got["terms"][3] == np.float32(1.0 / wsum), (what, got["terms"][3], wsum)
    print("chain loss dOut: largest error / bound per mode %s; terms: %.3f"
          % (", ".join("%s %.3f" % kv for kv in worst.items()), worst_terms))
    assert not fails, "\n".join(fails[:20])
    assert len(runs) == len(SETS) * len(L.MODES) * len(CONFIGS)


@pytest.mark.gpu
def test_chain_backward_gemms_from_the_kernels_own_inputs(chain_runs):
    """In mixed mode (gradients of every sign), for set R (H2 with rounded entries) and two sets P whose W2 permutations put
    different rows into every k-step: dH2[:B] against (the kernel's dOut @ W3) . (H2 > 0) under gemm_bound(K = 64), dH1[:B]
    against (the kernel's dH2 @ W2) . (H1 > 0) under gemm_bound(K = 256), both EQUAL to 0 wherever the mask is 0."""
    runs, fwd = chain_runs
    Wa, Wb = fwd[SETS[1]][0][2].numpy(), fwd[SETS[2]][0][2].numpy()
    for ks in range(16):                                         # the rows whose non-zero lies in k-step ks
        assert set(np.nonzero(Wa[:, 16 * ks:16 * ks + 16])[0]) != set(np.nonzero(Wb[:, 16 * ks:16 * ks + 16])[0])
    worst = dict(dH2=0.0, dH1=0.0)
    fails = []
    judged = 0
    for e in runs:
        if e["mode"] != "mixed":
            continue
        W, r = fwd[e["set"]]
        got = e["got"]
        m2, m1 = r["h2"].numpy()[e["rows"]] > 0, r["h1"].numpy()[e["rows"]] > 0
        assert 0.05 < m2.mean() < 0.95 and 0.05 < m1.mean() < 0.95
        for name, inp, Wl, K, mask in (("dH2", got["dOut"], W[4].numpy(), 64, m2), ("dH1", got["dH2"], W[2].numpy(), 256, m1)):
            assert np.abs(inp).max() > 0
            assert (got[name][~mask] == 0).all(), "%s, %s: not zero where the ReLU mask is 0" % (name, e["what"])
            ratio, msgs = L.violations(got[name], L.gemm_reference(inp, Wl, mask), L.gemm_bound(inp, Wl, K, mask),
                                       "backward GEMM (%s), %s" % (name, e["what"]))
            worst[name] = max(worst[name], ratio)
            fails += msgs
        judged += 1
    print("backward GEMMs: largest error / bound dH2 %.3f, dH1 %.3f" % (worst["dH2"], worst["dH1"]))
    assert not fails, "\n".join(fails[:20])
    assert judged == len(SETS) * len(CONFIGS)


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed", [(M, SEED), (N2, SEED2)])
def test_ppo_loss_term_by_term(T, chain_runs, n, seed):
    """tarok_ppo_loss on the same cases and modes, fed the logits of a set P cast to bf16 (exact: the very numbers the chain
    computed): dout against (w / wsum) part under loss_bound and the three terms under terms_bound, at n = 333 and 257 (a full
    block and one sample).  wsum is the sum of the weights the kernel is GIVEN (a known row without a card counts in it).
    At n = 333 the chain's dOut (B = 333, index NULL) and wsum dout agree within the sum of their two bounds."""
    import torch
    runs, _ = chain_runs
    name = SETS[1]
    x, masks = features(n, seed)
    W, r = forward_of(name, x)
    logits = r["out"].numpy()
    out = r["out"].to(torch.bfloat16)
    assert torch.equal(out.double(), r["out"])
    env = T.TarokVecEnv(256, seed=1)
    worst, worst_terms, worst_pair = 0.0, 0.0, 0.0
    fails = []
    for mode in L.MODES:
        clip, vf, ent = L.MODES[mode]
        cases = L.build_cases(n, seed, mode)
        logp_old, ref = L.finish_cases(cases, logits)
        L.check_cases(cases, ref)
        given = cases["known"].astype(np.float32)
        wsum = max(float(given.sum()), 1.0)
        assert wsum > ref["w"].sum()
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        terms, dout = env.ppo_loss(out.cuda().contiguous(), cuda(masks.view(np.int64)), cuda(cases["card"].astype(np.int64)), cuda(logp_old),
                                   cuda(cases["A"].astype(np.float32)), cuda(cases["ret"].astype(np.float32)), cuda(given), clip, vf, ent)
        torch.cuda.synchronize()
        dout, terms = dout.double().cpu().numpy(), terms.double().cpu().numpy()
        what = "set %s, %s mode, n = %d" % (name, mode, n)
        part = L.loss_gradient(ref)
        scale = ref["w"] / wsum
        bound = L.loss_bound(ref, part, scale)
        ratio, msgs = L.violations(dout, scale[:, None] * part, bound, "tarok_ppo_loss (dout), " + what)
        worst = max(worst, ratio)
        fails += msgs
        means, _ = L.loss_means(ref, wsum)
        tb = L.terms_bound(ref, wsum)
        terr = np.abs(terms - means)
        worst_terms = max(worst_terms, float((terr / tb).max()))
        for k in range(3):
            if terr[k] > tb[k]:
                fails.append("tarok_ppo_loss (terms[%d]), %s: kernel %r, reference %r, bound %.3g" % (k, what, terms[k], means[k], tb[k]))
        if n == M:
            twin = [e for e in runs if e["set"] == name and e["mode"] == mode and e["B"] == M and not e["indexed"]]
            assert len(twin) == 1
            ratio, msgs = L.violations(twin[0]["got"]["dOut"], wsum * dout, L.loss_bound(ref, part, ref["w"]) + wsum * bound,
                                       "chain dOut against wsum x tarok_ppo_loss dout, " + what)
            worst_pair = max(worst_pair, ratio)
            fails += msgs
    env.close()
    print("tarok_ppo_loss, n = %d: largest error / bound dout %.3f, terms %.3f, against the chain %.3f" % (n, worst, worst_terms, worst_pair))
    assert not fails, "\n".join(fails[:20])


@pytest.mark.gpu
def test_played_card_sweep(T):
    """B = 96 (one full tile), every card legal, logits of a set P, sample i plays card i % 54 with an advantage of sign
    (-1)^i and a ratio of 1, policy only.  d loss / d logit = g (delta - p) with g = -A ratio: column act_i is the ONLY entry
    of row i whose sign is that of -A_i (the loss falls when a card with a positive advantage becomes likelier) and the
    largest in magnitude (1 - p_a = the sum of the others); every other entry of the row has the sign of A_i or is zero.
    The whole row is within loss_bound.  A played-card match that is off by a lane, a nibble or a tile moves the odd entry."""
    import torch
    B = 96
    name = SETS[1]
    x = L.features_with_masks(synthetic_features(B, 5).numpy(), np.ones((B, 54), bool))
    W, r = forward_of(name, x)
    logits = r["out"].numpy()
    i = np.arange(B)
    u = np.where(i % 2 == 0, 1.0, -1.0) * (64 + 16 * i) * 2.0 ** -10
    mean, inv_std = L.STATS["policy"]
    val = (i % 17 - 8) / 8.0
    cases = dict(n=B, mode="policy", legal=np.ones((B, 54), bool), card=(i % 54).astype(np.uint8), known=np.ones(B, bool),
                 log_ratio=np.zeros(B), A=u * inv_std, ret=val + mean + u, val=val)
    logp_old, ref = L.finish_cases(cases, logits)
    assert (np.abs(ref["ratio"] - 1) < 1e-6).all() and (ref["g"] != 0).all() and (np.sign(ref["A"]) == np.where(i % 2 == 0, 1, -1)).all()
    want = L.loss_gradient(ref)
    others = np.abs(np.where(np.arange(64)[None, :] == ref["act"][:, None], 0.0, want))
    assert (np.abs(want[i, ref["act"]]) > 1.05 * others.max(1)).all()           # (a condition on the reference: clear of a bf16 tie)
    learner = Learner(T, W)
    words = torch.from_numpy(L.pack_feature_words(x)).cuda().contiguous()
    stats = torch.tensor([mean, inv_std, 1.0, 0.0], device="cuda")
    got = learner.chain(B, words, None, torch.from_numpy(L.records(cases, logp_old)).cuda().contiguous(), stats, "policy")
    learner.close()
    d = got["dOut"]
    what = "played-card sweep (dOut), set %s, policy mode" % name
    for k in range(B):
        odd = np.flatnonzero(np.sign(d[k]) == -np.sign(ref["A"][k]))
        assert odd.tolist() == [ref["act"][k]] and np.abs(d[k]).argmax() == ref["act"][k], \
            "%s: sample %d plays card %d, but the entries against the advantage's sign are %s and the largest is column %d" % (
                what, k, ref["act"][k], odd.tolist(), np.abs(d[k]).argmax())
    ratio, msgs = L.violations(d, want, L.loss_bound(ref, want, ref["w"]), what)
    print("played-card sweep: largest error / bound %.3f" % ratio)
    assert not msgs, "\n".join(msgs)
