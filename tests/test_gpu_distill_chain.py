"""GPU: the distillation term of the fused chain (tarok_learn_chain_distill) element by element against
tests/distill_model.py, on the hand-made samples, weight sets and configurations of tests/test_gpu_loss_exact.py: the
logits are exact, so dOut is judged against scale_i (d_policy + vf d_value - ent d_entropy + coef d_distill) under
distill_bound, and everything the term does not touch — H1, H2, terms_out — must equal a plain tarok_learn_chain launch.

Run on the GPU box:  python -m pytest tests/test_gpu_distill_chain.py -m gpu -q -s
"""
import numpy as np
import pytest

import distill_model as DM
import loss_model as L
from gpu_harness import T  # noqa: F401  (the module fixture)
from learner_cases import CONFIGS, M, SEED, SENTINEL_BF16, SENTINEL_WORD, SETS, Learner, features, forward_of, subset_reference

pytestmark = pytest.mark.gpu
COEF = 0.75
KINDS = ("onehot", "uniform", "random", "zero")


def chain_distill(learner, B, words, idx, rec, stats, mode, target, coef, running=None):
    """One tarok_learn_chain_distill launch: Learner.chain's dict and `distill` [2], raw dOut words for byte comparisons."""
    import torch
    K = learner.K
    clip, vf, ent = L.MODES[mode]
    act_t = lambda k: torch.zeros((B + K.LEARN_PAD, k), dtype=torch.bfloat16, device="cuda")
    arr = dict(H1=act_t(256), H2=act_t(256), dH2=act_t(256), dH1=act_t(256), dOut=act_t(64))
    for t_ in arr.values():
        t_[B:].view(torch.int16).fill_(SENTINEL_BF16)
    Xw = torch.zeros((B + K.LEARN_PAD, 4), dtype=torch.int64, device="cuda")
    Xw[B:] = SENTINEL_WORD
    blocks = (B + 95) // 96
    scratch, terms = torch.empty((blocks, 4), device="cuda"), torch.empty(4, device="cuda")
    dscratch, dterms = torch.full((blocks, 2), float("nan"), device="cuda"), torch.full((2,), float("nan"), device="cuda")
    learner.env.learn_chain_distill(B, words, idx, rec, stats, clip, vf, ent, learner.wf, learner.bias, Xw, arr["H1"], arr["H2"],
                                    arr["dOut"], arr["dH2"], arr["dH1"], scratch, terms, None, target, coef, dscratch, dterms, running)
    torch.cuda.synchronize()
    out = {k: v[:B].double().cpu().numpy() for k, v in arr.items()}
    out["raw"] = {k: v[:B].view(torch.int16).cpu().numpy() for k, v in arr.items()}
    out["pads"] = {k: bool((v[B:].view(torch.int16) == SENTINEL_BF16).all().item()) for k, v in arr.items()}
    out["pads"]["Xw"] = bool((Xw[B:] == SENTINEL_WORD).all().item())
    out["terms"], out["distill"] = terms.cpu().numpy(), dterms.cpu().numpy()
    return out


def test_distill_term_element_by_element(T):
    import torch
    x, masks = features(M, SEED)
    words = torch.from_numpy(L.pack_feature_words(x)).cuda().contiguous()
    rnd = np.random.RandomState(SEED)
    index = {B: rnd.permutation(M)[:B] for B, _ in CONFIGS}
    mode = "mixed"
    clip, vf, ent = L.MODES[mode]
    cases = L.build_cases(M, SEED, mode)
    assert (cases["kind"][cases["known"]] == "one").sum() >= 16                       # forced plays among the weighted rows
    targets = {k: DM.target_rows(cases["legal"], k, seed=7) for k in KINDS}
    worst, worst_means, fails, launches = 0.0, 0.0, [], 0
    for name in SETS[:2]:                                                            # set R and one set P
        W, r = forward_of(name, x)
        logits = r["out"].numpy()
        logp_old, ref_all = L.finish_cases(cases, logits)
        L.check_cases(cases, ref_all)
        rec = torch.from_numpy(L.records(cases, logp_old)).cuda().contiguous()
        stats = torch.from_numpy(cases["stats"]).cuda()
        learner = Learner(T, W)
        for B, indexed in CONFIGS:
            rows = index[B] if indexed else np.arange(B)
            idx = torch.from_numpy(rows).cuda().contiguous() if indexed else None
            what0 = "set %s, B = %d, %s" % (name, B, "through an index" if indexed else "index NULL")
            plain = learner.chain(B, words, idx, rec, stats, mode)
            # its dOut as 16-bit words (the float64 copy of a bf16 number converts back exactly, the sign of a zero included)
            plain_raw = torch.from_numpy(plain["dOut"]).to(torch.bfloat16).view(torch.int16).numpy()
            ref = subset_reference(cases, logits, logp_old, rows)
            dead = ref["w"] == 0
            for kind in KINDS:
                q = targets[kind]
                tdev = lambda a: torch.from_numpy(a).to(torch.bfloat16).cuda().contiguous()
                got = chain_distill(learner, B, words, idx, rec, stats, mode, tdev(q), COEF)
                launches += 1
                what = "%s, %s rows" % (what0, kind)
                assert all(got["pads"].values()), (what, got["pads"])
                for k in ("H1", "H2"):
                    assert np.array_equal(got[k], plain[k]), (what, k)
                assert np.array_equal(got["terms"].view(np.uint32), plain["terms"].view(np.uint32)), what
                assert np.array_equal(got["raw"]["dOut"][dead], plain_raw[dead]), what + ": dOut of a row of weight 0 is not the no-teacher dOut"
                d = DM.distill_reference(ref, q[rows])
                part = DM.distill_gradient(d, COEF)
                ratio, msgs = L.violations(got["dOut"], d["w"][:, None] * part, DM.distill_bound(d, part, d["w"], COEF), "dOut, " + what)
                worst = max(worst, ratio)
                fails += msgs
                means, _ = DM.distill_means(d)
                mb = DM.distill_means_bound(d)
                merr = np.abs(got["distill"].astype(np.float64) - means)
                worst_means = max(worst_means, float((merr / mb).max()))
                if not (merr <= mb).all():
                    fails.append("distill_out, %s: kernel %r, reference %r, bound %r" % (what, got["distill"], means, mb))
                if kind == "zero":
                    assert np.array_equal(got["raw"]["dOut"], plain_raw) and (got["distill"] == 0).all(), what
                if kind == "random":
                    # NaN in every column the term must not look at changes no byte; a second launch gives the same bytes;
                    # coef = 0 gives the plain launch's dOut; distill_running accumulates
                    again = chain_distill(learner, B, words, idx, rec, stats, mode, tdev(q), COEF)
                    for k in ("H1", "H2", "dOut", "dH2", "dH1"):
                        assert np.array_equal(again["raw"][k], got["raw"][k]), what + ": two launches differ in " + k
                    assert np.array_equal(again["distill"].view(np.uint32), got["distill"].view(np.uint32)), what
                    nan = chain_distill(learner, B, words, idx, rec, stats, mode, tdev(DM.with_nans(q, cases["legal"])), COEF)
                    for k in ("dOut", "dH2", "dH1"):
                        assert np.array_equal(nan["raw"][k], got["raw"][k]), what + ": NaN in an ignored column reached " + k
                    assert np.array_equal(nan["distill"].view(np.uint32), got["distill"].view(np.uint32)), what
                    running = torch.tensor([1.0, 2.0], device="cuda")
                    zero = chain_distill(learner, B, words, idx, rec, stats, mode, tdev(q), 0.0, running)
                    assert np.array_equal(zero["raw"]["dOut"], plain_raw), what + ": coef = 0 changed dOut"
                    assert np.array_equal(zero["distill"].view(np.uint32), got["distill"].view(np.uint32))
                    assert np.array_equal(running.cpu().numpy(), np.array([1.0, 2.0], np.float32) + zero["distill"]), what
        learner.close()
    print("distill dOut: largest error / bound %.3f; distill_out %.3f (%d launches)" % (worst, worst_means, launches))
    assert not fails, "\n".join(fails[:20])
    assert launches == 2 * len(CONFIGS) * len(KINDS)


def test_distill_chain_and_dw_vs_torch_autograd(T):
    """End to end at B = 333 (three tiles plus 45, through an index): tarok_learn_chain_distill + tarok_learn_dw with
    stats = {0, 0} (advantage 0), vf = ent = 0 and coef = 1 against float64 torch autograd of the weighted mean ce on the
    same bf16 weights — the comparison and the tolerances of test_gpu_learner.py's
    test_learn_chain_and_dw_vs_torch_autograd (_chain_vs_autograd), unchanged: dOut 0.01, dH2 0.02, dH1 0.03 of the array's
    largest entry; every weight and bias gradient 0.02 in relative norm and 0.03 of its largest entry."""
    import torch
    import torch.nn.functional as F
    from tarok_amd import selfplay as SP
    from learner_cases import _rollout_words
    K = T.karte
    f64 = torch.float64
    B, n, steps = 333, 2048, 3
    env = T.TarokVecEnv(n, seed=5, mix=K.MIX_ALL)
    torch.manual_seed(1)
    net = SP.PolicyNet(256).cuda()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(2.0)
    ps = [net.fc1.weight, net.fc1.bias, net.fc2.weight, net.fc2.bias, net.head.weight, net.head.bias]
    flat = torch.cat([p.detach().reshape(-1) for p in ps]).contiguous()
    bf = lambda k: torch.empty(k, dtype=torch.bfloat16, device="cuda")
    wf = dict(w1=bf(65536), w2=bf(65536), w3=bf(16384), w3t=bf(16384), w2t=bf(65536))
    env.learn_adam(flat, None, None, None, None, wf, apply=False)
    bias = (flat[K.MLP_B1:K.MLP_B1 + 256], flat[K.MLP_B2:K.MLP_B2 + 256], flat[K.MLP_B3:K.MLP_B3 + 64])
    roll_w = [wf["w1"].view(256, 256), bias[0], wf["w2"].view(256, 256), bias[1], wf["w3"].view(64, 256), bias[2]]
    words, obs_words = _rollout_words(T, env, roll_w, steps)
    M = words.shape[0]
    g = torch.Generator(device="cuda"); g.manual_seed(7)
    idx = torch.randperm(M, device="cuda", generator=g)[:B].contiguous()
    legal_all = SP.legal_matrix(obs_words & K.OBS_MASK)
    act_all = torch.multinomial(legal_all.float(), 1, generator=g).squeeze(1)
    # target rows: a bf16-rounded softmax of random scores over the legal cards, NaN-free junk (0.5) everywhere else
    sc = (2.0 * torch.randn((M, 54), device="cuda", generator=g)).masked_fill(~legal_all, float("-inf"))
    target = torch.full((M, 64), 0.5, device="cuda")
    target[:, :54] = torch.where(legal_all, torch.softmax(sc, -1), torch.full_like(sc, 0.5))
    target = target.to(torch.bfloat16).contiguous()
    Wq = [p.detach().to(torch.bfloat16).to(f64).requires_grad_(True) if p.dim() == 2 else p.detach().to(f64).requires_grad_(True) for p in ps]
    x = env.expand_feature_words(words[idx], f64)
    z1 = x @ Wq[0].T + Wq[1]; z1.retain_grad()
    h1 = torch.relu(z1).to(torch.bfloat16).to(f64)
    z2 = h1 @ Wq[2].T + Wq[3]; z2.retain_grad()
    h2 = torch.relu(z2).to(torch.bfloat16).to(f64)
    out = h2 @ Wq[4].T + Wq[5]; out.retain_grad()
    legal = legal_all[idx]
    rec = torch.zeros((M, 4), device="cuda")
    rec[:, 1] = torch.randn(M, device="cuda", generator=g)
    rec[:, 2] = 0.5 * torch.randn(M, device="cuda", generator=g)
    known = torch.rand(M, device="cuda", generator=g) < 0.8
    rec[:, 3] = (act_all.to(torch.int32) | (known.to(torch.int32) << 8)).view(torch.float32)
    stats = torch.tensor([0.0, 0.0, 0.8, 0.0], device="cuda")
    w = known[idx].to(f64)
    wsum = w.sum().clamp(min=1)
    logp_all = F.log_softmax(out[:, :54].masked_fill(~legal, float("-inf")), dim=-1)
    q = torch.where(legal, target[idx][:, :54].to(f64), torch.zeros_like(logp_all))
    ce = (-(q * torch.where(legal, logp_all, torch.zeros_like(logp_all))).sum(-1) * w).sum() / wsum
    ce.backward()
    act_t = lambda k: torch.zeros((B + K.LEARN_PAD, k), dtype=torch.bfloat16, device="cuda")
    H1, H2, dH2, dH1, dOut = act_t(256), act_t(256), act_t(256), act_t(256), act_t(64)
    blocks = (B + 95) // 96
    scratch, terms = torch.empty((blocks, 4), device="cuda"), torch.empty(4, device="cuda")
    dscratch, dterms = torch.empty((blocks, 2), device="cuda"), torch.empty(2, device="cuda")
    Xw = torch.zeros((B + K.LEARN_PAD, 4), dtype=torch.int64, device="cuda")
    env.learn_chain_distill(B, words, idx, rec, stats, 0.2, 0.0, 0.0, wf, bias, Xw, H1, H2, dOut, dH2, dH1, scratch, terms, None,
                            target, 1.0, dscratch, dterms)
    assert abs(dterms[0].item() - ce.item()) < 5e-3 * abs(ce.item()) + 5e-4, (dterms, ce)
    assert abs(terms[3].item() - 1.0 / wsum.item()) < 1e-9
    for got, want, name, tol in ((dOut, out.grad, "dOut", 0.01), (dH2, z2.grad, "dH2", 0.02), (dH1, z1.grad, "dH1", 0.03)):
        want = want * wsum
        err = (got[:B].to(f64) - want).abs()
        scale = want.abs().max().item()
        print("%s: largest error %.3g of %.3g" % (name, err.max().item(), scale))
        assert err.max().item() < tol * scale + 1e-9, (name, err.max().item(), scale)
    assert (dOut[:B, 54:] == 0).all().item() and (dOut[:B, :54][~legal] == 0).all().item()
    work = torch.empty(env.learn_workspace_bytes(), dtype=torch.uint8, device="cuda")
    grad = torch.zeros(K.MLP_PARAMS, device="cuda")
    env.learn_dw(B, Xw, H1, H2, dOut, dH2, dH1, terms, work, grad)
    off = 0
    for p_, name in zip(Wq, ("W1", "b1", "W2", "b2", "W3", "b3")):
        gk = grad[off:off + p_.numel()].view_as(p_).to(f64)
        off += p_.numel()
        rel = (gk - p_.grad).norm().item() / (p_.grad.norm().item() + 1e-12)
        print("%s: relative error %.3g" % (name, rel))
        assert rel < 0.02, (name, rel)
        assert (gk - p_.grad).abs().max().item() < 0.03 * p_.grad.abs().max().item() + 1e-9, name
    env.close()
