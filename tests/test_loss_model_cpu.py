"""The model behind tests/test_gpu_loss_exact.py, checked without a GPU (tests/loss_model.py):
  * the hand-written float64 loss gradient equals float64 torch autograd of the loss as tests/test_gpu_parity.py states it;
  * a float32 restatement of the kernel's order of operations (f32_loss below: max, exp2(z log2 e), sum, log, p = e (1 / sum),
    log p = z - log sum, the gradient, the bf16 store) stays inside loss_bound in every mode, and a float32 GEMM whose terms
    are added in a shuffled order stays inside gemm_bound: the bounds' derivations hold for an honest evaluation;
  * eight mutants of the restatement are each reported by the comparator — and the three that touch the entropy gradient
    pass the criterion the older tests use (largest error < 1 % of the largest entry), which is the gap the new tests close;
  * the case sets of the seeds the GPU tests use meet their conditions.
"""
import numpy as np
import pytest

import loss_model as L
from policy_exact_ref import reference, synthetic_features, weights_p, weights_r

SEEDS = ((333, 17), (257, 18))            # (n, seed) of the case sets of tests/test_gpu_loss_exact.py
F = np.float32
LOG2E = F(1.4426950408889634)


def bf16(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def random_logits(n, seed):
    """float32 numbers (the kernels' logits are float32): sd 3, a fifth of the rows two and a half times as wide."""
    rnd = np.random.RandomState(seed)
    wide = np.where(rnd.rand(n, 1) < 0.2, 2.5, 1.0)
    return (rnd.randn(n, 64) * 3 * wide).astype(np.float32).astype(np.float64)


def f32_exp(x):
    """__expf: exp2 of the float32 product with log2 e."""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp2((x.astype(F) * LOG2E).astype(F)).astype(F)


def fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 numbers is exact in float64, so only the sum rounds — to float64
    and then to float32, which differs from fmaf's single rounding on about 2^-29 of all inputs (a tie after the first)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def f32_loss(logits, legal, act, logp_old, A, ret, scale, clip, vf, ent, mutant=0):
    """The loss phase of k_learn_chain in numpy float32, all 64 outputs of a sample at once; returns the bf16 output as
    float64 [n,64].  mutant 1..6, 8: the wrong kernels of test_the_comparator_reports_every_mutant."""
    n = logits.shape[0]
    rows = np.arange(n)
    l = logits.astype(F)
    assert (l.astype(np.float64) == logits).all()
    m = np.zeros((n, 64), bool)
    m[:, :54] = legal
    if mutant == 6:                                              # the h = 1 lanes (outputs o % 8 >= 4) read the next nibble
        full = m.copy()
        for o in range(64):
            if o % 8 >= 4:
                m[:, o] = full[:, o + 4] if o + 4 < 64 else False
    w = np.where(m.any(1), scale, 0.0).astype(F)
    m[~m.any(1), 0] = True                                       # nothing to play: m = 1, weight 0
    act = np.where(np.asarray(act).astype(np.int64) < 54, act, 53).astype(np.int64)
    value = l[:, 54]
    lm = np.where(m, l, F(-1.0e30))
    z = lm - lm.max(1)[:, None]
    e = f32_exp(z)
    s = e.sum(1, dtype=F)
    ls, inv = np.log(s).astype(F), F(1.0) / s
    p = e * inv[:, None]
    lp = z - ls[:, None]
    H = -(p * lp).sum(1, dtype=F)
    la = lp[rows, act]
    ratio = f32_exp(la - logp_old.astype(F))
    Af = A.astype(F)
    assert (Af.astype(np.float64) == A).all()
    lo, hi = F(1.0) - F(clip), F(1.0) + F(clip)
    s1, s2 = ratio * Af, np.minimum(np.maximum(ratio, lo), hi) * Af
    keep = (s1 <= s2) | ((ratio > lo) & (ratio < hi))
    g = np.where(keep | (mutant == 4), -Af * ratio, F(0.0)).astype(F)
    dv = value - ret.astype(F)
    gw, ew = g * w, F(ent) * w
    dval = w * F(vf) * (F(1.0) if mutant == 8 else F(2.0)) * dv
    delta = np.zeros((n, 64), F)
    delta[rows, act + (1 if mutant == 5 else 0)] = 1
    t = delta - p
    with np.errstate(over="ignore", invalid="ignore"):
        if mutant == 1:
            d = gw[:, None] * t - ew[:, None] * p * (lp + H[:, None])
        elif mutant == 2:
            d = gw[:, None] * t + ew[:, None] * p * lp
        elif mutant == 3:
            d = gw[:, None] * t
        else:
            # the kernel's written-out order (tarok_learner.inc, "ONE ROUNDING SEQUENCE"): e = (ew p)(log p + H) rounds twice,
            # then fma(gw, t, e) — but gw t + e with both products rounded in output 50 and fma(ew p, log p + H, gw t) in 51
            ep, lh = (ew[:, None] * p).astype(F), (lp + H[:, None]).astype(F)
            e_, gt = (ep * lh).astype(F), (gw[:, None] * t).astype(F)
            d = fma32(np.broadcast_to(gw[:, None], t.shape), t, e_)
            d[:, 50] = (gt + e_).astype(F)[:, 50]
            d[:, 51] = fma32(ep, lh, gt)[:, 51]
    d = d.astype(F)
    d[:, 54] = dval
    assert np.isfinite(d).all()
    return bf16(d)


def f32_gemm(inp, W, mask, seed, mutant=0):
    """(inp @ W) . mask with float32 accumulation, the K terms added in a shuffled order (another one per call), then the
    bf16 store.  mutant 7: the ReLU mask of the neighbouring sample."""
    inp, W = inp.astype(F), W.astype(F)
    acc = np.zeros((inp.shape[0], W.shape[1]), F)
    for k in np.random.RandomState(seed).permutation(inp.shape[1]):
        acc = (acc + inp[:, k, None] * W[None, k, :]).astype(F)
    if mutant == 7:
        mask = np.roll(mask, 1, axis=0)
    return bf16(acc * mask)


def case_set(n, seed, mode):
    cases = L.build_cases(n, seed, mode)
    logits = random_logits(n, seed + 100)
    logp_old, ref = L.finish_cases(cases, logits)
    return cases, logits, logp_old, ref


def run_f32(cases, logits, logp_old, ref, scale, mutant=0):
    clip, vf, ent = L.MODES[cases["mode"]]
    return f32_loss(logits, cases["legal"], cases["card"], logp_old, cases["A"], cases["ret"], scale, clip, vf, ent, mutant)


@pytest.mark.parametrize("n,seed", SEEDS)
def test_case_sets_meet_their_conditions(n, seed):
    for mode in L.MODES:
        cases, logits, logp_old, ref = case_set(n, seed, mode)
        L.check_cases(cases, ref)
        rec = L.records(cases, logp_old)
        bits = rec[:, 3].view(np.uint32)
        assert ((bits & 255) == cases["card"]).all() and (((bits >> 8) & 1) == cases["known"]).all()


@pytest.mark.parametrize("mode", list(L.MODES))
def test_reference_is_the_stated_loss(mode):
    """loss_reference's hand-written gradient against float64 autograd of the loss of test_ppo_loss_kernel_vs_torch
    (masked log_softmax, min / clamp, entropy), weighted by w / wsum: 1e-12 relative, in each isolated mode (every part at
    its own scale) and in the mixed one; and the three means."""
    import torch
    import torch.nn.functional as Fn
    cases, logits, logp_old, ref = case_set(333, SEEDS[0][1], mode)
    clip, vf, ent = L.MODES[mode]
    legal = torch.from_numpy(cases["legal"])
    act = torch.from_numpy(ref["act"])
    w = torch.from_numpy(ref["w"])
    x = torch.from_numpy(logits).requires_grad_(True)
    lg = x[:, :54].masked_fill(~legal, float("-inf"))
    live = legal.any(1)
    lg = torch.where(live[:, None], lg, torch.zeros_like(lg))            # (rows without a card: weight 0, finite arithmetic)
    logp_all = Fn.log_softmax(lg, dim=-1)
    logp = logp_all.gather(-1, act[:, None]).squeeze(-1)
    wsum = w.sum().clamp(min=1)
    ratio = (logp - torch.from_numpy(logp_old).double()).exp()
    adv, ret = torch.from_numpy(cases["A"]), torch.from_numpy(cases["ret"])
    pi = -(torch.min(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv) * w).sum() / wsum
    v = (((x[:, 54] - ret) ** 2) * w).sum() / wsum
    p = logp_all.exp()
    H = (-(p * torch.where(legal, logp_all, torch.zeros_like(logp_all))).sum(-1) * w).sum() / wsum
    (pi + vf * v - ent * H).backward()
    want = x.grad.numpy()
    means, ws = L.loss_means(ref)
    assert ws == wsum.item()
    got = (ref["w"] / ws)[:, None] * L.loss_gradient(ref)
    assert np.abs(want).max() > 0
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max()), np.abs(got - want).max()
    assert np.allclose(means, [pi.item(), v.item(), H.item()], rtol=1e-12, atol=1e-15)
    # the parts add up the way the callers are told
    parts = {"policy": ref["d_policy"], "entropy": -ref["d_entropy"], "value": ref["d_value"]}
    if mode in parts:
        assert np.array_equal(L.loss_gradient(ref), parts[mode])


@pytest.mark.parametrize("n,seed", SEEDS)
@pytest.mark.parametrize("mode", list(L.MODES))
def test_float32_restatement_stays_inside_loss_bound(n, seed, mode):
    """Both scalings (w: the chain; w / wsum: tarok_ppo_loss).  Prints the largest error / bound it saw (-s)."""
    cases, logits, logp_old, ref = case_set(n, seed, mode)
    part = L.loss_gradient(ref)
    _, wsum = L.loss_means(ref)
    for name, scale in (("w", ref["w"]), ("w / wsum", (ref["w"].astype(F) * F(1.0 / wsum)).astype(np.float64))):
        got = run_f32(cases, logits, logp_old, ref, scale)
        worst, msgs = L.violations(got, scale[:, None] * part, L.loss_bound(ref, part, scale), "float32 restatement, %s, %s" % (mode, name))
        print("float32 restatement, n = %d, %s, scale %s: largest error / bound %.3f" % (n, mode, name, worst))
        assert not msgs, "\n".join(msgs)


def _gemm_inputs():
    """dOut of the float32 restatement (mixed mode) on set R's logits, and the two backward products of the chain."""
    n, seed = SEEDS[0]
    cases = L.build_cases(n, seed, "mixed")
    W = weights_r()
    x = L.features_with_masks(synthetic_features(n, seed).numpy(), cases["legal"])
    import torch
    r = reference(torch.from_numpy(x), W)
    logits = r["out"].numpy()
    logp_old, ref = L.finish_cases(cases, logits)
    dout = run_f32(cases, logits, logp_old, ref, ref["w"])
    m2, m1 = r["h2"].numpy() > 0, r["h1"].numpy() > 0
    return dout, W[4].numpy(), m2, W[2].numpy(), m1


def test_shuffled_float32_gemm_stays_inside_gemm_bound_and_a_neighbours_mask_does_not():
    """dH2 = (dOut W3) . (H2 > 0), K = 64, and dH1 = (dH2 W2) . (H1 > 0), K = 256, each from the bf16 output of the stage
    before, in float32 with the terms in a shuffled order: inside gemm_bound.  Mutant 7 (the ReLU mask of the neighbouring
    sample) is reported at both stages."""
    dout, W3, m2, W2, m1 = _gemm_inputs()
    dh2 = f32_gemm(dout, W3, m2, 1)
    for name, inp, Wl, K, mask, got in (("dH2", dout, W3, 64, m2, dh2), ("dH1", dh2, W2, 256, m1, f32_gemm(dh2, W2, m1, 2))):
        want, bound = L.gemm_reference(inp, Wl, mask), L.gemm_bound(inp, Wl, K, mask)
        assert (bound[~mask] == 0).all() and (bound[mask & (want != 0)] > 0).all()
        worst, msgs = L.violations(got, want, bound, name)
        print("float32 GEMM, %s: largest error / bound %.3f" % (name, worst))
        assert not msgs, "\n".join(msgs)
        assert 0.2 < mask.mean() < 0.8 and (mask != np.roll(mask, 1, axis=0)).mean() > 0.1
        worst, msgs = L.violations(f32_gemm(inp, Wl, mask, 3, mutant=7), want, bound, name + ", mutant 7")
        assert msgs and worst > 1


MUTANTS = {1: ("entropy term sign flipped", ("entropy", "mixed")),
           2: ("log p in place of log p + H", ("entropy", "mixed")),
           3: ("entropy term dropped", ("entropy", "mixed")),
           4: ("g not zeroed when clipped", ("policy", "mixed")),
           5: ("delta on the card after the played one", ("policy", "mixed")),
           6: ("legal bits of the h = 1 lanes shifted by one nibble", ("policy", "entropy", "mixed")),
           8: ("value gradient without the factor 2", ("value", "mixed"))}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_comparator_reports_every_mutant(mutant):
    """Each wrong kernel, applied to the float32 restatement, lands outside loss_bound — in the isolated mode of the term it
    breaks and in the mixed mode (0.2, 0.5, 0.01) the learner runs.  Mutants 1-3 (the entropy gradient) at ent = 0.01 PASS
    the older criterion, err.max() < 0.01 max |want|: nothing in the suite saw them before."""
    n, seed = SEEDS[0]
    name, modes = MUTANTS[mutant]
    for mode in modes:
        cases, logits, logp_old, ref = case_set(n, seed, mode)
        part = L.loss_gradient(ref)
        scale = ref["w"]
        want, bound = scale[:, None] * part, L.loss_bound(ref, part, scale)
        got = run_f32(cases, logits, logp_old, ref, scale, mutant)
        worst, msgs = L.violations(got, want, bound, "%s, %s" % (name, mode))
        assert msgs and worst > 1, (name, mode)
        if mode == "mixed" and mutant in (1, 2, 3):
            err = np.abs(got - want).max()
            assert 0 < err < 0.01 * np.abs(want).max(), (name, err, np.abs(want).max())
            good = np.abs(run_f32(cases, logits, logp_old, ref, scale) - want).max()
            assert good < 0.01 * np.abs(want).max()
