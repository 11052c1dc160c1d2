"""The fused learner (tarok_learn_*) at the sizes it runs at: exact probes of the weight-gradient pass over a sweep of
minibatch sizes chosen from its tiling, float64 references of the weight gradients, the returns and Adam at their
edges, and the split of a minibatch past TAROK_LEARN_MAX_BATCH (SelfPlay.update_fused).

The GPU tests are marked `gpu`; the model of k_learn_dw's tiling and its coverage test run anywhere.
Run on the GPU box:  python -m pytest tests/test_gpu_learner_sizes.py -m gpu -q
"""
import os
import re

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- a model of k_learn_dw's work split (tarok_env.hip learn_chunks, tarok_learner.inc dw_chunk / dw_layer)
DW_KT = 32                   # samples per staged tile
DW_ST = 4                    # register stages of a chunk's ring: a chunk of more than DW_ST tiles wraps it
LEARN_MAX_BATCH = 4194048    # TAROK_LEARN_MAX_BATCH


def learn_chunks(n_cus):
    """(chunks of layer 2, layer 1, layer 3): one workgroup per CU, shared 96 : 108 : 52."""
    total = max(8, n_cus)
    c2, c1 = total * 96 // 256, total * 108 // 256
    return c2, c1, total - c2 - c1


def dw_chunk(B, chunks, c):
    """[s0, s1) of chunk c of a layer with `chunks` chunks over B samples."""
    per = (-(-B // chunks) + DW_KT - 1) // DW_KT * DW_KT
    s0 = min(per * c, B)
    return s0, min(s0 + per, B)


def chunk_plan(B, n_cus):
    """{layer: [(s0, s1) of every chunk]} for layers 2, 1, 3."""
    return {layer: [dw_chunk(B, c, k) for k in range(c)] for layer, c in zip((2, 1, 3), learn_chunks(n_cus))}


def plan_features(B, n_cus):
    """The tiling situations minibatch B puts at least one chunk of at least one layer in."""
    f = set()
    for chunks in chunk_plan(B, n_cus).values():
        tiles = [-(-(s1 - s0) // DW_KT) for s0, s1 in chunks]
        if 0 in tiles:
            f.add("empty chunk")
        for k, name in ((1, "1 tile"), (DW_ST - 1, "DW_ST - 1 tiles"), (DW_ST, "DW_ST tiles"), (DW_ST + 1, "DW_ST + 1 tiles"),
                        (2 * DW_ST + 1, "2 DW_ST + 1 tiles")):
            if k in tiles:
                f.add(name)
        s0, s1 = [c for c in chunks if c[1] > c[0]][-1]
        if (s1 - s0) % DW_KT:
            f.add("ragged last chunk")
        if s1 - s0 < DW_KT:
            f.add("last chunk under one tile")
    return f


FEATURES = {"empty chunk", "1 tile", "DW_ST - 1 tiles", "DW_ST tiles", "DW_ST + 1 tiles", "2 DW_ST + 1 tiles",
            "ragged last chunk", "last chunk under one tile"}
# 1 / 31 / 33: a lone partial tile; 5000: 4-tile chunks; 12,289: 4- and 5-tile chunks and a last chunk of 1 row;
# 14,000: 3-, 5- and 9-tile chunks (layer 3: 52 chunks of 288 samples); 393,216 = the bench's minibatch (90 - 237 tiles
# per chunk); 1,000,003: ragged at size; the largest minibatch tarok_learn_dw takes
PROBE_B = [1, 31, 33, 5000, 12289, 14000, 393216, 1000003, LEARN_MAX_BATCH]


def test_the_tiling_model_mirrors_the_kernel_source():
    """The constants and the chunk split the model copies are the ones the library is compiled with."""
    inc = open(os.path.join(ROOT, "tarok_amd", "csrc", "tarok_learner.inc")).read()
    hip = open(os.path.join(ROOT, "tarok_amd", "csrc", "tarok_env.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "tarok_env.h")).read()
    assert int(re.search(r"#define DW_KT (\d+)", inc).group(1)) == DW_KT
    assert int(re.search(r"#define DW_ST (\d+)", inc).group(1)) == DW_ST
    assert int(re.search(r"#define TAROK_LEARN_MAX_BATCH (\d+)", hdr).group(1)) == LEARN_MAX_BATCH
    assert "c2 = total * 96 / 256; c1 = total * 108 / 256; c3 = total - c2 - c1;" in hip
    assert "u32 total = (u32)e->n_cus < 8 ? 8 : (u32)e->n_cus;" in hip
    assert "int64_t per = ((B + chunks - 1) / chunks + DW_KT - 1) / DW_KT * DW_KT;" in inc
    assert "s0 = per * c < B ? per * c : B;" in inc and "s1 = s0 + per < B ? s0 + per : B;" in inc
    for B in (1, 5000, 393216, LEARN_MAX_BATCH):                            # the chunks tile [0, B) in order
        for chunks in chunk_plan(B, 256).values():
            assert chunks[0][0] == 0 and chunks[-1][1] == B
            assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))


def test_the_probe_sizes_cover_the_tiling_edges():
    """On 256 CUs the exact probe's minibatch sizes put some chunk of some layer in every tiling situation that a dropped,
    doubled or leaked tile could hide in — and the large sizes wrap the register ring many times."""
    covered = set().union(*(plan_features(B, 256) for B in PROBE_B))
    assert covered == FEATURES, FEATURES - covered
    longest = max(-(-(s1 - s0) // DW_KT) for ch in chunk_plan(393216, 256).values() for s0, s1 in ch)
    shortest = min(-(-(s1 - s0) // DW_KT) for ch in chunk_plan(393216, 256).values() for s0, s1 in ch)
    assert (shortest, longest) == (90, 237)


# ---- GPU
@pytest.fixture(scope="module")
def env(T):
    e = T.TarokVecEnv(256, seed=1)
    yield e
    e.close()


def _free():
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _integer_minibatch(T, B, seed):
    """Synthetic tarok_learn_dw inputs on which float32 is exact: H1, H2 in {0, 1}, dH2, dH1, dOut in {-2 .. 2}, random
    feature words (layer 1's input: bits).  Every product is an integer and every partial sum is at most 2 B < 2^24 in
    magnitude, so any summation order gives the same, exact float32 result.  The padding rows [B, B + LEARN_PAD) hold NaN
    (all-ones words in Xw): one padding row read anywhere turns some gradient into NaN or moves it by an integer."""
    import torch
    K = T.karte
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    rows = B + K.LEARN_PAD
    a = {}
    for name, width, lo, hi in (("H1", 256, 0, 2), ("H2", 256, 0, 2), ("dOut", 64, -2, 3), ("dH2", 256, -2, 3), ("dH1", 256, -2, 3)):
        t = torch.empty((rows, width), dtype=torch.bfloat16, device="cuda")
        t[:B].random_(0, hi - lo, generator=g)
        t[:B] += lo
        t[B:] = float("nan")
        a[name] = t
    Xw = torch.empty((rows, 4), dtype=torch.int64, device="cuda")
    Xw[:B].view(torch.int32).random_(-2 ** 31, 2 ** 31, generator=g)  # (all 64 bits of every word random)
    Xw[B:] = -1
    a["Xw"] = Xw
    return a


def _integer_reference(T, B, a, rows=1 << 18):
    """dH^T H and the column sums of dH of every layer, in the flat parameter order, in float64 (exact: integers below
    2^53), taken in row chunks.  Layer 1's H: the expanded feature words."""
    import torch
    K = T.karte
    f64 = torch.float64
    ref = torch.zeros(K.MLP_PARAMS, dtype=f64, device="cuda")
    W1, b1 = ref[K.MLP_W1:K.MLP_B1].view(256, 256), ref[K.MLP_B1:K.MLP_W2]
    W2, b2 = ref[K.MLP_W2:K.MLP_B2].view(256, 256), ref[K.MLP_B2:K.MLP_W3]
    W3, b3 = ref[K.MLP_W3:K.MLP_B3].view(64, 256), ref[K.MLP_B3:]
    for r0 in range(0, B, rows):
        r1 = min(B, r0 + rows)
        X = T.TarokVecEnv.expand_feature_words(a["Xw"][r0:r1], f64)
        for W, b, dH, H in ((W1, b1, a["dH1"], X), (W2, b2, a["dH2"], a["H1"][r0:r1]), (W3, b3, a["dOut"], a["H2"][r0:r1])):
            d = dH[r0:r1].to(f64)
            W += d.T @ H.to(f64)
            b += d.sum(0)
        del X, d
    assert ref.abs().max().item() < 2 ** 24
    return ref.float()


@pytest.mark.gpu
@pytest.mark.parametrize("B", PROBE_B)
def test_learn_dw_is_exact_on_integer_inputs(T, env, B):
    """tarok_learn_dw + k_learn_reduce on _integer_minibatch give EXACTLY dH^T H and the column sums of dH of all three
    layers (terms = {0, 0, 0, 1}): a sample dropped or counted twice anywhere — a tile, a chunk boundary, a register
    stage of the ring — changes some entry by an integer; a padding row read makes it NaN.  The sizes come from the
    model above, which is checked to be the library's at this device's CU count.  At the bench's minibatch the launch is
    also repeated (bit-identical: fixed summation order), and at the largest one the first size past the limit is refused
    before anything runs."""
    import torch
    K = T.karte
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    c2, c1, c3 = learn_chunks(n_cus)
    assert env.learn_workspace_bytes() == 4 * ((c2 + c1) * 65792 + c3 * 16448), "the library split the work for another CU count"
    covered = set().union(*(plan_features(b, n_cus) for b in PROBE_B))
    assert covered == FEATURES, ("the probe sizes miss tiling edges at %d CUs" % n_cus, FEATURES - covered)
    a = _integer_minibatch(T, B, seed=B % 1000 + 3)
    terms = torch.tensor([0.0, 0.0, 0.0, 1.0], device="cuda")
    work = torch.empty(env.learn_workspace_bytes(), dtype=torch.uint8, device="cuda")
    grad = torch.full((K.MLP_PARAMS,), 7.0, device="cuda")
    acts = [a[k] for k in ("Xw", "H1", "H2", "dOut", "dH2", "dH1")]
    env.learn_dw(B, *acts, terms, work, grad)
    ref = _integer_reference(T, B, a)
    if not torch.equal(grad, ref):
        bad = (grad != ref).nonzero().flatten()
        pytest.fail("%d of %d gradient entries differ (B = %d); first at %d: %r vs %r"
                    % (bad.numel(), grad.numel(), B, bad[0].item(), grad[bad[0]].item(), ref[bad[0]].item()))
    if B == 393216:
        again = torch.full_like(grad, -7.0)
        env.learn_dw(B, *acts, terms, work, again)
        assert torch.equal(again, grad)
    if B == LEARN_MAX_BATCH:
        again = torch.full_like(grad, -7.0)
        with pytest.raises(T.TarokNativeError):
            env.learn_dw(B + 1, *acts, terms, work, again)
        torch.cuda.synchronize()
        assert (again == -7.0).all().item()                            # refused before any launch
    del a, acts, work, grad, ref
    _free()


@pytest.mark.gpu
def test_split_learn_dw_equals_one_launch(T, env):
    """selfplay.learn_dw_ranges (update_fused's path past TAROK_LEARN_MAX_BATCH) with the limit lowered to 1,000: five
    launches on row-offset views, the later ones added in — the same bits as one launch over the 5,000 samples, on
    the exact probe's inputs.  The padding rows behind each range are the next range's samples: they must not be read."""
    import torch
    from tarok_amd import selfplay as SP
    K = T.karte
    B = 5000
    assert SP.dw_ranges(B, 1000) == [(k, k + 1000) for k in range(0, B, 1000)]
    a = _integer_minibatch(T, B, seed=17)
    acts = [a[k] for k in ("Xw", "H1", "H2", "dOut", "dH2", "dH1")]
    terms = torch.tensor([0.0, 0.0, 0.0, 1.0], device="cuda")
    work = torch.empty(env.learn_workspace_bytes(), dtype=torch.uint8, device="cuda")
    one = torch.zeros(K.MLP_PARAMS, device="cuda")
    env.learn_dw(B, *acts, terms, work, one)
    split, part = torch.full_like(one, 3.0), torch.empty_like(one)
    SP.learn_dw_ranges(env, B, acts, terms, work, split, part, cap=1000)
    assert torch.equal(split, one) and torch.equal(one, _integer_reference(T, B, a))
    terms[3] = 0.125                                                   # (the scale applies to every range)
    SP.learn_dw_ranges(env, B, acts, terms, work, split, part, cap=1000)
    assert torch.equal(split, one * 0.125)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5000, 393216])
def test_learn_dw_vs_float64_on_realistic_values(T, env, B):
    """tarok_learn_dw on bf16 values as the chain writes them — H ReLU-like (about half zeros), dH signed — against float64,
    entry by entry: |g - ref| <= c (|dH|^T |H|) w for the weights, c (sum |dH|) w for the biases, w = terms[3].

    Where c comes from: every product of two bf16 is exact in float32 (8 + 8 significant bits), so all error is
    accumulation.  A chunk of L samples is summed in float32 — MFMA accumulators for the weights, per-thread column sums
    and a reduction over at most 32 thread groups for the biases — which by the standard bound for recursive summation
    errs by at most (L + 32) u times the sum of the magnitudes, u = 2^-24.  k_learn_reduce adds the chunks (at most
    108 at 256 CUs) as eight interleaved sums and a 3-level tree, at most (chunks / 8 + 3) u more, and the scaling by w
    rounds once more: c = (L_max + 32 + chunks / 8 + 4) u with L_max the longest chunk of any layer (7,584 samples at the
    bench's minibatch: c = 4.5e-4).  A worst-case bound: typical errors are far below it."""
    import torch
    K = T.karte
    f64 = torch.float64
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan = chunk_plan(B, n_cus)
    L = max(s1 - s0 for ch in plan.values() for s0, s1 in ch)
    c = (L + 32 + max(learn_chunks(n_cus)) / 8 + 4) * 2.0 ** -24
    g = torch.Generator(device="cuda"); g.manual_seed(B)
    rows = B + K.LEARN_PAD
    bf = lambda t: t.to(torch.bfloat16)
    H1 = bf(torch.randn((rows, 256), device="cuda", generator=g).relu_())
    H2 = bf(torch.randn((rows, 256), device="cuda", generator=g).relu_() * 3)
    dOut = bf(torch.randn((rows, 64), device="cuda", generator=g) * 0.01)
    dH2 = bf(torch.randn((rows, 256), device="cuda", generator=g) * 0.02 * (torch.rand((rows, 256), device="cuda", generator=g) < 0.5))
    dH1 = bf(torch.randn((rows, 256), device="cuda", generator=g) * 0.05 * (torch.rand((rows, 256), device="cuda", generator=g) < 0.5))
    for t in (H1, H2, dOut, dH2, dH1):
        t[B:] = float("nan")
    Xw = torch.empty((rows, 4), dtype=torch.int64, device="cuda")
    Xw[:B].view(torch.int32).random_(-2 ** 31, 2 ** 31, generator=g)
    Xw[B:] = -1
    w = 1.0 / (0.8 * B)
    terms = torch.tensor([0.0, 0.0, 0.0, w], device="cuda")
    work = torch.empty(env.learn_workspace_bytes(), dtype=torch.uint8, device="cuda")
    grad = torch.zeros(K.MLP_PARAMS, device="cuda")
    env.learn_dw(B, Xw, H1, H2, dOut, dH2, dH1, terms, work, grad)
    X = T.TarokVecEnv.expand_feature_words(Xw[:B], f64)
    wt = float(terms[3].item())
    off = 0
    for name, dH, H in (("1", dH1, X), ("2", dH2, H1), ("3", dOut, H2)):
        d, h = dH[:B].to(f64), H[:B].to(f64)
        for kind, ref, mag in (("W", d.T @ h, d.abs().T @ h.abs()), ("b", d.sum(0), d.abs().sum(0))):
            got = grad[off:off + ref.numel()].view_as(ref).to(f64)
            off += ref.numel()
            err, bound = (got - ref * wt).abs(), c * mag * wt
            assert ref.abs().max().item() > 0
            assert (err <= bound).all().item(), (kind + name, (err / bound.clamp(min=1e-300)).max().item(), c)
    assert off == K.MLP_PARAMS
    del X, H1, H2, dOut, dH2, dH1, Xw, work, d, h
    _free()


@pytest.mark.gpu
def test_learn_returns_at_full_size(T):
    """tarok_learn_returns at n = 65,536 + 77 slots (a ragged last workgroup of 77) and T = 48, with slots whose game never
    ends inside the rollout, games that end at t = 0 and at t = T - 1, vs selfplay.assign_returns and the advantage
    statistics in float64.

    The tolerances are today's (1e-4 absolute on the mean, 1e-3 relative on 1 / std), and they cover k_returns' float32
    sums: each thread adds at most T = 48 advantages |a| <= 90 / 70 + |v| (v ~ N(0, 1)), then 256 threads are combined in
    8 more float32 additions; k_adv_stats adds the per-workgroup sums in float64.  So the sums err by at most
    (48 + 8) 2^-24 = 3.3e-6 times the sums of |a| and a^2: the mean by 3.3e-6 E|a| ~ 5e-6, the variance E[a^2] - mean^2
    (mean ~ 0: no cancellation) and so 1 / std by about 2e-6 relative — both far inside the tolerances."""
    import torch
    from tarok_amd import selfplay as SP
    n, Tn = 65536 + 77, 48
    env = T.TarokVecEnv(n, seed=1)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    done = (torch.rand((Tn, n), device="cuda", generator=g) < 0.06).to(torch.uint8)
    slot = torch.arange(n, device="cuda")
    never = (slot % 7 == 3) | (slot == n - 1)                           # games that never end inside the rollout
    first = (slot % 11 == 5) & ~never                                   # games that end at t = 0 and nowhere else
    last = ((slot % 13 == 6) | (slot == n - 2)) & ~never & ~first       # games that end on the last lock-step
    done[Tn - 1, last] = 1
    done[:, first] = 0
    done[0, first] = 1
    done[:, never] = 0
    reward = torch.randint(-90, 91, (Tn, n, 4), device="cuda", generator=g, dtype=torch.int16)
    seat = torch.randint(0, 4, (Tn, n), device="cuda", generator=g)
    words = (seat << T.karte.OBS_SEAT_SHIFT) | torch.randint(0, 1 << 50, (Tn, n), device="cuda", generator=g)
    logp = -torch.rand((Tn, n), device="cuda", generator=g)
    val = torch.randn((Tn, n), device="cuda", generator=g)
    act = torch.randint(0, 54, (Tn, n), device="cuda", generator=g, dtype=torch.uint8)
    rec = torch.empty((Tn, n, 4), device="cuda"); stats = torch.empty(4, device="cuda")
    scratch = torch.empty(((n + 255) // 256, 4), device="cuda")
    env.learn_returns(Tn, done, reward, words, logp, val, act, 1.0 / 70.0, rec, stats, scratch)
    ret, known = SP.assign_returns(done.bool(), reward, seat)
    ret = ret / 70.0
    assert not known[:, never].any() and known[0, first].all() and not known[1:, first].any()
    assert known[:, last].all()
    assert torch.equal(rec[..., 0], logp) and torch.equal(rec[..., 2], val)
    assert torch.allclose(rec[..., 1], ret, rtol=1e-6, atol=1e-7)
    bits = rec[..., 3].contiguous().view(torch.int32)
    assert torch.equal((bits & 255).to(torch.uint8), act) and torch.equal(((bits >> 8) & 1).bool(), known)
    adv = (ret.double() - val.double())[known]
    mean, std = adv.mean().item(), adv.std(unbiased=False).item()
    assert abs(stats[0].item() - mean) < 1e-4 and abs(stats[1].item() - 1.0 / std) < 1e-3 / std
    assert abs(stats[2].item() - known.double().mean().item()) < 1e-6
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["no_clip", "zero_grad", "step_10000", "norm_at_max"])
def test_learn_adam_edges(T, env, case):
    """tarok_learn_adam vs clip_grad_norm_ + torch.optim.Adam at its edges: max_norm <= 0 (no clipping, on a gradient
    whose norm is far above 1), an all-zero gradient (after a real step: m and v decay, the parameters still move), a
    step counter and m, v as if at step 10,000 (loaded into torch's optimizer state too), and a gradient whose norm
    equals max_norm exactly (256 entries of +-1/16: the float32 sum of squares is exactly 1; not clipped — torch scales
    by 1 / (1 + 1e-6), which Adam's step does not see at this tolerance).  Parameter and norm tolerances as in
    test_learn_adam_vs_torch.  m and v: the kernel forms 1 - beta in float32 (1 - 0.999f = 9.99987e-4, 1.3e-5 below torch's
    1e-3; 1 - 0.9f: 2.4e-7 above), so v is 1.3e-5 relative off torch's after a step on a fresh state: rtol 1e-5 on m,
    2e-5 on v.  (The bias correction 1 - 0.999f^t carries the same factor, which is why the steps still agree.)"""
    import torch
    K = T.karte
    P = K.MLP_PARAMS
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    flat = (torch.randn(P, device="cuda", generator=g) * 0.05).contiguous()
    ref = flat.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3)
    m, v = torch.zeros(P, device="cuda"), torch.zeros(P, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    gn = torch.zeros(1, device="cuda")
    max_norm = 0.0 if case == "no_clip" else 1.0
    grads = [torch.randn(P, device="cuda", generator=g)]                 # (norm ~385)
    if case == "zero_grad":
        grads.append(torch.zeros(P, device="cuda"))
    elif case == "step_10000":
        m.copy_(torch.randn(P, device="cuda", generator=g) * 0.01)
        v.copy_(torch.rand(P, device="cuda", generator=g) * 1e-4)
        step.fill_(10000)
        opt.state[ref] = dict(step=torch.tensor(10000.0), exp_avg=m.clone(), exp_avg_sq=v.clone())
    elif case == "norm_at_max":
        e = torch.zeros(P, device="cuda")
        e[torch.randperm(P, device="cuda", generator=g)[:256]] = torch.where(torch.rand(256, device="cuda", generator=g) < 0.5, -1.0, 1.0) / 16
        grads = [e]
    for gr in grads:
        env.learn_adam(flat, gr, m, v, step, None, lr=1e-3, max_norm=max_norm, gnorm=gn)
        ref.grad = gr.clone()
        norm = torch.nn.utils.clip_grad_norm_([ref], max_norm) if max_norm > 0 else gr.norm()
        opt.step()
        assert abs(gn.item() - norm.item()) <= 1e-4 * norm.item(), (gn.item(), norm.item())
        assert torch.allclose(flat, ref.detach(), rtol=2e-5, atol=2e-7), case
    st = opt.state[ref]
    assert step.item() == int(st["step"].item())
    assert torch.allclose(m, st["exp_avg"], rtol=1e-5, atol=1e-9) and torch.allclose(v, st["exp_avg_sq"], rtol=2e-5, atol=1e-12)
    if case == "norm_at_max":
        assert gn.item() == 1.0


@pytest.mark.gpu
def test_selfplay_update_past_the_learn_dw_limit(T):
    """SelfPlay on 2^20 games, one rollout of 8 lock-steps updated as ONE minibatch: 8,388,608 samples, twice
    TAROK_LEARN_MAX_BATCH — update_fused computes the weight gradients over three row ranges (dw_ranges) instead of
    failing in tarok_learn_dw.  About 20 GB of activations."""
    import torch
    from tarok_amd import selfplay as SP
    K = T.karte
    n = 1 << 20
    env = T.TarokVecEnv(n, seed=3, mix=K.MIX_ALL)
    sp = SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True)
    obs = env.legal_actions()
    for _ in range(40):                                                  # (most games end inside the 8 lock-steps)
        obs, _, _ = env.step(env.policy_random(obs), auto_reset=True)
    sp.obs_words.copy_(obs.words)
    p0 = sp.flat.clone()
    st = sp.iterate(T=8, epochs=1, minibatches=1)
    assert st["env_errors"] == 0 and np.isfinite(st["loss"]) and 0.05 < st["known_frac"] < 1, st
    assert torch.isfinite(sp.flat).all().item() and (sp.flat != p0).float().mean().item() > 0.5
    assert len(SP.dw_ranges(8 * n)) == 3
    del sp
    env.close()
    _free()
