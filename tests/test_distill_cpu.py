"""CPU-side checks of the playout teacher's distillation: the float64 statements of tests/distill_model.py against float64
autograd, a float32 restatement of the kernel's arithmetic against the model's bounds, four mutants of that restatement that
the comparator must reject, the one-hot rows at tau = 0 against the playout model's card, and the argument validation of
the two C entry points, which makes no HIP call and so runs without a GPU."""
import ctypes

import numpy as np
import pytest

import distill_model as DM
import loss_model as L
import playout_model as PM
from oracle import oracle as O
from oracle import tarok_spec as S

N, SEED = 333, 29
COEF = 0.75


def cases_and_logits():
    cases = L.build_cases(N, SEED, "entropy")                 # (A = 0 exactly: nothing but the new term moves the logits)
    rnd = np.random.RandomState(SEED)
    logits = np.round(rnd.randn(N, 64) * 3.0 * 256) / 256
    ref = L.loss_reference(logits, cases["legal"], cases["card"], np.zeros(N), np.zeros(N), cases["ret"],
                           cases["known"].astype(np.float64), 0.2, 0.0, 0.0)
    return cases, logits, ref


def test_model_gradient_against_float64_autograd():
    import torch
    cases, logits, ref = cases_and_logits()
    for kind in ("onehot", "uniform", "random", "zero"):
        q = DM.target_rows(cases["legal"], kind, seed=3)
        d = DM.distill_reference(ref, DM.with_nans(q, cases["legal"]))
        x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
        legal = torch.from_numpy(cases["legal"])
        lp = torch.log_softmax(x[:, :54].masked_fill(~legal, float("-inf")), dim=-1)
        lp = torch.where(legal, lp, torch.zeros_like(lp))
        qt = torch.where(legal, torch.from_numpy(q[:, :54]), torch.zeros_like(lp))
        has = legal.any(1)
        ce = -(qt * lp).sum(1)
        ce = torch.where(has, ce, torch.zeros_like(ce))
        ce.sum().backward()
        assert np.allclose(ce.detach().numpy(), d["ce"], rtol=0, atol=1e-12)
        assert np.allclose(x.grad.numpy(), d["d_distill"], rtol=0, atol=1e-12), kind
        assert (d["d_distill"][:, 54:] == 0).all() and (d["d_distill"][:, :54][~cases["legal"]] == 0).all()
        if kind in ("onehot", "uniform"):
            live = cases["legal"].any(1)
            assert np.abs(d["S"][live] - 1).max() < 2.0 ** -6 and (d["S"][~live] == 0).all()


def restate32(logits, legal, w, q, coef, mutant=None):
    """The loss phase's arithmetic for the new term alone, in float32 as the kernel orders it: (dOut [n,64] as bf16 numbers,
    {mean ce, mean S})."""
    import torch
    f = np.float32
    n = logits.shape[0]
    has = legal.any(1)
    l = np.where(legal, logits[:, :54].astype(f), f(-1.0e30))
    l[~has, 0] = logits[~has, 0].astype(f)                     # (the kernel's stand-in: card 0 alone, weight 0)
    w = np.where(has, w, 0.0).astype(f)
    z = (l - l.max(1, keepdims=True)).astype(f)
    e = np.exp(z.astype(np.float64)).astype(f)
    s = e.sum(1, dtype=f)
    p = (e * (f(1) / s)[:, None]).astype(f)
    lp = (z - np.log(s.astype(np.float64)).astype(f)[:, None]).astype(f)
    sel = legal & has[:, None]
    q54 = q[:, :54].astype(f)
    if mutant == "multiply":
        with np.errstate(invalid="ignore"):
            qs = (q54 * sel.astype(f)).astype(f)
    elif mutant == "all54":
        qs = np.nan_to_num(q54, nan=f(0.25))
    else:
        qs = np.where(sel, q54, f(0))
    Ssum = qs.sum(1, dtype=f)
    ce = -(qs * lp).sum(1, dtype=f)
    Sg = np.ones_like(Ssum) if mutant == "noS" else Ssum
    cw = (f(coef) * (np.ones_like(w) if mutant == "unweighted" else w)).astype(f)
    d = np.zeros((n, 64), f)
    with np.errstate(invalid="ignore"):                        # the kernel's order: fma(cw, fma(S, p, -q), the other terms = 0)
        inner = (Sg[:, None].astype(np.float64) * p.astype(np.float64) - qs.astype(np.float64)).astype(f)
        d[:, :54] = np.where(cw[:, None] != 0, cw[:, None] * inner, f(0))
    wsum = max(float(w.sum()), 1.0)
    means = np.array([float((w * ce).sum(dtype=f)) / wsum, float((w * Ssum).sum(dtype=f)) / wsum])
    return torch.from_numpy(d).to(torch.bfloat16).double().numpy(), means


def judge(ref, q, got, means, coef):
    d = DM.distill_reference(ref, q)
    part = DM.distill_gradient(d, coef)
    ratio, msgs = L.violations(got, d["w"][:, None] * part, DM.distill_bound(d, part, d["w"], coef), "restatement")
    want, _ = DM.distill_means(d)
    mb = DM.distill_means_bound(d)
    with np.errstate(invalid="ignore"):
        bad_means = ~(np.abs(means - want) <= mb)
    return ratio, msgs, bad_means


def test_float32_restatement_within_the_bounds_and_mutants_rejected():
    cases, logits, ref = cases_and_logits()
    w = cases["known"].astype(np.float64)
    worst = 0.0
    for kind in ("onehot", "uniform", "random", "zero"):
        q = DM.with_nans(DM.target_rows(cases["legal"], kind, seed=5), cases["legal"])
        got, means = restate32(logits, cases["legal"], w, q, COEF)
        ratio, msgs, bad_means = judge(ref, q, got, means, COEF)
        assert not msgs and not bad_means.any(), (kind, msgs, means)
        worst = max(worst, ratio)
    print("float32 restatement: largest error / bound %.3f" % worst)
    # the mutants, on rows whose sums are far from 1 (uniform rows scaled by 1/2: still bf16 numbers)
    q = DM.with_nans(0.5 * DM.target_rows(cases["legal"], "uniform"), cases["legal"])
    for mutant in ("noS", "unweighted", "multiply", "all54"):
        got, means = restate32(logits, cases["legal"], w, q, COEF, mutant)
        _, msgs, bad_means = judge(ref, q, got, means, COEF)
        assert msgs or bad_means.any(), "the comparator lets the mutant '%s' through" % mutant
        if mutant == "all54":
            assert bad_means.any()


def test_target_rows_random_is_target_rows_without_the_loop():
    """The generator for large sample sets against the row-by-row one: rows without a card, one-card rows, full rows."""
    rnd = np.random.RandomState(3)
    legal = rnd.rand(4096, 54) < rnd.rand(4096, 1) * 0.4
    legal[::97] = False
    legal[1::97] = False
    legal[1::97, 5] = True
    legal[2::97] = True
    for seed in (0, 7):
        a, b = DM.target_rows(legal, "random", seed=seed), DM.target_rows_random(legal, seed=seed)
        assert a.shape == b.shape == (4096, 64) and np.array_equal(a, b)
    assert (b[::97] == 0).all() and (b[1::97, 5] == 1).all() and (b[:, 54:] == 0).all() and (b[~np.pad(legal, ((0, 0), (0, 10)))] == 0).all()


def test_target_rows_model_on_hand_made_sums():
    words = np.array([0b1011 | (2 << 54), 0b1011 | (1 << 54), 0, 0b110 | (3 << 54) | (1 << 62)], np.uint64)
    sums = np.zeros((4, 12, 4), np.int64)
    sums[0, :3, 2] = (10, 30, 30)
    sums[3, :2, 3] = (-(1 << 20), 1 << 20)
    q, has, card = DM.targets_reference(sums, words, 4, 0.0, [15, 13, 15, 15])
    assert has.tolist() == [True, False, False, True] and card.tolist() == [1, 255, 255, 2]
    assert q[0].nonzero()[0].tolist() == [1] and q[0, 1] == 1.0 and not q[1].any() and not q[2].any()
    q, has, _ = DM.targets_reference(sums, words, 4, 5.0, 15)
    assert has.tolist() == [True, True, False, True]
    e = np.exp(np.array([-1.0, 0.0, 0.0]))
    assert np.allclose(q[0, [0, 1, 3]], e / e.sum()) and q[0].sum() == pytest.approx(1.0)
    assert np.allclose(q[1, [0, 1, 3]], 1 / 3)                 # all ranks equal: uniform
    q, _, _ = DM.targets_reference(sums, words, 4, 0.5, 15)
    assert q[3, 1] == 0.0 and q[3, 2] == 1.0 and np.isfinite(q).all()   # 2^21 / 2 apart: the loser underflows to 0, no NaN
    assert (DM.target_bound(q)[q == 0] == 0).all()


def test_one_hot_rows_at_tau_0_are_the_playout_models_card():
    seen = 0
    for gidx in range(6):
        for cards in (0, 1, 3, 22):
            g = O.Game.synth(31, gidx, 2, S.MIX_ALL)
            key = O.game_key(31, gidx, 2)
            for qn in range(cards):
                if g.done:
                    break
                g.step(O.policy_action(key, qn, g.legal()))
            in_play, seat, legal, _ = PM.position(g)
            sums, card = PM.playout_cards(g.lanes(), 2, 31, 9, gidx, 15, 2)
            word = (legal | (seat << 54)) if in_play else (1 << 62)
            q, has, c = DM.targets_reference(sums[None], [word], 2, 0.0, 15)
            assert bool(has[0]) == in_play
            if in_play:
                assert c[0] == card and q[0].nonzero()[0].tolist() == [card] and q[0, card] == 1.0
                seen += 1
            else:
                assert card == 255 and not q.any()
    assert seen >= 12


@pytest.fixture(scope="module")
def lib():
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_abi_version_and_surface(lib):
    import inspect
    from tarok_amd import _native
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.selfplay import SelfPlay
    assert lib.tarok_abi_version() == 5
    assert "tarok_playout_targets" in _native.SYMBOLS and "tarok_learn_chain_distill" in _native.SYMBOLS
    sig = inspect.signature(TarokVecEnv.playout_targets).parameters
    assert list(sig)[1:] == ["sums", "obs_words", "playouts", "tau", "seats", "seats_per_game", "target_out"]
    assert sig["seats"].default == 15
    assert hasattr(TarokVecEnv, "learn_chain_distill")
    sp = inspect.signature(SelfPlay.__init__).parameters
    assert sp["teacher"].default is None and sp["distill_coef"].default == 0.0


def test_both_entry_points_validate_before_any_hip_call(lib):
    """Every refusal comes before the first HIP call: a zeroed stand-in for an env (no GPU, no tarok_create) is enough."""
    z = ctypes.c_void_p(0)
    env = ctypes.cast(ctypes.create_string_buffer(1 << 16), ctypes.c_void_p)
    buf = ctypes.cast(ctypes.create_string_buffer(256), ctypes.c_void_p)
    T = lib.tarok_playout_targets
    assert T(None, buf, buf, 4, 1.0, 15, z, buf, z) == -1
    assert T(env, z, buf, 4, 1.0, 15, z, buf, z) == -1
    assert T(env, buf, z, 4, 1.0, 15, z, buf, z) == -1
    assert T(env, buf, buf, 4, 1.0, 15, z, z, z) == -1
    assert T(env, buf, buf, 0, 1.0, 15, z, buf, z) == -1
    assert T(env, buf, buf, -2, 1.0, 15, z, buf, z) == -1
    for tau in (-0.5, float("nan"), float("inf"), float("-inf")):
        assert T(env, buf, buf, 4, tau, 15, z, buf, z) == -1
    assert T(env, buf, buf, 1024, 1.0e37, 15, z, buf, z) == -1          # the float32 product playouts * tau overflows
    assert T(env, buf, buf, 1, 1.0e-40, 15, z, buf, z) == -1            # ... or is not a normal number
    assert T(env, buf, buf, 4, 1.0, 16, z, buf, z) == -1
    assert T(env, buf, buf, 4, 1.0, -1, z, buf, z) == -1
    D = lib.tarok_learn_chain_distill
    good = [env, 96] + [buf, z, buf, buf] + [0.2, 0.5, 0.01] + [buf] * 16 + [z] + [buf, 1.0, buf, buf, z, z]
    assert len(good) == len(D.argtypes)

    def call(**change):
        a = list(good)
        for k, v in change.items():
            a[int(k[1:])] = v
        return D(*a)
    assert call(a0=None) == -1 and call(a1=0) == -1
    for k in (2, 4, 5) + tuple(range(9, 25)) + (26, 28, 29):       # every required array, the four new ones included
        assert call(**{"a%d" % k: z}) == -1, k
    assert call(a27=float("nan")) == -1 and call(a27=float("inf")) == -1
