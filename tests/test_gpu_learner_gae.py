"""GPU tests of tarok_learn_returns_gae (k_returns_gae: per-seat GAE(gamma, lambda) returns for the fused learner)
against the float64 per-slot loop of tests/gae_model.py — exactly, on inputs where float32 cannot round; within a bound
derived from each seat's chain of decisions otherwise — with every output between guard bands, and SelfPlay driven
through it end to end.  Build-owned code (the reference has no policy-gradient learner).

Shapes: n = 300 slots (two workgroups, the second a ragged one of 44) at T = 12 and at T = 13 (not a multiple of the
walk's unroll of 4), and one slot at T = 1.  Among the 300 slots: games that never end inside the rollout (the last
slot among them), that end at t = 0 only, at t = T - 1, on two consecutive lock-steps, and slots where seat 2 never moves.

Run on the GPU box:  python -m pytest tests -m gpu -x -q
"""
import ctypes

import numpy as np
import pytest

from gae_model import gae_model
from tarok_amd import karte as K
from gae_cases import F32, SEAT_SHIFT, SHAPES, arrays, check_bits, launch, model
from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
assert K.OBS_SEAT_SHIFT == SEAT_SHIFT, "the GAE tests' seat field is not the observation word's"


@pytest.fixture(scope="module")
def envs(T):
    es = {n: T.TarokVecEnv(n, seed=1) for n in (300, 1)}
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("gamma,lam", [(1.0, 1.0), (1.0, 0.5), (0.5, 1.0)])
@pytest.mark.parametrize("Tn,n", [(12, 300), (1, 1)])
def test_returns_gae_exact(T, envs, Tn, n, gamma, lam):
    """Values in eighths within [-4, 4], scores in [-90, 90] scaled by 1/64, gamma and lambda in {1, 1/2}, T <= 12: the
    model itself checks that every intermediate of the recursion is a float32 (at most 12 decisions of a seat, each
    halving the grid of 1/64 at most once: 2^-17 under a magnitude below 32, 22 bits), so the kernel's returns must EQUAL
    the float64 model's, whatever the association or fusing of its multiply-adds; logp and val pass through bit for bit;
    card and known bits are the model's.  For gamma = lambda = 1 the return is tarok_learn_returns' wherever that one
    knows it."""
    import torch
    a = arrays(Tn, n, True, n == 1)                                              # (the single slot: its game ends)
    scale = 1.0 / 64.0
    m = model(Tn, n, True, n == 1, gamma, lam, scale)
    assert m["lossless"].all()                                                   # the precondition of "equal"
    r, written, *_ = launch(envs[n], a, gamma, lam, scale)
    assert written.all()
    assert (r[..., 1].astype(np.float64) == m["ret"]).all()
    check_bits(r, a, m)
    if n > 1:
        assert m["known"].any() and (~m["known"]).any()
    if (gamma, lam) == (1.0, 1.0):
        dev = {k: torch.from_numpy(a[k]).cuda() for k in ("done", "reward", "words", "logp", "val", "act")}
        rec = torch.empty((Tn, n, 4), device="cuda"); stats = torch.empty(4, device="cuda")
        scratch = torch.empty(((n + 255) // 256, 4), device="cuda")
        envs[n].learn_returns(Tn, dev["done"], dev["reward"], dev["words"], dev["logp"], dev["val"], dev["act"], scale, rec, stats, scratch)
        mc = rec.cpu().numpy()
        mc_known = ((np.ascontiguousarray(mc[..., 3]).view(np.uint32) >> 8) & 1).astype(bool)
        assert m["known"][mc_known].all()
        assert (r[..., 1][mc_known] == mc[..., 1][mc_known]).all()
        if n > 1:
            assert mc_known.any() and (m["known"] & ~mc_known).any()


@pytest.mark.parametrize("Tn,n", SHAPES)
def test_returns_gae_general(T, envs, Tn, n):
    """Normal values, gamma = 0.99, lambda = 0.95, scale 1/70 (each as the float32 the ABI passes).  Every return lies
    within the model's own bound for a float32 evaluation (tests/gae_model.py: <= 8 roundings of 2^-24 of the running
    magnitude per decision, carried along the seat's chain with the factor gamma * lambda — about 1e-5 at the end of
    the longest chains here, five times what a plain float32 evaluation misses by; no guessed constant).  stats against the float64 mean, 1 / std and known fraction of the
    model's advantages at the tolerances of test_learn_returns_vs_torch (1e-4, 1e-3 relative, 1e-6): the sums are
    float32 over at most 13 + 8 additions, (13 + 8) 2^-24 = 1.3e-6 relative.  1 / std is compared where it is defined,
    with two or more known samples: of a single sample the reference is 1 / 0 (the one slot at T = 1: there it must only
    be finite and positive — k_adv_stats' floor on std)."""
    gamma, lam, scale = F32(0.99), F32(0.95), F32(1.0 / 70.0)
    a = arrays(Tn, n, False, True)
    m = model(Tn, n, False, True, gamma, lam, scale)
    r, written, s, s_written, *_ = launch(envs[n], a, gamma, lam, scale)
    assert written.all() and s_written.all()
    err = np.abs(r[..., 1].astype(np.float64) - m["ret"])
    print("shape", (Tn, n), "max error", err.max(), "max bound", m["bound"].max(), "max error / bound", (err / m["bound"]).max())
    assert (err <= m["bound"]).all()
    check_bits(r, a, m)
    adv = m["adv"][m["known"]]
    assert adv.size >= 1
    mean, std = adv.mean(), adv.std()
    print("stats", s, "model", mean, std, m["known"].mean())
    assert abs(s[0] - mean) < 1e-4
    if adv.size >= 2:
        assert abs(s[1] - 1.0 / std) < 1e-3 / std
    else:
        assert np.isfinite(s[1]) and s[1] > 0
    assert abs(s[2] - m["known"].mean()) < 1e-6 and s[3] == 0


@pytest.mark.parametrize("Tn,n", SHAPES)
def test_returns_gae_writes_only_its_arrays(T, envs, Tn, n):
    """rec, stats and scratch between guard bands (launch() checks the bands): all of rec and stats is written, of
    scratch exactly the first ceil(n / 256) rows."""
    a = arrays(Tn, n, False, True)
    r, written, s, s_written, c, c_written, blocks = launch(envs[n], a, F32(0.99), F32(0.95), F32(1.0 / 70.0), spare_rows=5)
    assert written.all() and s_written.all()
    assert c_written[:blocks].all() and not c_written[blocks:].any()
    m = model(Tn, n, False, True, F32(0.99), F32(0.95), F32(1.0 / 70.0))
    known = m["known"].reshape(Tn, -1)
    per_block = [known[:, b * 256:(b + 1) * 256].sum() for b in range(blocks)]
    assert [float(x) for x in c[:blocks, 0]] == [float(x) for x in per_block] and (c[:blocks, 3] == 0).all()


def test_returns_gae_is_reproducible(T, envs):
    a = arrays(13, 300, False, True)
    one = launch(envs[300], a, F32(0.99), F32(0.95), F32(1.0 / 70.0))
    two = launch(envs[300], a, F32(0.99), F32(0.95), F32(1.0 / 70.0))
    assert one[0].tobytes() == two[0].tobytes() and one[2].tobytes() == two[2].tobytes()


def test_returns_gae_rejects_bad_arguments(T, envs):
    """gamma or lambda outside [0, 1] or NaN, a NULL array, T < 1: TAROK_EINVAL, and nothing is launched (rec, stats and
    scratch keep their fill)."""
    from tarok_amd import _native
    env = envs[300]
    L = _native.lib()
    a = arrays(12, 300, False, True)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nan = float("nan")

    def raw(Tn=12, gamma=0.99, lam=0.95, null=None):
        def call(dev, rec, stats, scratch):
            args = [p(dev["done"]), p(dev["reward"]), p(dev["words"]), p(dev["logp"]), p(dev["val"]), p(dev["act"])]
            outs = [p(rec), p(stats), p(scratch)]
            if null is not None:
                (args + outs)[null].value = None
            code = L.tarok_learn_returns_gae(env._h, Tn, *args, 1.0 / 70.0, gamma, lam, *outs, env._stream())
            assert code == -1, (Tn, gamma, lam, null, code)
        return call

    cases = [raw(gamma=1.5), raw(lam=-0.1), raw(gamma=nan), raw(lam=nan), raw(gamma=-0.01), raw(lam=1.001), raw(Tn=0)]
    cases += [raw(null=k) for k in range(9)]
    for call in cases:
        r, written, s, s_written, c, c_written, _ = launch(env, a, 0.0, 0.0, 0.0, call=call)
        assert not written.any() and not s_written.any() and not c_written.any()
    with pytest.raises(_native.TarokNativeError):
        launch(env, a, 1.5, 0.95, 1.0 / 70.0)
    assert L.tarok_learn_returns_gae(None, 12, *([ctypes.c_void_p(0)] * 6), 1.0, 1.0, 1.0, *([ctypes.c_void_p(0)] * 4)) == -1


def test_selfplay_with_gae_end_to_end(T):
    """SelfPlay(gamma = 0.99, gae_lambda = 0.95) on 512 games that stand in the middle of their play, one iteration of
    T = 16 lock-steps: the known fraction the fused update reports is the model's count on the rollout it returns, at
    least 1 - 4/16, and strictly above what Monte-Carlo returns know of the same rollout (a default SelfPlay on a twin
    env).  The torch update (fused_learner = False) on assign_gae reports the same fraction as the kernel on its
    rollout."""
    import torch
    from tarok_amd import selfplay as SP
    K = T.karte
    Tn, n = 16, 512
    made = []

    def fresh(**kw):
        env = T.TarokVecEnv(n, seed=7, mix=K.MIX_ALL)
        sp = SP.SelfPlay(env, seed=0, **kw)
        obs = env.legal_actions()
        for _ in range(40):                                                      # games end inside the 16 lock-steps
            obs, _, _ = env.step(env.policy_random(obs), auto_reset=True)
        sp.obs_words.copy_(obs.words)
        made.append(env)
        return env, sp

    def model_known(buf):
        done = buf["done"].cpu().numpy().astype(bool)
        seat = ((buf["words"][:Tn] >> K.OBS_SEAT_SHIFT) & 3).cpu().numpy()
        m = gae_model(done, buf["reward"].cpu().numpy(), seat, buf["val"].cpu().numpy(), 0.99, 0.95, 1.0 / 70.0)
        return m["known"], done

    env, sp = fresh(gamma=0.99, gae_lambda=0.95)
    assert sp.fused_learner
    st = sp.iterate(T=Tn, minibatches=2)
    assert st["env_errors"] == 0 and np.isfinite(st["loss"])
    known, done = model_known(sp._buf)
    assert done.any()
    assert st["known_frac"] == known.sum() / (Tn * n) and st["known_frac"] >= 1 - 4 / Tn
    _, mc_known = SP.assign_returns(sp._buf["done"].bool(), sp._buf["reward"], (sp._buf["words"][:Tn] >> K.OBS_SEAT_SHIFT) & 3)
    assert st["known_frac"] > mc_known.float().mean().item()

    env2, sp2 = fresh()
    st2 = sp2.iterate(T=Tn, minibatches=2)
    assert st2["env_errors"] == 0 and np.isfinite(st2["loss"])
    print("known_frac: GAE", st["known_frac"], "Monte-Carlo", st2["known_frac"])
    assert st["known_frac"] > st2["known_frac"]

    env3, sp3 = fresh(gamma=0.99, gae_lambda=0.95, fused_learner=False)
    assert not sp3.fused_learner
    st3 = sp3.iterate(T=Tn, minibatches=2)
    assert st3["env_errors"] == 0 and np.isfinite(st3["loss"])
    buf = sp3._buf
    known3, _ = model_known(buf)
    assert st3["known_frac"] == known3.sum() / (Tn * n)
    rec = torch.empty((Tn, n, 4), device="cuda"); stats = torch.empty(4, device="cuda"); scratch = torch.empty((2, 4), device="cuda")
    env3.learn_returns_gae(Tn, buf["done"], buf["reward"], buf["words"][:Tn], buf["logp"], buf["val"], buf["act"], 1.0 / 70.0, 0.99, 0.95,
                           rec, stats, scratch)
    assert st3["known_frac"] == float(stats[2])                                  # the fused path on the same rollout
    for k in ("act", "words", "done", "reward"):
        assert torch.equal(buf[k], sp._buf[k]), k                                # (same weights, same games, same draws)
    assert st3["known_frac"] == st["known_frac"]
    del sp, sp2, sp3
    for e in made:
        e.close()
