#!/usr/bin/env python3
"""Diagnostic (GPU box): what training against a frozen opponent costs and saves in update_fused, in ONE process on one
real rollout — SelfPlay(opponent = a snapshot).collect(48) at 65,536 games with the learner on one seat per slot (the
default seats), after a few iterations so that the slots stand at the phases of a running job.  Three figures:

  (a) the default path on that rollout (opponent = None, what update_fused did before opponent mode existed): every
      sample of the rollout is trained on, the opponent's included — the cost to compare with, not a way to train;
  (b) opponent mode: masked returns, compaction, one host read of the count, minibatches of the learner's samples only;
  (c) the same masked rollout with the compaction switched off: the masked returns, then minibatches over arange(M) in
      which the opponent's samples carry weight 0 — the forward, loss and backward of every row all the same.

From the code the chain and dW work of (b) should scale with count / M against (c); nobody has measured it.  Each
figure is a host clock around update_fused(epochs = 2, minibatches = 8) ending in a device synchronise, the three
alternating over `runs` runs; the learners are copies of one set of weights and every run updates its own copy.

usage: opponent_update_time.py [out.txt = profiles/opponent_update_times.txt] [games = 65536]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K, selfplay as SP  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "opponent_update_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
T, EPOCHS, MINIBATCHES, RUNS = 48, 2, 8, 5
assert torch.cuda.is_available(), "this tool measures on the GPU"

env = TarokVecEnv(n, seed=0, mix=K.MIX_ALL)
old = SP.SelfPlay(env, seed=1).snapshot()
sp = SP.SelfPlay(env, seed=0, opponent=old)
for _ in range(3):                                   # graph capture, warm-up of every update kernel, slots spread over the game
    st = sp.iterate(T=T, epochs=EPOCHS, minibatches=MINIBATCHES)
    assert st["env_errors"] == 0
buf = sp.collect(T)
torch.cuda.synchronize()
M = T * n


def update_default():
    """(a): the rollout through the path without an opponent."""
    opp, seats = sp._opp, sp._seats
    sp._opp, sp._seats = None, None
    try:
        return sp.update_fused(buf, EPOCHS, MINIBATCHES)
    finally:
        sp._opp, sp._seats = opp, seats


def update_masked_uncompacted():
    """(c): update_fused's launches with the masked record and index = a run of a permutation of arange(M)."""
    lb = sp._learn_bufs(M, -(-M // MINIBATCHES))
    env.learn_returns_seats(T, buf["done"], buf["reward"], buf["words"][:T], buf["logp"], buf["val"], buf["act"], sp.reward_scale,
                            lb["rec"], lb["stats"], lb["scratch"], gae=sp.gae, gamma=sp.gamma, lam=sp.gae_lambda, seats_per_game=sp._seats)
    words = buf["obs"].view(M, 4)
    lb["running"].zero_()
    bias = (sp._w[1], sp._w[3], sp._w[5])
    for _ in range(EPOCHS):
        for idx in sp._epoch_permutation(M).chunk(MINIBATCHES):
            b = idx.numel()
            env.learn_chain(b, words, idx, lb["rec"], lb["stats"], sp.clip, sp.vf_coef, sp.ent_coef, sp._wf, bias,
                            lb["Xw"], lb["H1"], lb["H2"], lb["dOut"], lb["dH2"], lb["dH1"], lb["scratch"], lb["terms"], lb["running"])
            SP.learn_dw_ranges(env, b, [lb[a] for a in ("Xw", "H1", "H2", "dOut", "dH2", "dH1")], lb["terms"], lb["work"], sp.gflat, lb["gpart"])
            SP.allreduce_flat(sp.gflat)
            env.learn_adam(sp.flat, sp.gflat, sp.adam_m, sp.adam_v, sp.adam_step, sp._wf, lr=sp.lr, max_norm=sp.max_grad_norm)
    return dict(known_frac=float(lb["stats"][2]))


legs = {"(a) default path, every sample": update_default,
        "(b) opponent mode, compacted": lambda: sp.update_fused(buf, EPOCHS, MINIBATCHES),
        "(c) masked, weight 0, not compacted": update_masked_uncompacted}
ms = {k: [] for k in legs}
info = {}
for fn in legs.values():                             # one untimed pass of each
    fn()
for _ in range(RUNS):
    for name, fn in legs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info[name] = fn()
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3)

count = info["(b) opponent mode, compacted"]["learner_samples"]
lines = ["update_fused(epochs = %d, minibatches = %d) on one rollout: %d games x T = %d lock-steps (%d samples)" % (EPOCHS, MINIBATCHES, n, T, M),
         "learner on one seat per slot (slot g: seat g %% 4): %d samples are the learner's and known, count / M = %.4f" % (count, count / M),
         "known_frac: (a) %.4f  (b) %.4f  (c) %.4f" % tuple(info[k]["known_frac"] for k in legs),
         "ms per update (host clock to a device synchronise; %d runs each, alternating):" % RUNS]
med = {}
for name, v in ms.items():
    med[name] = statistics.median(v)
    lines.append("  %-38s median %7.2f ms   min %7.2f   max %7.2f" % (name, med[name], min(v), max(v)))
a, b, c = (med[k] for k in legs)
lines.append("  ratio (b) / (c): %.3f   (b) / (a): %.3f   (c) / (a): %.3f" % (b / c, b / a, c / a))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps({"update_ms": med, "learner_samples": count, "samples": M}))
env.close()
