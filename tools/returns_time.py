#!/usr/bin/env python3
"""Diagnostic (GPU box): tarok_learn_returns (Monte-Carlo) and tarok_learn_returns_gae (per-seat GAE) timed in ONE
process on the same arrays — a real SelfPlay.collect(48) at 65,536 games, after a few iterations so that the slots
stand at the phases of a running job — the known fraction either estimator leaves of that rollout, and the time of
update_fused with and without GAE.

Times are device events around `reps` back-to-back calls (each call = the returns kernel + k_adv_stats), the two
estimators alternating over `rounds` rounds; the median round and the spread over the rounds are reported.  The
update is a host clock around update_fused ending in a device synchronise, alternating as well.

usage: returns_time.py [out.txt = profiles/gae_returns_times.txt] [games = 65536]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K, selfplay as SP  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gae_returns_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
T, GAMMA, LAM = 48, 0.99, 0.95
assert torch.cuda.is_available(), "this tool measures on the GPU"

env = TarokVecEnv(n, seed=0, mix=K.MIX_ALL)
sp = SP.SelfPlay(env, seed=0)
for _ in range(3):                                   # graph capture, warm-up of every update kernel, slots spread over the game
    st = sp.iterate(T=T, epochs=2, minibatches=8)
    assert st["env_errors"] == 0
buf = sp.collect(T)
torch.cuda.synchronize()
lb = sp._learn_bufs(T * n, -(-T * n // 8))
args = (T, buf["done"], buf["reward"], buf["words"][:T], buf["logp"], buf["val"], buf["act"], sp.reward_scale)
outs = (lb["rec"], lb["stats"], lb["scratch"])
calls = {"tarok_learn_returns": lambda: env.learn_returns(*args, *outs),
         "tarok_learn_returns_gae": lambda: env.learn_returns_gae(*args, GAMMA, LAM, *outs)}

known = {}
for name, fn in calls.items():
    fn()
    torch.cuda.synchronize()
    known[name] = float(lb["stats"][2])

reps, rounds = 50, 7
us = {name: [] for name in calls}
for _ in range(rounds):
    for name, fn in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us[name].append(e0.elapsed_time(e1) * 1e3 / reps)

upd = {"update_fused, Monte-Carlo returns": [], "update_fused, GAE returns": []}
for _ in range(4):
    for name, gae in zip(upd, (False, True)):
        sp.gae, sp.gamma, sp.gae_lambda = gae, GAMMA, LAM
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sp.update_fused(buf, 2, 8)
        torch.cuda.synchronize()
        upd[name].append((time.perf_counter() - t0) * 1e3)

done_frac = float(buf["done"].float().mean())
nbytes = T * n * (1 + 8 + 4 + 4 + 1 + 16 + 8 * done_frac)      # done, word, logp, value, card; the record; scores where done
lines = ["returns of one rollout: %d games x T = %d lock-steps (%d samples), %.4f of them end a game" % (n, T, T * n, done_frac),
         "GAE: gamma = %g, lambda = %g.  %d calls per round, %d rounds, the two kernels alternating; us per call" % (GAMMA, LAM, reps, rounds),
         "(call = returns kernel + k_adv_stats; %.1f MB read and written per call)" % (nbytes / 1e6)]
med = {}
for name, v in us.items():
    med[name] = statistics.median(v)
    lines.append("  %-26s median %7.1f us   min %7.1f   max %7.1f   %6.0f GB/s   known_frac %.6f"
                 % (name, med[name], min(v), max(v), nbytes / med[name] / 1e3, known[name]))
lines.append("  ratio GAE / Monte-Carlo: %.3f" % (med["tarok_learn_returns_gae"] / med["tarok_learn_returns"]))
lines.append("1 - 4/T = %.6f" % (1 - 4 / T))
lines.append("update_fused(epochs = 2, minibatches = 8) on that rollout, ms (host clock to a device synchronise; 4 runs each, alternating):")
for name, v in upd.items():
    lines.append("  %-36s median %7.2f ms   min %7.2f   max %7.2f" % (name, statistics.median(v), min(v), max(v)))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps({"us": med, "known_frac": known, "update_ms": {k: statistics.median(v) for k, v in upd.items()}}))
env.close()
