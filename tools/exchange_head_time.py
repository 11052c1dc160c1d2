#!/usr/bin/env python3
"""Diagnostic (GPU box): what the exchange head costs at 65,536 games that wait for the exchange — tarok_exchange_values
with choice and discards only, with raw_out too, and tarok_exchange_candidates — beside its teacher in the same process,
tarok_playout_exchange at (16, 1, 4), and beside one tarok_policy_mlp launch on the same env.  Each figure is the median
of 9 launches, each between two device events, after two untimed ones.

No time or ratio is fixed in advance.  The yardsticks are the teacher and tarok_policy_mlp per row: the head runs the
same forward on eight rows per game (two to six of them live) where the policy runs one.

usage: exchange_head_time.py [out.txt = profiles/exchange_head_times.txt] [games = 65536]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402
from tarok_amd.exchange import ExchangeLearner  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "exchange_head_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
RUNS, WORLDS, SAMPLES, SETS = 9, 16, 1, 4
assert torch.cuda.is_available(), "this tool measures on the GPU"


def timed_us(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us), max(us)


env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT)           # tools/playout_exchange_time.py's games: Klop does not wait
w = ExchangeLearner(None, seed=0).weights()           # an untrained head: the time does not depend on the numbers
res = {}
with torch.cuda.device(env.device):
    w = tuple(t.to(env.device) for t in w)
    env.reset(episode=0, defer_exchange=True)
    choice = torch.empty(n, dtype=torch.int8, device=env.device)
    disc = torch.empty((n, 3), dtype=torch.uint8, device=env.device)
    sums = torch.empty((n, 6 * SETS, 4), dtype=torch.int32, device=env.device)
    res["head"] = timed_us(lambda: env.exchange_values(w, choice_out=choice, discards_out=disc))
    res["head+raw"] = timed_us(lambda: env.exchange_values(w, raw=True, choice_out=choice, discards_out=disc))
    res["candidates"] = timed_us(lambda: env.exchange_candidates(SETS))
    res["teacher"] = timed_us(lambda: env.playout_exchange(WORLDS, SAMPLES, SETS, sum_out=sums, choice_out=choice, discards_out=disc))
    waiting = int((choice >= 0).sum())
    obs = env.exchange(choice, disc)
    a = torch.empty(n, dtype=torch.uint8, device=env.device)
    lp = torch.empty(n, dtype=torch.float32, device=env.device)
    v = torch.empty(n, dtype=torch.float32, device=env.device)
    res["mlp"] = timed_us(lambda: env.policy_mlp(w, obs.words, action_out=a, logp_out=lp, value_out=v))
labels = (("head", "tarok_exchange_values (choice and discards)"), ("head+raw", "tarok_exchange_values (with raw_out, allocated per call)"),
          ("candidates", "tarok_exchange_candidates (D = %d, output allocated per call)" % SETS),
          ("teacher", "tarok_playout_exchange (%d, %d, %d)" % (WORLDS, SAMPLES, SETS)), ("mlp", "tarok_policy_mlp (one row per game)"))
lines = ["the exchange head at %d games of TAROK_MIX_BOT, %d of them waiting for the exchange, seats = 15" % (n, waiting),
         "us between device events, median of %d (min, max)" % RUNS]
out = dict(games=n, waiting=waiting)
for key, label in labels:
    med, lo, hi = res[key]
    lines.append("  %-62s %10.1f us (%.1f, %.1f)" % (label, med, lo, hi))
    out[key + "_us"] = med
lines.append("  teacher / head: %.1f x;  tarok_exchange_values / (8 x tarok_policy_mlp), per row: %.3f"
             % (res["teacher"][0] / res["head"][0], res["head"][0] / (8 * res["mlp"][0])))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
env.close()
