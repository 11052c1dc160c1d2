#!/usr/bin/env python3
"""Diagnostic (GPU box): what the bidding head costs at 65,536 games with every seat bidding — tarok_bid_values (its
k_bid_deal inside the figure) + tarok_bid_round — beside its teacher in the same process, tarok_playout_bids at (16, 1) +
tarok_bid_round, with the default contract mask and the full one, and beside tarok_policy_mlp on the same env.  Each
figure is the median of 9 launches, each between two device events, after two untimed ones.

No time or ratio is fixed in advance.  The yardsticks are the teacher and 4 x tarok_policy_mlp: the head runs the same
forward on four rows per game where the policy runs one, with a cheaper front (a popcount feature build against the
policy's 32-byte state decode) and a cheaper back (no sampler); its extra launch is the deal's sorting network.

usage: bid_head_time.py [out.txt = profiles/bid_head_times.txt] [games = 65536]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402
from tarok_amd.bidding import BidLearner  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bid_head_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
RUNS, WORLDS, SAMPLES = 9, 16, 1
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


env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
w = BidLearner(env, seed=0).weights()                 # an untrained head: the time does not depend on the numbers
scale = 16 * 70.0
res = {}
with torch.cuda.device(env.device):
    vals = torch.empty((n, 4, K.BID_ROWS), dtype=torch.int32, device=env.device)
    for mask in (K.BID_DEFAULT_CONTRACTS, K.BID_ALL_CONTRACTS):
        res["head", mask] = timed_us(lambda: env.bid_values(0, w, scale, contracts=mask, value_out=vals))
        res["round", mask] = timed_us(lambda: env.bid_round(0, vals, 16, contracts=mask))
        res["head+round", mask] = timed_us(lambda: (env.bid_values(0, w, scale, contracts=mask, value_out=vals),
                                                    env.bid_round(0, vals, 16, contracts=mask)))
        res["teacher+round", mask] = timed_us(lambda: (env.playout_bids(0, WORLDS, SAMPLES, contracts=mask, sum_out=vals),
                                                       env.bid_round(0, vals, WORLDS * SAMPLES, contracts=mask)))
    obs = env.reset(episode=0)
    a = torch.empty(n, dtype=torch.uint8, device=env.device)
    lp = torch.empty(n, dtype=torch.float32, device=env.device)
    v = torch.empty(n, dtype=torch.float32, device=env.device)
    mlp = timed_us(lambda: env.policy_mlp(w, obs.words, action_out=a, logp_out=lp, value_out=v))
lines = ["the bidding head at %d games, seats = 15; the teacher at (worlds, samples) = (%d, %d)" % (n, WORLDS, SAMPLES),
         "us between device events, median of %d (min, max)" % RUNS]
out = dict(games=n, policy_mlp_us=mlp[0])
for mask in (K.BID_DEFAULT_CONTRACTS, K.BID_ALL_CONTRACTS):
    for what, label in (("head", "tarok_bid_values (k_bid_deal + k_bid_values)"), ("round", "tarok_bid_round on its values"),
                        ("head+round", "tarok_bid_values + tarok_bid_round"), ("teacher+round", "tarok_playout_bids + tarok_bid_round")):
        med, lo, hi = res[what, mask]
        lines.append("  contracts 0x%03X  %-46s %10.1f us (%.1f, %.1f)" % (mask, label, med, lo, hi))
        out["%s_0x%03X_us" % (what, mask)] = med
    lines.append("  contracts 0x%03X  teacher / head (both with the round): %.1f x;  tarok_bid_values / (4 x tarok_policy_mlp): %.3f"
                 % (mask, res["teacher+round", mask][0] / res["head+round", mask][0], res["head", mask][0] / (4 * mlp[0])))
lines.append("  %-63s %10.1f us (%.1f, %.1f)" % ("tarok_policy_mlp, fresh deal (one row per game)", mlp[0], mlp[1], mlp[2]))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
env.close()
