#!/usr/bin/env python3
"""Diagnostic (GPU box): what valuing the pass costs.  At 65,536 games, (worlds, samples) = (16, 1), every seat a viewer,
both contract masks, each new launch beside its sibling in the same process, alternating:
  tarok_playout_bids_pass  against tarok_playout_bids   (both figures hold the deal's kernel too)
  tarok_bid_values_pass    against tarok_bid_values     (random weights; the deal's kernel too)
  tarok_bid_round_pass     against tarok_bid_round      (on the pass launch's sums, every seat in the set)
Each figure is the median of 9 launches, each between two device events, after two untimed ones of every shape.

Prediction from the code: a viewer's playout sets go from `rows` to rows + 1, so the playout launch should take 14 / 13
of its sibling's time with the default mask and 20 / 19 with the full one — if a pass item cost what a row item costs.
It also runs a bidding round of up to 36 calls in front of the game, which a row item does not.

usage: playout_pass_time.py [out.txt = profiles/playout_pass_times.txt] [games = 65536] [worlds = 16] [samples = 1]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402
from tarok_amd.bidding import pack_weights  # noqa: E402
from tarok_amd.selfplay import PolicyNet  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_pass_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
worlds = int(sys.argv[3]) if len(sys.argv) > 3 else 16
samples = int(sys.argv[4]) if len(sys.argv) > 4 else 1
RUNS = 9
assert torch.cuda.is_available(), "this tool measures on the GPU"


def timed_pair(plain, passing):
    """(median, min, max) in us of both launches, alternating them run by run."""
    for _ in range(2):
        plain(); passing()
    torch.cuda.synchronize()
    us = ([], [])
    for _ in range(RUNS):
        for k, fn in enumerate((plain, passing)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3)
    return [(statistics.median(u), min(u), max(u)) for u in us]


env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
rows = {K.BID_DEFAULT_CONTRACTS: 13, K.BID_ALL_CONTRACTS: 19}
lines = ["the value of a pass at %d games, (worlds, samples) = (%d, %d), seats = 15" % (n, worlds, samples),
         "us per launch between device events, median of %d (min, max), sibling and _pass launch alternating" % RUNS]
out = {}
with torch.cuda.device(env.device):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        weights = pack_weights(PolicyNet(256).to(env.device))
    bs = torch.empty((n, 4, K.BID_ROWS), dtype=torch.int32, device=env.device)
    vs = torch.empty((n, 4, K.BID_ROWS), dtype=torch.int32, device=env.device)
    for mask in (K.BID_DEFAULT_CONTRACTS, K.BID_ALL_CONTRACTS):
        tag = "0x%03X" % mask
        a, b = timed_pair(lambda: env.playout_bids(0, worlds, samples, contracts=mask, sum_out=vs),
                          lambda: env.playout_bids(0, worlds, samples, contracts=mask, sum_out=bs, pass_value=True))
        predicted = (rows[mask] + 1) / rows[mask]
        lines.append("  tarok_playout_bids       %s  %10.1f us (%.1f, %.1f)" % ((tag,) + a))
        lines.append("  tarok_playout_bids_pass  %s  %10.1f us (%.1f, %.1f)   ratio %.4f, predicted %d/%d = %.4f, measured / predicted %.4f"
                     % ((tag,) + b + (b[0] / a[0], rows[mask] + 1, rows[mask], predicted, b[0] / a[0] / predicted)))
        out["bids_" + tag], out["bids_pass_" + tag] = a[0], b[0]
        a, b = timed_pair(lambda: env.bid_values(0, weights, 1120.0, contracts=mask, value_out=vs),
                          lambda: env.bid_values(0, weights, 1120.0, contracts=mask, value_out=vs, pass_value=True))
        lines.append("  tarok_bid_values         %s  %10.1f us (%.1f, %.1f)" % ((tag,) + a))
        lines.append("  tarok_bid_values_pass    %s  %10.1f us (%.1f, %.1f)   ratio %.4f" % ((tag,) + b + (b[0] / a[0],)))
        out["values_" + tag], out["values_pass_" + tag] = a[0], b[0]
        a, b = timed_pair(lambda: env.bid_round(0, bs, worlds * samples, contracts=mask),
                          lambda: env.bid_round(0, bs, worlds * samples, contracts=mask, pass_value=True))
        lines.append("  tarok_bid_round          %s  %10.1f us (%.1f, %.1f)" % ((tag,) + a))
        lines.append("  tarok_bid_round_pass     %s  %10.1f us (%.1f, %.1f)   ratio %.4f" % ((tag,) + b + (b[0] / a[0],)))
        out["round_" + tag], out["round_pass_" + tag] = a[0], b[0]
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
env.close()
