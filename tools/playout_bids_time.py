#!/usr/bin/env python3
"""Diagnostic (GPU box): what one tarok_playout_bids launch costs at 65,536 games, (worlds, samples) = (16, 1), every seat a
viewer, with the default contract mask (Klop .. Ena: 13 rows) and the full one (19 rows), and what tarok_bid_round costs
on its sums, beside tarok_playout_cards_det at (16, 1) from a fresh TAROK_MIX_BOT deal in the same process.  Each figure
is the median of 9 launches, each between two device events, after two untimed ones.  (tarok_playout_bids is two
kernels: the deal's and the playouts'; both are inside the figure.)

Prediction from the code: a game costs 4 viewers x rows playout sets of `worlds` whole games, the fresh-deal card launch
one set per legal card (about 12), so the ratio of the two times should sit near 4 * rows / (mean legal cards).  A Berac
row may end early, so the full mask's playouts are a little shorter than 48 cards on average.

usage: playout_bids_time.py [out.txt = profiles/playout_bids_times.txt] [games = 65536] [worlds = 16] [samples = 1]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_bids_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
worlds = int(sys.argv[3]) if len(sys.argv) > 3 else 16
samples = int(sys.argv[4]) if len(sys.argv) > 4 else 1
RUNS = 9
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
rows = {K.BID_DEFAULT_CONTRACTS: 13, K.BID_ALL_CONTRACTS: 19}
res = {}
with torch.cuda.device(env.device):
    bs = torch.empty((n, 4, K.BID_ROWS), dtype=torch.int32, device=env.device)
    sums = torch.empty((n, K.PLAYOUT_RANKS, 4), dtype=torch.int32, device=env.device)
    acts = torch.empty(n, dtype=torch.uint8, device=env.device)
    for mask in (K.BID_DEFAULT_CONTRACTS, K.BID_ALL_CONTRACTS):
        res[mask] = timed_us(lambda: env.playout_bids(0, worlds, samples, contracts=mask, sum_out=bs))
    rnd = timed_us(lambda: env.bid_round(0, bs, worlds * samples, contracts=K.BID_ALL_CONTRACTS))
    env.reset(episode=0)
    words = env.legal_actions().words.cpu().numpy().view(np.uint64)
    legal = np.array([bin(int(w) & K.OBS_MASK).count("1") for w in words], np.int64)
    card = timed_us(lambda: env.playout_cards_det(worlds, samples, sum_out=sums, action_out=acts))
lines = ["tarok_playout_bids at %d games, (worlds, samples) = (%d, %d), seats = 15" % (n, worlds, samples),
         "us per launch between device events, median of %d (min, max); a playout set = worlds * samples whole games" % RUNS]
out = dict(cards_det_us=card[0], bid_round_us=rnd[0], legal=float(legal.mean()))
for mask in (K.BID_DEFAULT_CONTRACTS, K.BID_ALL_CONTRACTS):
    med, lo, hi = res[mask]
    ratio, predicted = med / card[0], 4 * rows[mask] / legal.mean()
    lines.append("  %-46s %10.1f us (%.1f, %.1f)   %2d playout sets per game: measured ratio %.3f, predicted %.3f, measured / predicted %.3f"
                 % ("tarok_playout_bids, contracts 0x%03X (%d rows)" % (mask, rows[mask]), med, lo, hi, 4 * rows[mask], ratio, predicted,
                    ratio / predicted))
    out["bids_0x%03X_us" % mask] = med
lines.append("  %-46s %10.1f us (%.1f, %.1f)   %.2f playout sets per game (legal cards)" % ("tarok_playout_cards_det, fresh deal", card[0], card[1], card[2], legal.mean()))
lines.append("  %-46s %10.1f us (%.1f, %.1f)" % ("tarok_bid_round, seats = 15, full mask", rnd[0], rnd[1], rnd[2]))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
env.close()
