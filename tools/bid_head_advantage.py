#!/usr/bin/env python3
"""Diagnostic (GPU box): does the bidding head learn its teacher, and what is its bid worth?  A BidLearner (teacher
tarok_playout_bids at (8, 2), default contract mask) is trained at 4,096 games for `iterations` fresh episodes; every
`every` iterations the loss on one held-out episode (number 1,000,000, never trained on) is recorded.  Then, on the same
4,096 x 4 deals (seed 0, episodes 0..3 of an evaluation env of its own): evaluate_bidnet_vs_bot with the trained head and
evaluate_bidding_vs_bot(8, 2) with the teacher itself.  The held-out loss of the per-row mean predictor — every row
answered by the mean of its targets over the held-out episode — says how much of the loss the hand explains.

Findings, not bars: no test asserts a sign or a size.

usage: bid_head_advantage.py [out.txt = profiles/bid_head_advantage.txt] [iterations = 300] [every = 25] [games = 4096] [episodes = 4]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402
from tarok_amd import evaluate as E  # noqa: E402
from tarok_amd.bidding import BID_OPTIONS, BidLearner, bid_loss, row_mask  # noqa: E402

argv = sys.argv
out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "bid_head_advantage.txt")
iterations = int(argv[2]) if len(argv) > 2 else 300
every = int(argv[3]) if len(argv) > 3 else 25
n = int(argv[4]) if len(argv) > 4 else 4096
episodes = int(argv[5]) if len(argv) > 5 else 4
HELD_OUT, TRAIN_SEED = 1000000, 1                     # the training env's seed differs from the evaluation's (0)
assert torch.cuda.is_available(), "this tool trains and measures on the GPU"

env = TarokVecEnv(n, seed=TRAIN_SEED, mix=K.MIX_BOT)
lr = BidLearner(env, worlds=8, samples=2, seed=0)
fw, sums, playouts = lr.collect(HELD_OUT)
with torch.no_grad():
    target = sums.reshape(-1, K.BID_ROWS)[:, :BID_OPTIONS].float() * (lr.reward_scale / playouts)
    mean_row = torch.zeros((1, 64), device=target.device)
    mean_row[0, :BID_OPTIONS] = target.mean(0)
    baseline = float(bid_loss(mean_row.expand(target.shape[0], 64), sums.reshape(-1, K.BID_ROWS), playouts, lr.reward_scale, lr.contracts))
    curve = [(0, float(lr.loss(fw, sums, playouts)))]
for it in range(1, iterations + 1):
    lr.iterate()
    if it % every == 0 or it == iterations:
        with torch.no_grad():
            curve.append((it, float(lr.loss(fw, sums, playouts))))
weights = lr.weights()
env.close()
head = E.evaluate_bidnet_vs_bot(weights, n, episodes, seed=0, contracts=lr.contracts, playouts_equiv=lr.playouts_equiv,
                                reward_scale=lr.reward_scale)
teacher = E.evaluate_bidding_vs_bot(8, 2, n, episodes, seed=0, contracts=lr.contracts)
out = dict(games=n, iterations=iterations, teacher=(8, 2), contracts=lr.contracts, rows_learned=int(row_mask(lr.contracts).sum()),
           held_out_loss=curve, held_out_loss_of_the_per_row_mean=baseline, eval_deals=n * episodes,
           bidnet_vs_bot=head, teacher_bidding_vs_bot=teacher)
text = json.dumps(out)
with open(out_path, "w") as f:
    f.write(text + "\n")
print(text)
