#!/usr/bin/env python3
"""Diagnostic (GPU box): does the exchange head learn its teacher, and what is its exchange worth?  An ExchangeLearner
(teacher tarok_playout_exchange at (8, 2, 4)) is trained at 4,096 games for `iterations` fresh episodes; the loss on one
held-out episode (number 1,000,000, never trained on) is recorded before training and after 25, 150 and `iterations`
iterations.  Then, on the same 4,096 x 4 deals (seed 0, episodes 0..3 of an evaluation env of its own):
evaluate_exchangenet_vs_bot with the trained head and evaluate_exchange_vs_bot(8, 2, 4) with the teacher itself.  The
held-out loss of the per-row mean predictor — row i's value answered by the mean value target of the rows i, card c's
score in row i by the mean of its known targets — says how much of the loss the cards explain.

Findings, not bars: no test asserts a sign or a size.

usage: exchange_head_advantage.py [out.txt = profiles/exchange_head_advantage.txt] [iterations = 300] [games = 4096] [episodes = 4]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402
from tarok_amd import evaluate as E  # noqa: E402
from tarok_amd.exchange import ExchangeLearner, exchange_loss, exchange_targets  # noqa: E402

argv = sys.argv
out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "exchange_head_advantage.txt")
iterations = int(argv[2]) if len(argv) > 2 else 300
n = int(argv[3]) if len(argv) > 3 else 4096
episodes = int(argv[4]) if len(argv) > 4 else 4
HELD_OUT, TRAIN_SEED = 1000000, 1                     # the training env's seed differs from the evaluation's (0)
TEACHER = (8, 2, 4)
assert torch.cuda.is_available(), "this tool trains and measures on the GPU"

env = TarokVecEnv(n, seed=TRAIN_SEED, mix=K.MIX_BOT)
lr = ExchangeLearner(env, worlds=TEACHER[0], samples=TEACHER[1], discard_sets=TEACHER[2], seed=0)
held = lr.collect(HELD_OUT)
with torch.no_grad():
    live, value, score, known = exchange_targets(held[0], held[1], held[2], held[3], lr.reward_scale)
    mean = torch.zeros((1, 6, 64), device=value.device)
    mean[0, :, 54] = (value * live).sum(0) / live.sum(0).clamp(min=1)
    mean[0, :, :54] = (score * known).sum(0) / known.sum(0).clamp(min=1)
    baseline = float(exchange_loss(mean.expand(value.shape[0], 6, 64), live, value, score, known))
    curve = [(0, float(lr.loss(*held)))]
for it in range(1, iterations + 1):
    lr.iterate()
    if it in (25, 150, iterations):
        with torch.no_grad():
            curve.append((it, float(lr.loss(*held))))
weights = lr.weights()
env.close()
head = E.evaluate_exchangenet_vs_bot(weights, n, episodes, seed=0)
teacher = E.evaluate_exchange_vs_bot(TEACHER[0], TEACHER[1], TEACHER[2], n, episodes, seed=0)
out = dict(games=n, iterations=iterations, teacher=TEACHER, live_rows_held_out=int(live.sum()), known_scores_held_out=int(known.sum()),
           held_out_loss=curve, held_out_loss_of_the_per_row_mean=baseline, eval_deals=n * episodes,
           exchangenet_vs_bot=head, teacher_exchange_vs_bot=teacher)
text = json.dumps(out)
with open(out_path, "w") as f:
    f.write(text + "\n")
print(text)
