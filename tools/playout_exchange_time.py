#!/usr/bin/env python3
"""Diagnostic (GPU box): what one tarok_playout_exchange launch costs at 65,536 games of TAROK_MIX_BOT waiting for the
exchange, at (worlds, samples, discard_sets) = (16, 1, 4) with every seat in the set, beside tarok_playout_cards_det at
(16, 1) on the same env after the exchange (0 cards played), in the same process.  Each figure is the median of 9
launches, each between two device events, after two untimed ones.

Prediction from the code: a game that takes part costs ngroups * discard_sets playout sets of `worlds` whole games; the
fresh-deal card launch costs one set per legal card (about 12) in EVERY game, so the ratio of the two times should sit
near  (sum over waiting games of ngroups * discard_sets) / (sum over all games of legal cards).  Both sums are computed
here from the env's state; the measured ratio and its distance from that prediction are written beside them.

usage: playout_exchange_time.py [out.txt = profiles/playout_exchange_times.txt] [games = 65536] [worlds = 16] [samples = 1] [discard_sets = 4]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_exchange_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
worlds = int(sys.argv[3]) if len(sys.argv) > 3 else 16
samples = int(sys.argv[4]) if len(sys.argv) > 4 else 1
sets = int(sys.argv[5]) if len(sys.argv) > 5 else 4
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
env.reset(episode=0, defer_exchange=True)
meta = env.state()[9]
phase = (meta >> np.uint64(52)) & np.uint64(3)
contract = ((meta >> np.uint64(33)) & np.uint64(15)).astype(np.int64)
waiting = phase == 1
ngroups = np.where(waiting, 6 // np.maximum(3 - ((contract - 1) % 3), 1), 0)     # group size 3, 2, 1 for Tri.., Dve.., Ena..
cand_sets = int((ngroups * sets).sum())
with torch.cuda.device(env.device):
    xs = torch.empty((n, 6 * sets, 4), dtype=torch.int32, device=env.device)
    ch = torch.empty(n, dtype=torch.int8, device=env.device)
    di = torch.empty((n, 3), dtype=torch.uint8, device=env.device)
    sums = torch.empty((n, K.PLAYOUT_RANKS, 4), dtype=torch.int32, device=env.device)
    acts = torch.empty(n, dtype=torch.uint8, device=env.device)
    xmed, xlo, xhi = timed_us(lambda: env.playout_exchange(worlds, samples, sets, sum_out=xs, choice_out=ch, discards_out=di))
    env.exchange(ch, di)
    words = env.legal_actions().words.cpu().numpy().view(np.uint64)
    legal = np.array([bin(int(w) & K.OBS_MASK).count("1") for w in words], np.int64)
    assert (((words >> np.uint64(K.OBS_STEP_SHIFT)) & np.uint64(63)) == 0).all() and (legal > 0).all()
    card_sets = int(legal.sum())
    cmed, clo, chi = timed_us(lambda: env.playout_cards_det(worlds, samples, sum_out=sums, action_out=acts))
ratio, predicted = xmed / cmed, cand_sets / card_sets
lines = ["tarok_playout_exchange at %d games of TAROK_MIX_BOT, (worlds, samples, discard_sets) = (%d, %d, %d), seats = 15" % (n, worlds, samples, sets),
         "us per launch between device events, median of %d (min, max); a playout set = worlds * samples whole games of 48 cards" % RUNS,
         "  games waiting for the exchange: %d of %d (the others are Klop); candidates per game over ALL games: %.3f (%.3f per waiting game)"
         % (int(waiting.sum()), n, cand_sets / n, cand_sets / max(int(waiting.sum()), 1)),
         "  %-44s %10.1f us (%.1f, %.1f)   %10d playout sets" % ("tarok_playout_exchange", xmed, xlo, xhi, cand_sets),
         "  %-44s %10.1f us (%.1f, %.1f)   %10d playout sets   (%.2f legal cards per game)"
         % ("tarok_playout_cards_det after the exchange", cmed, clo, chi, card_sets, legal.mean()),
         "  measured ratio %.3f; predicted from the playout sets %.3f; measured / predicted %.3f" % (ratio, predicted, ratio / predicted)]
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(dict(exchange_us=xmed, cards_det_us=cmed, ratio=ratio, predicted=predicted, waiting=int(waiting.sum()),
                      candidate_sets=cand_sets, card_sets=card_sets)))
env.close()
