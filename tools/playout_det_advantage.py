#!/usr/bin/env python3
"""Diagnostic (CPU only, no GPU): the determinized Monte-Carlo player's duplicate advantage over the Bot, from the model
alone — tests/playout_det_model.replay_pass on the CPU oracle over the five passes of evaluate_playout_vs_bot (seed 0,
TAROK_MIX_BOT, episode 0) — so the figure in DESIGN 8.4 does not come from the code it describes.  The deals are spread
over worker processes; the result is a function of the arguments alone.

usage: playout_det_advantage.py [deals = 512] [worlds = 8] [samples = 2] [processes = 8]"""
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

PASS_SEATS = (0, 1, 2, 4, 8)
SEED, MIX_BOT = 0, 2


def one_deal(args):
    import playout_det_model as DM
    i, worlds, samples = args
    return [DM.replay_pass(SEED, MIX_BOT, i, 0, seats, worlds, samples)[1] for seats in PASS_SEATS]


def main():
    deals = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    worlds = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    samples = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    procs = int(sys.argv[4]) if len(sys.argv) > 4 else 8
    from oracle import oracle as O
    O.build()
    with multiprocessing.Pool(procs) as pool:
        rows = pool.map(one_deal, [(i, worlds, samples) for i in range(deals)], chunksize=4)
    scores = np.asarray(rows, np.int64).transpose(1, 0, 2)               # [5, deals, 4]
    k = np.arange(4)
    diff = scores[1 + k, :, k].T - scores[0][:, k]                       # evaluate.duplicate_advantage, in integers
    per_deal = diff.mean(axis=1)
    out = dict(deals=deals, worlds=worlds, samples=samples, diff_sum=int(diff.sum()), advantage=float(diff.mean()),
               stderr=float(per_deal.std(ddof=1) / np.sqrt(deals)), policy_mean=float(scores[1 + k, :, k].mean()),
               bot_mean=float(scores[0][:, k].mean()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
