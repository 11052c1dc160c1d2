#!/usr/bin/env python3
"""Diagnostic (CPU only, no GPU): what the playout-valued talon exchange is worth, from the model alone —
tests/playout_exchange_model.replay_pass on the CPU oracle over the five duplicate passes (seed 0, TAROK_MIX_BOT,
episode 0) — so the figures in DESIGN 8.7 do not come from the code they describe.  Two figures on the same deals:

  exchange_vs_bot   evaluate_exchange_vs_bot's: the playout player makes the exchange of its seat's declared games, the
                    Bot plays every card; duplicate advantage over the Bot everywhere.
  paired            the determinized card player (tests/playout_det_model.py) with the exchange front end
                    (evaluate_playout_vs_bot(worlds=W, exchange=D)) minus the same player without it, per deal.

The deals are spread over worker processes; the result is a function of the arguments alone.

usage: playout_exchange_advantage.py [deals = 512] [worlds = 8] [samples = 2] [discard_sets = 4] [processes = 8] [--no-cards]"""
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


def exchange_only(args):
    import playout_exchange_model as XM
    i, worlds, samples, sets = args
    return [XM.replay_pass(SEED, MIX_BOT, i, 0, seats, worlds, samples, sets)[3] for seats in PASS_SEATS]


def cards_with_exchange(args):
    import playout_exchange_model as XM
    i, worlds, samples, sets = args
    return [XM.replay_pass(SEED, MIX_BOT, i, 0, seats, worlds, samples, sets, cards=True)[3] for seats in PASS_SEATS]


def cards_alone(args):
    import playout_det_model as DM
    i, worlds, samples, _ = args
    return [DM.replay_pass(SEED, MIX_BOT, i, 0, seats, worlds, samples)[1] for seats in PASS_SEATS]


def figures(rows, deals):
    scores = np.asarray(rows, np.int64).transpose(1, 0, 2)               # [5, deals, 4]
    k = np.arange(4)
    diff = scores[1 + k, :, k].T - scores[0][:, k]                       # evaluate.duplicate_advantage, in integers
    per_deal = diff.mean(axis=1)
    return diff, dict(diff_sum=int(diff.sum()), advantage=float(diff.mean()), stderr=float(per_deal.std(ddof=1) / np.sqrt(deals)),
                      policy_mean=float(scores[1 + k, :, k].mean()), bot_mean=float(scores[0][:, k].mean()))


def main():
    argv = [a for a in sys.argv if a != "--no-cards"]
    with_cards = len(argv) == len(sys.argv)
    deals = int(argv[1]) if len(argv) > 1 else 512
    worlds = int(argv[2]) if len(argv) > 2 else 8
    samples = int(argv[3]) if len(argv) > 3 else 2
    sets = int(argv[4]) if len(argv) > 4 else 4
    procs = int(argv[5]) if len(argv) > 5 else 8
    from oracle import oracle as O
    O.build()
    work = [(i, worlds, samples, sets) for i in range(deals)]
    out = dict(deals=deals, worlds=worlds, samples=samples, discard_sets=sets)
    with multiprocessing.Pool(procs) as pool:
        _, out["exchange_vs_bot"] = figures(pool.map(exchange_only, work, chunksize=4), deals)
        print(json.dumps(out), flush=True)
        if with_cards:
            xdiff, out["cards_with_exchange"] = figures(pool.map(cards_with_exchange, work, chunksize=2), deals)
            pdiff, out["cards_alone"] = figures(pool.map(cards_alone, work, chunksize=2), deals)
            paired = (xdiff - pdiff).mean(axis=1)                        # per deal: with the exchange minus without
            out["paired_difference"] = float(paired.mean())
            out["paired_stderr"] = float(paired.std(ddof=1) / np.sqrt(deals))
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
