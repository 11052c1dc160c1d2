#!/usr/bin/env python3
"""Diagnostic (CPU only, no GPU): what the playout-valued bid is worth, from the model alone —
tests/playout_bids_model.replay_pass on the CPU oracle over the five duplicate passes (seed 0, the device's own deals of
episode 0, the Bot's exchange and the Bot's card on every seat) — so the figures in DESIGN 8.9 do not come from the code
they describe.  evaluate_bidding_vs_bot's figure, once with the default contract mask (Klop .. Ena, the Bot's own range)
and once with the full one, on the same deals; with each the contracts the playout bidder ended up playing.

The deals are spread over worker processes; the result is a function of the arguments alone.

usage: playout_bids_advantage.py [out.txt = profiles/playout_bids_advantage.txt] [deals = 512] [worlds = 8] [samples = 2] [processes = 8]"""
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

PASS_SEATS = (0, 1, 2, 4, 8)
SEED = 0
MASKS = (("default", 0x00F), ("full", 0x3FF))


def bidding_only(args):
    import playout_bids_model as BM
    i, worlds, samples, contracts = args
    out = [BM.replay_pass(SEED, i, 0, seats, worlds, samples, contracts=contracts) for seats in PASS_SEATS]
    return [o[4] for o in out], [(o[0], o[1]) for o in out]


def figures(rows, deals):
    scores = np.asarray(rows, np.int64).transpose(1, 0, 2)               # [5, deals, 4]
    k = np.arange(4)
    diff = scores[1 + k, :, k].T - scores[0][:, k]                       # evaluate.duplicate_advantage, in integers
    per_deal = diff.mean(axis=1)
    return dict(diff_sum=int(diff.sum()), advantage=float(diff.mean()), stderr=float(per_deal.std(ddof=1) / np.sqrt(deals)),
                policy_mean=float(scores[1 + k, :, k].mean()), bot_mean=float(scores[0][:, k].mean()))


def main():
    argv = sys.argv
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "playout_bids_advantage.txt")
    deals = int(argv[2]) if len(argv) > 2 else 512
    worlds = int(argv[3]) if len(argv) > 3 else 8
    samples = int(argv[4]) if len(argv) > 4 else 2
    procs = int(argv[5]) if len(argv) > 5 else 8
    from oracle import oracle as O
    O.build()
    lines = []
    with multiprocessing.Pool(procs) as pool:
        for name, contracts in MASKS:
            res = pool.map(bidding_only, [(i, worlds, samples, contracts) for i in range(deals)], chunksize=4)
            out = dict(mask=name, contracts=contracts, deals=deals, worlds=worlds, samples=samples, bidding_vs_bot=figures([r[0] for r in res], deals))
            declared = [0] * 10                                         # contracts of the games the playout bidder's seat declared
            own = 0
            for r in res:
                for p in range(1, 5):
                    c, d = r[1][p]
                    if c == 0 or d == p - 1:
                        declared[c] += 1
                        own += c != 0
            out["contracts_with_the_playout_bidder_declaring_or_klop"] = declared
            out["games_declared_by_the_playout_bidder"] = own
            out["bot_round_contracts"] = [sum(1 for r in res if r[1][0][0] == c) for c in range(10)]
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
