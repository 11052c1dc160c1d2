#!/usr/bin/env python3
"""Diagnostic (CPU only, no GPU): what valuing the pass by playouts is worth, from the model alone —
tests/playout_pass_model.replay_pass (the pass-aware bidder, margin 0) beside tests/playout_bids_model.replay_pass (the
threshold-0 bidder of DESIGN 8.9) on the SAME deals over the five duplicate passes (seed 0, the device's own deals of
episode 0, the Bot's exchange and the Bot's card on every seat) — so the figures in DESIGN 8.12 do not come from the code
they describe.  Per contract mask: both advantages over the Bot and their paired difference with its standard error.

The deals are spread over worker processes; the result is a function of the arguments alone.

usage: playout_pass_advantage.py [out.txt = profiles/playout_pass_advantage.txt] [deals = 512] [worlds = 8] [samples = 2] [processes = 8]"""
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


def both_bidders(args):
    import playout_bids_model as BM
    import playout_pass_model as PS
    i, worlds, samples, contracts = args
    plain = [BM.replay_pass(SEED, i, 0, seats, worlds, samples, contracts=contracts) for seats in PASS_SEATS]
    aware = [PS.replay_pass(SEED, i, 0, seats, worlds, samples, contracts=contracts, margin=0) for seats in PASS_SEATS]
    return [o[4] for o in plain], [o[4] for o in aware], [(o[0], o[1]) for o in plain], [(o[0], o[1]) for o in aware]


def seat_diffs(rows):
    """[deals, 4]: the bidder's score on seat k in pass 1 + k minus the Bot's on that seat in pass 0."""
    scores = np.asarray(rows, np.int64).transpose(1, 0, 2)               # [5, deals, 4]
    k = np.arange(4)
    return scores[1 + k, :, k].T - scores[0][:, k], scores


def figures(diff, scores, deals):
    k = np.arange(4)
    return dict(diff_sum=int(diff.sum()), advantage=float(diff.mean()), stderr=float(diff.mean(axis=1).std(ddof=1) / np.sqrt(deals)),
                policy_mean=float(scores[1 + k, :, k].mean()), bot_mean=float(scores[0][:, k].mean()))


def main():
    argv = sys.argv
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "playout_pass_advantage.txt")
    deals = int(argv[2]) if len(argv) > 2 else 512
    worlds = int(argv[3]) if len(argv) > 3 else 8
    samples = int(argv[4]) if len(argv) > 4 else 2
    procs = int(argv[5]) if len(argv) > 5 else 8
    from oracle import oracle as O
    O.build()
    lines = []
    with multiprocessing.Pool(procs) as pool:
        for name, contracts in MASKS:
            res = pool.map(both_bidders, [(i, worlds, samples, contracts) for i in range(deals)], chunksize=4)
            d_plain, s_plain = seat_diffs([r[0] for r in res])
            d_aware, s_aware = seat_diffs([r[1] for r in res])
            paired = (d_aware - d_plain).mean(axis=1)                       # per deal: the mean over the four seats
            out = dict(mask=name, contracts=contracts, deals=deals, worlds=worlds, samples=samples, margin=0,
                       threshold_0_vs_bot=figures(d_plain, s_plain, deals), pass_aware_vs_bot=figures(d_aware, s_aware, deals),
                       pass_aware_minus_threshold_0=dict(diff_sum=int((d_aware - d_plain).sum()), difference=float(paired.mean()),
                                                         stderr=float(paired.std(ddof=1) / np.sqrt(deals))))
            out["rounds_that_differ"] = sum(1 for r in res for p in range(1, 5) if r[2][p] != r[3][p])
            out["games_declared_by_the_bidder"] = dict(
                threshold_0=sum(1 for r in res for p in range(1, 5) if r[2][p][0] != 0 and r[2][p][1] == p - 1),
                pass_aware=sum(1 for r in res for p in range(1, 5) if r[3][p][0] != 0 and r[3][p][1] == p - 1))
            lines.append(json.dumps(out))
            print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
