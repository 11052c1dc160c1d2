#!/usr/bin/env python3
"""Diagnostic (CPU only, no GPU): the determinized Monte-Carlo player's duplicate advantage over the Bot, from the model
alone — tests/playout_det_model.replay_pass on the CPU oracle over the five passes of evaluate_playout_vs_bot (seed 0,
TAROK_MIX_BOT, episode 0) — so the figure in DESIGN 8.4 does not come from the code it describes.  The deals are spread
over worker processes; the result is a function of the arguments alone.

--voids: the void-aware player instead (tests/playout_voids_model.replay_pass: worlds that honour the voids shown so far,
DESIGN 8.6), and beside its own figure the paired difference to the determinized player on the same deals.

--hidden: the player whose worlds also re-deal Klop's face-down talon and the declarer's discards instead
(tests/playout_hidden_model.replay_pass), with the same paired difference.

--halving a,b,c,d: the sequential-halving player instead (tests/playout_halving_model.replay_pass) at that
schedule and `samples`, beside the uniform player at `worlds` (give the schedule's sum: the same finalists' worlds) and the
uniform player at the nearest number of card-worlds (worlds = round(the schedule's items at twelve cards / 12)), with the
paired differences halving minus each.

usage: playout_det_advantage.py [deals = 512] [worlds = 8] [samples = 2] [processes = 8] [--voids | --hidden | --halving a,b,c,d]"""
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


def one_deal_voids(args):
    import playout_voids_model as VM
    i, worlds, samples = args
    return [VM.replay_pass(SEED, MIX_BOT, i, 0, seats, worlds, samples)[1] for seats in PASS_SEATS]


def one_deal_hidden(args):
    import playout_hidden_model as HM
    i, worlds, samples = args
    return [HM.replay_pass(SEED, MIX_BOT, i, 0, seats, worlds, samples)[1] for seats in PASS_SEATS]


def one_deal_halving(args):
    import playout_halving_model as HM
    i, schedule, samples = args
    return [HM.replay_pass(SEED, MIX_BOT, i, 0, seats, schedule, samples)[1] for seats in PASS_SEATS]


def figures(rows, deals):
    scores = np.asarray(rows, np.int64).transpose(1, 0, 2)               # [5, deals, 4]
    k = np.arange(4)
    diff = scores[1 + k, :, k].T - scores[0][:, k]                       # evaluate.duplicate_advantage, in integers
    per_deal = diff.mean(axis=1)
    return diff, dict(diff_sum=int(diff.sum()), advantage=float(diff.mean()), stderr=float(per_deal.std(ddof=1) / np.sqrt(deals)),
                      policy_mean=float(scores[1 + k, :, k].mean()), bot_mean=float(scores[0][:, k].mean()))


def main():
    argv, schedule = list(sys.argv), None
    if "--halving" in argv:
        at = argv.index("--halving")
        schedule = tuple(int(w) for w in argv[at + 1].split(","))
        del argv[at:at + 2]
    argv = [a for a in argv if a not in ("--voids", "--hidden")]
    voids, hidden = "--voids" in sys.argv, "--hidden" in sys.argv
    assert not (voids and hidden), "--voids or --hidden, not both"
    deals = int(argv[1]) if len(argv) > 1 else 512
    worlds = int(argv[2]) if len(argv) > 2 else 8
    samples = int(argv[3]) if len(argv) > 3 else 2
    procs = int(argv[4]) if len(argv) > 4 else 8
    from oracle import oracle as O
    O.build()
    work = [(i, worlds, samples) for i in range(deals)]
    with multiprocessing.Pool(procs) as pool:
        diff, out = figures(pool.map(one_deal, work, chunksize=4), deals)
        out = dict(dict(deals=deals, worlds=worlds, samples=samples), **out)
        if voids:
            vdiff, vout = figures(pool.map(one_deal_voids, work, chunksize=4), deals)
            paired = (vdiff - diff).mean(axis=1)                         # per deal: void-aware minus determinized
            out = dict(deals=deals, worlds=worlds, samples=samples, voids=vout, determinized=out,
                       paired_difference=float(paired.mean()), paired_stderr=float(paired.std(ddof=1) / np.sqrt(deals)))
        if hidden:
            hdiff, hout = figures(pool.map(one_deal_hidden, work, chunksize=4), deals)
            paired = (hdiff - diff).mean(axis=1)                         # per deal: hidden-aware minus determinized
            out = dict(deals=deals, worlds=worlds, samples=samples, hidden=hout, determinized=out,
                       paired_difference=float(paired.mean()), paired_stderr=float(paired.std(ddof=1) / np.sqrt(deals)))
        if schedule:
            assert sum(schedule) == worlds, "--halving: give worlds = the schedule's sum"
            items, alive = 0, 12
            for w in schedule:
                items, alive = items + alive * w, max(1, (alive + 1) // 2)
            near = max(1, round(items / 12.0))
            hdiff, hout = figures(pool.map(one_deal_halving, [(i, schedule, samples) for i in range(deals)], chunksize=4), deals)
            ndiff, nout = figures(pool.map(one_deal, [(i, near, samples) for i in range(deals)], chunksize=4), deals)
            pair = lambda d: dict(paired_difference=float((hdiff - d).mean(axis=1).mean()),
                                  paired_stderr=float((hdiff - d).mean(axis=1).std(ddof=1) / np.sqrt(deals)))
            out = dict(deals=deals, samples=samples, halving=dict(schedule=list(schedule), card_worlds_at_12=items, **hout),
                       uniform_full=dict(out, **pair(diff)), uniform_same_cost=dict(dict(worlds=near, card_worlds_at_12=12 * near), **nout, **pair(ndiff)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
