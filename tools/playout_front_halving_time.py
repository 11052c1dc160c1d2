#!/usr/bin/env python3
"""Diagnostic (GPU box): what tarok_playout_exchange_net_halving / tarok_playout_bids_net_halving cost beside the _net_list
launch at the same total W in the same session, by 8.22's method: TAROK_MIX_BOT, net_seats = 15, the exchange at
4 discard sets, the bids at the default contracts, each to the last card (depth None) and stopped at the viewer's first decision
(depth 1), the bids also with the pass.  The schedules are (W,), (2,2,4,8) and (4,4,4,4), at 65,536 and at 4,096 games.  A
figure is the median of 5 launches between two device events (min, max), after two untimed ones, all in one process, the
launches taken in turn.  The weights are random.

Beside each pair stands the share of items run: the sum of count_out over the live rows against W for each of them.  No ratio
is asserted anywhere.

usage: playout_front_halving_time.py [out.txt = profiles/playout_front_halving_times.txt]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_front_halving_times.txt")
GAMES = (65536, 4096)
SCHEDULES = ((16,), (2, 2, 4, 8), (4, 4, 4, 4))
SETS, TIMED, UNTIMED = 4, 5, 2
assert torch.cuda.is_available(), "this tool measures on the GPU"


def launch_us(fns):
    """{name: (median, min, max) us} of TIMED launches each after UNTIMED untimed ones, the launches taken in turn."""
    us = {k: [] for k in fns}
    for r in range(UNTIMED + TIMED):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= UNTIMED:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


def share(count, W):
    """The items run over those of the uniform launch: the counts summed over the rows that played, against W for each."""
    live = count > 0
    return float(count.sum()) / max(1.0, float(live.sum()) * W)


lines = ["tarok_playout_exchange_net_halving / tarok_playout_bids_net_halving beside the _net_list launch at W = 16, TAROK_MIX_BOT, net_seats = 15",
         "us per launch between device events, median of %d launches (min, max) after %d untimed, the launches taken in turn, one process"
         % (TIMED, UNTIMED),
         "items: the sum of count_out over the rows that played, against W for each of them"]
out = []
g = torch.Generator(); g.manual_seed(0)
order = TarokVecEnv.mfma_weight_order
r = lambda *s: torch.randn(*s, generator=g)
W = 16
for n in GAMES:
    env, bid_env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT), TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
    with torch.cuda.device(env.device):
        w = [order((r(256, 256) / 6).to(env.device)), (r(256) / 4).to(env.device), order((r(256, 256) / 12).to(env.device)),
             (r(256) / 4).to(env.device), order((r(64, 256) / 12).to(env.device)), (r(64) / 4).to(env.device)]
        env.reset(episode=0, defer_exchange=True)
        xs, xn = (torch.empty((n, 6 * SETS, k), dtype=torch.int32, device=env.device) for k in (4, 1))
        xc, xd = torch.empty(n, dtype=torch.int8, device=env.device), torch.empty((n, 3), dtype=torch.uint8, device=env.device)
        bs, bn, bv = (torch.empty((n, 4, K.BID_ROWS), dtype=torch.int32, device=env.device) for _ in range(3))
        lines.append("%d games, W = %d:" % (n, W))
        for schedule in SCHEDULES:
            rows = []
            for depth in (None, 1):
                rows.append(("exchange, depth %s" % depth,
                             lambda d=depth: env.playout_exchange_net_list(w, W, SETS, d, 70.0, sum_out=xs, choice_out=xc, discards_out=xd),
                             lambda d=depth: env.playout_exchange_net_halving(w, schedule, SETS, d, 70.0, sum_out=xs, count_out=xn.view(n, -1),
                                                                              choice_out=xc, discards_out=xd),
                             lambda: share(xn, W)))
            for depth, pas in ((None, False), (1, False), (1, True)):
                rows.append(("bids, depth %s, pass_value %d" % (depth, pas),
                             lambda d=depth, p=pas: bid_env.playout_bids_net_list(w, 0, W, d, 70.0, pass_value=p, sum_out=bs),
                             lambda d=depth, p=pas: bid_env.playout_bids_net_halving(w, 0, schedule, d, 70.0, pass_value=p, sum_out=bs,
                                                                                     count_out=bn, value_out=bv),
                             lambda: share(bn, W)))
            for name, lst, halving, items in rows:
                t = launch_us({"list": lst, "halving": halving})
                torch.cuda.synchronize()
                frac = items()
                lines.append("  %-16s %-32s list %10.1f us (%.1f, %.1f)   halving %10.1f us (%.1f, %.1f)   halving / list %.3f   items %.3f"
                             % (schedule, name, *t["list"], *t["halving"], t["halving"][0] / t["list"][0], frac))
                out.append(dict(n=n, schedule=list(schedule), row=name, list_us=t["list"][0], halving_us=t["halving"][0], items=frac))
    env.close()
    bid_env.close()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
