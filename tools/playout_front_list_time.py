#!/usr/bin/env python3
"""Diagnostic (GPU box): what tarok_playout_exchange_net_list / tarok_playout_bids_net_list cost beside their dense parents in
the same session, at 8.14's table rows: 65,536 games at 4 worlds and 4,096 games at 8 worlds of TAROK_MIX_BOT,
net_seats = 15, the exchange at 4 discard sets, the bids at the default contracts — each to the last card (depth None) and
stopped at the viewer's first decision (depth 1); for the bids also with seats = 1 (one viewer) and with pass_value.  A figure
is the median of 5 launches between two device events (min, max), after two untimed ones, all in one process, the launches
taken in turn.  The weights are random: the time does not depend on them, but for where a Berac ends.

Beside each pair stand the list's live items (its total word) over the host's bound and over the dense grid, and the scratch
bytes of both launches.  No ratio is asserted anywhere.

usage: playout_front_list_time.py [out.txt = profiles/playout_front_list_times.txt]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_front_list_times.txt")
SHAPES = ((65536, 4), (4096, 8))
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


def total_word(scratch, bound, units, extra):
    """The list's total: the word after the items, the bids' deal, the units' on and base words and the scan's partials."""
    at = 48 * bound + extra + 8 * units + 4 * ((units + 255) // 256)
    return int(scratch[at:at + 4].cpu().numpy().view("uint32")[0])


lines = ["tarok_playout_exchange_net_list / tarok_playout_bids_net_list beside their dense parents, TAROK_MIX_BOT, net_seats = 15",
         "us per launch between device events, median of %d launches (min, max) after %d untimed, the launches taken in turn, one process"
         % (TIMED, UNTIMED),
         "live: the list's total word; bound: the host's item bound; grid: the dense launch's slots"]
out = []
g = torch.Generator(); g.manual_seed(0)
order = TarokVecEnv.mfma_weight_order
r = lambda *s: torch.randn(*s, generator=g)
for n, W in SHAPES:
    env, bid_env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT), TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
    with torch.cuda.device(env.device):
        w = [order((r(256, 256) / 6).to(env.device)), (r(256) / 4).to(env.device), order((r(256, 256) / 12).to(env.device)),
             (r(256) / 4).to(env.device), order((r(64, 256) / 12).to(env.device)), (r(64) / 4).to(env.device)]
        env.reset(episode=0, defer_exchange=True)
        xs = torch.empty((n, 6 * SETS, 4), dtype=torch.int32, device=env.device)
        xc, xd = torch.empty(n, dtype=torch.int8, device=env.device), torch.empty((n, 3), dtype=torch.uint8, device=env.device)
        bs = torch.empty((n, 4, K.BID_ROWS), dtype=torch.int32, device=env.device)
        xio = dict(sum_out=xs, choice_out=xc, discards_out=xd)
        rows = []
        for depth in (None, 1):
            rows.append(("exchange, depth %s" % depth,
                         lambda d=depth: env.playout_exchange_net_value(w, W, SETS, d, 70.0, **xio),
                         lambda d=depth: env.playout_exchange_net_list(w, W, SETS, d, 70.0, **xio),
                         env.playout_exchange_net_scratch(W, SETS), env.playout_exchange_net_list_scratch(W, SETS),
                         n * 6 * SETS * W, n * 6 * SETS * W, 6 * n, 0))
        for depth, seats, pas in ((None, 15, False), (1, 15, False), (None, 1, False), (1, 1, False), (1, 15, True), (1, 1, True)):
            rcount = 13 + int(pas)
            bound = n * bin(seats).count("1") * rcount * W
            dense = (lambda d=depth, s=seats, p=pas: bid_env.playout_bids_net_value(w, 0, W, d, 70.0, pass_value=p, seats=s, sum_out=bs))
            rows.append(("bids, depth %s, seats %d, pass_value %d" % (depth, seats, pas), dense,
                         lambda d=depth, s=seats, p=pas: bid_env.playout_bids_net_list(w, 0, W, d, 70.0, pass_value=p, seats=s, sum_out=bs),
                         bid_env.playout_bids_net_scratch(W), bid_env.playout_bids_net_list_scratch(W, seats=seats, pass_value=pas),
                         bound, n * 80 * W, 4 * n, 40 * n))
        lines.append("%d games, %d worlds:" % (n, W))
        for name, dense, lst, dscr, lscr, bound, grid, units, extra in rows:
            t = launch_us({"dense": dense, "list": lst})
            torch.cuda.synchronize()
            live = total_word(lscr, bound, units, extra)
            lines.append("  %-40s dense %10.1f us (%.1f, %.1f)   list %10.1f us (%.1f, %.1f)   list / dense %.3f"
                         % (name, *t["dense"], *t["list"], t["list"][0] / t["dense"][0]))
            lines.append("  %-40s live %d = %.3f of the bound %d = %.3f of the grid %d; scratch %d bytes against %d"
                         % ("", live, live / max(1, bound), bound, live / grid, grid, lscr.numel(), dscr.numel()))
            out.append(dict(n=n, worlds=W, row=name, dense_us=t["dense"][0], list_us=t["list"][0], live=live, bound=bound, grid=grid,
                            list_scratch=lscr.numel(), dense_scratch=dscr.numel()))
    env.close()
    bid_env.close()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
