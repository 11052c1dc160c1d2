#!/usr/bin/env python3
"""Diagnostic (GPU box): what tarok_playout_exchange_net_value and tarok_playout_bids_net_value cost at depths 1, 2, 3 and
13 beside tarok_playout_exchange_net / tarok_playout_bids_net of the same session, net_seats = 15, random weights, on
TAROK_MIX_BOT envs at 65,536 games with worlds = 4 and at 4,096 games with worlds = 8 (the learners' size); and the pass
item's share (pass_value = 1 against 0) at depths 1 and 13.  Every launch is captured into a graph once; a figure is the
median of RUNS replays, each between two device events, with min and max.  The exchange runs at D = 4 discard sets on a
reset with the exchange deferred; the bids at the default contracts (13 rows, 14 with the pass).

Prediction from the forward rounds: an item starts at 0 cards played and runs 48 forward rounds to its last
card; the viewer's first decision falls within the first four positions and a seat plays once per trick, so depth d runs
at most 4 d rounds:  predicted(d) = min(4 d, 48) / 48 x (the existing launch's time of this session).  It is an upper
bound on the play kernel's share and leaves out the item kernel and the sums, which do not shrink with the depth.
Nothing is asserted.  Depth 13 is to lie inside the existing launch's replay spread.

usage: playout_front_net_value_time.py [out.txt = profiles/playout_front_net_value_times.txt]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_front_net_value_times.txt")
RUNS, SETS = 7, 4
SIZES = ((65536, 4), (4096, 8))          # (games, worlds)
DEPTHS = (1, 2, 3, 13)
assert torch.cuda.is_available(), "this tool measures on the GPU"


def replayed_us(fn):
    """fn captured once (after two eager calls), then RUNS replays between device events: (median, min, max) in us."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us), max(us)


g = torch.Generator(); g.manual_seed(0)
order = TarokVecEnv.mfma_weight_order
r = lambda *s: torch.randn(*s, generator=g)
lines = ["tarok_playout_exchange_net_value (D = %d) and tarok_playout_bids_net_value (default contracts) on TAROK_MIX_BOT, net_seats = 15, "
         "seats = 15, value_scale = 70" % SETS,
         "us per captured replay between device events, median of %d (min, max); predicted = min(4 d, 48) / 48 x the existing launch" % RUNS]
out = []
for n, worlds in SIZES:
    env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
    with torch.cuda.device(env.device):
        w = [order((r(256, 256) / 6).to(env.device)), (r(256) / 4).to(env.device), order((r(256, 256) / 12).to(env.device)),
             (r(256) / 4).to(env.device), order((r(64, 256) / 12).to(env.device)), (r(64) / 4).to(env.device)]
        env.reset(episode=0, defer_exchange=True)
        xs = torch.empty((n, 6 * SETS, 4), dtype=torch.int32, device=env.device)
        xc, xd = torch.empty(n, dtype=torch.int8, device=env.device), torch.empty((n, 3), dtype=torch.uint8, device=env.device)
        bs = torch.empty((n, 4, K.BID_ROWS), dtype=torch.int32, device=env.device)
        env.playout_exchange_net_scratch(worlds, SETS), env.playout_bids_net_scratch(worlds)      # allocated before any capture
        x_full = replayed_us(lambda: env.playout_exchange_net(w, worlds, SETS, sum_out=xs, choice_out=xc, discards_out=xd))
        b_full = replayed_us(lambda: env.playout_bids_net(w, 0, worlds, sum_out=bs))
        lines.append("%d games, worlds = %d" % (n, worlds))
        lines.append("  %-44s %12.1f us (%.1f, %.1f)" % ("tarok_playout_exchange_net", *x_full))
        lines.append("  %-44s %12.1f us (%.1f, %.1f)" % ("tarok_playout_bids_net", *b_full))
        for d in DEPTHS:
            x = replayed_us(lambda: env.playout_exchange_net_value(w, worlds, SETS, d, sum_out=xs, choice_out=xc, discards_out=xd))
            b = replayed_us(lambda: env.playout_bids_net_value(w, 0, worlds, d, sum_out=bs))
            row = dict(games=n, worlds=worlds, depth=d, exchange_us=x[0], bids_us=b[0], exchange_full_us=x_full[0], bids_full_us=b_full[0])
            for name, t, full in (("tarok_playout_exchange_net_value", x, x_full), ("tarok_playout_bids_net_value", b, b_full)):
                bound = min(4 * d, 48) / 48.0
                inside = "" if d < 13 else ("   inside the existing launch's spread" if full[1] <= t[0] <= full[2] else "   OUTSIDE the existing launch's spread")
                lines.append("  %-34s depth %2d %12.1f us (%.1f, %.1f)   / existing %.3f   predicted <= %.3f (%.1f us)%s"
                             % (name, d, t[0], t[1], t[2], t[0] / full[0], bound, bound * full[0], inside))
            if d in (1, 13):
                p = replayed_us(lambda: env.playout_bids_net_value(w, 0, worlds, d, pass_value=True, sum_out=bs))
                row["bids_pass_us"] = p[0]
                lines.append("  %-34s depth %2d %12.1f us (%.1f, %.1f)   the pass's share %+.1f us = %.1f %% (one row more on 13: %.1f %%)"
                             % ("  ... with pass_value = 1", d, p[0], p[1], p[2], p[0] - b[0], 100.0 * (p[0] - b[0]) / b[0], 100.0 / 13))
            out.append(row)
    env.close()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
