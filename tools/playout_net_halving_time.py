#!/usr/bin/env python3
"""Diagnostic (GPU box): what tarok_playout_cards_net_halving costs beside tarok_playout_cards_net at the same total worlds
in the same session, at 65,536 games of TAROK_MIX_BOT, net_seats = 15, at the three positions of 8.13's table:
from a fresh deal, after 24 and after 44 Bot cards.  Measured: tarok_playout_cards_net(16) — the dense item layout —, the
new launch at (16,) — the same playouts on the compacted list —, at (2, 2, 4, 8) and at (4, 4, 4, 4), each to the last card
(depth None) and stopped at the viewer's first decision (depth 1).  A figure is the median of 5 launches between two device
events (min, max), after two untimed ones, all in one process, the launches taken in turn.  The weights are random: the
time does not depend on them, but for where a Berac ends.

Beside each time stands the share of the dense launch's (card, world) items the launch played, read off its count_out, and
the share 8.20's table predicts from a fresh deal (0.33 and 0.48).  No ratio is asserted anywhere.

usage: playout_net_halving_time.py [out.txt = profiles/playout_net_halving_times.txt] [games = 65536]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_net_halving_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
WORLDS, TIMED, UNTIMED = 16, 5, 2
SCHEDULES = ((16,), (2, 2, 4, 8), (4, 4, 4, 4))
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


env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
g = torch.Generator(); g.manual_seed(0)
order = TarokVecEnv.mfma_weight_order
r = lambda *s: torch.randn(*s, generator=g)
lines = ["tarok_playout_cards_net_halving beside tarok_playout_cards_net(%d) at %d games of TAROK_MIX_BOT, net_seats = 15, seats = 15" % (WORLDS, n),
         "us per launch between device events, median of %d launches (min, max) after %d untimed, the launches taken in turn, one process"
         % (TIMED, UNTIMED),
         "items: the (card, world) playouts the launch ran over the dense launch's (legal cards x %d), read off count_out" % WORLDS]
out = []
with torch.cuda.device(env.device):
    w = [order((r(256, 256) / 6).to(env.device)), (r(256) / 4).to(env.device), order((r(256, 256) / 12).to(env.device)),
         (r(256) / 4).to(env.device), order((r(64, 256) / 12).to(env.device)), (r(64) / 4).to(env.device)]
    sums = torch.empty((n, K.PLAYOUT_RANKS, 4), dtype=torch.int32, device=env.device)
    counts = torch.empty((n, K.PLAYOUT_RANKS), dtype=torch.int32, device=env.device)
    acts = torch.empty(n, dtype=torch.uint8, device=env.device)
    env.playout_net_scratch(WORLDS)
    for s in SCHEDULES:
        env.playout_net_halving_scratch(s)
    for cards in (0, 24, 44):
        env.reset(episode=0)
        for _ in range(cards):
            env.step_random(auto_reset=False)
        torch.cuda.synchronize()
        io = dict(sum_out=sums, action_out=acts)
        for depth in (None, 1):
            fns = {"net(%d)" % WORLDS: (lambda d=depth: env.playout_cards_net_value(w, WORLDS, d, 70.0, **io))}
            share = {}
            for s in SCHEDULES:
                name = "halving (%s)" % ",".join(map(str, s))
                fns[name] = lambda s=s, d=depth: env.playout_cards_net_halving(w, s, depth=d, count_out=counts, **io)
                fns[name]()
                torch.cuda.synchronize()
                c = counts.cpu().numpy().astype("int64")
                share[name] = c.sum() / float(max(1, (c > 0).sum() * WORLDS))
            t = launch_us(fns)
            base = t["net(%d)" % WORLDS][0]
            lines.append("after %d cards, depth %s:" % (cards, depth))
            for name in fns:
                lines.append("  %-24s %12.1f us (%.1f, %.1f)   / dense %.3f%s"
                             % (name, t[name][0], t[name][1], t[name][2], t[name][0] / base,
                                "   items %.3f" % share[name] if name in share else ""))
            out.append(dict(cards=cards, depth=depth, **{k: v[0] for k, v in t.items()}, **{"items " + k: v for k, v in share.items()}))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
env.close()
