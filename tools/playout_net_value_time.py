#!/usr/bin/env python3
"""Diagnostic (GPU box): what tarok_playout_cards_net_value costs at depth 1, 2, 3 and 12 (kind 0, the determinized
worlds) beside tarok_playout_cards_net of the same session, at 65,536 games of TAROK_MIX_BOT, worlds = 4, net_seats = 15,
from a fresh deal, after 24 and after 44 Bot cards.  The method is tools/playout_net_worlds_time.py's: each launch (its
three kernels) is captured once into a graph, the graphs are replayed in turn, ROUNDS times after two untimed rounds, every
replay between two device events; a figure is the median of a launch's replays (min, max).  The weights are random: the
time does not depend on them, but for where a Berac ends.

Beside each time stands the forward-row count of tools/playout_net_time.py's prediction: live items (legal cards x worlds
over the games in play) x the card rounds an item can be live for — 47 - cards played for the full playout, and at most
min(that, 7 D) for depth D (6 cards and the stop round for the first decision, at most 7 cards per further one), an upper
bound.  No ratio is asserted anywhere.

usage: playout_net_value_time.py [out.txt = profiles/playout_net_value_times.txt] [games = 65536] [worlds = 4]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_net_value_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
worlds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
ROUNDS = 7
DEPTHS = (1, 2, 3, 12)
assert torch.cuda.is_available(), "this tool measures on the GPU"


def captured(fn):
    fn()                                             # (first launch: code objects, outputs)
    torch.cuda.synchronize()
    graph, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            fn()
    return graph


def replay_us(graphs):
    """{name: (median, min, max) us} of ROUNDS replays each, the graphs taken in turn."""
    us = {k: [] for k in graphs}
    for r in range(2 + ROUNDS):
        for k, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            if r >= 2:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in us.items()}


env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
g = torch.Generator(); g.manual_seed(0)
order = TarokVecEnv.mfma_weight_order
r = lambda *s: torch.randn(*s, generator=g)
lines = ["tarok_playout_cards_net_value (kind 0) by depth at %d games of TAROK_MIX_BOT, worlds = %d, net_seats = 15, seats = 15" % (n, worlds),
         "us per captured launch between device events, median of %d replays (min, max), the launches replayed in turn" % ROUNDS]
out = []
with torch.cuda.device(env.device):
    w = [order((r(256, 256) / 6).to(env.device)), (r(256) / 4).to(env.device), order((r(256, 256) / 12).to(env.device)),
         (r(256) / 4).to(env.device), order((r(64, 256) / 12).to(env.device)), (r(64) / 4).to(env.device)]
    sums = torch.empty((n, K.PLAYOUT_RANKS, 4), dtype=torch.int32, device=env.device)
    acts = torch.empty(n, dtype=torch.uint8, device=env.device)
    env.playout_net_scratch(worlds)
    for cards in (0, 24, 44):
        env.reset(episode=0)
        for _ in range(cards):
            env.step_random(auto_reset=False)
        torch.cuda.synchronize()
        legal = env.legal_actions()
        in_play = ((torch.from_numpy(env.state()[9].astype("int64")) >> 52) & 3) == 2
        items = int(sum(bin(int(m) & ((1 << 54) - 1)).count("1") for m, p in zip(legal.mask_numpy(), in_play.tolist()) if p)) * worlds
        io = dict(sum_out=sums, action_out=acts)
        graphs = dict(net=captured(lambda: env.playout_cards_net(w, worlds, **io)))
        for d in DEPTHS:
            graphs["depth %d" % d] = captured(lambda d=d: env.playout_cards_net_value(w, worlds, d, 70.0, **io))
        t = replay_us(graphs)
        to_go = 47 - cards
        lines.append("after %d cards: %d live items at most" % (cards, items))
        for name in graphs:
            rounds = to_go if name in ("net", "depth 12") else min(to_go, 7 * int(name.split()[1]))
            lines.append("  %-34s %12.1f us (%.1f, %.1f)   / tarok_playout_cards_net %.3f   forward rows <= %.3e"
                         % ("tarok_playout_cards_net" if name == "net" else "tarok_playout_cards_net_value " + name, t[name][0], t[name][1],
                            t[name][2], t[name][0] / t["net"][0], items * rounds))
        out.append(dict(cards=cards, worlds=worlds, items=items, **{k.replace(" ", "_") + "_us": v[0] for k, v in t.items()}))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
env.close()
