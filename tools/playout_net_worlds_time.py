#!/usr/bin/env python3
"""Diagnostic (GPU box): what the net-played card launch costs in each of its three world kinds — tarok_playout_cards_net,
tarok_playout_cards_net_voids, tarok_playout_cards_net_hidden — at 65,536 games of TAROK_MIX_BOT, worlds = 4,
net_seats = 15, from a fresh deal, after 24 and after 44 Bot cards, in one process on one env that keeps its history.
The yardstick is tarok_playout_cards_net of the same session, not an absolute time.

Each launch (its three kernels: the items', the playouts', the sums') is captured once into a graph on the words the env
computed for the position (tarok_shown_voids / tarok_played_cards run before the capture and are outside the figure:
their cost is in profiles/playout_voids_times.txt and profiles/playout_hidden_times.txt).  The three graphs are replayed
in turn, ROUNDS times after two untimed rounds, every replay between two device events; a figure is the median of a
kind's replays (min, max).  The Bot-played launches at (worlds, 1) are timed the same way beside them: their deal-side
ratios bound what the items' kernel can add, and the playouts' kernel dominates the net launch.  The
weights are random: the time does not depend on them, but for where a Berac ends.

usage: playout_net_worlds_time.py [out.txt = profiles/playout_net_worlds_times.txt] [games = 65536] [worlds = 4]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_net_worlds_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
worlds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
ROUNDS = 7
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


env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT, history=True)
g = torch.Generator(); g.manual_seed(0)
order = TarokVecEnv.mfma_weight_order
r = lambda *s: torch.randn(*s, generator=g)
lines = ["the net-played card launch by world kind at %d games of TAROK_MIX_BOT, worlds = %d, net_seats = 15, seats = 15" % (n, worlds),
         "us per captured launch between device events, median of %d replays (min, max), the kinds replayed in turn" % ROUNDS]
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
        voids, played = env.shown_voids(), env.played_cards()
        torch.cuda.synchronize()
        io = dict(sum_out=sums, action_out=acts)
        graphs = dict(net=captured(lambda: env.playout_cards_net(w, worlds, **io)),
                      net_voids=captured(lambda: env.playout_cards_net(w, worlds, voids=voids, **io)),
                      net_hidden=captured(lambda: env.playout_cards_net(w, worlds, hidden=played, **io)),
                      det=captured(lambda: env.playout_cards_det(worlds, 1, **io)),
                      voids=captured(lambda: env.playout_cards_voids(worlds, 1, voids=voids, **io)),
                      hidden=captured(lambda: env.playout_cards_hidden(worlds, 1, played=played, **io)))
        t = replay_us(graphs)
        lines.append("after %d cards: %d games with a shown void" % (cards, int(voids.ne(0).sum())))
        for name, base in (("net", "net"), ("net_voids", "net"), ("net_hidden", "net"), ("det", "det"), ("voids", "det"), ("hidden", "det")):
            lines.append("  %-34s %12.1f us (%.1f, %.1f)   / %s %.3f"
                         % ("tarok_playout_cards_" + name + ("" if name.startswith("net") else "(W, 1)"), t[name][0], t[name][1], t[name][2],
                            "tarok_playout_cards_" + base, t[name][0] / t[base][0]))
        out.append(dict(cards=cards, worlds=worlds, **{k + "_us": v[0] for k, v in t.items()}))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
env.close()
