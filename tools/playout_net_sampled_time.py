#!/usr/bin/env python3
"""Diagnostic (GPU box): what tarok_playout_cards_net_sampled costs, at tools/playout_net_versus_time.py's settings — 65,536 games
of TAROK_MIX_BOT with 16 worlds, from a fresh deal and after 24 Bot cards, (own_rel, opp_rel) = (1, 14) with A != B.
  - the new launch at (samples = 1, temperature 0 on both networks) beside tarok_playout_cards_net_versus of the same session:
    they run the same playouts, so what differs is the sampler's unfolded draw and the row's q byte — a ratio near 1;
  - (worlds 4, samples 4, temperature 1) beside (worlds 16, samples 1, temperature 1): the same 16 playouts a card, from 4
    dealt worlds instead of 16.
The method is that tool's: each launch (its three kernels) is captured once into a graph, the graphs are replayed in turn,
ROUNDS times after two untimed rounds, every replay between two device events; a figure is the median of a launch's replays
(min, max).  The weights are random.  No ratio is asserted anywhere.

usage: playout_net_sampled_time.py [out.txt = profiles/playout_net_sampled_times.txt] [games = 65536] [worlds = 16]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_net_sampled_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
worlds = int(sys.argv[3]) if len(sys.argv) > 3 else 16
ROUNDS = 9
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


def random_net(seed, device):
    g = torch.Generator(); g.manual_seed(seed)
    order = TarokVecEnv.mfma_weight_order
    r = lambda *s: torch.randn(*s, generator=g)
    return [order((r(256, 256) / 6).to(device)), (r(256) / 4).to(device), order((r(256, 256) / 12).to(device)), (r(256) / 4).to(device),
            order((r(64, 256) / 12).to(device)), (r(64) / 4).to(device)]


env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
few = max(1, worlds // 4)
lines = ["tarok_playout_cards_net_sampled beside tarok_playout_cards_net_versus at %d games of TAROK_MIX_BOT, (own_rel, opp_rel) = (1, 14), A != B, "
         "seats = 15" % n,
         "us per captured launch between device events, median of %d replays (min, max), the launches replayed in turn" % ROUNDS]
out = []
with torch.cuda.device(env.device):
    a, b = random_net(0, env.device), random_net(1, env.device)
    sums = torch.empty((n, K.PLAYOUT_RANKS, 4), dtype=torch.int32, device=env.device)
    acts = torch.empty(n, dtype=torch.uint8, device=env.device)
    env.playout_net_scratch(worlds)
    env.playout_net_sampled_scratch(worlds, 1)
    env.playout_net_sampled_scratch(few, worlds // few)
    for cards in (0, 24):
        env.reset(episode=0)
        for _ in range(cards):
            env.step_random(auto_reset=False)
        torch.cuda.synchronize()
        io = dict(sum_out=sums, action_out=acts)
        yard = "versus, worlds %d" % worlds
        graphs = {yard: captured(lambda: env.playout_cards_net_versus(a, b, worlds, 1, 14, **io)),
                  "sampled, worlds %d, samples 1, T = 0" % worlds: captured(
                      lambda: env.playout_cards_net_sampled(a, b, worlds, 1, 1, 14, temperature=0.0, **io)),
                  "sampled, worlds %d, samples 1, T = 1" % worlds: captured(
                      lambda: env.playout_cards_net_sampled(a, b, worlds, 1, 1, 14, temperature=1.0, **io)),
                  "sampled, worlds %d, samples %d, T = 1" % (few, worlds // few): captured(
                      lambda: env.playout_cards_net_sampled(a, b, few, worlds // few, 1, 14, temperature=1.0, **io))}
        t = replay_us(graphs)
        base = t[yard][0]
        lines.append("after %d cards:" % cards)
        for name in graphs:
            lines.append("  %-42s %12.1f us (%.1f, %.1f)   / the versus launch %.3f" % (name, t[name][0], t[name][1], t[name][2], t[name][0] / base))
        out.append(dict(cards=cards, worlds=worlds, **{k: v[0] for k, v in t.items()}))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
env.close()
