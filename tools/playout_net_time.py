#!/usr/bin/env python3
"""Diagnostic (GPU box): what one tarok_playout_cards_net launch costs at 65,536 games of TAROK_MIX_BOT, worlds in
{4, 8}, net_seats = 15, from a fresh deal, after 24 and after 44 Bot cards — beside tarok_playout_cards_det at
(worlds, 1) and ONE tarok_policy_mlp launch on the same env in the same process.  Each figure is the median of RUNS
launches, each between two device events, after two untimed ones.  (The net launch is three kernels: the items', the
playouts' and the sums'; all are inside the figure.)  The weights are random: the time does not depend on them, but for
where a Berac ends.

Prediction from the forward-row count: a live item needs one forward row per card it has to go, and one
tarok_policy_mlp launch is `games` forward rows, so
    predicted = live items x mean cards to go / games x (the tarok_policy_mlp time),
with live items = legal cards x worlds summed over the games in play and cards to go = 47 - cards played (a Berac may end
earlier; a tile's forward also runs for its dead rows, which the prediction does not count).

usage: playout_net_time.py [out.txt = profiles/playout_net_times.txt] [games = 65536]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_net_times.txt")
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
RUNS = 5
assert torch.cuda.is_available(), "this tool measures on the GPU"


def timed_us(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(us), min(us), max(us)


env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
g = torch.Generator(); g.manual_seed(0)
order = TarokVecEnv.mfma_weight_order
r = lambda *s: torch.randn(*s, generator=g)
lines = ["tarok_playout_cards_net at %d games of TAROK_MIX_BOT, net_seats = 15, seats = 15" % n,
         "us per launch between device events, median of %d (min, max)" % RUNS]
out = []
with torch.cuda.device(env.device):
    w = [order((r(256, 256) / 6).to(env.device)), (r(256) / 4).to(env.device), order((r(256, 256) / 12).to(env.device)),
         (r(256) / 4).to(env.device), order((r(64, 256) / 12).to(env.device)), (r(64) / 4).to(env.device)]
    sums = torch.empty((n, K.PLAYOUT_RANKS, 4), dtype=torch.int32, device=env.device)
    acts = torch.empty(n, dtype=torch.uint8, device=env.device)
    a, lp, v = (torch.empty(n, dtype=dt, device=env.device) for dt in (torch.uint8, torch.float32, torch.float32))
    for cards in (0, 24, 44):
        env.reset(episode=0)
        for _ in range(cards):
            env.step_random(auto_reset=False)
        obs = env.legal_actions()
        words = obs.words.cpu().numpy().view(np.uint64)
        legal = np.array([bin(int(x) & K.OBS_MASK).count("1") for x in words], np.int64)
        mlp = timed_us(lambda: env.policy_mlp(w, obs.words, a, lp, v))
        lines.append("after %d cards: %.2f legal cards per game (%d games in play), tarok_policy_mlp %.1f us (%.1f, %.1f)"
                     % (cards, legal.mean(), int((legal > 0).sum()), mlp[0], mlp[1], mlp[2]))
        for worlds in (4, 8):
            env.playout_net_scratch(worlds)
            net = timed_us(lambda: env.playout_cards_net(w, worlds, sum_out=sums, action_out=acts))
            det = timed_us(lambda: env.playout_cards_det(worlds, 1, sum_out=sums, action_out=acts))
            rows = float(legal.sum()) * worlds * (47 - cards)
            predicted = rows / n * mlp[0]
            lines.append("  worlds %d: tarok_playout_cards_net %12.1f us (%.1f, %.1f)   tarok_playout_cards_det(W, 1) %10.1f us (%.1f, %.1f)   "
                         "forward rows %.3e, predicted %.1f us, measured / predicted %.2f, net / det %.1f"
                         % (worlds, net[0], net[1], net[2], det[0], det[1], det[2], rows, predicted, net[0] / predicted if predicted else 0.0,
                            net[0] / det[0]))
            out.append(dict(cards=cards, worlds=worlds, net_us=net[0], det_us=det[0], mlp_us=mlp[0], predicted_us=predicted))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
env.close()
