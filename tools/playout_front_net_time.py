#!/usr/bin/env python3
"""Diagnostic (GPU box): what tarok_playout_exchange_net and tarok_playout_bids_net cost, net_seats = 15, random weights,
on TAROK_MIX_BOT envs at the two sizes that matter — 4,096 games with worlds = 8 (the learners' size) and 65,536 games
with worlds = 4 — beside the Bot launches tarok_playout_exchange(W, 1, D) and tarok_playout_bids(W, 1) and ONE
tarok_policy_mlp launch at 65,536 rows, all in one process.  Each figure is the median of RUNS launches, each between two
device events, after two untimed ones; a net launch's three (the bid's four) kernels are all inside its figure.  The
exchange runs at D = 4 discard sets on a reset with the exchange deferred; the bids at the default contracts (13 rows).

Prediction from the forward-row count: an item starts at 0 cards played, so it needs 48 forward rows, and
one tarok_policy_mlp launch is 65,536 forward rows:
    predicted = live items x 48 / 65,536 x (the tarok_policy_mlp time),
with live items = candidates x worlds summed over the waiting games (exchange) or games x 4 viewers x 13 rows x worlds
(bids).  A tile's forward also runs for its dead rows, which the prediction does not count.

usage: playout_front_net_time.py [out.txt = profiles/playout_front_net_times.txt]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "playout_front_net_times.txt")
RUNS, SETS, MLP_ROWS = 5, 4, 65536
SIZES = ((65536, 4), (4096, 8))          # (games, worlds); the first env also times the tarok_policy_mlp launch
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


g = torch.Generator(); g.manual_seed(0)
order = TarokVecEnv.mfma_weight_order
r = lambda *s: torch.randn(*s, generator=g)
lines = ["tarok_playout_exchange_net (D = %d) and tarok_playout_bids_net (default contracts) on TAROK_MIX_BOT, net_seats = 15, seats = 15" % SETS,
         "us per launch between device events, median of %d (min, max); predicted = live items x 48 / %d x the tarok_policy_mlp time" % (RUNS, MLP_ROWS)]
out, mlp = [], None
for n, worlds in SIZES:
    env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
    with torch.cuda.device(env.device):
        w = [order((r(256, 256) / 6).to(env.device)), (r(256) / 4).to(env.device), order((r(256, 256) / 12).to(env.device)),
             (r(256) / 4).to(env.device), order((r(64, 256) / 12).to(env.device)), (r(64) / 4).to(env.device)]
        if mlp is None:
            assert n == MLP_ROWS
            obs = env.reset(episode=0)
            a, lp, v = (torch.empty(n, dtype=dt, device=env.device) for dt in (torch.uint8, torch.float32, torch.float32))
            mlp = timed_us(lambda: env.policy_mlp(w, obs.words, a, lp, v))
            lines.append("tarok_policy_mlp at %d rows: %.1f us (%.1f, %.1f)" % (n, mlp[0], mlp[1], mlp[2]))
        # the exchange
        env.reset(episode=0, defer_exchange=True)
        meta = env.state()[9]
        waiting = ((meta >> np.uint64(52)) & np.uint64(3)) == K.PHASE_EXCHANGE
        contract = ((meta >> np.uint64(33)) & np.uint64(15)).astype(np.int64)
        groups = np.where(waiting, 6 // (3 - ((np.maximum(contract, 1) - 1) % 3)), 0)
        live_x = int(groups.sum()) * SETS * worlds
        xs = torch.empty((n, 6 * SETS, 4), dtype=torch.int32, device=env.device)
        xc, xd = torch.empty(n, dtype=torch.int8, device=env.device), torch.empty((n, 3), dtype=torch.uint8, device=env.device)
        x_scr = env.playout_exchange_net_scratch(worlds, SETS).numel()
        x_net = timed_us(lambda: env.playout_exchange_net(w, worlds, SETS, sum_out=xs, choice_out=xc, discards_out=xd))
        x_bot = timed_us(lambda: env.playout_exchange(worlds, 1, SETS, sum_out=xs, choice_out=xc, discards_out=xd))
        # the bids (the env's games are not read)
        live_b = n * 4 * 13 * worlds
        bs = torch.empty((n, 4, K.BID_ROWS), dtype=torch.int32, device=env.device)
        b_scr = env.playout_bids_net_scratch(worlds).numel()
        b_net = timed_us(lambda: env.playout_bids_net(w, 0, worlds, sum_out=bs))
        b_bot = timed_us(lambda: env.playout_bids(0, worlds, 1, sum_out=bs))
    lines.append("%d games, worlds = %d: %d games wait for the exchange, %.2f groups each" % (n, worlds, int(waiting.sum()), groups.sum() / max(1, waiting.sum())))
    for name, net, bot, live, slots, scr in (("tarok_playout_exchange_net", x_net, x_bot, live_x, n * 6 * SETS * worlds, x_scr),
                                             ("tarok_playout_bids_net", b_net, b_bot, live_b, n * 80 * worlds, b_scr)):
        predicted = live * 48.0 / MLP_ROWS * mlp[0]
        lines.append("  %-28s %12.1f us (%.1f, %.1f)   Bot launch at (W, 1) %10.1f us (%.1f, %.1f)   live items %d of %d slots, scratch %d bytes, "
                     "predicted %.1f us, measured / predicted %.2f, net / Bot %.1f"
                     % (name, net[0], net[1], net[2], bot[0], bot[1], bot[2], live, slots, scr, predicted, net[0] / predicted, net[0] / bot[0]))
        out.append(dict(launch=name, games=n, worlds=worlds, net_us=net[0], bot_us=bot[0], mlp_us=mlp[0], live_items=live, slots=slots,
                        scratch_bytes=scr, predicted_us=predicted))
    env.close()
lines.append("scratch by formula: exchange 288 x D x worlds bytes per game, bids 3,840 x worlds + 40; the bid launch at 65,536 games and "
             "worlds = 16 would need %.2f GB" % ((65536 * (3840 * 16 + 40)) / 1e9))
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(out))
