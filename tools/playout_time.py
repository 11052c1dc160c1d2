#!/usr/bin/env python3
"""Diagnostic (GPU box): what one tarok_playout_cards launch costs (open-hand Monte-Carlo playouts, every seat the
playout player) at 65,536 games with samples = 16, from three positions — a fresh deal, after 24 random cards and after
44 — beside tarok_rollout_random, the nearest existing kernel (whole games in registers), in the same process.

The env plays TAROK_MIX_BOT (the contracts of a Bot bidding round: Klop, Tri, Dve, Ena — no Berac), so every game lasts
exactly 48 cards and the cards a launch plays follow from the positions alone, on the host:
    playout cards = sum over games of  legal cards * samples * (48 - cards played)
(each playout plays its candidate card and then the game to its end); tarok_rollout_random plays 48 * games.
Each figure is the median of `runs` launches, each between two device events, after two untimed ones.

--worlds W adds, at every position and in the same process, the determinized launch tarok_playout_cards_det at
(W, samples) beside the open-hand launch at W * samples playouts per card — the same number of playouts and of cards —
and prints the ratio of the two times (default output then: profiles/playout_det_times.txt).

--voids (with --worlds W): the env keeps the play history, and at every position the void-aware launch
tarok_playout_cards_voids at (W, samples) on tarok_shown_voids' words is timed beside tarok_playout_cards_det at the same
sizes, with the ratio of the two, and tarok_shown_voids alone (default output then: profiles/playout_voids_times.txt).  On a
fresh deal every word is 0 and every game falls back: that ratio is the overhead of the path alone.

--hidden (with --worlds W): the env keeps the play history, and at every position tarok_playout_cards_hidden at
(W, samples) on tarok_played_cards' words is timed beside tarok_playout_cards_det, with the ratio, and tarok_played_cards
alone (default output then: profiles/playout_hidden_times.txt).

usage: playout_time.py [out.txt = profiles/playout_times.txt] [games = 65536] [samples = 16] [--worlds W] [--voids | --hidden]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tarok_amd import TarokVecEnv, karte as K  # noqa: E402

argv = list(sys.argv)
voids = "--voids" in argv
if voids:
    argv.remove("--voids")
hidden = "--hidden" in argv
if hidden:
    argv.remove("--hidden")
worlds = None
if "--worlds" in argv:
    at = argv.index("--worlds")
    worlds = int(argv[at + 1])
    del argv[at:at + 2]
out_path = argv[1] if len(argv) > 1 else os.path.join(
    ROOT, "profiles", "playout_hidden_times.txt" if hidden else "playout_voids_times.txt" if voids else ("playout_det_times.txt" if worlds else "playout_times.txt"))
assert worlds or not (voids or hidden), "--voids and --hidden go with --worlds W"
assert not (voids and hidden), "--voids or --hidden, not both"
n = int(argv[2]) if len(argv) > 2 else 65536
per_world = int(argv[3]) if len(argv) > 3 else (1 if worlds else 16)
samples = per_world * (worlds or 1)          # playouts per card of both launches
RUNS = 9
assert torch.cuda.is_available(), "this tool measures on the GPU"

env = TarokVecEnv(n, seed=0, mix=K.MIX_BOT, history=voids or hidden)


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


lines = ["tarok_playout_cards at %d games, samples = %d, seats = 15 (TAROK_MIX_BOT: every game is 48 cards long)" % (n, samples),
         "us per launch between device events, median of %d (min, max); cards = legal cards * samples * (48 - cards played), summed" % RUNS]
result = {}
with torch.cuda.device(env.device):
    sums = torch.empty((n, K.PLAYOUT_RANKS, 4), dtype=torch.int32, device=env.device)
    acts = torch.empty(n, dtype=torch.uint8, device=env.device)
    med, lo, hi = timed_us(lambda: env.rollout_random(episode=0))
    rate_rollout = 48.0 * n / (med * 1e-6)
    lines.append("  %-28s %10.1f us (%.1f, %.1f)   %12d cards   %8.2f G cards/s" % ("tarok_rollout_random", med, lo, hi, 48 * n, rate_rollout / 1e9))
    result["rollout_random"] = dict(us=med, cards=48 * n, cards_per_s=rate_rollout)
    env.reset(episode=0)
    at = 0
    for cards in (0, 24, 44):
        while at < cards:
            env.step_random(auto_reset=False)
            at += 1
        words = env.legal_actions().words.cpu().numpy().view(np.uint64)
        legal = np.array([bin(int(w) & K.OBS_MASK).count("1") for w in words], np.int64)
        played = ((words >> np.uint64(K.OBS_STEP_SHIFT)) & np.uint64(63)).astype(np.int64)
        assert (played == cards).all() and (legal > 0).all()
        total = int((legal * samples * (48 - played)).sum())
        med, lo, hi = timed_us(lambda: env.playout_cards(samples, sum_out=sums, action_out=acts))
        rate = total / (med * 1e-6)
        lines.append("  %-28s %10.1f us (%.1f, %.1f)   %12d cards   %8.2f G cards/s   %.2f x rollout_random   (%.2f legal cards per game)"
                     % ("playouts after %2d cards" % cards, med, lo, hi, total, rate / 1e9, rate / rate_rollout, legal.mean()))
        result["after_%d" % cards] = dict(us=med, cards=total, cards_per_s=rate, legal_mean=float(legal.mean()))
        if worlds:
            dmed, dlo, dhi = timed_us(lambda: env.playout_cards_det(worlds, per_world, sum_out=sums, action_out=acts))
            lines.append("  %-28s %10.1f us (%.1f, %.1f)   %12d cards   %8.2f G cards/s   %.3f x the open-hand time"
                         % ("  determinized (%d, %d)" % (worlds, per_world), dmed, dlo, dhi, total, total / (dmed * 1e-6) / 1e9, dmed / med))
            result["after_%d" % cards].update(det_us=dmed, det_over_open=dmed / med, worlds=worlds, samples_per_world=per_world)
        if voids:
            vw = torch.empty(n, dtype=torch.int32, device=env.device)
            smed, slo, shi = timed_us(lambda: env.shown_voids(vw))
            torch.cuda.synchronize()
            shown = int((vw != 0).sum().item())
            vmed, vlo, vhi = timed_us(lambda: env.playout_cards_voids(worlds, per_world, voids=vw, sum_out=sums, action_out=acts))
            lines.append("  %-28s %10.1f us (%.1f, %.1f)   %12d cards   %8.2f G cards/s   %.3f x the determinized time   (%d games show a void)"
                         % ("  void-aware (%d, %d)" % (worlds, per_world), vmed, vlo, vhi, total, total / (vmed * 1e-6) / 1e9, vmed / dmed, shown))
            lines.append("  %-28s %10.1f us (%.1f, %.1f)" % ("  tarok_shown_voids", smed, slo, shi))
            result["after_%d" % cards].update(voids_us=vmed, voids_over_det=vmed / dmed, shown_voids_us=smed, games_with_a_void=shown)
        if hidden:
            pw = torch.empty(n, dtype=torch.int64, device=env.device)
            smed, slo, shi = timed_us(lambda: env.played_cards(pw))
            hmed, hlo, hhi = timed_us(lambda: env.playout_cards_hidden(worlds, per_world, played=pw, sum_out=sums, action_out=acts))
            lines.append("  %-28s %10.1f us (%.1f, %.1f)   %12d cards   %8.2f G cards/s   %.3f x the determinized time"
                         % ("  hidden-aware (%d, %d)" % (worlds, per_world), hmed, hlo, hhi, total, total / (hmed * 1e-6) / 1e9, hmed / dmed))
            lines.append("  %-28s %10.1f us (%.1f, %.1f)" % ("  tarok_played_cards", smed, slo, shi))
            result["after_%d" % cards].update(hidden_us=hmed, hidden_over_det=hmed / dmed, played_cards_us=smed)
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(result))
env.close()
