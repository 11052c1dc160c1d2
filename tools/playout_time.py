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

--halving a,b,c,d[/a,b,c,d ...] (with --worlds W, W the schedules' sum): at every position tarok_playout_cards_halving at each
schedule (the det kind, `samples` per world) is timed beside tarok_playout_cards_det at (W, samples), with the measured
ratio next to the one the item count predicts for twelve legal cards (default output then:
profiles/playout_halving_times.txt).  The dealing of all W worlds and the two barriers a round are not halved.
--teacher (with --halving): also the rollout of DESIGN 8.5's table — SelfPlay.collect(48) at the same games, median of 5
between device events — without a teacher, with teacher=dict(worlds=W, samples=...), with teacher=dict(halving=...) at
every schedule, and the uniform teacher once more to show the session's spread.

usage: playout_time.py [out.txt = profiles/playout_times.txt] [games = 65536] [samples = 16] [--worlds W] [--voids | --hidden]
                       [--halving a,b,c,d[/...] [--teacher]]"""
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
teacher = "--teacher" in argv
if teacher:
    argv.remove("--teacher")
halving = []
if "--halving" in argv:
    at = argv.index("--halving")
    halving = [tuple(int(w) for w in sch.split(",")) for sch in argv[at + 1].split("/")]
    del argv[at:at + 2]
worlds = None
if "--worlds" in argv:
    at = argv.index("--worlds")
    worlds = int(argv[at + 1])
    del argv[at:at + 2]
out_path = argv[1] if len(argv) > 1 else os.path.join(
    ROOT, "profiles", "playout_halving_times.txt" if halving else "playout_hidden_times.txt" if hidden else "playout_voids_times.txt" if voids else ("playout_det_times.txt" if worlds else "playout_times.txt"))
assert worlds or not (voids or hidden), "--voids and --hidden go with --worlds W"
assert not (voids and hidden), "--voids or --hidden, not both"
assert all(sum(sch) == worlds for sch in halving), "--halving goes with --worlds W, W the sum of every schedule"
assert halving or not teacher, "--teacher goes with --halving"
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
        for sch in halving:
            counts = torch.empty((n, K.PLAYOUT_RANKS), dtype=torch.int32, device=env.device)
            hmed, hlo, hhi = timed_us(lambda: env.playout_cards_halving(sch, per_world, sum_out=sums, count_out=counts, action_out=acts))
            torch.cuda.synchronize()
            items, alive = 0, 12                        # the item count of twelve legal cards: what a fresh deal's leader plays
            for w in sch:
                items, alive = items + alive * w, max(1, (alive + 1) // 2)
            done = int(counts.sum().item())             # the playouts the launch did run, over all games
            lines.append("  %-28s %10.1f us (%.1f, %.1f)   %.3f x the determinized time   (items: %.3f predicted at 12 legal cards, %.3f run here)"
                         % ("  halving %s" % ",".join(map(str, sch)), hmed, hlo, hhi, hmed / dmed, items / (12.0 * worlds),
                            done / float((legal * samples).sum())))
            result["after_%d" % cards]["halving_" + "_".join(map(str, sch))] = dict(us=hmed, over_det=hmed / dmed, items_over_det=done / float((legal * samples).sum()))
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
env.close()
if teacher:
    from tarok_amd import selfplay as SP
    T = 48
    lines += ["", "rollout T = %d at %d games (SelfPlay.collect, hidden = 256, fused learner), median of 5 between device events (min, max)" % (T, n)]
    uniform = dict(worlds=worlds, samples=per_world)
    for label, tc in [("no teacher", None), ("teacher worlds = %d, samples = %d" % (worlds, per_world), uniform)] + \
            [("teacher halving = (%s)" % ",".join(map(str, sch)), dict(halving=sch, samples=per_world)) for sch in halving] + \
            [("teacher worlds = %d, samples = %d (again)" % (worlds, per_world), uniform)]:
        tenv = TarokVecEnv(n, seed=0, mix=K.MIX_BOT)
        sp = SP.SelfPlay(tenv, hidden=256, seed=0, fused_learner=True, teacher=tc)
        sp.collect(T)
        torch.cuda.synchronize()
        us = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            sp.collect(T)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        lines.append("  %-44s %10.0f us (%.0f, %.0f)" % (label, statistics.median(us), min(us), max(us)))
        result["rollout " + label] = statistics.median(us)
        tenv.close()
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(text)
print(json.dumps(result))
