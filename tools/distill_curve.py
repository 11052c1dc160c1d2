"""SelfPlay with and without the playout teacher for the same number of iterations from the same seed, then evaluate()
against the Bot for both (profiles/distill_curve.txt).  A record, not a bar.

usage: python tools/distill_curve.py OUT [ITERATIONS] [N_GAMES]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tarok_amd
from tarok_amd import karte as K, selfplay as SP

out_path = sys.argv[1]
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 20
n = int(sys.argv[3]) if len(sys.argv) > 3 else 16384
tarok_amd.build()
lines = ["%d iterations of T = 48 at %d games, teacher = dict(worlds=8, samples=2, tau=8), seed 0" % (iters, n)]
for label, kw in (("no teacher      ", {}), ("teacher, coef 0 ", dict(teacher=dict(worlds=8, samples=2, tau=8.0), distill_coef=0.0)),
                  ("teacher, coef 1 ", dict(teacher=dict(worlds=8, samples=2, tau=8.0), distill_coef=1.0))):
    env = tarok_amd.TarokVecEnv(n, seed=0, mix=K.MIX_ALL)
    sp = SP.SelfPlay(env, hidden=256, seed=0, fused_learner=True, **kw)
    ce = []
    for _ in range(iters):
        st = sp.iterate(T=48)
        ce.append(st.get("distill_ce", float("nan")))
    ev = sp.evaluate(n_games=4096, episodes=4)
    lines.append("%s distill_ce first %.4f last %.4f | vs Bot: %s" % (label, ce[0], ce[-1], {k: (round(v, 3) if isinstance(v, float) else v)
                                                                                          for k, v in ev.items() if not hasattr(v, "shape")}))
    env.close()
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
