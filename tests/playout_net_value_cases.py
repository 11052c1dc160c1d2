"""TEST INFRASTRUCTURE — the plan of the value-bootstrapped net playouts' comparison (positions, weight sets, seat sets,
depths, scales), shared by tests/test_playout_net_value_cpu.py (the model alone) and tests/test_gpu_playout_net_value.py
(the kernels against the model).  No GPU."""
import numpy as np

import playout_net_value_model as VM
import playout_net_worlds_model as WM
from oracle import tarok_spec as S


SEED, EPISODE, OFFSET = 41, 3, 1000               # tests/test_gpu_playout_det.py's: the GPU tests' envs
KLOP, DVE = 0, 2
SALT = 3
SCALES = (1.0, 0.5, 1e9)                          # 0.5: odd integer values land on ties; 1e9: every V is +-32767 or 0
SHAPES = ((5, 3), (1, 1))                         # 180 item slots: a full tile of 128 and a partial one; one partial tile
# the positions of the comparison with the GPU: (mix, cards).  voids and hidden: the constraining positions that
# tests/test_gpu_playout_net_worlds.py builds come first
POSITIONS = dict(det=[(S.MIX_ALL, c) for c in (0, 9, 24, 40, 44)],
                 voids=[(S.MIX_ALL, c) for c in (5, 24, 44, 0, 9, 40)],
                 hidden=[(S.MIX_FIXED + KLOP, 5), (S.MIX_FIXED + DVE, 24), (S.MIX_ALL, 44), (S.MIX_ALL, 0), (S.MIX_ALL, 9), (S.MIX_ALL, 40)])
CASES = [(kind, at) for kind in VM.KINDS for at in range(len(POSITIONS[kind]))]


def weight_sets():
    """The exactly summable sets of tests/policy_exact_ref.py, R and one P, and V: set R with row 54 of W3 and b3[54]
    redrawn wider (W3[54] in {-8..8} 2^-10, b3[54] = 3.5), so that the value varies over the stop positions in sign and
    size whatever R's own row gives."""
    import torch
    import policy_exact_ref as PE
    WR, WP = PE.weights_r(), PE.weights_p(*PE.P_PARAMS[2])
    WV = [t.clone() for t in WR]
    g = torch.Generator(); g.manual_seed(54)
    WV[4][54] = torch.randint(-8, 9, (256,), generator=g).double() * 2.0 ** -10
    WV[5][54] = 3.5
    return dict(R=WR, P=WP, V=WV)


def plan(kind, at):
    """The launches of case (kind, at): [(n, worlds, depth, weight set name, net_seats or "no viewer")].  Over the cases
    every depth meets every set and every seat choice."""
    k = VM.KINDS.index(kind) + at
    sets, seats = ("R", "P", "V"), (15, 0, "no viewer")
    rows = [(5, 3, d, sets[(k + d) % 3], seats[(k + d // 2) % 3]) for d in (1, 2, 3)]
    return rows + [(1, 1, 1 + k % 3, sets[k % 3], seats[(k + 1) % 3])]


def games_at(kind, at, n):
    mix, cards = POSITIONS[kind][at]
    games, words, objs = WM.bot_games("voids" if kind == "det" else kind, SEED, EPISODE, mix, n, cards, first=OFFSET)
    return games, (None if kind == "det" else words), objs


def net_seats_of(choice, objs):
    """"no viewer": every seat but game 0's mover — a set without (that game's) viewer."""
    return 15 ^ (1 << objs[0].seat()) if choice == "no viewer" else choice


def at_scale(n, worlds, info, value_scale, rule="spec"):
    """The sums [n, 12, 4] of a model run re-formed at another value_scale: the playouts do not depend on it."""
    sums = np.zeros((n, 12, 4), np.int64)
    for (g, j, w), d in info:
        if d["stopped"]:
            V = VM.points(d["v"], value_scale, half_even=rule != "away")
            sums[g, j, d["viewer"]] += V
        else:
            sums[g, j] += d["scores"]
    return sums


def model(kind, at, n, worlds, depth, W, choice, value_scale=1.0, rule="spec"):
    games, words, objs = games_at(kind, at, n)
    net_seats = net_seats_of(choice, objs)
    sums, acts, info = VM.playout_cards(kind, games, SEED, SALT, 15, worlds, W, net_seats, depth, value_scale, words, rule=rule)
    return games, words, net_seats, sums, acts, info
