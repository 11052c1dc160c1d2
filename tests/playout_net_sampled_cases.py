"""TEST INFRASTRUCTURE — the plan of the sampled net playouts' comparison (weight sets, sizes, positions, roles, play modes),
shared by tests/test_playout_net_sampled_cpu.py (the model alone: the mutants and the ambiguity cap) and
tests/test_gpu_playout_net_sampled.py (the kernels against the model and against the existing launches).  No GPU.

The launches run on N = 300 games of MIX_ALL (21,600 items at 2 worlds x 3 samples: 168 full tiles of 128 and a last
workgroup partly past the items).  The float64 model plays its items card by card in Python — some seconds for 300 games from
a fresh deal, times fourteen cases —, so it states the games of MODEL_GAMES only: every fifth game and the last one, 61 games
whose items straddle tile borders like every other game's (72 items a game against tiles of 128); every launch is a function of the game alone
(asserted by the batch test), so the rows of those games are compared item key by item key and the other games' rows by the
byte equalities and the contract tests."""
import functools

import numpy as np

import playout_net_sampled_model as SM
import playout_net_value_cases as PC
import playout_net_versus_cases as XC
import playout_net_worlds_model as WM
from oracle import tarok_spec as S

SEED, EPISODE, OFFSET, SALT = PC.SEED, PC.EPISODE, PC.OFFSET, PC.SALT
N, WORLDS, SAMPLES = 300, 2, 3
MODEL_GAMES = tuple(range(0, N, 5)) + (N - 1,)
POSITIONS = (6, 24, 44)                           # cards played: a fresh deal's second trick, mid-game, the last trick (all forced)
KINDS = ("det", "voids", "hidden")
BYTE_DEPTHS = (0, 1, 3, 12)
NEAR = 1e-5                                       # tests/test_gpu_play_mode.py::test_temperature's margin (restated in the GPU test)
CAP = 0.10                                        # of the rows with a card left to choose: at most this share is left out
ROLES = ((15, 0), (1, 14), (14, 1))
MODES = (((0.5, 0.0), (2.0, 0.0)), ((1.0, 0.0), (0.5, 0.0)), ((2.0, 0.0), (1.0, 0.0)), ((1.0, 0.25), (2.0, 0.5)))


def _tempered():
    """(kind, cards, worlds, samples, (own_rel, opp_rel), A's mode, B's mode, depth): every mode with every role set, the
    kinds and positions going round, depth 3 from the fresh deals (where a viewer has decisions left to stop at); then one case at samples = 1 and one at worlds = 1."""
    out = []
    for m, (ma, mb) in enumerate(MODES):
        for r, roles in enumerate(ROLES):
            i = 3 * m + r
            out.append((KINDS[i % 3], POSITIONS[(m + r) % 3], WORLDS, SAMPLES, roles, ma, mb, (3, 0, 0)[(m + r) % 3]))
    out.append(("det", 24, WORLDS, 1, (1, 14), (1.0, 0.0), (0.5, 0.0), 0))
    out.append(("voids", 6, 1, SAMPLES, (14, 1), (2.0, 0.0), (1.0, 0.25), 2))
    return out


TEMPERED = _tempered()
weight_sets = XC.weight_sets                      # A and B: exactly summable integer sets (tests/policy_exact_ref.py), so logits are exact


@functools.lru_cache(maxsize=None)
def games_at(kind, cards, n=N):
    """(games, words or None) of n MIX_ALL games after `cards` Bot cards, on the oracle."""
    games, words, _ = WM.bot_games("voids" if kind == "det" else kind, SEED, EPISODE, S.MIX_ALL, n, cards, first=OFFSET)
    return games, (None if kind == "det" else [int(w) for w in words])


def model_rows(case, games, words, W, rule="spec", value_scale=1.0, only=MODEL_GAMES):
    """The model of `case` on the games `only` of (games, words): (sum [len(only), 12, 4], cards, row_margin [len(only), 12], info)."""
    kind, cards, worlds, samples, (own, opp), ma, mb, depth = case
    sub = [games[g] for g in only]
    sub_words = None if words is None else [words[g] for g in only]
    return SM.playout_cards(kind, sub, SEED, SALT, 15, worlds, samples, W["A"], W["B"], own, opp, depth, value_scale, ma, mb, sub_words, rule)


def left_out(case, games, row_margin, only=MODEL_GAMES):
    """(rows left out [len(only), 12] bool, rows with a card left to choose): a row is left out when some tempered draw of some
    item of it lies within NEAR of a CDF edge."""
    choice = SM.rows_with_a_choice([games[g] for g in only])
    return (row_margin < NEAR) & choice, choice
