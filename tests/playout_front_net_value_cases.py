"""TEST INFRASTRUCTURE — the plan of the value-stopped front launches' comparison (positions, weight sets, seat sets,
depths, scales), shared by tests/test_playout_front_net_value_cpu.py (the model alone) and the two GPU test modules
(the kernels against the model).  The positions are rebuilt on the oracle, so the CPU tests see the GPU tests' inputs; the
GPU tests check that their envs hold them.  No GPU."""
import functools

import numpy as np

import playout_exchange_model as XM
import playout_front_net_value_model as FV
from oracle import tarok_spec as S
from playout_net_value_cases import weight_sets  # noqa: F401  (R, P and V: V is R with a wider row 54)

SCALES = (1.0, 0.5, 1e9)                          # 0.5: odd integer values land on ties; 1e9: every V is +-32767 or 0
DEPTHS = (1, 2, 3, 12)
SALT = 3

# ---- the exchange: tests/test_gpu_playout_exchange_net.py's games (envs waiting for the exchange)
X_SEED, X_OFFSET, X_EPISODE = 43, 2000, 5
X_MIXES = dict(tri=S.MIX_FIXED + S.TRI, dve=S.MIX_FIXED + S.DVE, ena=S.MIX_FIXED + S.ENA, solo_ena=S.MIX_FIXED + S.SOLO_ENA, bot=S.MIX_BOT)
X_SHAPE = (5, 3, 2)                               # n, worlds, discard sets: 180 item slots, a full tile of 128 and a partial one
X_WIDE = (37, 2, 2)


@functools.lru_cache(maxsize=None)
def exchange_games(mix, n):
    return tuple((XM.deferred_game(X_SEED, X_OFFSET + g, X_EPISODE, X_MIXES[mix]).lanes(), X_EPISODE, X_OFFSET + g, None) for g in range(n))


def declarers(games):
    return [int((int(lanes[9]) >> 37) & 3) for lanes, _, _, _ in games]


def seats_of(choice, games):
    """net_seats of a launch: 15, 0, or "no declarer" — every seat but game 0's declarer."""
    return 15 ^ (1 << declarers(games)[0]) if choice == "no declarer" else choice


def exchange_plan(mix):
    """The launches of one env of X_WIDE: [(depth, weight set name, net_seats choice)].  Over the five mixes every depth
    meets every set and every seat choice."""
    k = list(X_MIXES).index(mix)
    sets, seats = ("R", "P", "V"), (15, 0, "no declarer")
    return [(d, sets[(k + i) % 3], seats[(k + i // 2 + d) % 3]) for i, d in enumerate(DEPTHS)]


X_SMALL = [(5, 1, "V", 15), (5, 2, "P", 0), (5, 3, "R", "no declarer"), (5, 12, "V", 15), (1, 1, "R", 15), (1, 12, "P", 0)]   # (n, depth, set, seats) at X_SHAPE's worlds and sets on the Bot's mix


# ---- the bids: tests/test_gpu_playout_bids_net.py's deals (envs that are not reset)
B_SEED, B_OFFSET, B_EPISODE = 2, 3000, 4
DEFAULT, ALL = 0x00F, 0x3FF
# (n, worlds, contracts, depth, weight set, net_seats, pass_value)
B_PLAN = [(2, 1, DEFAULT, 1, "V", 15, True), (2, 1, DEFAULT, 12, "R", 0, True),
          (5, 3, ALL, 2, "P", 10, True), (5, 3, ALL, 1, "R", 15, False),
          (16, 2, DEFAULT, 3, "V", 0, False), (16, 2, DEFAULT, 1, "P", 5, False), (16, 2, DEFAULT, 2, "R", 15, True),
          (16, 2, DEFAULT, 12, "V", 15, True)]


@functools.lru_cache(maxsize=None)
def bid_deals(n):
    return tuple((tuple(S.deal(S.game_key(B_SEED, B_OFFSET + g, B_EPISODE))), B_EPISODE, B_OFFSET + g, None) for g in range(n))


def with_sets(rows, per_game):
    return [r[:3] + (int(per_game[g]) & 15,) for g, r in enumerate(rows)]


@functools.lru_cache(maxsize=None)
def _sets():
    return weight_sets()


@functools.lru_cache(maxsize=None)
def exchange_model(mix, n, worlds, sets, depth, name, choice, rule="spec"):
    """(games, net_seats, info) of one planned exchange launch: the model's items, played once (value_scale comes after)."""
    games = exchange_games(mix, n)
    net_seats = seats_of(choice, games)
    return games, net_seats, FV.exchange_info(games, X_SEED, SALT, 15, worlds, sets, _sets()[name], net_seats, depth, rule=rule)


@functools.lru_cache(maxsize=None)
def bid_model(n, worlds, contracts, depth, name, net_seats, pass_value, rule="spec"):
    """(deals, info) of one planned bid launch."""
    deals = bid_deals(n)
    return deals, FV.bid_info(deals, B_SEED, SALT, 15, worlds, contracts, _sets()[name], net_seats, depth, pass_value, rule=rule)
