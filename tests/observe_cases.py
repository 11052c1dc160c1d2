"""TEST INFRASTRUCTURE — the positions tests/test_gpu_observe_features.py compares, computable without a GPU.

Every env of that test plays synthetic games with the Bot's cards (tarok_step_random and its multi-card kin), so the
oracle alone says which positions its rows are: tests/test_observe_model_cpu.py counts what they cover (the census)
and runs its mutants over them; the GPU test walks the same generators beside the device.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O
from oracle import tarok_spec as S
from oracle_model import SlotModel

# (name, mix, n, seed): the whole-game runs, STEPS lock-steps of tarok_step_random with auto-reset each
WHOLE = (("all", S.MIX_ALL, 773, 31), ("klop", S.MIX_FIXED + S.KLOP, 257, 32), ("berac", S.MIX_FIXED + S.BERAC, 257, 33),
         ("bot", S.MIX_BOT, 257, 34))
STEPS = 60
# the phase runs: (n, seed), mixed contracts — waiting games sit beside games in play in the same wave
PHASES = ((65, 35), (257, 36), (773, 37))
PHASE_MIX = S.MIX_ALL
FINISH_STEPS = 48                      # lock-steps without auto-reset after which every game is finished


def copy_of(game):
    h = O.Game()
    C.memmove(C.byref(h.g), C.byref(game.g), C.sizeof(O.ToGame))
    return h


def slots_of(seed, mix, n, episode=0):
    return [SlotModel(seed, i, mix, episode=episode) for i in range(n)]


def play(slots, auto):
    """One lock-step of the Bot's cards (one row of tarok_step_random each)."""
    for s in slots:
        s.card(None, auto=auto)


def waiting_game(seed, index, episode, mix):
    """The synthetic game of a slot as reset(defer_exchange=True) leaves it: dealt and set up, the exchange not made
    (a contract without one is in play at once)."""
    key = S.game_key(seed, index, episode)
    contract, declarer, king = S.sample_setup(key, mix)
    return O.Game(S.deal(key), contract, declarer, king)


def census_positions():
    """[(what, Game before, Game after or None)]: every synthetic position whose row the GPU test compares, as copies.
    `after` is the slot's game once the Bot's card has been played and, in the whole-game runs, a finished game renewed."""
    out = []
    for name, mix, n, seed in WHOLE:
        slots = slots_of(seed, mix, n)
        before = [copy_of(s.g) for s in slots]
        for t in range(STEPS):
            play(slots, auto=True)
            after = [copy_of(s.g) for s in slots]
            out += [("whole:" + name, b, a) for b, a in zip(before, after)]
            before = after
    for n, seed in PHASES:
        out += [("waiting", waiting_game(seed, i, 0, PHASE_MIX), None) for i in range(n)]
        slots = slots_of(seed, PHASE_MIX, n)
        out += [("exchanged", copy_of(s.g), None) for s in slots]
        for t in range(FINISH_STEPS + 1):
            play(slots, auto=False)
            out += [("to the finish", copy_of(s.g), None) for s in slots]
        assert all(s.g.done for s in slots), "not true: all(s.g.done for s in slots)"
    return out


def sample_games(tr, per_contract=24):
    idx = []
    for c in range(10):
        w = np.where(tr["contract"] == c)[0]
        idx += list(w[:: max(1, len(w) // per_contract)][:per_contract])
    return np.array(sorted(idx))


def reset_from_traces(env, tr, idx, **kw):
    king = np.where(tr["king"][idx] < 0, 0, tr["king"][idx]).astype(np.int8)
    choice = np.where(tr["choice"][idx] < 0, 0, tr["choice"][idx]).astype(np.int8)
    return env.reset(deals=tr["deals"][idx], contract=tr["contract"][idx], declarer=tr["declarer"][idx], king_suit=king,
                     talon_choice=choice, discards=tr["discards"][idx], **kw)
