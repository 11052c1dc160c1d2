"""TEST INFRASTRUCTURE — the seat-set patterns of the frozen-opponent tests (tests/test_opponent_cpu.py and
tests/test_gpu_learner_opponent.py): numpy, no GPU."""
import numpy as np


SETS = ["0", "1", "6", "15", "cycle"]


def seat_sets(n, which):
    """[n] uint8: the learner's seat set of every slot."""
    if which == "cycle":
        return (1 << (np.arange(n) % 4)).astype(np.uint8)
    return np.full(n, int(which), np.uint8)


def moves(seat, sets):
    return ((sets[None, :].astype(np.int64) >> seat) & 1).astype(bool)


def monte_carlo_known(done):
    """known of the Monte-Carlo returns: a game ends at or after t inside the rollout."""
    return np.flip(np.maximum.accumulate(np.flip(done.astype(bool), 0), 0), 0)
