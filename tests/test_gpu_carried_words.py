"""GPU differential for the carried words of k_play_wide's trick-aligned card loop (the contract's FamilyWord, the trick's
LeadWord, the error bit and the seat's smears inside the observation carry): the same games through the trick-aligned loop
(tarok_krog_random, cards = 8) and through the generic one-card kernel (tarok_step_random), which rebuilds everything from the
state on every card.  Every row of every output, the final state and the counters must be equal.

Run on the GPU box:  python -m pytest tests/test_gpu_carried_words.py -m gpu -q
"""

import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

N = 512                                                 # full waves only: a wave with an idle lane does not play the trick-aligned loop


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


def mix_of(S, name):
    return S.MIX_FIXED + getattr(S, name) if name in ("KLOP", "BERAC") else getattr(S, name)


def same_end_state(a, b):
    assert (a.state() == b.state()).all()
    ea, sa = a.counters(); eb, sb = b.counters()
    assert (ea == eb).all() and (sa == sb).all()
    assert ea.sum() > 0                                 # games did end and were replaced on the way


def krog_against_steps(a, b, tricks, at, rounds=12, cards=8):
    """`rounds` launches of `cards` cards on a, the same cards one by one on b; returns (games finished, rows with the error bit)."""
    finished, errors = 0, 0
    for r in range(rounds):
        kb = a.krog_random(cards, auto_reset=True, tricks=tricks)
        for c in range(cards):
            ob, rw, dn = b.step_random(auto_reset=True, tricks=True)
            where = at + (r, c)
            assert (kb["action"][c] == b.action).all().item(), where
            assert (kb["done"][c] == dn).all().item(), where
            assert (kb["obs"][c] == ob.words).all().item(), where
            if tricks:
                assert (kb["trick"][c] == b.trick).all().item(), where
            d = dn.bool()
            assert (kb["reward"][c][d] == rw[d]).all().item(), where
            finished += int(d.sum().item())
            errors += int((kb["obs"][c] < 0).sum().item())
    return finished, errors


# MIX_ALL changes the contract from game to game of a slot; all Klop has the pagat rule and a talon gift in six tricks of
# twelve; all Berac ends most games after a trick or two, so the per-game words are set again on almost every trick.
# tricks = False is the STD copy of the loop (the one the benchmark times), tricks = True the copy that writes the trick rows.
@pytest.mark.parametrize("mix_name,tricks", [("MIX_ALL", False), ("KLOP", False), ("MIX_NAVADNA3", False), ("BERAC", False), ("BERAC", True)])
def test_trick_aligned_loop_equals_single_card_steps(T, S, mix_name, tricks):
    a = T.TarokVecEnv(N, seed=31, mix=mix_of(S, mix_name))
    b = T.TarokVecEnv(N, seed=31, mix=mix_of(S, mix_name))
    a.reset(); b.reset()
    finished, errors = krog_against_steps(a, b, tricks, (mix_name, tricks))         # 96 cards
    assert finished > 0 and errors == 0
    if mix_name == "BERAC":
        assert finished > 4 * N                          # games of a trick or two: several per slot
    same_end_state(a, b)
    a.close(); b.close()


def test_trick_aligned_loop_equals_unaligned_launches(T, S):
    """cards = 6 leaves every lane in the middle of a trick after the first launch: from then on the loop that is not
    trick-aligned plays, which carries nothing.  48 lock-steps both ways."""
    import torch
    a = T.TarokVecEnv(N, seed=37, mix=S.MIX_ALL)
    b = T.TarokVecEnv(N, seed=37, mix=S.MIX_ALL)
    a.reset(); b.reset()
    keys = ("action", "done", "obs", "reward")
    rows_a, rows_b = {k: [] for k in keys}, {k: [] for k in keys}
    for env, cards, rows in ((a, 8, rows_a), (b, 6, rows_b)):
        for r in range(48 // cards):
            kb = env.krog_random(cards, auto_reset=True, tricks=False)
            for k in keys:
                rows[k].append(kb[k].clone())
    cat_a = {k: torch.cat(v) for k, v in rows_a.items()}
    cat_b = {k: torch.cat(v) for k, v in rows_b.items()}
    assert cat_a["action"].shape[0] == 48 and cat_b["action"].shape[0] == 48
    for k in ("action", "done", "obs"):
        assert (cat_a[k] == cat_b[k]).all().item(), k
    d = cat_a["done"].bool()
    assert d.any().item()
    assert (cat_a["reward"][d] == cat_b["reward"][d]).all().item()
    same_end_state(a, b)
    a.close(); b.close()


def test_partial_last_group_plays_the_untouched_loops(T, S):
    """320 games: the second workgroup is a quarter full, and a workgroup with idle waves is not all in play, so the loops
    that carry nothing run beside the trick-aligned one.  Same rows, same end state."""
    a = T.TarokVecEnv(320, seed=41, mix=S.MIX_ALL)
    b = T.TarokVecEnv(320, seed=41, mix=S.MIX_ALL)
    a.reset(); b.reset()
    finished, errors = krog_against_steps(a, b, False, ("320",))
    assert finished > 0 and errors == 0
    same_end_state(a, b)
    a.close(); b.close()


def test_error_bit_of_the_starting_state_is_carried(T, S):
    """Every slot takes an illegal card through the step API first (nothing changes but the game's error bit, so the slots stay
    at their trick boundary); the sibling env is set the same way.  The games then played keep the bit in every observation
    until they end, and the fresh games that replace them do not have it: the second launch starts from a state with the bit
    set in some slots and clear in others."""
    import numpy as np
    a = T.TarokVecEnv(N, seed=43, mix=S.MIX_ALL)
    b = T.TarokVecEnv(N, seed=43, mix=S.MIX_ALL)
    a.reset(); b.reset()
    bad = np.full(N, 200, np.uint8)                      # no such card
    for env in (a, b):
        ob, _, dn = env.step(bad, auto_reset=True)
        assert ob.error.all().item() and not dn.bool().any().item()
        assert (ob.step == 0).all().item()               # no card was played
    kb = a.krog_random(8, auto_reset=True, tricks=False)
    first = kb["obs"].clone()
    for c in range(8):
        ob, rw, dn = b.step_random(auto_reset=True, tricks=True)
        assert (first[c] == ob.words).all().item(), c
        assert (kb["action"][c] == b.action).all().item(), c
        assert (kb["done"][c] == dn).all().item(), c
    assert (first[0] < 0).all().item()                   # the carried error word was non-zero in every lane ...
    start = first[7] < 0
    assert start.any().item() and not start.all().item() # ... and the next launch starts with it set in some slots only
    finished, errors = krog_against_steps(a, b, False, ("error",), rounds=11)
    assert finished > 0 and errors > 0
    same_end_state(a, b)
    a.close(); b.close()
