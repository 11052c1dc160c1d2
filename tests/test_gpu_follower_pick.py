"""GPU differential for the follower-card forms of k_play_wide's trick-aligned card loop (one-word legal mask and pick,
C plane padded for the length of the loop): the same games through the trick-aligned loop (tarok_krog_random, cards = 8),
through the generic one-card kernel (tarok_step_random: legal_now, kth_bit) and through launches that do not stay on whole
tricks (cards = 6).  Every row of every output and the final state must be equal.

Run on the GPU box:  python -m pytest tests/test_gpu_follower_pick.py -m gpu -q
"""

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

N = 512


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


def same_end_state(a, b):
    assert (a.state() == b.state()).all()
    ea, sa = a.counters(); eb, sb = b.counters()
    assert (ea == eb).all() and (sa == sb).all()
    assert ea.sum() > 0                                 # games did end and were replaced on the way


# mix 0 is MIX_ALL; "all Klop" (the pagat rule with talon gifts in every game) is MIX_FIXED + KLOP: both are run.
# tricks = False is the set of outputs of a rollout (the STD copy of the loop, the one the benchmark times),
# tricks = True the copy that also writes the per-trick rows.
@pytest.mark.parametrize("mix_name,tricks", [("MIX_ALL", False), ("KLOP", False), ("MIX_NAVADNA3", False), ("MIX_ALL", True)])
def test_trick_aligned_loop_equals_single_card_steps(T, S, mix_name, tricks):
    mix = S.MIX_FIXED + S.KLOP if mix_name == "KLOP" else getattr(S, mix_name)
    a = T.TarokVecEnv(N, seed=23, mix=mix)
    b = T.TarokVecEnv(N, seed=23, mix=mix)
    a.reset(); b.reset()
    cards, finished = 8, 0
    for r in range(96 // cards):
        kb = a.krog_random(cards, auto_reset=True, tricks=tricks)
        for c in range(cards):
            ob, rw, dn = b.step_random(auto_reset=True, tricks=True)
            at = (mix_name, tricks, r, c)
            assert (kb["action"][c] == b.action).all().item(), at
            assert (kb["done"][c] == dn).all().item(), at
            assert (kb["obs"][c] == ob.words).all().item(), at
            if tricks:
                assert (kb["trick"][c] == b.trick).all().item(), at
            d = dn.bool()
            assert (kb["reward"][c][d] == rw[d]).all().item(), at
            finished += int(d.sum().item())
    assert finished > 0
    same_end_state(a, b)
    a.close(); b.close()


def test_trick_aligned_loop_equals_unaligned_launches(T, S):
    """cards = 6 leaves every lane in the middle of a trick after the first launch: from then on the generic copy of the loop
    plays.  48 lock-steps both ways."""
    a = T.TarokVecEnv(N, seed=29, mix=S.MIX_ALL)
    b = T.TarokVecEnv(N, seed=29, mix=S.MIX_ALL)
    a.reset(); b.reset()
    rows_a = {k: [] for k in ("action", "done", "obs", "reward")}
    rows_b = {k: [] for k in rows_a}
    for r in range(48 // 8):
        kb = a.krog_random(8, auto_reset=True, tricks=False)
        for k in rows_a:
            rows_a[k].append(kb[k].clone())
    for r in range(48 // 6):
        kb = b.krog_random(6, auto_reset=True, tricks=False)
        for k in rows_b:
            rows_b[k].append(kb[k].clone())
    import torch
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
