"""GPU differential for the store addressing of k_play_wide's trick-aligned card loops: the action and done rows (and the
per-trick row) are addressed by one 32-bit element offset per lane, the observation row by a pointer advanced per card.
The same seeded batch is played

  (a) through the trick-aligned loop (tarok_krog_random, whole tricks per launch, three launches), into output arrays
      with guard bands and a row stride wider than the batch (tests/guarded.py: a stray store shows), and
  (b) card by card through the one-card kernel (tarok_step_random),

and every output row (action, done, observation word, reward rows of finished games), the final state, the episode
counters and the score sums must be equal; every guard byte and padding column must be untouched and every payload
element written.  256 games are one play workgroup of four full waves; 320 add a workgroup with one full wave and three
empty ones (the loops that are not trick-aligned, beside the changed one).

Run on the GPU box:  python -m pytest tests/test_gpu_scalar_diet.py -m gpu -q
"""

import numpy as np
import pytest

from guarded import Guarded, assert_guards_intact
from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

SEED = 41
LAUNCHES = 3
PAD = 192            # row stride = games + PAD


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


def mix_of(S, name):
    return {"berac": S.MIX_FIXED + S.BERAC, "klop": S.MIX_FIXED + S.KLOP, "all": S.MIX_ALL}[name]


_replays = {}


def single_card_replay(T, n, mix, total):
    """`total` cards of every game through the one-card kernel, with the per-trick row: computed once per (size, mix,
    length), shared, read only."""
    key = (n, mix, total)
    if key not in _replays:
        env = T.TarokVecEnv(n, seed=SEED, mix=mix)
        env.reset()
        rows = {k: [] for k in ("action", "obs", "done", "reward", "trick")}
        for _ in range(total):
            ob, rw, dn = env.step_random(auto_reset=True, tricks=True)
            for k, v in (("action", env.action), ("obs", ob.words), ("done", dn), ("reward", rw), ("trick", env.trick)):
                rows[k].append(v.cpu().numpy().copy())
        ref = {k: np.stack(v) for k, v in rows.items()}
        ref["state"] = env.state()
        ref["episode"], ref["score_sum"] = env.counters()
        env.close()
        _replays[key] = ref
    return _replays[key]


def run_krog(T, n, mix, cards, launches, std=True):
    """`launches` launches of `cards` cards through tarok_krog_random into guarded arrays.  std: action, reward, done and
    observation rows (the set of outputs of a rollout: the STD copy of the loop); otherwise the per-trick row is asked for
    and the done row is not (the other copy, with its own set of stores)."""
    from tarok_amd import _native, karte as K
    env = T.TarokVecEnv(n, seed=SEED, mix=mix)
    env.reset()
    stride = n + PAD
    spec = dict(action=(np.uint8, ()), reward=(np.int16, (4,)), obs=(np.uint64, ()))
    spec.update(dict(done=(np.uint8, ())) if std else dict(trick=(np.uint16, ())))
    got = {k: [] for k in spec}
    for launch in range(launches):
        out = {k: Guarded(k, cards, n, dt, inner=inner, stride=stride, device="cuda") for k, (dt, inner) in spec.items()}
        ptr = lambda k: out[k].ptr if k in out else None
        import torch
        with torch.cuda.device(env.device):
            _native.check(env.L.tarok_krog_random(env._h, cards, stride, ptr("action"), ptr("reward"), ptr("done"), ptr("trick"),
                                                  ptr("obs"), K.AUTO_RESET, env._stream()))
            torch.cuda.synchronize()
        assert_guards_intact(out.values(), tag=(n, cards, launch))
        for k, a in out.items():
            vals, written = a.host()
            if k != "reward":
                assert written.all(), "%s: %d elements of launch %d not written" % (k, int((~written).sum()), launch)
            got[k].append(vals)
    res = {k: np.concatenate(v) for k, v in got.items()}
    res["state"] = env.state()
    res["episode"], res["score_sum"] = env.counters()
    env.close()
    return res


def assert_same(got, ref, what):
    for k in ("action", "obs", "done", "trick"):
        if k in got:
            bad = np.argwhere(got[k] != ref[k].astype(got[k].dtype))
            assert bad.size == 0, "%s: %s differs first at (card, slot) %s" % (what, k, bad[0].tolist())
    d = ref["done"].astype(bool)
    assert d.any(), what
    assert (got["reward"][d] == ref["reward"][d]).all(), what + ": reward rows"
    assert (got["episode"] == ref["episode"]).all(), what + ": episode counters"
    assert (got["score_sum"] == ref["score_sum"]).all(), what + ": score sums"
    assert (got["state"] == ref["state"]).all(), what + ": get_state lanes"
    assert ref["episode"].sum() > 0, what


def check(T, S, n, mixname, cards, std=True):
    mix = mix_of(S, mixname)
    ref = single_card_replay(T, n, mix, cards * LAUNCHES)
    assert_same(run_krog(T, n, mix, cards, LAUNCHES, std), ref, "%s, %d games, %d x %d cards" % (mixname, n, LAUNCHES, cards))
    return ref


@pytest.mark.parametrize("cards", [4, 8, 128, 192])
def test_mixed_contracts_every_card_position(T, S, cards):
    """One play workgroup of four full waves: the stores of every card position, the largest row index of each launch
    length; with 128 and 192 cards the ring fills past 64 entries and drains inside the loop."""
    ref = check(T, S, 256, "all", cards)
    if cards >= 128:
        per_wave = ref["done"].astype(np.int64).reshape(cards * LAUNCHES, 4, 64).sum(axis=(0, 2))
        assert (per_wave > 64 * LAUNCHES).all(), "no wave finished more than 64 games per launch: the ring did not drain in the loop"


def test_all_berac_lanes_run_out_of_lines(T, S):
    """All Berac, 192 cards: finishes on nearly every trick.  A launch may take fourteen lines less those the launch before
    it listed for re-dealing (one per game it finished): slots that finish more games than that (asserted from the
    replay) run out of lines, deal in place and stop fetching."""
    ref = check(T, S, 256, "berac", 192)
    per_launch = ref["done"].astype(np.int64).reshape(LAUNCHES, 192, 256).sum(axis=1)
    assert (per_launch[1:] + np.minimum(per_launch[:-1], 14) > 14).any(), "no slot runs out of lines: choose another seed"


@pytest.mark.parametrize("cards", [48, 52])
def test_all_klop_every_lane_finishes_at_once(T, S, cards):
    """All Klop: no game ends before its 12th trick, where every lane of the wave finishes at once; a full drain."""
    ref = check(T, S, 256, "klop", cards)
    d = ref["done"].astype(bool)
    assert d[47].all() and not d[:47].any()


def test_partial_workgroup_beside_the_aligned_loop(T, S):
    """320 games: the second workgroup has one full wave and three empty ones."""
    check(T, S, 320, "all", 128)


def test_trick_row_requested_done_row_absent(T, S):
    """The other copy of the trick-aligned loop (std_tag false): the per-trick row asked for, no done row."""
    check(T, S, 256, "all", 8, std=False)
