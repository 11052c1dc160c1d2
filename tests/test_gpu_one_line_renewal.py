"""GPU differential for the next-game line of k_play_wide's trick-aligned card loops: a lane holds ONE line, the line of its
next game, and fetches the following one at the first card of the trick after it took one.  The same games are played

  (a) through the trick-aligned loop (tarok_krog_random, whole tricks per launch),
  (b) card by card through the one-card kernel (tarok_step_random), which has no such line registers, and
  (c) through launches that are not whole tricks long (the loops that keep two buffered lines),

and every row of every output, the per-slot counters and the final state must be equal.  A workgroup is 256 slots, four
waves.  256 games: four full waves.  320: a second workgroup with one full wave and three empty ones (no slot in play:
the loop that is not trick-aligned).  300: that second workgroup's wave holds 44 slots and 20 lanes without one — a
wave of valid and invalid lanes, which plays the loop with per-lane predicates and keeps two lines.

Run on the GPU box:  python -m pytest tests/test_gpu_one_line_renewal.py -m gpu -q
"""

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

SEED = 41            # all-Berac: slots that finish in consecutive tricks of one launch (asserted from the oracle below)
SIZES = (256, 300, 320)


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def mix_of(S, name):
    return {"berac": S.MIX_FIXED + S.BERAC, "klop": S.MIX_FIXED + S.KLOP, "all": S.MIX_ALL}[name]


class Rows:
    """The output rows of a run, one per card, and the env's end state."""

    def __init__(self):
        self.rows = {k: [] for k in ("action", "obs", "done", "reward")}

    def add(self, action, obs, done, reward):
        for k, v in (("action", action), ("obs", obs), ("done", done), ("reward", reward)):
            self.rows[k].append(v.clone().reshape((-1,) + tuple(v.shape[-2 if k == "reward" else -1:])))

    def close(self, env):
        import torch
        self.cat = {k: torch.cat(v).cpu().numpy() for k, v in self.rows.items()}
        self.state = env.state()
        self.episode, self.score_sum = env.counters()
        env.close()
        return self


def krog(env, rows, cards):
    kb = env.krog_random(cards, auto_reset=True, tricks=False)
    rows.add(kb["action"], kb["obs"], kb["done"], kb["reward"])


def single(env, rows, cards):
    for _ in range(cards):
        ob, rw, dn = env.step_random(auto_reset=True)
        rows.add(env.action, ob.words, dn, rw)


_replays = {}


def single_card_replay(T, n, mix, total):
    """`total` cards of every game through the one-card kernel: computed once per (size, mix, length), shared, read only."""
    key = (n, mix, total)
    if key not in _replays:
        env = T.TarokVecEnv(n, seed=SEED, mix=mix)
        env.reset()
        rows = Rows()
        single(env, rows, total)
        _replays[key] = rows.close(env)
    return _replays[key]


def unaligned_chunks(total):
    """Launch lengths that add up to `total`, none a multiple of 4: the first leaves every lane inside a trick."""
    out = []
    while total:
        c = next(p for p in (50, 22, 6, 3, 2, 1) if p <= total)
        out.append(c)
        total -= c
    assert all(c % 4 for c in out)
    return out


def unaligned_run(T, n, mix, total):
    env = T.TarokVecEnv(n, seed=SEED, mix=mix)
    env.reset()
    rows = Rows()
    for c in unaligned_chunks(total):
        krog(env, rows, c)
    return rows.close(env)


def assert_same(got, ref, what):
    assert got.cat["action"].shape == ref.cat["action"].shape, what
    for k in ("action", "obs", "done"):
        bad = np.argwhere(got.cat[k] != ref.cat[k])
        assert bad.size == 0, "%s: %s differs first at (card, slot) %s" % (what, k, bad[0].tolist())
    d = ref.cat["done"].astype(bool)
    assert d.any(), what
    assert (got.cat["reward"][d] == ref.cat["reward"][d]).all(), what + ": reward rows"
    assert (got.episode == ref.episode).all(), what + ": episode counters"
    assert (got.score_sum == ref.score_sum).all(), what + ": score sums"
    assert (got.state == ref.state).all(), what + ": get_state lanes"
    assert ref.episode.sum() > 0, what


def check_schedule(T, n, mix, schedule, what):
    """schedule: ("krog", cards) | ("single", cards) | ("fan", value), run on one env; compared with the one-card replay
    and with unaligned launches of the same number of cards."""
    env = T.TarokVecEnv(n, seed=SEED, mix=mix)
    env.reset()
    rows, total = Rows(), 0
    for op, v in schedule:
        if op == "krog":
            krog(env, rows, v); total += v
        elif op == "single":
            single(env, rows, v); total += v
        else:
            env.set_option(refill_fan=v)
    got = rows.close(env)
    ref = single_card_replay(T, n, mix, total)
    assert_same(got, ref, what + ", trick-aligned launches vs single cards")
    assert_same(unaligned_run(T, n, mix, total), ref, what + ", unaligned launches vs single cards")
    return ref


# launches per case: enough cards for every slot to take several games (a Berac lasts 1..12 tricks)
BERAC_LAUNCHES = {4: 12, 8: 6, 48: 2, 128: 2, 192: 2}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cards", sorted(BERAC_LAUNCHES))
def test_berac_slots_finishing_on_consecutive_tricks(T, S, O, n, cards):
    """All Berac: a game is over with the first trick the declarer takes, so slots finish in consecutive tricks — the
    lane takes its line at one trick's 4th card, fetches at the next trick's 1st and takes again at its 4th.  That the
    batch does contain such slots, within one launch, is asserted from the oracle's rollouts of the same seeds."""
    mix, launches = mix_of(S, "berac"), BERAC_LAUNCHES[cards]
    total = cards * launches
    ns = np.stack([O.rollout(SEED, 0, n, e, mix, trace=False)["nsteps"] for e in range(total // 4 + 1)]).astype(np.int64)
    end = np.cumsum(ns, 0)                                   # cards played by the slot when its episode e ends
    one_trick = (ns[1:] == 4) & (end[1:] <= total)           # ends one trick after the game before it
    if cards > 4:
        one_trick &= (end[:-1] - 1) // cards == (end[1:] - 1) // cards      # both ends in the same launch
    assert one_trick.any(), "no slot finishes in two consecutive tricks: choose another seed"
    ref = check_schedule(T, n, mix, [("krog", cards)] * launches, "berac, %d games, %d x %d cards" % (n, launches, cards))
    assert (ref.episode == (end <= total).sum(0)).all()     # the replay itself agrees with the oracle's game lengths


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("mixname", ["all", "klop"])
def test_three_launches_back_to_back(T, S, n, mixname):
    """The second and third launch start with cprev > 0: the lines the launch before listed are being re-dealt, fewer
    than fourteen may be taken."""
    check_schedule(T, n, mix_of(S, mixname), [("krog", 128)] * 3, "%s, %d games, 3 x 128 cards" % (mixname, n))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("between", ["one_card_launches", "refill_fan"])
def test_stale_lines_are_dealt_in_place(T, S, n, between):
    """Lines that are not what their slot expects: four one-card launches between two 128-card launches (the multi-card
    launch drops the stretch lists the one-card launches filled, those lines stay stale), and a change of the refill fan
    between launches.  A finishing lane whose line carries another tag deals its game in place.  (That a lane did take
    that path is not asserted: `cprev` and the refill lists are not visible through the C ABI.)"""
    mid = [("single", 4)] if between == "one_card_launches" else [("fan", 2)]
    check_schedule(T, n, mix_of(S, "berac"), [("krog", 128)] + mid + [("krog", 128)], "berac, %d games, %s between" % (n, between))


@pytest.mark.parametrize("n", SIZES)
def test_refill_selftest_smallest_size(T, S, n):
    """tarok_debug_refill_selftest (hand-built refill lists for every kernel that carries the refill role, every line
    compared with a re-deal): green beside the one-line loop, also with a partial last group (300, 320: its lists hold
    the 44 or 64 slots the group has, not 256)."""
    env = T.TarokVecEnv(n, seed=11, mix=S.MIX_ALL)
    env.reset()
    for kind, per_slot, order in [(0, 1, 0), (0, 14, 2), (1, 4, 1), (2, 4, 0), (2, 14, 2), (3, 14, 1)]:
        wrong, recs = env.refill_selftest(kind, per_slot, episode0=100 + 20 * per_slot, order=order, reps=1)
        assert wrong == 0, "kind %d, %d entries per slot, order %d: %d wrong lines, first %s" % (kind, per_slot, order, wrong, recs[:2].tolist())
    env.close()
