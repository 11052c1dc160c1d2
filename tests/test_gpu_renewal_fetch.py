"""GPU differential for the words k_play_wide's trick-aligned card loop carries from card to card — the card's RNG counter
and the seat / position half of the observation word, advanced by a constant per card and reset where a finishing lane
takes its next game — and for the renewal of a lane's next-game line around them (taken at a trick's 4th card, the next
one fetched at the following first card).

The same games are played through the trick-aligned loop (tarok_krog_random, whole tricks per launch) and card by card
through the one-card kernel (tarok_step_random), which has neither line registers nor carried words.  Compared: every
row of every output, then the end state (tarok_get_state), the per-slot counters, and the slots' RNG keys — those are
not visible through the C ABI, so both envs play one more trick card by card from where they stand: the one-card
kernel draws from the stored keys.

A workgroup is 256 slots, four waves.  256 games: one full group.  320: a second group with one full wave and three
without a slot in play, which run the loop that is not trick-aligned beside it.

Run on the GPU box:  python -m pytest tests/test_gpu_renewal_fetch.py -m gpu -q
"""

import numpy as np
import pytest

from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu

BERAC_SEED = 41      # all-Berac: slots that finish in consecutive tricks of one launch (asserted below)
SIZES = (256, 320)
TAIL = 4             # cards played one by one after the compared run: they draw from the stored keys
AHEAD = 14           # next-game lines per slot (TAROK_GAMES_AHEAD)


@pytest.fixture(scope="module")
def S():
    from oracle import tarok_spec
    return tarok_spec


def berac(S):
    return S.MIX_FIXED + S.BERAC


class Rows:
    """The output rows of a run, one per card, the env's end state, and the rows of one more trick played card by card."""

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
        tail = Rows()
        single(env, tail, TAIL)
        self.tail = {k: torch.cat(v).cpu().numpy() for k, v in tail.rows.items()}
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


def single_card_replay(T, n, mix, seed, total):
    """`total` cards of every game through the one-card kernel: computed once per (size, mix, seed, length), read only."""
    key = (n, mix, seed, total)
    if key not in _replays:
        env = T.TarokVecEnv(n, seed=seed, mix=mix)
        env.reset()
        rows = Rows()
        single(env, rows, total)
        _replays[key] = rows.close(env)
    return _replays[key]


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
    for k in ("action", "obs", "done"):
        assert (got.tail[k] == ref.tail[k]).all(), "%s: %s of the trick played from the stored keys" % (what, k)


def run_schedule(T, n, mix, seed, schedule):
    """schedule: ("krog", cards) | ("single", cards) | ("fan", value), on one env."""
    env = T.TarokVecEnv(n, seed=seed, mix=mix)
    env.reset()
    rows, total = Rows(), 0
    for op, v in schedule:
        if op == "krog":
            krog(env, rows, v); total += v
        elif op == "single":
            single(env, rows, v); total += v
        else:
            env.set_option(refill_fan=v)
    return rows.close(env), total


def check_schedule(T, n, mix, seed, schedule, what):
    got, total = run_schedule(T, n, mix, seed, schedule)
    ref = single_card_replay(T, n, mix, seed, total)
    assert_same(got, ref, what)
    return ref


def finishes_per_launch(ref, cards):
    """[launch, slot]: games the slot finishes in each launch of `cards` cards (from the one-card replay's done rows)."""
    d = ref.cat["done"].astype(np.int64)
    return d.reshape(d.shape[0] // cards, cards, d.shape[1]).sum(1)


@pytest.mark.parametrize("n", SIZES)
def test_line_fetched_at_a_4th_card_is_taken_at_the_next(T, S, n):
    """All Berac, four launches of 64 cards: a game is over with the first trick the declarer takes, so a lane renews on
    consecutive tricks — the line it asks for after one 4th card is the one it takes at the very next 4th card, and
    the carried words are reset on consecutive tricks.  That such slots exist within one launch is asserted from the reference rows."""
    ref = check_schedule(T, n, berac(S), BERAC_SEED, [("krog", 64)] * 4, "berac, %d games, 4 x 64 cards" % n)
    d = ref.cat["done"].astype(bool)
    ends = d[3::4]                                           # [trick, slot]: a game ends with this trick
    same_launch = (np.arange(1, ends.shape[0]) % 16 != 0)[:, None]
    assert (ends[1:] & ends[:-1] & same_launch).any(), "no slot finishes in two consecutive tricks of a launch: choose another seed"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cards", [128, 192])
def test_lanes_that_run_through_their_lines_stop_fetching(T, S, n, cards):
    """All Berac, long launches: lanes use up the lines they may take (fourteen less those the launch before listed),
    deal in place, stop fetching (lim = 0) and have all their lines re-dealt.  Two further launches show that the
    refill has restored them.  That lanes do run out is asserted from the reference rows."""
    ref = check_schedule(T, n, berac(S), BERAC_SEED, [("krog", cards)] * 4, "berac, %d games, 4 x %d cards" % (n, cards))
    f = finishes_per_launch(ref, cards)
    allowed = AHEAD - np.minimum(f[0], AHEAD)                # what the second launch may take from lines
    assert (f[1] > allowed).any(), "no slot runs out of lines in the second launch: choose another seed"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mixed_contracts_five_launches(T, S, n, seed):
    check_schedule(T, n, S.MIX_ALL, seed, [("krog", 128)] * 5, "all contracts, seed %d, %d games, 5 x 128 cards" % (seed, n))


STALE = {
    # one-card launches fill the stretch lists, which the multi-card launch drops: those lines stay stale.  Five single
    # cards and a 3-card launch end on a trick boundary; the 4-card launch after them is trick-aligned and preloads.
    "one_card_launches": [("krog", 128), ("single", 5), ("krog", 3), ("krog", 4), ("krog", 128), ("krog", 128)],
    "four_one_card_launches": [("krog", 128), ("single", 4), ("krog", 4), ("krog", 128), ("krog", 128)],
    "from_the_start": [("single", 4), ("krog", 4), ("krog", 128), ("krog", 128)],
    "refill_fan": [("krog", 128), ("fan", 2), ("krog", 4), ("krog", 128), ("krog", 128)],
}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("between", sorted(STALE))
def test_stale_preloaded_tags(T, S, n, between):
    """A lane whose preloaded line carries another game's tag finishes, deals in place and drops to lim = 0: the carried
    words are reset on that path as on the usual one.  (That a lane did take that path is not asserted: `cprev` and the refill lists are not visible
    through the C ABI.)"""
    check_schedule(T, n, berac(S), BERAC_SEED, STALE[between], "berac, %d games, %s" % (n, between))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cards", [4, 8])
def test_short_launches_replayed_from_a_graph(T, S, n, cards):
    """One launch of 4 or 8 cards captured in a graph and replayed 16 times: the carried words are set up from the stored
    state at the top of every launch, and the launch's preload must find the right line on its own."""
    import torch
    mix = berac(S)
    env = T.TarokVecEnv(n, seed=BERAC_SEED, mix=mix)
    env.reset()
    rows, total = Rows(), 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up on the capture stream (allocations outside the capture)
        krog(env, rows, cards); total += cards
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        kb = env.krog_random(cards, auto_reset=True, tricks=False)
    for _ in range(16):
        g.replay()
        rows.add(kb["action"], kb["obs"], kb["done"], kb["reward"]); total += cards
    torch.cuda.synchronize()
    got = rows.close(env)
    assert_same(got, single_card_replay(T, n, mix, BERAC_SEED, total), "berac, %d games, %d cards x 17, graph" % (n, cards))


@pytest.mark.parametrize("n", SIZES)
def test_launches_that_are_not_whole_tricks(T, S, n):
    """cards = 6: the loop that is not trick-aligned keeps its two buffered lines and its fetch on the spot."""
    check_schedule(T, n, berac(S), BERAC_SEED, [("krog", 6)] * 16, "berac, %d games, 16 x 6 cards" % n)
