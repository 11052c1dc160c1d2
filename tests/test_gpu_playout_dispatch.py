"""GPU: TarokVecEnv.playout_cards_fair, the one dispatcher over the four card launches, against the direct methods: the
same sum and action bytes for the same arguments, the caller's words tensor left holding shown_voids() / played_cards(),
and the refusal of voids together with hidden.  Outputs sit inside guard bands (tests/guarded.py).  What the launches
themselves compute is the business of tests/test_gpu_playout*.py.

Run on the GPU box:  python -m pytest tests/test_gpu_playout_dispatch.py -m gpu -q
"""
import functools
import numpy as np
import pytest

import gpu_harness as H
from gpu_harness import T  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
SEED, OFFSET, EPISODE = 41, 1000, 3               # tests/test_gpu_playout_det.py's: the same games
make_env = functools.partial(H.make_env, seed=SEED, offset=OFFSET, episode=EPISODE)
N = 67                                   # at (1, 1) a workgroup holds 64 four-lane teams: the second workgroup is ragged
CARDS = 5
SIZES = ((1, 1), (3, 2))
KINDS = ("open", "det", "voids", "hidden")


@pytest.fixture(scope="module")
def env(T):
    from oracle import tarok_spec as S
    env = make_env(T, N, S.MIX_ALL, CARDS, history=True)
    yield env
    env.close()


@pytest.fixture(scope="module")
def per_game(env):
    import torch
    sets = np.random.RandomState(7).randint(0, 16, N).astype(np.uint8)
    return torch.from_numpy(sets).to(env.device)


def guarded_call(env, call):
    """call(sum_out=, action_out=) on tensors inside guard bands -> (sum [N,12,4] i32, action [N] u8) host arrays."""
    import torch
    from guarded import Guarded, assert_guards_intact
    g_sum = Guarded("sum_out", 1, N, np.int32, inner=(12, 4), device="cuda")
    g_act = Guarded("action_out", 1, N, np.uint8, device="cuda")
    call(sum_out=g_sum.payload().view(torch.int32).view(N, 12, 4), action_out=g_act.payload())
    torch.cuda.synchronize()
    assert_guards_intact([g_sum, g_act])
    acts, written = g_act.host()
    assert written.all(), "a byte of action_out was not written"
    return g_sum.host()[0][0], acts[0]


def direct(env, kind, worlds, samples, **kw):
    if kind == "open":
        return lambda **out: env.playout_cards(samples, **kw, **out)
    method = dict(det=env.playout_cards_det, voids=env.playout_cards_voids, hidden=env.playout_cards_hidden)[kind]
    return lambda **out: method(worlds, samples, **kw, **out)


def dispatched(env, kind, worlds, samples, words=None, **kw):
    return lambda **out: env.playout_cards_fair(None if kind == "open" else worlds, samples, voids=kind == "voids",
                                                hidden=kind == "hidden", words=words, **kw, **out)


@pytest.mark.parametrize("kind", KINDS)
def test_the_dispatcher_gives_the_direct_methods_bytes(env, per_game, kind):
    """Every kind at (1, 1) and (3, 2) under a salt and a per-game seat set: sums and cards equal the direct method's."""
    for worlds, samples in SIZES:
        kw = dict(salt=5, seats_per_game=per_game)
        want_sum, want_act = guarded_call(env, direct(env, kind, worlds, samples, **kw))
        got_sum, got_act = guarded_call(env, dispatched(env, kind, worlds, samples, **kw))
        assert (got_sum == want_sum).all(), (kind, worlds, samples, "sums differ")
        assert (got_act == want_act).all(), (kind, worlds, samples, "cards differ")
        assert want_sum.any() and (want_act != 255).any(), "the positions give the launches nothing to do"


def test_worlds_zero_is_the_open_hand_launch(env, per_game):
    want = guarded_call(env, direct(env, "open", None, 2, seats_per_game=per_game))
    got = guarded_call(env, lambda **out: env.playout_cards_fair(0, 2, seats_per_game=per_game, **out))
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


@pytest.mark.parametrize("kind", ["voids", "hidden"])
def test_the_callers_words_tensor_holds_the_words_afterwards(env, per_game, kind):
    import torch
    dtype, own = (torch.int32, env.shown_voids) if kind == "voids" else (torch.int64, env.played_cards)
    words = torch.full((N,), -1, dtype=dtype, device=env.device)
    want = guarded_call(env, direct(env, kind, 3, 2, seats_per_game=per_game))
    got = guarded_call(env, dispatched(env, kind, 3, 2, words=words, seats_per_game=per_game))
    assert torch.equal(words, own())
    assert (words != 0).any(), "no game has a word to show"
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


def test_voids_together_with_hidden_is_refused(env):
    with pytest.raises(ValueError):
        env.playout_cards_fair(3, 2, voids=True, hidden=True)
