"""CPU-side checks of the play mode (tarok_set_play_mode: greedy, temperature and epsilon-greedy play): the float64
model of tests/play_mode_model.py against the existing sampler reference and the oracle's Bot card, and the argument
validation of the two new entry points, which make no HIP call and so run without a GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import play_mode_model as PM
from oracle import tarok_spec as S
from policy_exact_ref import sampler_reference

SEED = 17


def inputs(n, seed, ties=False):
    """Random float32 logits (bf16 values; with `ties` small integers, so that maxima repeat), legal sets of 1..12 cards
    anywhere in 0..53, cards played 0..47, the keys of games 0..n-1 at episode 0."""
    rnd = np.random.RandomState(seed)
    logits = (rnd.randint(-2, 3, (n, 64)) if ties else np.round(rnd.randn(n, 64) * 2 * 64) / 64).astype(np.float32)
    masks = np.zeros(n, np.uint64)
    for i in range(n):
        for c in rnd.choice(54, rnd.randint(1, 13), replace=False):
            masks[i] |= np.uint64(1) << np.uint64(c)
    played = rnd.randint(0, 48, n)
    return logits, masks, played, PM.keys_of(SEED, 0, np.zeros(n, np.int64))


def test_model_at_the_default_mode_is_the_existing_sampler_reference():
    logits, masks, played, keys = inputs(4000, 1)
    m = PM.play_mode(logits, masks, played, keys, 1.0, 0.0)
    r = np.array([S.rng32(k, 192 + int(p)) for k, p in zip(keys, played)], np.uint64)
    ref = sampler_reference(logits.astype(np.float64), masks, r)
    rows = np.arange(len(masks))
    assert (m["card"] == ref["card"]).all() and not m["explored"].any()
    assert np.abs(m["logp"] - ref["logp_all"][rows, ref["card"]]).max() < 1e-12
    assert ((m["margin"] < 1e-5) == ref["near"]).all()


def test_greedy_picks_the_lowest_tied_card_with_logp_zero():
    logits, masks, played, keys = inputs(4000, 2, ties=True)
    m = PM.play_mode(logits, masks, played, keys, 0.0, 0.0)
    tied = 0
    for i in range(len(masks)):
        cards = [c for c in range(54) if (int(masks[i]) >> c) & 1]
        top = max(logits[i, c] for c in cards)
        at_top = [c for c in cards if logits[i, c] == top]
        tied += len(at_top) > 1
        assert m["card"][i] == at_top[0]
    assert tied > 1000                                                   # ties are the rule on these inputs
    assert (m["logp"] == 0.0).all() and np.isinf(m["margin"]).all()
    # by hand: the maximum on both sides of the lane-pair seam (cards 26 and 27) -> 26
    lg = np.zeros((1, 64), np.float32); lg[0, [26, 27]] = 3.0
    one = PM.play_mode(lg, [(1 << 5) | (1 << 26) | (1 << 27)], [7], keys[:1], 0.0, 0.0)
    assert one["card"][0] == 26 and one["logp"][0] == 0.0


def test_epsilon_one_plays_the_oracles_bot_card_everywhere():
    logits, masks, played, keys = inputs(3000, 3)
    for temperature in (0.0, 1.0):
        m = PM.play_mode(logits, masks, played, keys, temperature, 1.0)
        assert m["explored"].all()
        want = [S.policy_action(k, int(p), int(mk)) for k, p, mk in zip(keys, played, masks)]
        assert m["card"].tolist() == want
    # greedy with epsilon 1: the mode is the uniform one, whatever the card
    g = PM.play_mode(logits, masks, played, keys, 0.0, 1.0)
    assert np.abs(g["logp"] + np.log(g["k"])).max() < 1e-12


def test_epsilon_quarter_explores_on_its_share_of_rows():
    n = 100000
    rnd = np.random.RandomState(4)
    logits = np.zeros((n, 64), np.float32)
    masks = np.full(n, (1 << 3) | (1 << 30) | (1 << 31), np.uint64)
    played = rnd.randint(0, 48, n)
    keys = PM.keys_of(SEED, 0, np.zeros(n, np.int64))
    m = PM.play_mode(logits, masks, played, keys, 0.0, 0.25)
    share = PM.threshold(0.25) / 2.0 ** 24
    assert share == 0.25
    sigma = np.sqrt(share * (1 - share) / n)
    assert abs(m["explored"].mean() - share) < 4 * sigma, (m["explored"].mean(), sigma)
    # the log-probability is the mixture's, explored or not: greedy card 3 has 1 - e + e / 3, the others e / 3
    want = np.where(m["card"] == 3, np.log(0.75 + 0.25 / 3), np.log(0.25 / 3))
    assert np.abs(m["logp"] - want).max() < 1e-12
    assert (m["card"][~m["explored"]] == 3).all() and (m["card"][m["explored"]] == m["bot"][m["explored"]]).all()


def test_threshold_is_the_floor_in_double():
    assert PM.threshold(0.0) == 0 and PM.threshold(1.0) == 1 << 24 and PM.threshold(0.1) == 1677721
    assert PM.threshold(2.0 ** -25) == 0 and PM.threshold(2.0 ** -24) == 1


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  -- before the dlopen: one HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_abi_list_and_python_surface_have_the_play_mode():
    from tarok_amd import _native, karte as K
    from tarok_amd import evaluate as EV
    from tarok_amd.env import TarokVecEnv
    from tarok_amd.selfplay import SelfPlay
    assert "tarok_set_play_mode" in _native.SYMBOLS and "tarok_get_play_mode" in _native.SYMBOLS
    assert K.DRAW_EXPLORE == 256 == PM.DRAW_EXPLORE
    sig = inspect.signature(TarokVecEnv.set_play_mode).parameters
    assert sig["temperature"].default == 1.0 and sig["epsilon"].default == 0.0
    assert isinstance(TarokVecEnv.play_mode, property)
    for f in (EV.evaluate_vs_bot, EV.evaluate_vs_policy):
        sig = inspect.signature(f).parameters
        assert sig["temperature"].default == 1.0 and sig["epsilon"].default == 0.0
    sig = inspect.signature(SelfPlay.evaluate).parameters
    assert sig["greedy"].default is False and sig["temperature"].default is None and sig["epsilon"].default == 0.0


def test_set_play_mode_validates_before_any_hip_call(L):
    """The setter and the getter touch only the env's host record: a zeroed stand-in for one (no GPU, no tarok_create)
    is enough to see every refusal leave the mode as it was and every accepted mode come back from the getter."""
    f32 = ctypes.c_float
    nan = float("nan")
    assert L.tarok_set_play_mode(None, 1.0, 0.0) == -1
    assert L.tarok_get_play_mode(None, None, None) == -1
    stand_in = ctypes.create_string_buffer(1 << 16)
    env = ctypes.cast(stand_in, ctypes.c_void_p)

    def get():
        t, e = f32(-7), f32(-7)
        assert L.tarok_get_play_mode(env, ctypes.byref(t), ctypes.byref(e)) == 0
        return t.value, e.value

    assert L.tarok_set_play_mode(env, 0.5, 0.25) == 0 and get() == (0.5, 0.25)
    for t, e in ((nan, 0.0), (1.0, nan), (1.0, -0.001), (1.0, 1.001), (-1.0, 0.0), (-0.0001, 0.0), (1e-7, 0.0), (9e-7, 0.0),
                 (1.1e6, 0.0), (float("inf"), 0.0), (1.0, float("inf"))):
        assert L.tarok_set_play_mode(env, t, e) == -1, (t, e)
        assert get() == (0.5, 0.25), (t, e)
    for t, e in ((0.0, 0.0), (0.0, 1.0), (1e-6, 0.0), (1e6, 1.0), (1.0, 0.0), (2.0, 0.1)):
        assert L.tarok_set_play_mode(env, t, e) == 0, (t, e)
        assert get() == (f32(t).value, f32(e).value)
    assert L.tarok_get_play_mode(env, None, None) == 0
