"""CPU: the model of tarok_front_lines (tests/front_lines_model.py), the argument checks of the Python surface, the
declared C entry points, and the launch list of SelfPlay with and without front=."""
import ctypes
import os

import pytest
import torch

import front_lines_model as FM
from oracle import tarok_spec as S
from tarok_amd import _native, karte as K
from tarok_amd import selfplay as SP
from tarok_amd.env import TarokVecEnv
from front_lines_cpu_cases import GIDX, SEED, model_weights, zero_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the model
def test_empty_set_is_the_bot_line():
    bid = dict(W=model_weights(1), scale=70.0, playouts=1, margin=0, contracts=0x3FF, pass_value=False)
    for nep in range(1, 9):
        want = FM.bot_line(SEED, GIDX + nep, nep, S.MIX_BOT).lanes()
        for b in (None, bid, dict(bid, pass_value=True)):
            got = FM.front_game(SEED, GIDX + nep, nep, 0, S.MIX_BOT, bid=b, exchange=model_weights(2)).lanes()
            assert list(got) == list(want)


def test_the_heads_change_lines_and_only_where_seated():
    bid = dict(W=model_weights(1), scale=70.0, playouts=1, margin=0, contracts=0x3FF, pass_value=False)
    differ = 0
    for nep in range(1, 13):
        bot = FM.bot_line(SEED, GIDX, nep, S.MIX_BOT)
        g = FM.front_game(SEED, GIDX, nep, 15, S.MIX_BOT, bid=bid, exchange=model_weights(2))
        differ += list(g.lanes()) != list(bot.lanes())
        assert sorted(int(c) for h in g.g.hand for c in FM.XH.cards_of(int(h))) is not None
    assert differ > 0


def test_line_selection():
    ep = 20
    lines = [(FM.EMPTY, 0)] * FM.AHEAD
    assert FM.call(ep, lines)[1] == []                                       # empty lines
    for e in range(ep + 1, ep + 1 + FM.AHEAD):
        lines = FM.redeal(lines, e)
    after, taken = FM.call(ep, lines)
    assert sorted(taken) == list(range(FM.AHEAD)) and all(m == n for n, m in after)      # valid: all fourteen
    assert FM.call(ep, after)[1] == []                                       # already marked
    ep += 2                                                                  # two games consumed: their lines are stale ...
    assert FM.call(ep, [(n, 0) for n, _ in after])[1] == sorted(b for b in range(FM.AHEAD) if b not in (21 % 14, 22 % 14))
    pending = FM.redeal(after, ep + FM.AHEAD - 1)                            # ... one is re-dealt, the other still pending
    assert FM.call(ep, pending)[1] == [(ep + FM.AHEAD - 1) % FM.AHEAD]


def test_mutants_are_caught():
    ep = 20
    lines = [(FM.EMPTY, 0)] * FM.AHEAD
    for e in range(ep + 1, ep + 1 + FM.AHEAD):
        lines = FM.redeal(lines, e)
    after, _ = FM.call(ep, lines)
    stale_too = lambda episode, b, nep, mark: nep % FM.AHEAD == b and mark != nep                  # fronts a stale tag
    assert any(stale_too(ep + 1, b, n, 0) != FM.takes(ep + 1, b, n, 0) for b, (n, _) in enumerate(after))
    keeps = lambda lines, episode: [(episode, episode) if k == episode % FM.AHEAD and m == n else ((episode, m) if k == episode % FM.AHEAD else (n, m))
                                    for k, (n, m) in enumerate(lines)]          # a re-deal that carries "fronted" over
    good, bad = FM.redeal(after, ep + 1 + FM.AHEAD), keeps(after, ep + 1 + FM.AHEAD)
    assert FM.call(ep + 1, good)[1] == [(ep + 1) % FM.AHEAD] and FM.call(ep + 1, bad)[1] == []


# ---- the surface
def bare_env(mix=K.MIX_BOT):
    env = TarokVecEnv.__new__(TarokVecEnv)
    env._h, env.n, env.mix, env.device = None, 8, mix, torch.device("cpu")
    return env


def test_front_lines_value_errors():
    env, w = bare_env(), zero_weights()
    bad = [dict(), dict(bid=w), dict(bid=w, scale=0.0), dict(bid=w, scale=2.0 ** 21), dict(bid=w, scale=1.0, contracts=0),
           dict(bid=w, scale=1.0, contracts=0x400), dict(bid=w, scale=1.0, playouts=0), dict(exchange=w, seats=16),
           dict(exchange=w, seats=-1), dict(exchange=w, seats_per_game=torch.zeros(7, dtype=torch.uint8)),
           dict(exchange=w, seats_per_game=torch.zeros(8, dtype=torch.int32)), dict(exchange=w, count_out=torch.zeros(1, dtype=torch.int32)),
           dict(exchange=w, hist_out=torch.zeros(9, dtype=torch.int64))]
    for kw in bad:
        with pytest.raises(ValueError):
            env.front_lines(**kw)
    with pytest.raises(ValueError, match="MIX_BOT"):
        bare_env(K.MIX_ALL).front_lines(bid=w, scale=1.0)
    with pytest.raises((AssertionError, ValueError)):
        env.front_lines(exchange=w[:5] + [torch.zeros(63)])


def test_selfplay_front_value_errors():
    env, w = bare_env(), zero_weights()
    for front in (dict(), dict(bid=w), dict(bid=w, scale=70.0, every=0), dict(exchange=w, contracts=0), dict(exchange=w, salt=1),
                  dict(bid=w, scale=70.0, playouts=0)):
        with pytest.raises(ValueError):
            SP.SelfPlay.check_front(front, env)
    with pytest.raises(ValueError, match="MIX_BOT"):
        SP.SelfPlay.check_front(dict(bid=w, scale=70.0), bare_env(K.MIX_ALL))
    assert SP.SelfPlay.check_front(None, env) is None
    f = SP.SelfPlay.check_front(dict(exchange=w), bare_env(K.MIX_ALL))
    assert f["every"] == 1 and f["bid"] is None and f["contracts"] == K.BID_DEFAULT_CONTRACTS


def test_the_entry_points_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "tarok_env.h")).read()
    for name in ("tarok_front_lines_scratch_bytes", "tarok_front_lines", "tarok_get_lines"):
        assert name + "(" in header and name in _native.SYMBOLS
    if os.path.exists(_native.LIB_PATH):
        L = ctypes.CDLL(_native.LIB_PATH)
        L.tarok_front_lines_scratch_bytes.restype = ctypes.c_int64
        L.tarok_front_lines_scratch_bytes.argtypes = [ctypes.c_int64]
        assert L.tarok_front_lines_scratch_bytes(300) == 128 + 8 * 14 * 300
        assert L.tarok_front_lines_scratch_bytes(0) < 0
        assert L.tarok_abi_version() == 5                                   # additions only


# ---- the launch list of SelfPlay
class Recorder:
    """What SelfPlay reads of an env, on the CPU; every call is recorded by name."""
    mfma_weight_order = staticmethod(TarokVecEnv.mfma_weight_order)
    check_mlp_weights = staticmethod(TarokVecEnv.check_mlp_weights)

    def __init__(self, n=4):
        self.n, self.device, self.mix, self.game_offset, self.history, self.calls = n, torch.device("cpu"), K.MIX_BOT, 0, False, []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def method(*args, **kwargs):
            self.calls.append(name)
            if name in ("reset", "exchange", "legal_actions"):
                return type("Obs", (), dict(words=torch.zeros(self.n, dtype=torch.int64)))()
            if name == "bid_round":
                return tuple(torch.zeros(self.n, dtype=torch.int8) for _ in range(3))
            if name == "exchange_values":
                return torch.zeros(self.n, dtype=torch.int8), torch.zeros((self.n, 3), dtype=torch.uint8)
            return None
        return method


def launches(front, T=3):
    env = Recorder()
    sp = SP.SelfPlay(env, use_graph=False, fused_learner=False, front=front)
    sp.collect(T)
    return env.calls


def test_front_none_issues_the_launches_it_issued_before():
    assert launches(None) == ["reset"] + ["policy_step"] * 3


def test_front_adds_the_chain_and_one_call_a_rollout():
    w = zero_weights()
    start = ["reset", "bid_values", "bid_round", "reset", "exchange_values", "exchange", "prefetch", "front_lines_scratch", "front_lines"]
    assert launches(dict(bid=w, exchange=w, scale=70.0)) == start + ["front_lines"] + ["policy_step"] * 3
    assert launches(dict(exchange=w)) == ["reset", "reset", "exchange_values", "exchange", "prefetch", "front_lines_scratch",
                                          "front_lines", "front_lines"] + ["policy_step"] * 3
    with pytest.raises(ValueError, match="never fronted"):
        launches(dict(exchange=w), T=49)
