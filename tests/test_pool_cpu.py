"""CPU: the opponent pool's host side — TarokVecEnv.stack_pool / check_pool_weights, SelfPlay's group rule and argument
errors, evaluate.pool_block_scores, and tarok_policy_step_pool's declaration, binding and argument checks (which come
before any HIP call: no GPU is needed)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tarok_amd import evaluate as EV
from tarok_amd import karte as K
from tarok_amd import selfplay as SP
from tarok_amd.env import TarokVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def weight_set(fill=0.0):
    bf = lambda *s: torch.full(s, fill, dtype=torch.bfloat16)
    fl = lambda *s: torch.full(s, fill, dtype=torch.float32)
    return [bf(256, 256), fl(256), bf(256, 256), fl(256), bf(64, 256), fl(64)]


def test_stack_pool_shapes_and_dtypes():
    sets = [weight_set(float(k)) for k in range(3)]
    pool = TarokVecEnv.stack_pool(sets)
    assert [tuple(t.shape) for t in pool] == [(3, 256, 256), (3, 256), (3, 256, 256), (3, 256), (3, 64, 256), (3, 64)]
    assert [t.dtype for t in pool] == [torch.bfloat16, torch.float32] * 3 and all(t.is_contiguous() for t in pool)
    for k in range(3):
        for t, s in zip(pool, sets[k]):
            assert torch.equal(t[k], s) and t[k].data_ptr() != s.data_ptr()
    # entry k of an array starts k * size elements after its base: the sizes of include/tarok_env.h
    assert [t[1].data_ptr() - t[0].data_ptr() for t in pool] == [2 * 65536, 4 * 256, 2 * 65536, 4 * 256, 2 * 16384, 4 * 64]
    assert TarokVecEnv.check_pool_weights(pool) == (3, tuple(pool))
    assert TarokVecEnv.check_pool_weights(list(TarokVecEnv.stack_pool(sets[:1])))[0] == 1
    with pytest.raises(ValueError):
        TarokVecEnv.stack_pool([])
    with pytest.raises(ValueError):
        TarokVecEnv.stack_pool([weight_set()] * (K.POOL_MAX + 1))
    assert TarokVecEnv.stack_pool([weight_set()] * K.POOL_MAX)[0].shape[0] == K.POOL_MAX == 64
    wrong = weight_set()
    wrong[2] = wrong[2].float()
    with pytest.raises((AssertionError, ValueError)):
        TarokVecEnv.stack_pool([weight_set(), wrong])
    with pytest.raises((AssertionError, ValueError)):
        TarokVecEnv.stack_pool([weight_set()[:5]])
    for bad in (pool[:5], [t.float() for t in pool], [pool[0][:2]] + list(pool[1:]), [pool[0].transpose(1, 2)] + list(pool[1:]),
                weight_set(), [t[:0] for t in pool], None, [None] * 6):
        with pytest.raises(ValueError):
            TarokVecEnv.check_pool_weights(bad)


def test_group_rule():
    """Group g meets opponent g % K; with self_play_groups = f every group with g % max(1, round(1 / f)) == 0 is the
    learner's own (index K)."""
    assert SP.SelfPlay.pool_group_net(7, 3) == [0, 1, 2, 0, 1, 2, 0]
    assert SP.SelfPlay.pool_group_net(4, 1) == [0] * 4
    assert SP.SelfPlay.pool_group_net(8, 3, 0.25) == [3, 1, 2, 0, 3, 2, 0, 1]
    assert SP.SelfPlay.pool_group_net(4, 2, 0.25) == [2, 1, 0, 1]
    assert SP.SelfPlay.pool_group_net(5, 2, 0.5) == [2, 1, 2, 1, 2]
    assert SP.SelfPlay.pool_group_net(3, 2, 1.0) == [2, 2, 2]
    assert SP.SelfPlay.pool_group_net(6, 4, 0.3) == [4, 1, 2, 4, 0, 1]          # round(1 / 0.3) = 3
    assert [SP.SelfPlay.pool_period(f) for f in (0, 0.0, 1, 0.5, 0.34, 0.1, 0.001)] == [0, 0, 1, 2, 3, 10, 1000]
    for f in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            SP.SelfPlay.pool_period(f)
    w = weight_set()
    assert not SP.SelfPlay.is_pool(w) and not SP.SelfPlay.is_pool(tuple(w)) and not SP.SelfPlay.is_pool(None)
    assert SP.SelfPlay.is_pool([w]) and SP.SelfPlay.is_pool((w, w)) and SP.SelfPlay.is_pool([])


def test_argument_errors():
    w = weight_set()
    with pytest.raises(ValueError, match="pool"):
        SP.SelfPlay(None, opponent=[])
    with pytest.raises(ValueError, match="pool"):
        SP.SelfPlay(None, opponent=[w] * 65)
    with pytest.raises(ValueError, match="self_play_groups"):
        SP.SelfPlay(None, opponent=w, self_play_groups=0.25)                     # one opponent is no pool
    with pytest.raises(ValueError, match="self_play_groups"):
        SP.SelfPlay(None, self_play_groups=0.25)
    with pytest.raises(ValueError, match="self_play_groups"):
        SP.SelfPlay(None, opponent=[w], self_play_groups=2.0)
    with pytest.raises(RuntimeError, match="tarok_policy_step_versus"):
        SP.SelfPlay(None, opponent=[w], hidden=128)
    sig = inspect.signature(SP.SelfPlay.__init__).parameters
    assert sig["self_play_groups"].default == 0.0
    assert list(inspect.signature(SP.SelfPlay.set_opponent).parameters) == ["self", "weights", "index"]
    # policy_step: the checks come before the env is touched (a stand-in object for self)
    pool = TarokVecEnv.stack_pool([w, w])
    sig = inspect.signature(TarokVecEnv.policy_step).parameters
    assert sig["opponent_pool"].default is None and sig["group_net"].default is None
    with pytest.raises(ValueError, match="exclude"):
        TarokVecEnv.policy_step(object(), w, None, None, None, opponent=w, opponent_pool=pool)
    with pytest.raises(ValueError, match="opponent_pool"):
        TarokVecEnv.policy_step(object(), w, None, None, None, opponent_pool=pool[:5])
    with pytest.raises(ValueError, match="group_net"):
        TarokVecEnv.policy_step(object(), w, None, None, None, group_net=torch.zeros(1, dtype=torch.uint8))
    with pytest.raises(ValueError):
        EV.evaluate_vs_pool(w, [], 256, 1)
    with pytest.raises(ValueError):
        EV.evaluate_vs_pool([w], [w], 256, 1)


def test_pool_block_scores():
    """[5, episodes * K * G, 4] -> block k's first n_games slots of every episode, in evaluate_vs_policy's order."""
    k, n, episodes, G = 3, 300, 2, 512
    s = np.arange(5 * episodes * k * G * 4).reshape(5, episodes * k * G, 4)
    for j in range(k):
        got = EV.pool_block_scores(s, j, n, k)
        assert got.shape == (5, episodes * n, 4)
        want = np.concatenate([s[:, e * k * G + j * G:e * k * G + j * G + n] for e in range(episodes)], axis=1)
        assert (got == want).all()
    one = np.arange(5 * 2 * 256 * 4).reshape(5, 512, 4)
    assert (EV.pool_block_scores(one, 0, 256, 1) == one).all()


@pytest.fixture(scope="module")
def lib():
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_the_entry_point_is_declared_and_bound(lib):
    from tarok_amd import _native
    src = open(os.path.join(ROOT, "include", "tarok_env.h")).read()
    assert int(re.search(r"#define TAROK_POOL_MAX (\d+)", src).group(1)) == K.POOL_MAX == TarokVecEnv.POOL_MAX
    assert "tarok_policy_step_pool" in re.search(r"/\* The play mode of an env:.*?\*/", src, flags=re.S).group(0)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    params = lambda name: [" ".join(p.split()) for p in re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src).group(1).split(",")]
    pool, versus = params("tarok_policy_step_pool"), params("tarok_policy_step_versus")
    assert pool[:9] == versus[:9]                                 # env, seats, seats_per_game, the learner's six
    assert pool[9:17] == ["int pool_size", "const void *p1", "const float *q1", "const void *p2", "const float *q2", "const void *p3",
                          "const float *q3", "const uint8_t *group_net"]
    assert pool[17:] == versus[15:]                               # then exactly the versus launch's remaining arguments
    assert "tarok_policy_step_pool" in _native.SYMBOLS
    types = lib.tarok_policy_step_pool.argtypes
    assert len(types) == len(pool) == 28 and types[9] is ctypes.c_int and types[1] is ctypes.c_int and types[26] is ctypes.c_int
    assert lib.tarok_abi_version() == 5                           # an addition


def test_bad_arguments_are_refused_without_a_gpu(lib):
    """Every check comes before the first HIP call: a zeroed stand-in env is never followed."""
    z = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(4096)
    q = ctypes.cast(buf, ctypes.c_void_p)
    r = ctypes.c_void_p(q.value + 2048)
    fn = lib.tarok_policy_step_pool

    def call(env=q, seats=6, learner=None, k=3, pool=None, obs=q, action=q, obs_out=r):
        return fn(env, seats, z, *(learner or [q] * 6), k, *(pool or [q] * 6), z, obs, action, z, z, z, z, z, z, obs_out, 0, z)
    for kw in (dict(env=z), dict(seats=16), dict(seats=-1), dict(k=0), dict(k=65), dict(k=-3), dict(obs=z), dict(action=z), dict(obs_out=z),
               dict(obs_out=q)):
        assert call(**kw) == -1, kw
    for j in range(6):
        holed = [q] * 6
        holed[j] = z
        assert call(pool=holed) == -1 and call(learner=holed) == -1, j
