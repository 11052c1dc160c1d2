"""CPU-side checks of the two-network launch: tarok_policy_step_versus is declared, exported and bound, and refuses bad
arguments before any HIP call; TarokVecEnv.policy_step takes an opponent; evaluate_vs_policy refuses malformed weight
tuples before it creates an env."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tarok_policy_step_versus"


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  -- before any dlopen of libtarokenv.so: both must share ONE HIP runtime
    import tarok_amd
    from tarok_amd import _native
    tarok_amd.build()
    return _native.lib()


def test_entry_point_is_declared_exported_and_bound(lib):
    from tarok_amd import _native
    src = open(os.path.join(ROOT, "include", "tarok_env.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, src)
    assert m, "include/tarok_env.h does not declare %s" % NAME
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert len(params) == 26
    assert params[0] == "tarok_env *env" and params[1] == "int seats" and params[2] == "const uint8_t *seats_per_game"
    # two groups of six weight parameters: bf16 matrices as void, f32 biases
    for group in (params[3:9], params[9:15]):
        kinds = [p.rsplit("*", 1)[0].strip() for p in group]
        assert kinds == ["const void", "const float"] * 3, group
    assert len(set(p.rsplit("*", 1)[1] for p in params[3:15])) == 12
    # ... then the arguments of tarok_policy_step from obs onward, in its order
    ps = re.search(r"\bint\s+tarok_policy_step\s*\(([^;]*)\)\s*;", src)
    plain = [" ".join(p.split()) for p in ps.group(1).split(",")]
    assert plain[7] == "const uint64_t *obs" and plain[7:] == params[15:]
    assert re.fullmatch(r"tarok_[a-z_]+", NAME)                              # (tests/test_abi_cpu.py finds functions by this pattern)
    assert NAME in _native.SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), NAME)
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == 26 and fn.argtypes[1] is ctypes.c_int and fn.argtypes[24] is ctypes.c_int
    assert fn.restype is ctypes.c_int
    assert lib.tarok_abi_version() == 5                                      # an additive change


def test_entry_point_rejects_bad_arguments_without_a_gpu(lib):
    fn = getattr(lib, NAME)
    z = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(4096)                                  # stands in for the pointers that must not be NULL
    q = ctypes.cast(buf, ctypes.c_void_p)
    q8 = ctypes.c_void_p(q.value + 8)

    def args(obs=q, action=q, obs_out=q8, missing=None):
        w = [q] * 12
        if missing is not None:
            w[missing] = z
        return w + [obs, action, z, z, z, z, z, z, obs_out, 0, z]

    assert fn(z, 15, z, *args()) == -1                                       # NULL env
    assert fn(z, 1, q, *args()) == -1
    # the seat set is checked before the env is looked at: a pointer to zeroed memory is never followed
    for seats in (16, -1, 255):
        assert fn(q, seats, z, *args()) == -1, seats
    # obs == obs_out with everything else in order (a zeroed stand-in env, with and without the per-game array)
    assert fn(q, 3, z, *args(obs=q, obs_out=q)) == -1
    assert fn(q, 15, q, *args(obs=ctypes.c_void_p(q.value + 64), obs_out=ctypes.c_void_p(q.value + 64))) == -1
    # each of the twelve weight and bias pointers in turn
    for k in range(12):
        assert fn(q, 6, z, *args(missing=k)) == -1, k
    # ... and the required arrays
    assert fn(q, 6, z, *args(obs=z)) == -1
    assert fn(q, 6, z, *args(action=z)) == -1
    assert fn(q, 6, z, *args(obs_out=z)) == -1


def test_policy_step_takes_an_opponent():
    from tarok_amd.env import TarokVecEnv
    sig = inspect.signature(TarokVecEnv.policy_step)
    assert "opponent" in sig.parameters and sig.parameters["opponent"].default is None
    # the arguments that were there keep their places
    assert list(sig.parameters)[:5] == ["self", "weights", "obs_words", "obs_out", "action_out"]
    from tarok_amd import evaluate as EV
    sig = inspect.signature(EV._play_passes)
    assert list(sig.parameters) == ["weights", "n_games", "episodes", "seed", "mix", "device", "inspect", "opponent"]
    assert sig.parameters["opponent"].default is None
    from tarok_amd.selfplay import SelfPlay
    assert "opponent" in inspect.signature(SelfPlay.evaluate).parameters and hasattr(SelfPlay, "snapshot")


def cpu_weights(torch):
    return [torch.zeros((256, 256), dtype=torch.bfloat16), torch.zeros(256), torch.zeros((256, 256), dtype=torch.bfloat16),
            torch.zeros(256), torch.zeros((64, 256), dtype=torch.bfloat16), torch.zeros(64)]


def test_evaluate_vs_policy_refuses_malformed_weights_before_creating_an_env(monkeypatch):
    import torch
    from tarok_amd import evaluate as EV

    def no_env(*a, **k):
        raise RuntimeError("an env was created")
    monkeypatch.setattr(EV, "TarokVecEnv", type("NoEnv", (), {"__init__": no_env, "check_mlp_weights": staticmethod(EV.TarokVecEnv.check_mlp_weights)}))
    good = cpu_weights(torch)
    bad = []
    w = cpu_weights(torch); w[0] = w[0].float(); bad.append(w)               # wrong dtype of a matrix
    w = cpu_weights(torch); w[5] = w[5].double(); bad.append(w)              # ... of a bias
    w = cpu_weights(torch); w[4] = torch.zeros((54, 256), dtype=torch.bfloat16); bad.append(w)   # wrong shape
    w = cpu_weights(torch); w[1] = torch.zeros(255); bad.append(w)
    bad.append(cpu_weights(torch)[:5])                                       # five tensors
    bad.append(None)
    for b in bad:
        for pair in ((b, good), (good, b)):
            with pytest.raises((ValueError, AssertionError)):
                EV.evaluate_vs_policy(pair[0], pair[1], 16, 1)
    # well-formed tuples get as far as the env
    with pytest.raises(RuntimeError, match="an env was created"):
        EV.evaluate_vs_policy(good, good, 16, 1)
