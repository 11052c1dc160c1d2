"""CPU-side checks of the duplicate evaluation: tarok_policy_step_seats is declared, exported and bound, and refuses
bad arguments before any HIP call; tarok_amd.evaluate.duplicate_advantage against hand-computed figures."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tarok_policy_step_seats"


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
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 20
    assert params[1] == "int seats" and params[2] == "const uint8_t *seats_per_game"
    # ... then the arguments of tarok_policy_step, in its order
    ps = re.search(r"\bint\s+tarok_policy_step\s*\(([^;]*)\)\s*;", src)
    assert [p.strip() for p in ps.group(1).split(",")][1:] == params[3:]
    assert NAME in _native.SYMBOLS
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), NAME)
    fn = getattr(lib, NAME)
    assert len(fn.argtypes) == 20 and fn.argtypes[1] is ctypes.c_int and fn.restype is ctypes.c_int
    assert lib.tarok_abi_version() == 5                                      # an additive change


def test_entry_point_rejects_bad_arguments_without_a_gpu(lib):
    fn = getattr(lib, NAME)
    z = ctypes.c_void_p(0)
    buf = ctypes.create_string_buffer(4096)                                  # stands in for the pointers that must not be NULL
    q = ctypes.cast(buf, ctypes.c_void_p)
    rest = lambda obs, obs_out: [q] * 6 + [obs, q, z, z, z, z, z, z, obs_out, 0, z]
    assert fn(z, 15, z, *rest(q, q)) == -1                                   # NULL env
    assert fn(z, 1, z, *rest(q, ctypes.c_void_p(q.value + 8))) == -1
    # the seat set is checked before the env is looked at: a pointer to zeroed memory is never followed
    for seats in (16, -1, 255):
        assert fn(q, seats, z, *rest(q, ctypes.c_void_p(q.value + 8))) == -1, seats
    # obs == obs_out with everything else in order (a zeroed stand-in env, a valid seat set, with and without the per-game
    # array): refused before the env is looked at, before any HIP call
    assert fn(q, 3, z, *rest(q, q)) == -1
    assert fn(q, 15, q, *rest(ctypes.c_void_p(q.value + 64), ctypes.c_void_p(q.value + 64))) == -1
    # ... and so is a missing required array
    assert fn(q, 3, z, *rest(z, ctypes.c_void_p(q.value + 8))) == -1


def hand_scores():
    """Two deals.  Pass 0 (Bot everywhere) and the four network passes; only scores[1 + k, d, k] and scores[0, d, k]
    enter the statistic, the other entries are there to be ignored."""
    s = np.full((5, 2, 4), 999, np.int32)
    s[0] = [[10, -20, 30, 0], [-5, 5, 15, -35]]
    own = [[20, -10, 30, -40], [5, 25, -15, -35]]                            # [d][k] = scores[1 + k, d, k]
    for d in range(2):
        for k in range(4):
            s[1 + k, d, k] = own[d][k]
    return s


def test_duplicate_advantage_hand_computed():
    from tarok_amd.evaluate import duplicate_advantage
    r = duplicate_advantage(hand_scores())
    # differences by deal: [10, 10, 0, -40] and [10, 20, -30, 0]
    assert r["deals"] == 2
    assert r["policy_mean"] == (20 - 10 + 30 - 40 + 5 + 25 - 15 - 35) / 8.0 == -2.5
    assert r["bot_mean"] == (10 - 20 + 30 + 0 - 5 + 5 + 15 - 35) / 8.0 == 0.0
    assert r["advantage"] == -2.5
    assert r["by_seat"] == [10.0, 15.0, -15.0, -20.0]
    # per-deal means -5 and 0: sample standard deviation sqrt(12.5), over sqrt(2 deals) = 2.5
    assert math.isclose(r["stderr"], 2.5, rel_tol=1e-12)
    assert set(r) == {"policy_mean", "bot_mean", "advantage", "stderr", "by_seat", "deals"}


def test_duplicate_advantage_takes_torch_tensors_and_checks_the_shape():
    import torch
    from tarok_amd.evaluate import duplicate_advantage
    assert duplicate_advantage(torch.from_numpy(hand_scores())) == duplicate_advantage(hand_scores())
    for shape in ((4, 2, 4), (5, 2, 3), (5, 4), (5, 0, 4)):
        with pytest.raises(ValueError):
            duplicate_advantage(np.zeros(shape, np.int32))
    assert math.isnan(duplicate_advantage(np.zeros((5, 1, 4)))["stderr"])   # one deal has no spread to estimate


def test_identical_passes_give_zero():
    from tarok_amd.evaluate import duplicate_advantage
    rnd = np.random.RandomState(5)
    one = rnd.randint(-300, 300, size=(37, 4)).astype(np.int32)
    r = duplicate_advantage(np.stack([one] * 5))
    assert r["advantage"] == 0.0 and r["stderr"] == 0.0 and r["by_seat"] == [0.0] * 4
    assert r["policy_mean"] == r["bot_mean"] == float(one.mean()) and r["deals"] == 37


def test_a_constant_on_the_networks_seat_moves_that_seat_by_the_constant():
    from tarok_amd.evaluate import duplicate_advantage
    rnd = np.random.RandomState(6)
    s = rnd.randint(-300, 300, size=(5, 64, 4)).astype(np.int64)
    base = duplicate_advantage(s)
    for k in range(4):
        for c in (7, -32):
            t = s.copy()
            t[1 + k, :, k] += c
            r = duplicate_advantage(t)
            for j in range(4):
                assert r["by_seat"][j] - base["by_seat"][j] == (c if j == k else 0), (k, c, j)   # integers over 64 deals: exact
            assert r["advantage"] - base["advantage"] == c / 4.0
            assert math.isclose(r["stderr"], base["stderr"], rel_tol=1e-9)   # a shift of every deal: no more spread
            assert r["bot_mean"] == base["bot_mean"]
            # a constant anywhere else in that pass is not looked at
            u = s.copy()
            u[1 + k, :, (k + 1) & 3] += c
            assert duplicate_advantage(u) == base
